"""mdg_attn_fwd_paged8 (multi-token attention straight from the paged fp8 cache; page 64, a shuffled block table) in one process,
the sides ALTERNATING run by run, under the COLD protocol of attn_decode_paged8_timing.py (calls rotate over enough distinct caches
that their total exceeds --cold-mib, so no call finds its cache in the 256 MiB Infinity Cache), HIP events around back-to-back calls,
the min / median / max of 5 runs after a warm-up.  32 query heads, 8 kv heads, bf16, causal; the T queries are the last T of S keys.
Every side is called through the C entries with its buffers allocated beforehand.  Three comparisons:

  (a) replaced  mdg_kv8_paged_dequant x 2 into bf16 [B, n_kv, S, r] tensors + mdg_attn_fwd on them: what such a call cost before
  (b) flat      mdg_attn_fwd_kv8 on the contiguous cache that holds the same rows, at equal lengths: what the table costs
  (c) ragged    16 sequences with lengths spread evenly over 2048 .. 32768, seq_lens on the device, against (a) at S = 32768

    python scripts/probes/attn_fwd_paged8_timing.py [--shapes 1x64x2048,... --widths 90x77,... --json out.json]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import _lib, ops  # noqa: E402
from scripts.probes.attn_decode_paged8_timing import PAGE, timed_pair  # noqa: E402
from scripts.probes.attn_decode_timing import write_json  # noqa: E402

SHAPES = ",".join("%dx%dx%d" % (B, T, S) for B in (1, 16) for T in (64, 512) for S in (2048, 8192, 32768))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="BxTxS list")
    ap.add_argument("--widths", default="90x77,90x90,128x128", help="r_qk x r_vo list")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-calls", type=int, default=8)
    ap.add_argument("--cold-mib", type=float, default=320.0, help="total cache bytes a rotation must exceed (Infinity Cache: 256)")
    ap.add_argument("--ragged", default="16x2048x32768", help="B x shortest x longest of the ragged batch ('' skips it)")
    ap.add_argument("--ragged-T", default="64,512")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_fwd_paged8_timing: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    stream = torch.cuda.current_stream(dev).cuda_stream
    records = []
    print("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    rand = lambda *s: torch.randn(*s, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731

    def caches(B, S, r_qk, r_vo):
        """One contiguous fp8 cache of S rows a sequence and the pools that hold the same rows behind a shuffled table."""
        P = S // PAGE
        table = torch.randperm(B * P, device=dev, generator=gen).to(torch.int32).view(B, P)
        flat, pools = [], []
        for r in (r_qk, r_vo):
            x = rand(B, a.kv, S, r)
            data = torch.empty(B, a.kv, S, ops.kv8_pitch(r), dtype=torch.uint8, device=dev)
            sc = torch.empty(B, a.kv, S, dtype=torch.float32, device=dev)
            ops.kv8_append(x, data, sc, 0)
            pd, ps = torch.empty(B * P, a.kv, PAGE, data.shape[3], dtype=torch.uint8, device=dev), torch.empty(B * P, a.kv, PAGE, device=dev)
            pd[table.flatten().long()] = data.view(B, a.kv, P, PAGE, -1).transpose(1, 2).reshape(B * P, a.kv, PAGE, -1)
            ps[table.flatten().long()] = sc.view(B, a.kv, P, PAGE).transpose(1, 2).reshape(B * P, a.kv, PAGE)
            flat += [data, sc]
            pools += [pd, ps]
            del x
        return tuple(flat), tuple(pools), table

    def sides_of(q, flat, pools, table, lens, B, T, S, r_qk, r_vo, out, kbuf, vbuf):
        """The three calls on one cache set: (paged8 with `lens`, dequant x 2 + fwd at S, fwd_kv8 at S)."""
        scale, (pk, pv), n_pages = float(r_qk) ** -0.5, (ops.kv8_pitch(r_qk), ops.kv8_pitch(r_vo)), pools[0].shape[0]
        tail = (out.data_ptr(), a.heads * r_vo, stream)
        p_args = (q.data_ptr(), *(t.data_ptr() for t in pools), _lib.MDG_BF16, B, T, S, a.heads, a.kv, r_qk, r_vo, n_pages, PAGE, pk, pv,
                  table.data_ptr(), table.shape[1], lens.data_ptr(), scale, 1, *tail, None, 0, 0, 0, 0, None, 0)
        f_args = (q.data_ptr(), *(t.data_ptr() for t in flat), _lib.MDG_BF16, B, T, S, a.heads, a.kv, r_qk, r_vo, S, pk, pv, scale, 1, *tail,
                  None, 0, 0, 0, 0, None, 0)
        d_args = [(pools[2 * i].data_ptr(), pools[2 * i + 1].data_ptr(), _lib.MDG_BF16, B, a.kv, S, r, n_pages, PAGE, p, table.data_ptr(),
                   table.shape[1], buf.data_ptr(), stream) for i, (r, p, buf) in enumerate(((r_qk, pk, kbuf), (r_vo, pv, vbuf)))]
        a_args = (q.data_ptr(), kbuf.data_ptr(), vbuf.data_ptr(), _lib.MDG_BF16, B, T, S, a.heads, a.kv, r_qk, r_vo, a.kv * S * r_qk, S * r_qk,
                  r_qk, a.kv * S * r_vo, S * r_vo, r_vo, scale, 1, *tail)

        def replaced():
            return lib.mdg_kv8_paged_dequant(*d_args[0]) or lib.mdg_kv8_paged_dequant(*d_args[1]) or lib.mdg_attn_fwd(*a_args)
        return (lambda: lib.mdg_attn_fwd_paged8(*p_args)), replaced, (lambda: lib.mdg_attn_fwd_kv8(*f_args))

    def report(rec, names, sides, calls):
        for fns in sides:
            rc = fns[0]()
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError(_lib.last_error())
        best = []
        for name, times in zip(names, timed_pair(sides, calls, a.runs)):
            e = dict(us_min=round(min(times) * 1e3, 2), us_median=round(statistics.median(times) * 1e3, 2), us_max=round(max(times) * 1e3, 2))
            e["spread"] = round((max(times) - min(times)) / min(times), 4)
            rec["paths"][name] = e
            best.append(min(times))
            print("  %-28s cold %10.1f us min / %10.1f med / %10.1f max  (spread %4.1f %%)"
                  % (name, e["us_min"], e["us_median"], e["us_max"], 100 * e["spread"]), flush=True)
        return best

    def buffers(B, T, S, r_qk, r_vo):
        return (rand(B, a.heads, T, r_qk), torch.empty(B, T, a.heads, r_vo, dtype=torch.bfloat16, device=dev),
                torch.empty(B, a.kv, S, r_qk, dtype=torch.bfloat16, device=dev), torch.empty(B, a.kv, S, r_vo, dtype=torch.bfloat16, device=dev))

    for shape in a.shapes.split(",") if a.shapes else ():
        B, T, S = (int(x) for x in shape.split("x"))
        for width in a.widths.split(","):
            r_qk, r_vo = (int(x) for x in width.split("x"))
            nbytes = B * a.kv * S * (ops.kv8_pitch(r_qk) + ops.kv8_pitch(r_vo) + 8)
            nbuf = max(2, int(a.cold_mib * 2 ** 20 // nbytes) + 1)
            calls = max(a.min_calls, nbuf)
            q, out, kbuf, vbuf = buffers(B, T, S, r_qk, r_vo)
            lens = torch.full((B,), S, dtype=torch.int32, device=dev)
            sets = [caches(B, S, r_qk, r_vo) for _ in range(nbuf)]
            trio = [sides_of(q, f, p, t, lens, B, T, S, r_qk, r_vo, out, kbuf, vbuf) for f, p, t in sets]
            rec = dict(kind="equal", B=B, T=T, S=S, r_qk=r_qk, r_vo=r_vo, heads=a.heads, kv=a.kv, bytes=nbytes, buffers=nbuf, calls=calls,
                       runs=a.runs, page=PAGE, paths={})
            print("B=%d T=%d S=%d r_qk=%d r_vo=%d: K+V fp8 %.1f MB; %d caches each, %d calls x %d runs"
                  % (B, T, S, r_qk, r_vo, nbytes / 1e6, nbuf, calls, a.runs), flush=True)
            t_new, t_old, t_flat = report(rec, ("fwd_paged8", "paged_dequant x 2 + fwd", "fwd_kv8 contiguous"),
                                          tuple([t[i] for t in trio] for i in range(3)), calls)
            rec["paged_over_replaced"], rec["paged_over_contiguous"] = round(t_new / t_old, 4), round(t_new / t_flat, 4)
            print("  paged8 / replaced = %.3f   paged8 / fwd_kv8 = %.3f" % (t_new / t_old, t_new / t_flat), flush=True)
            records.append(rec)
            del q, out, kbuf, vbuf, sets, trio
            torch.cuda.empty_cache()

    if a.ragged:
        B, lo, hi = (int(x) for x in a.ragged.split("x"))
        lens_host = [lo + (hi - lo) * b // (B - 1) // PAGE * PAGE for b in range(B)]
        lens = torch.tensor(lens_host, dtype=torch.int32, device=dev)
        for T in (int(x) for x in a.ragged_T.split(",")):
            for width in a.widths.split(","):
                r_qk, r_vo = (int(x) for x in width.split("x"))
                q, out, kbuf, vbuf = buffers(B, T, hi, r_qk, r_vo)
                sets = [caches(B, hi, r_qk, r_vo) for _ in range(2)]
                trio = [sides_of(q, f, p, t, lens, B, T, hi, r_qk, r_vo, out, kbuf, vbuf) for f, p, t in sets]
                rec = dict(kind="ragged", B=B, T=T, lens=lens_host, r_qk=r_qk, r_vo=r_vo, heads=a.heads, kv=a.kv, page=PAGE, runs=a.runs,
                           keys_read=round(sum(lens_host) / (B * hi), 4), paths={})
                print("ragged B=%d T=%d lengths %d .. %d r_qk=%d r_vo=%d" % (B, T, lens_host[0], lens_host[-1], r_qk, r_vo), flush=True)
                t_new, t_old = report(rec, ("fwd_paged8 seq_lens", "paged_dequant x 2 + fwd S=%d" % hi),
                                      tuple([t[i] for t in trio] for i in range(2)), a.min_calls)
                rec["paged_over_replaced"] = round(t_new / t_old, 4)
                print("  paged8 / replaced = %.3f (keys read %.3f)" % (t_new / t_old, rec["keys_read"]), flush=True)
                records.append(rec)
                del q, out, kbuf, vbuf, sets, trio
                torch.cuda.empty_cache()
    if a.json:
        write_json(a.json, dict(device=torch.cuda.get_device_name(0), torch=torch.__version__), records)


if __name__ == "__main__":
    main()
