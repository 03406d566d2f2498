"""mdg_attn_decode_paged8 on a paged fp8 cache (page 64, a shuffled block table) against mdg_attn_decode_kv8 on the contiguous cache
that holds the same rows, in one process and ALTERNATING run by run: the shapes, the COLD protocol (calls rotate over enough distinct
caches that their total exceeds --cold-mib, so no call finds its cache in the 256 MiB Infinity Cache), HIP events around back-to-back
calls and the min / median / max of 5 runs after a warm-up of attn_decode_kv8_timing.py.  32 query heads, 8 kv heads, bf16 q, causal,
T = 1, the split rule of the device.  Three comparisons:

  equal    every sequence S keys long: paged time / contiguous time per shape, beside each side's own max - min spread
  ragged   16 sequences with lengths spread evenly over 2048 .. 32768: the paged kernel with seq_lens against mdg_attn_decode_kv8
           under a padding mask at S = 32768 (what a ragged batch costs without pages), with the K + V bytes each side reads
  append   mdg_kv8_paged_append of one decode step (K and V in one launch) against the two mdg_kv8_append launches it replaces

    python scripts/probes/attn_decode_paged8_timing.py [--shapes 1x1x2048,... --widths 90x77,... --json out.json]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import _lib, ops  # noqa: E402
from scripts.probes.attn_decode_timing import COPY_TBPS, write_json  # noqa: E402

PAGE = 64


def timed_pair(sides, calls, runs):
    """ms per call of each side, `runs` times after a warm-up run, the sides alternating run by run; call i of a run is
    fns[i % len(fns)] (the rotation over the buffers)."""
    out = [[] for _ in sides]
    for run in range(runs + 1):
        for fns, times in zip(sides, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(calls):
                fns[i % len(fns)]()
            b.record()
            b.synchronize()
            if run:
                times.append(a.elapsed_time(b) / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x1x2048,1x1x8192,1x1x32768,16x1x2048,16x1x8192,16x1x32768", help="BxTxS list")
    ap.add_argument("--widths", default="90x77,90x90,128x128", help="r_qk x r_vo list")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-calls", type=int, default=8)
    ap.add_argument("--cold-mib", type=float, default=320.0, help="total cache bytes a rotation must exceed (Infinity Cache: 256)")
    ap.add_argument("--ragged", default="16x2048x32768", help="B x shortest x longest of the ragged batch ('' skips it)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_decode_paged8_timing: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    gen = torch.Generator(device=dev).manual_seed(5)
    stream = torch.cuda.current_stream(dev).cuda_stream
    records = []
    print("device %s, %d CUs, torch %s; copy bandwidth taken as %.2f TB/s" % (torch.cuda.get_device_name(0), n_cu, torch.__version__,
                                                                            COPY_TBPS))
    rand = lambda *s: torch.randn(*s, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731

    def caches(B, S, r_qk, r_vo):
        """One contiguous fp8 cache of S rows a sequence and the pools that hold the same rows behind a shuffled table."""
        P = S // PAGE
        table = torch.randperm(B * P, device=dev, generator=gen).to(torch.int32).view(B, P)
        flat, pools = [], []
        for x, r in ((rand(B, a.kv, S, r_qk), r_qk), (rand(B, a.kv, S, r_vo), r_vo)):
            data = torch.empty(B, a.kv, S, ops.kv8_pitch(r), dtype=torch.uint8, device=dev)
            sc = torch.empty(B, a.kv, S, dtype=torch.float32, device=dev)
            ops.kv8_append(x, data, sc, 0)
            pd, ps = torch.empty(B * P, a.kv, PAGE, data.shape[3], dtype=torch.uint8, device=dev), torch.empty(B * P, a.kv, PAGE, device=dev)
            pd[table.flatten().long()] = data.view(B, a.kv, P, PAGE, -1).transpose(1, 2).reshape(B * P, a.kv, PAGE, -1)
            ps[table.flatten().long()] = sc.view(B, a.kv, P, PAGE).transpose(1, 2).reshape(B * P, a.kv, PAGE)
            flat += [data, sc]
            pools += [pd, ps]
        return tuple(flat), tuple(pools), table

    def report(rec, names, sides, calls, nbytes):
        for fns in sides:
            rc = fns[0]()
            torch.cuda.synchronize()
            if isinstance(rc, int) and rc != 0:
                raise RuntimeError(_lib.last_error())
        best = []
        for name, times, nb in zip(names, timed_pair(sides, calls, a.runs), nbytes):
            e = dict(us_min=round(min(times) * 1e3, 2), us_median=round(statistics.median(times) * 1e3, 2),
                     us_max=round(max(times) * 1e3, 2), mb=round(nb / 1e6, 2), of_copy=round(nb / (min(times) * 1e-3) / 1e12 / COPY_TBPS, 4))
            rec["paths"][name] = e
            best.append(min(times))
            print("  %-26s cold %9.1f us min / %9.1f med / %9.1f max   %8.2f MB  (%4.1f %% of copy)"
                  % (name, e["us_min"], e["us_median"], e["us_max"], e["mb"], 100 * e["of_copy"]), flush=True)
        return best

    def decode_fns(q, flat, pools, table, lens, B, T, S, r_qk, r_vo, rule, ws, out, mask=None):
        scale, (pk, pv) = float(r_qk) ** -0.5, (ops.kv8_pitch(r_qk), ops.kv8_pitch(r_vo))
        m = (None, 0, 0, 0, 0) if mask is None else (mask.data_ptr(), 1, mask.stride(0), 0, 0)
        f_args = (q.data_ptr(), *(t.data_ptr() for t in flat), _lib.MDG_BF16, B, T, S, a.heads, a.kv, r_qk, r_vo, S, pk, pv, scale,
                  0 if mask is not None else 1, rule, ws.data_ptr(), ws.numel() * 4, out.data_ptr(), a.heads * r_vo, stream, *m)
        p_args = (q.data_ptr(), *(t.data_ptr() for t in pools), _lib.MDG_BF16, B, T, S, a.heads, a.kv, r_qk, r_vo, pools[0].shape[0], PAGE,
                  pk, pv, table.data_ptr(), table.shape[1], lens.data_ptr(), scale, 1, rule, ws.data_ptr(), ws.numel() * 4, out.data_ptr(),
                  a.heads * r_vo, stream, None, 0, 0, 0, 0)
        return (lambda: lib.mdg_attn_decode_kv8(*f_args)), (lambda: lib.mdg_attn_decode_paged8(*p_args))

    for shape in a.shapes.split(","):
        B, T, S = (int(x) for x in shape.split("x"))
        for width in a.widths.split(","):
            r_qk, r_vo = (int(x) for x in width.split("x"))
            row = ops.kv8_pitch(r_qk) + ops.kv8_pitch(r_vo) + 8
            nbytes = B * a.kv * S * row
            nbuf = max(2, int(a.cold_mib * 2 ** 20 // nbytes) + 1)
            calls = max(a.min_calls, nbuf)
            q = rand(B, a.heads, T, r_qk)
            out = torch.empty(B, T, a.heads, r_vo, dtype=q.dtype, device=dev)
            rule = ops.attn_decode_splits(B, a.kv, S, dev)
            ws = torch.empty(lib.mdg_attn_decode_ws_bytes(B, T, a.heads, r_vo, rule) // 4, dtype=torch.float32, device=dev)
            lens = torch.full((B,), S, dtype=torch.int32, device=dev)
            sets = [caches(B, S, r_qk, r_vo) for _ in range(nbuf)]
            pairs = [decode_fns(q, f, p, t, lens, B, T, S, r_qk, r_vo, rule, ws, out) for f, p, t in sets]
            rec = dict(kind="equal", B=B, T=T, S=S, r_qk=r_qk, r_vo=r_vo, heads=a.heads, kv=a.kv, bytes=nbytes, buffers=nbuf, calls=calls,
                       runs=a.runs, splits=rule, page=PAGE, paths={})
            print("B=%d T=%d S=%d r_qk=%d r_vo=%d: K+V fp8 %.1f MB; %d caches each, %d calls x %d runs, %d splits"
                  % (B, T, S, r_qk, r_vo, nbytes / 1e6, nbuf, calls, a.runs, rule), flush=True)
            t_flat, t_paged = report(rec, ("decode kv8 contiguous", "decode paged8"), ([p[0] for p in pairs], [p[1] for p in pairs]), calls,
                                     (nbytes, nbytes))
            rec["paged_over_contiguous"] = round(t_paged / t_flat, 4)
            print("  paged time / contiguous time = %.3f" % (t_paged / t_flat), flush=True)
            if B == 16 and S == 2048:      # one decode step's append: K and V in one launch against the two launches it replaces
                kn, vn = rand(B, a.kv, 1, r_qk), rand(B, 1, a.kv, r_vo).transpose(1, 2)
                pos = torch.full((B,), S - 1, dtype=torch.int32, device=dev)

                def two(f):
                    def call():
                        ops.kv8_append(kn, f[0], f[1], S - 1)
                        ops.kv8_append(vn, f[2], f[3], S - 1)
                    return call
                fused = [(lambda p=p, t=t: ops.kv8_paged_append(kn, vn, p[:2], p[2:], t, pos)) for _, p, t in sets]
                moved = B * a.kv * ((r_qk + r_vo) * 2 + row)
                report(rec, ("kv8_append x 2, T=1", "kv8_paged_append, T=1"), ([two(f) for f, _, _ in sets], fused), max(calls, 32), (moved, moved))
            records.append(rec)
            del q, sets, pairs, out, ws
            torch.cuda.empty_cache()

    if a.ragged:
        B, lo, hi = (int(x) for x in a.ragged.split("x"))
        lens_host = [lo + (hi - lo) * b // (B - 1) // PAGE * PAGE for b in range(B)]
        for width in a.widths.split(","):
            r_qk, r_vo = (int(x) for x in width.split("x"))
            row = ops.kv8_pitch(r_qk) + ops.kv8_pitch(r_vo) + 8
            q = rand(B, a.heads, 1, r_qk)
            out = torch.empty(B, 1, a.heads, r_vo, dtype=q.dtype, device=dev)
            rule = ops.attn_decode_splits(B, a.kv, hi, dev)
            ws = torch.empty(lib.mdg_attn_decode_ws_bytes(B, 1, a.heads, r_vo, rule) // 4, dtype=torch.float32, device=dev)
            lens = torch.tensor(lens_host, dtype=torch.int32, device=dev)
            mask = (torch.arange(hi, device=dev)[None, :] < lens[:, None]).view(B, 1, 1, hi).contiguous()
            sets = [caches(B, hi, r_qk, r_vo) for _ in range(2)]
            pairs = [decode_fns(q, f, p, t, lens, B, 1, hi, r_qk, r_vo, rule, ws, out, mask) for f, p, t in sets]
            read_masked, read_paged = B * a.kv * hi * row + B * hi, sum(lens_host) * a.kv * row
            rec = dict(kind="ragged", B=B, T=1, lens=lens_host, r_qk=r_qk, r_vo=r_vo, heads=a.heads, kv=a.kv, splits=rule, page=PAGE,
                       runs=a.runs, paths={})
            print("ragged B=%d lengths %d .. %d r_qk=%d r_vo=%d, %d splits" % (B, lens_host[0], lens_host[-1], r_qk, r_vo, rule), flush=True)
            t_mask, t_paged = report(rec, ("decode kv8 masked S=%d" % hi, "decode paged8 seq_lens"), ([p[0] for p in pairs], [p[1] for p in pairs]),
                                     a.min_calls, (read_masked, read_paged))
            rec["paged_over_masked"] = round(t_paged / t_mask, 4)
            print("  paged time / masked time = %.3f (bytes read %.3f)" % (t_paged / t_mask, read_paged / read_masked), flush=True)
            records.append(rec)
            del sets, pairs
            torch.cuda.empty_cache()
    if a.json:
        write_json(a.json, dict(device=torch.cuda.get_device_name(0), n_cu=n_cu, torch=torch.__version__, copy_tbps=COPY_TBPS), records)


if __name__ == "__main__":
    main()
