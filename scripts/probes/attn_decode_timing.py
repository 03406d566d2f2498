"""mdg_attn_decode (MODEGPT_FUSED_ATTN_DECODE=1) at decode shapes of a compressed Llama-3-8B, one GPU: 32 query heads, 8 kv heads,
bf16, causal, T = 1 (and T = 4) against a cache of S keys.  Decode is memory-bound -- K and V are each read once -- so the figure is
K+V bytes per second, against the 6.29 TB/s copy figure of the MI355X.

Per shape, on the same tensors:
  decode(rule)   mdg_attn_decode with mdg_attn_decode_splits for this device
  decode(s)      the same swept over splits 1, 2, 4, ... up to min(ceil(S / 64), 256)
  fwd            mdg_attn_fwd: unchanged code, the decode path before the split-key kernel
  sdpa           transformers' sdpa_attention_forward, no mask, as the compressed forward calls it with the switches off (is_causal
                 left to HF: off at T = 1; at T > 1 HF asks torch for the top-left aligned mask, which is another product than
                 the cache-aligned one -- the T = 4 row times it all the same and prints the difference); repeated under
                 torch.nn.attention.sdpa_kernel restricted to one back end at a time to NAME the one that served

COLD and WARM.  A 1 x 8192 cache is about 22 MB and stays in the 256 MiB Infinity Cache between back-to-back calls, which a decoding
model (32 layers, each with its own cache) never sees.  COLD rotates the calls over enough distinct k / v buffers that their total
exceeds --cold-mib, so every call reads a cache the previous ones have pushed out; WARM repeats one buffer and is labelled as such.
Both kernels are called through the C entry with a preallocated workspace and output, so the host adds one ctypes call per launch
sequence; sdpa is called as the forward calls it.  HIP events around `calls` back-to-back calls, `--runs` repeats after a warm-up
run; minimum and median per call.  A time of a few microseconds is a launch time, not a bandwidth: the table says so by its GB/s.

    python scripts/probes/attn_decode_timing.py [--shapes 1x1x2048,... --widths 90x77,90x90,128x128 --json out.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import _lib, ops  # noqa: E402

COPY_TBPS = 6.29                # MI355X measured HBM copy bandwidth (read + write streams), TB/s


def timed(fns, calls, runs):
    """ms per call, `runs` times: call i of a run is fns[i % len(fns)] (the rotation over the buffers)."""
    out = []
    n = len(fns)
    for run in range(runs + 1):                                   # (run 0 warms up)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(calls):
            fns[i % n]()
        b.record()
        b.synchronize()
        if run:
            out.append(a.elapsed_time(b) / calls)
    return out


def write_json(path, head, records):
    """One line per shape: a record holds some thirty timings, and an indented dump runs to thousands of lines."""
    with open(path, "w") as f:
        f.write("{" + json.dumps(head)[1:-1] + ', "records": [\n')
        f.write(",\n".join(json.dumps(r) for r in records))
        f.write("\n]}\n")


class _Module(torch.nn.Module):
    """What HF's attention functions read from the attention module."""

    def __init__(self, groups):
        super().__init__()
        self.num_key_value_groups, self.is_causal = groups, True
        self.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x1x2048,1x1x8192,1x1x32768,16x1x2048,16x1x8192,16x1x32768,1x4x8192", help="BxTxS list")
    ap.add_argument("--widths", default="90x77,90x90,128x128", help="r_qk x r_vo list")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-calls", type=int, default=8)
    ap.add_argument("--cold-mib", type=float, default=320.0, help="total k + v bytes the cold rotation must exceed (Infinity Cache: 256)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_decode_timing: no GPU")
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    gen = torch.Generator(device=dev).manual_seed(5)
    mod = _Module(a.heads // a.kv)
    backends = {"flash": SDPBackend.FLASH_ATTENTION, "efficient": SDPBackend.EFFICIENT_ATTENTION, "math": SDPBackend.MATH}
    stream = torch.cuda.current_stream(dev).cuda_stream
    records = []
    print("device %s, %d CUs, torch %s; copy bandwidth taken as %.2f TB/s" % (torch.cuda.get_device_name(0), n_cu, torch.__version__,
                                                                            COPY_TBPS))
    for shape in a.shapes.split(","):
        B, T, S = (int(x) for x in shape.split("x"))
        for width in a.widths.split(","):
            r_qk, r_vo = (int(x) for x in width.split("x"))
            rand = lambda *s: torch.randn(*s, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731
            kv_bytes = B * a.kv * S * (r_qk + r_vo) * 2
            nbuf = max(2, int(a.cold_mib * 2 ** 20 // kv_bytes) + 1)
            calls = max(a.min_calls, nbuf)
            q = rand(B, a.heads, T, r_qk)
            sets = [(rand(B, a.kv, S, r_qk), rand(B, a.kv, S, r_vo)) for _ in range(nbuf)]
            scale = float(r_qk) ** -0.5
            out = torch.empty(B, T, a.heads, r_vo, dtype=q.dtype, device=dev)
            rule = ops.attn_decode_splits(B, a.kv, S, dev)
            cap = min(-(-S // 64), 256)
            sweep = [s for s in (1, 2, 4, 8, 16, 32, 64, 128, 256) if s <= cap]
            ws = torch.empty(lib.mdg_attn_decode_ws_bytes(B, T, a.heads, r_vo, max(sweep + [rule])) // 4, dtype=torch.float32, device=dev)
            rec = dict(B=B, T=T, S=S, r_qk=r_qk, r_vo=r_vo, heads=a.heads, kv=a.kv, kv_bytes=kv_bytes, buffers=nbuf, calls=calls,
                       runs=a.runs, rule_splits=rule, paths={})
            print("B=%d T=%d S=%d heads=%d kv=%d r_qk=%d r_vo=%d bf16 causal: K+V %.1f MB, %d buffers (%.0f MiB), %d calls x %d runs, "
                  "rule: %d splits" % (B, T, S, a.heads, a.kv, r_qk, r_vo, kv_bytes / 1e6, nbuf, nbuf * kv_bytes / 2 ** 20, calls,
                                       a.runs, rule), flush=True)

            def decode_fn(k, v, splits):
                args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.MDG_BF16, B, T, S, a.heads, a.kv, r_qk, r_vo, k.stride(0),
                        k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), scale, 1, splits, ws.data_ptr(),
                        ws.numel() * 4, out.data_ptr(), a.heads * r_vo, stream)
                return lambda: lib.mdg_attn_decode(*args)

            def fwd_fn(k, v):
                args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.MDG_BF16, B, T, S, a.heads, a.kv, r_qk, r_vo, k.stride(0),
                        k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), scale, 1, out.data_ptr(), a.heads * r_vo,
                        stream)
                return lambda: lib.mdg_attn_fwd(*args)

            def sdpa_fn(k, v, be=None):
                def call():
                    return sdpa_attention_forward(mod, q, k, v, None, dropout=0.0, scaling=scale)
                if be is None:
                    return call

                def only():
                    with sdpa_kernel([be]):
                        return call()
                return only

            def put(name, make):
                """cold: the rotation over every buffer set; warm: buffer set 0 alone."""
                entry = {}
                for label, fns in (("cold", [make(k, v) for k, v in sets]), ("warm", [make(*sets[0])])):
                    try:
                        rc = fns[0]()
                        torch.cuda.synchronize()
                        if isinstance(rc, int) and rc != 0:
                            raise RuntimeError(_lib.last_error())
                        times = timed(fns, calls, a.runs)
                    except (RuntimeError, torch.OutOfMemoryError) as exc:
                        entry[label] = dict(refused=str(exc).splitlines()[0][:160])
                        continue
                    best, med, worst = min(times), statistics.median(times), max(times)
                    entry[label] = dict(us_min=round(best * 1e3, 2), us_median=round(med * 1e3, 2), us_max=round(worst * 1e3, 2),
                                        gbps=round(kv_bytes / (best * 1e-3) / 1e9, 1),
                                        of_copy=round(kv_bytes / (best * 1e-3) / 1e12 / COPY_TBPS, 4))
                rec["paths"][name] = entry
                cells = []
                for label in ("cold", "warm"):
                    e = entry[label]
                    cells.append("%s refused: %s" % (label, e["refused"]) if "refused" in e else
                                 "%s %9.1f us min / %9.1f med / %9.1f max  %7.0f GB/s (%4.1f %% of copy)"
                                 % (label, e["us_min"], e["us_median"], e["us_max"], e["gbps"], 100 * e["of_copy"]))
                print("  %-14s %s" % (name, "   |   ".join(cells)), flush=True)

            put("decode(rule=%d)" % rule, lambda k, v: decode_fn(k, v, rule))
            for s in sweep:
                put("decode(%d)" % s, lambda k, v, s=s: decode_fn(k, v, s))
            put("fwd", fwd_fn)
            ref = out.clone()
            decode_fn(*sets[0], rule)()                              # out: the decode kernel on buffer set 0 again
            torch.cuda.synchronize()
            with torch.no_grad():
                put("sdpa", sdpa_fn)
                err = float("nan")
                if "us_min" in rec["paths"]["sdpa"]["warm"]:
                    err = float((sdpa_fn(*sets[0])()[0].float() - out.float()).abs().max())
                for name, be in backends.items():
                    put("sdpa:" + name, lambda k, v, be=be: sdpa_fn(k, v, be))
            rec["max_abs_diff_decode_vs_sdpa"] = err
            rec["max_abs_diff_decode_vs_fwd"] = float((ref.float() - out.float()).abs().max())   # ref: fwd on buffer set 0 (its warm run)
            accepted = [n for n in backends if "us_min" in rec["paths"]["sdpa:" + n]["cold"]]
            chosen = None
            if "us_min" in rec["paths"]["sdpa"]["cold"] and accepted:
                chosen = min(accepted, key=lambda n: abs(rec["paths"]["sdpa:" + n]["cold"]["us_min"] - rec["paths"]["sdpa"]["cold"]["us_min"]))
            rec["sdpa_backends_accepting"], rec["sdpa_backend_closest_to_unrestricted"] = accepted, chosen
            print("  sdpa back ends that accept the shape: %s; the unrestricted call's time matches: %s; max |decode - sdpa| = %.3e, "
                  "max |decode - fwd| = %.3e" % (accepted, chosen, err, rec["max_abs_diff_decode_vs_fwd"]), flush=True)
            records.append(rec)
            del q, sets, out, ws, ref
            torch.cuda.empty_cache()
    if a.json:
        write_json(a.json, dict(device=torch.cuda.get_device_name(0), n_cu=n_cu, torch=torch.__version__, copy_tbps=COPY_TBPS), records)


if __name__ == "__main__":
    main()
