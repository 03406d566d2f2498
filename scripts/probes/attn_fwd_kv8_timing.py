"""mdg_attn_fwd_kv8 (multi-token attention straight from the fp8 cache) against what it replaces on the same commit -- mdg_kv8_dequant
of K and of V into fresh bf16 tensors, then mdg_attn_fwd on them -- in the same process, alternating, with mdg_attn_fwd alone on
already dequantised tensors beside them.  All three through modegpt_amd.ops, as the attention forward calls them.  The COLD protocol
and the min / median / max of attn_decode_timing.py: calls rotate over enough distinct caches that their total exceeds --cold-mib, so
no call finds its cache in the 256 MiB Infinity Cache.  32 query heads, 8 kv heads, bf16 q, causal chunks of T queries at the end of
S keys.  Per side also the peak device memory a call takes beyond its operands and its output.

    python scripts/probes/attn_fwd_kv8_timing.py [--shapes 1x512x8192,... --widths 90x77,... --json out.json]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import ops  # noqa: E402
from scripts.probes.attn_decode_timing import timed, write_json  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%dx%d" % (B, T, S) for B in (1, 16) for S in (8192, 32768) for T in (512, 2048)),
                    help="BxTxS list")
    ap.add_argument("--widths", default="90x77,90x90,128x128", help="r_qk x r_vo list")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-calls", type=int, default=4)
    ap.add_argument("--cold-mib", type=float, default=320.0, help="total fp8 cache bytes a rotation must exceed (Infinity Cache: 256)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_fwd_kv8_timing: no GPU")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    records = []
    print("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for shape in a.shapes.split(","):
        B, T, S = (int(x) for x in shape.split("x"))
        for width in a.widths.split(","):
            r_qk, r_vo = (int(x) for x in width.split("x"))
            rand = lambda *s: torch.randn(*s, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731
            pk, pv = ops.kv8_pitch(r_qk), ops.kv8_pitch(r_vo)
            bytes16 = B * a.kv * S * (r_qk + r_vo) * 2
            bytes8 = B * a.kv * S * (pk + pv + 8)
            nbuf = max(2, int(a.cold_mib * 2 ** 20 // bytes8) + 1)
            calls = max(a.min_calls, nbuf)
            q = rand(B, a.heads, T, r_qk)
            scale = float(r_qk) ** -0.5
            out = torch.empty(B, T, a.heads, r_vo, dtype=q.dtype, device=dev)
            sets8, sets16 = [], []
            for _ in range(nbuf):
                planes = []
                for r, p in ((r_qk, pk), (r_vo, pv)):
                    data = torch.empty(B, a.kv, S, p, dtype=torch.uint8, device=dev)
                    sc = torch.empty(B, a.kv, S, dtype=torch.float32, device=dev)
                    ops.kv8_append(rand(B, a.kv, S, r), data, sc, 0)
                    planes += [data, sc]
                sets8.append(tuple(planes))
                sets16.append((ops.kv8_dequant(planes[0], planes[1], S, r_qk), ops.kv8_dequant(planes[2], planes[3], S, r_vo)))
            rec = dict(B=B, T=T, S=S, r_qk=r_qk, r_vo=r_vo, heads=a.heads, kv=a.kv, bytes_bf16=bytes16, bytes_fp8=bytes8, buffers=nbuf,
                       calls=calls, runs=a.runs, paths={})
            print("B=%d T=%d S=%d r_qk=%d r_vo=%d: K+V fp8 %.1f MB, bf16 %.1f MB; %d caches, %d calls x %d runs"
                  % (B, T, S, r_qk, r_vo, bytes8 / 1e6, bytes16 / 1e6, nbuf, calls, a.runs), flush=True)

            def fp8_fn(kd, ks, vd, vs):
                return lambda: ops.attn_fwd_kv8(q, kd, ks, vd, vs, S, r_vo, scale, out=out)

            def both_fn(kd, ks, vd, vs):
                return lambda: ops.attn_fwd(q, ops.kv8_dequant(kd, ks, S, r_qk), ops.kv8_dequant(vd, vs, S, r_vo), scale, out=out)

            def fwd_fn(k, v):
                return lambda: ops.attn_fwd(q, k, v, scale, out=out)

            sides = {"fwd_kv8": [fp8_fn(*s) for s in sets8], "dequant + fwd": [both_fn(*s) for s in sets8],
                     "fwd alone": [fwd_fn(*s) for s in sets16]}
            times = {name: [] for name in sides}
            for name, fns in sides.items():                       # peak memory of one call beyond what is allocated around it
                fns[0]()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                fns[0]()
                torch.cuda.synchronize()
                rec["paths"][name] = dict(extra_mb=round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 2))
            for _ in range(a.runs):                               # the sides alternate, one cold rotation each (timed: one warm-up run first)
                for name, fns in sides.items():
                    times[name] += timed(fns, calls, 1)
            for name, ts in times.items():
                e = rec["paths"][name]
                e.update(us_min=round(min(ts) * 1e3, 1), us_median=round(statistics.median(ts) * 1e3, 1), us_max=round(max(ts) * 1e3, 1))
                print("  %-14s cold %10.1f us min / %10.1f med / %10.1f max   extra memory %8.2f MB"
                      % (name, e["us_min"], e["us_median"], e["us_max"], e["extra_mb"]), flush=True)
            rec["kv8_over_replaced_min"] = round(min(times["fwd_kv8"]) / min(times["dequant + fwd"]), 4)
            rec["kv8_over_replaced_median"] = round(statistics.median(times["fwd_kv8"]) / statistics.median(times["dequant + fwd"]), 4)
            print("  fwd_kv8 / (dequant + fwd): %.3f of the minima, %.3f of the medians" % (rec["kv8_over_replaced_min"],
                                                                                         rec["kv8_over_replaced_median"]), flush=True)
            records.append(rec)
            del q, sets8, sets16, out, sides
            torch.cuda.empty_cache()
    if a.json:
        write_json(a.json, dict(device=torch.cuda.get_device_name(0), torch=torch.__version__), records)


if __name__ == "__main__":
    main()
