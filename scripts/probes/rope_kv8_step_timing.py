"""ops.rope_kv8_step / ops.rope_kv8_paged_step (one launch) against the chain they replace on the same tensors -- ops.rope_gather (q) +
ops.rope_gather (k) + ops.kv8_append x 2, or + ops.kv8_paged_append -- in one process and ALTERNATING run by run.  Both sides go
through the ops wrappers and allocate their outputs as the forward does: at T = 1 the host time is the point.  HIP events around
back-to-back calls, a warm-up run, then the min / median / max of --runs runs.  32 query heads, 8 kv heads, head_dim 128, bf16, a
shuffled rotary mask; decode shapes (T = 1, a cache that already holds 2048 tokens) and a prefill shape (an empty cache), where the
fused call is timed without k_out (a chunk into a non-empty cache) and with it (the first chunk), beside the share of the copy
bandwidth its own bytes reach.

    python scripts/probes/rope_kv8_step_timing.py [--shapes 1x1,16x1,16x2048 --widths 90x77,128x128 --json out.json]

The shapes between 16 x 1 and 16 x 2048 locate the B * T up to which the fused call is the faster one: the bound the forward uses
(compressed_attention.KV_STEP_MAX_TOKENS)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import ops  # noqa: E402
from scripts.probes.attn_decode_paged8_timing import timed_pair  # noqa: E402
from scripts.probes.attn_decode_timing import COPY_TBPS, write_json  # noqa: E402

PAGE, HD, HELD = 64, 128, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x1,16x1,16x4,16x16,16x64,16x256,16x2048", help="BxT list (the middle ones locate the crossover)")
    ap.add_argument("--widths", default="90x77,128x128", help="r_qk x r_vo list")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rope_kv8_step_timing: no GPU")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11)
    rand = lambda *s: torch.randn(*s, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731
    print("device %s, torch %s; copy bandwidth taken as %.2f TB/s" % (torch.cuda.get_device_name(0), torch.__version__, COPY_TBPS))
    records = []
    for shape in a.shapes.split(","):
        B, T = (int(x) for x in shape.split("x"))
        pos = HELD if T == 1 else 0
        for width in a.widths.split(","):
            r_qk, r_vo = (int(x) for x in width.split("x"))
            q, k = rand(B, T, a.heads * r_qk), rand(B, T, a.kv * r_qk)
            v = rand(B, T, a.kv * r_vo).view(B, T, a.kv, r_vo).transpose(1, 2)
            ang = torch.rand(1, T, HD // 2, device=dev, generator=gen) * 6.28
            cos, sin = torch.cat((ang, ang), -1).cos().to(q.dtype), torch.cat((ang, ang), -1).sin().to(q.dtype)
            idx = torch.stack([torch.randperm(HD // 2, device=dev, generator=gen)[:r_qk // 2] for _ in range(a.kv)])
            mask = torch.cat((idx, idx + HD // 2), dim=1)
            cap = pos + T
            planes = [(torch.zeros(B, a.kv, cap, ops.kv8_pitch(r), dtype=torch.uint8, device=dev),
                       torch.zeros(B, a.kv, cap, device=dev)) for r in (r_qk, r_vo)]
            P = -(-cap // PAGE)
            pools = [(torch.zeros(B * P, a.kv, PAGE, ops.kv8_pitch(r), dtype=torch.uint8, device=dev),
                      torch.zeros(B * P, a.kv, PAGE, device=dev)) for r in (r_qk, r_vo)]
            table = torch.randperm(B * P, device=dev, generator=gen).to(torch.int32).view(B, P)
            dpos = torch.full((B,), pos, dtype=torch.int32, device=dev)
            rope = (cos, sin, mask)

            def chain(paged):
                qr = ops.rope_gather(q, *rope, a.heads, a.kv, HD)
                kr = ops.rope_gather(k, *rope, a.kv, a.kv, HD)
                if paged:
                    ops.kv8_paged_append(kr, v, pools[0], pools[1], table, dpos)
                else:
                    ops.kv8_append(kr, *planes[0], pos)
                    ops.kv8_append(v, *planes[1], pos)
                return qr

            def fused(paged, k_out=None):
                if paged:
                    return ops.rope_kv8_paged_step(q, k, v, *rope, a.heads, a.kv, HD, pools[0], pools[1], table, dpos, k_out=k_out)
                return ops.rope_kv8_step(q, k, v, *rope, a.heads, a.kv, HD, planes[0], planes[1], pos, k_out=k_out)

            moved = B * T * ((2 * a.heads * r_qk + a.kv * (r_qk + r_vo)) * 2 + a.kv * (ops.kv8_pitch(r_qk) + ops.kv8_pitch(r_vo) + 8))
            calls = max(8, min(200, 65536 // (B * T)))
            for paged in (False, True):
                layout = "paged" if paged else "planes"
                sides = [("chain", lambda p=paged: chain(p), moved + 2 * B * T * a.kv * r_qk * 2),
                         ("fused", lambda p=paged: fused(p), moved)]
                if T > 1:
                    sides.append(("fused + k_out", lambda p=paged: fused(p, True), moved + B * T * a.kv * r_qk * 2))
                assert torch.equal(sides[0][1](), sides[1][1]()[0])                     # the two sides give the same q
                rec = dict(B=B, T=T, r_qk=r_qk, r_vo=r_vo, heads=a.heads, kv=a.kv, layout=layout, pos=pos, calls=calls, runs=a.runs, paths={})
                print("B=%d T=%d r_qk=%d r_vo=%d %s: %d calls x %d runs" % (B, T, r_qk, r_vo, layout, calls, a.runs), flush=True)
                times = timed_pair([[fn] for _, fn, _ in sides], calls, a.runs)
                for (name, _, nb), ts in zip(sides, times):
                    e = dict(us_min=round(min(ts) * 1e3, 2), us_median=round(statistics.median(ts) * 1e3, 2), us_max=round(max(ts) * 1e3, 2),
                             mb=round(nb / 1e6, 3), of_copy=round(nb / (min(ts) * 1e-3) / 1e12 / COPY_TBPS, 4))
                    rec["paths"][name] = e
                    print("  %-14s %9.1f us min / %9.1f med / %9.1f max   %9.3f MB  (%4.1f %% of copy)"
                          % (name, e["us_min"], e["us_median"], e["us_max"], e["mb"], 100 * e["of_copy"]), flush=True)
                rec["fused_over_chain"] = round(min(times[1]) / min(times[0]), 4)
                print("  fused time / chain time = %.3f" % rec["fused_over_chain"], flush=True)
                records.append(rec)
            del q, k, v, planes, pools
            torch.cuda.empty_cache()
    if a.json:
        write_json(a.json, dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, copy_tbps=COPY_TBPS), records)


if __name__ == "__main__":
    main()
