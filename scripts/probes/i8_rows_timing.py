"""Whole-call time of ops.cov_accum_i8 at the sigma_mlp shape (32768 x 14336, bf16) with and without the rows option (MDG_I8_ROWS),
on SiLU-gated activations and on the same activations with 16 token rows scaled by 2^6.  HIP events around the whole call (split,
route, lists, products, remainder, column / row / fallback kernels), the four cases interleaved round by round so that clock and
thermal drift hit them alike; median and range over the rounds after warm-up.  Prints one JSON line.

    python scripts/probes/i8_rows_timing.py [--tokens 32768] [--features 14336] [--rounds 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from modegpt_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--features", type=int, default=14336)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    T, n = a.tokens, a.features
    plain = torch.empty(T, n, dtype=torch.bfloat16, device=dev)
    for t0 in range(0, T, 4096):         # (in slabs: the fp32 temporaries of the whole matrix are 2 x 1.9 GB)
        g = torch.randn(min(4096, T - t0), n, device=dev, generator=gen)
        u = torch.randn(min(4096, T - t0), n, device=dev, generator=gen)
        plain[t0:t0 + g.shape[0]] = (torch.nn.functional.silu(g) * u).to(torch.bfloat16)
    rows = [int(r) for r in torch.linspace(5, T - 7, 16).long().tolist()]
    outl = plain.clone()
    outl[rows] = (outl[rows].float() * 2.0 ** 6).to(torch.bfloat16)
    sigma = torch.zeros(n, n, dtype=torch.float64, device=dev)
    cases = [("silu_off", plain, False), ("silu_on", plain, True), ("silu_16rows_off", outl, False), ("silu_16rows_on", outl, True)]
    routes, times = {}, {name: [] for name, _, _ in cases}
    for name, x, flag in cases:          # the route of each case, once (a reporting call synchronises; the timed calls do not)
        info = {}
        sigma.zero_()
        planes = ops.cov_accum_i8(sigma, x, route_info=info, rows=flag)
        routes[name] = {"planes": planes, "exact": info["exact"], "columns": len(info["columns"]), "rows": len(info.get("rows", []))}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in cases]
    for rnd in range(a.warmup + a.rounds):
        order = list(range(len(cases)))
        if rnd % 2:
            order.reverse()              # alternate the order
        for i in order:
            name, x, flag = cases[i]
            ev[i][0].record()
            ops.cov_accum_i8(sigma, x, report=False, rows=flag)
            ev[i][1].record()
        torch.cuda.synchronize()
        if rnd >= a.warmup:
            for i, (name, _, _) in enumerate(cases):
                times[name].append(ev[i][0].elapsed_time(ev[i][1]))
    out = {"tokens": T, "features": n, "rounds": a.rounds, "routes": routes,
           "ms": {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
