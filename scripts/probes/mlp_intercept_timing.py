"""Cost of the three kernels of the mean-aware MLP refit (MODEGPT_MLP_INTERCEPT=1) at Llama-3-8B shapes, one GPU, HIP events:
20 back-to-back calls per run, 5 runs after a warm-up.

  1. mdg_col_sum_accum on 32768 x 14336 bf16 (0.94 GB of algorithmic bytes), beside what a user without the kernel would write,
     x.sum(0, dtype=torch.float64), on the same tensor in the same process, and beside the sigma_mlp call it rides on;
  2. mdg_cov_center at n = 14336 (1.5 n^2 8 bytes: the lower triangle read, both written);
  3. mdg_nystrom_intercept at d = 4096, n = 14336, r = 10035 (one read of W_d and of the stored down projection).

    python scripts/probes/mlp_intercept_timing.py [--tokens 32768 --n 14336 --d 4096 --r 10035]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import ops  # noqa: E402


def timed(fn, calls=20, runs=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)      # microseconds per call
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--n", type=int, default=14336)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--r", type=int, default=10035)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    fmt = lambda ts: " / ".join("%.1f" % t for t in ts)          # noqa: E731
    g = torch.Generator(device=dev).manual_seed(1)
    x = (torch.randn(a.tokens, a.n, device=dev, generator=g).abs() * 0.5).to(torch.bfloat16)
    s = torch.zeros(a.n, dtype=torch.float64, device=dev)
    gb = x.numel() * 2 / 1e9
    t_k = timed(lambda: ops.col_sum_accum(s, x))
    t_t = timed(lambda: x.sum(0, dtype=torch.float64))
    print(f"col_sum_accum {a.tokens} x {a.n} bf16: {fmt(t_k)} us/call -> {gb / (min(t_k) * 1e-6):.0f} GB/s at best, median {sorted(t_k)[2]:.1f} us")
    print(f"x.sum(0, dtype=float64)          : {fmt(t_t)} us/call -> {gb / (min(t_t) * 1e-6):.0f} GB/s at best, median {sorted(t_t)[2]:.1f} us")
    ref = x.sum(0, dtype=torch.float64)
    s.zero_()
    ops.col_sum_accum(s, x)
    print(f"largest relative difference of the two sums: {float(((s - ref).abs() / ref.abs()).max()):.2e}")
    C = torch.zeros(a.n, a.n, dtype=torch.float64, device=dev)
    t_c = timed(lambda: ops.cov_accum_multi([(C, x, 1)]), calls=3, runs=3)
    print(f"sigma_mlp call (ops.cov_accum_multi, mode {ops.COV_MODE}): {fmt(t_c)} us/call; the column sums add {100 * sorted(t_k)[2] / sorted(t_c)[1]:.1f} % to it")
    ops.cov_finalize(C, 1.0 / a.tokens)
    mu = s / a.tokens
    S = torch.empty_like(C)
    t_s = timed(lambda: ops.cov_center(C, mu, out=S))
    print(f"cov_center n = {a.n}: {fmt(t_s)} us/call -> {1.5 * a.n * a.n * 8 / 1e9 / (min(t_s) * 1e-6):.0f} GB/s at best")
    del C, S, x
    W = (torch.randn(a.d, a.n, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    D = (torch.randn(a.d, a.r, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    idx = torch.sort(torch.randperm(a.n, device=dev, generator=g)[:a.r]).values
    t_i = timed(lambda: ops.nystrom_intercept(W, D, idx, mu))
    print(f"nystrom_intercept d = {a.d}, n = {a.n}, r = {a.r}: {fmt(t_i)} us/call -> {(W.numel() + D.numel()) * 2 / 1e9 / (min(t_i) * 1e-6):.0f} GB/s at best")


if __name__ == "__main__":
    main()
