"""Cost of what the mean-aware V/O truncation (MODEGPT_VO_INTERCEPT=1) adds at Llama-3-8B attention shapes, one GPU, HIP events:
20 back-to-back calls per run, 5 runs after a warm-up, the median reported beside every run.

  1. mdg_col_sum_accum on x, 32768 x 4096 bf16 (0.27 GB of algorithmic bytes: one read of x), per calibration batch and layer;
  2. mdg_cov_center at n = 4096 (1.5 n^2 8 bytes: the lower triangle read, both triangles written), once per layer;
  3. mdg_vo_intercept at d = 4096, 32 query / 8 kv heads of 128, rank 88, bf16 weights and bf16 stored factors: W_v + v^ + W_o + o^
     read once (~71 MB), once per layer.  The operands of one layer fit the Infinity Cache, so the call is timed twice: on ONE set
     of operands (what back-to-back calls on a warm cache see) and rotating over `--sets` sets whose total exceeds it (what a layer in
     a real run sees: its weights come from HBM).  The fraction of the achievable HBM bandwidth (6.3 TB/s) is stated for the second.

    python scripts/probes/vo_intercept_timing.py [--tokens 32768 --d 4096 --heads 32 --kv 8 --hd 128 --rank 88 --sets 6]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import ops  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s, a streaming copy on one MI355X


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


def report(name, ts, nbytes):
    med = sorted(ts)[len(ts) // 2]
    print(f"{name}: {' / '.join('%.1f' % t for t in ts)} us/call, median {med:.1f} us; {nbytes / 1e6:.1f} MB algorithmic -> "
          f"{nbytes / (med * 1e-6) / 1e9:.0f} GB/s = {100 * nbytes / (med * 1e-6) / HBM_ACHIEVABLE:.0f} % of the achievable HBM bandwidth")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--rank", type=int, default=88)
    ap.add_argument("--sets", type=int, default=6)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    d, nh, nkv, hd, r = a.d, a.heads, a.kv, a.hd, a.rank
    x = (torch.randn(a.tokens, d, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    s = torch.zeros(d, dtype=torch.float64, device=dev)
    report(f"col_sum_accum {a.tokens} x {d} bf16", timed(lambda: ops.col_sum_accum(s, x)), x.numel() * 2)
    ref = x.sum(0, dtype=torch.float64)
    s.zero_()
    ops.col_sum_accum(s, x)
    print(f"largest relative difference from x.sum(0, dtype=float64): {float(((s - ref).abs() / ref.abs()).max()):.2e}")
    C = torch.zeros(d, d, dtype=torch.float64, device=dev)
    ops.cov_accum_multi([(C, x, 1)])
    ops.cov_finalize(C, 1.0 / a.tokens)
    mu = s / a.tokens
    S = torch.empty_like(C)
    report(f"cov_center n = {d}", timed(lambda: ops.cov_center(C, mu, out=S)), 1.5 * d * d * 8)
    del x, S, C
    mk = lambda rows, cols: (torch.randn(rows, cols, device=dev, generator=g) * 0.02).to(torch.bfloat16)      # noqa: E731
    sets = [(mk(nkv * hd, d), mk(d, nh * hd), mk(nkv * r, d), mk(d, nh * r)) for _ in range(a.sets)]
    nbytes = sum(t.numel() * 2 for t in sets[0])
    turn = [0]

    def one():
        Wv, Wo, v, o = sets[0]
        ops.vo_intercept(Wv, Wo, v, o, mu, nh, nkv, hd, r)

    def rotating():
        Wv, Wo, v, o = sets[turn[0] % a.sets]
        turn[0] += 1
        ops.vo_intercept(Wv, Wo, v, o, mu, nh, nkv, hd, r)

    report(f"vo_intercept d = {d}, {nh}/{nkv} heads of {hd}, rank {r}, one operand set (warm cache)", timed(one), nbytes)
    report(f"vo_intercept, rotating over {a.sets} operand sets ({a.sets * nbytes / 1e6:.0f} MB)", timed(rotating, calls=4 * a.sets), nbytes)
    bias, bias64, norms = ops.vo_intercept(*sets[0], mu, nh, nkv, hd, r)
    Wv, Wo, v, o = (t.double() for t in sets[0])
    a1 = (Wv @ mu).reshape(nkv, hd).repeat_interleave(nh // nkv, 0).reshape(-1)
    a2 = (v @ mu).reshape(nkv, r).repeat_interleave(nh // nkv, 0).reshape(-1)
    want = Wo @ a1 - o @ a2
    print(f"largest difference from the torch fp64 expression, relative to the largest entry: "
          f"{float((bias64 - want).abs().max() / want.abs().max()):.2e}; norms {norms.tolist()}")


if __name__ == "__main__":
    main()
