"""Cost of the Q/K logit error (mdg_qk_rank_curve) at Llama-3-8B shapes, one GPU: HIP events around `--calls` back-to-back calls
(the kernel is tens of microseconds: one call is below what an event pair resolves), repeated `--runs` times after a warm-up, for

  1. the curve call alone, with and without the greedy outputs,
  2. the extra scoring call at rank = hd that gives the order (mdg_qk_select),
  3. what compress_qk adds per layer with MODEGPT_QK_ERROR=1: 2. + 1. with the greedy outputs.

    python scripts/probes/qk_error_timing.py [--heads 32 --kv 8 --hd 128 --tokens 1024 --calls 200 --runs 5]

Inputs: sigma = X^T X / T of Gaussian columns mixed by I + 0.3 N, scales over four decades (tests/qk_error_model.py)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import _lib, ops  # noqa: E402


def sigma(n, hd, T, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn(n, T, hd, generator=g, dtype=torch.float64) @ (torch.eye(hd, dtype=torch.float64) +
                                                                    0.3 * torch.randn(n, hd, hd, generator=g, dtype=torch.float64))
    X = X * 10.0 ** (4.0 * torch.rand(n, 1, hd, generator=g, dtype=torch.float64) - 2.0)
    return (X.transpose(1, 2) @ X / T).to(dev)


def timed(fn, calls, runs):
    out = []
    for run in range(runs + 1):                                   # (run 0 warms up)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        if run:
            out.append(a.elapsed_time(b) * 1e3 / calls)           # microseconds per call
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qk_error_timing: no GPU")
    dev = torch.device("cuda:0")
    mode = _lib.MDG_QK_ROPE_GROUPED if a.heads != a.kv else _lib.MDG_QK_ROPE_MHA
    cq, ck = sigma(a.heads, a.hd, a.tokens, 1, dev), sigma(a.kv, a.hd, a.tokens, 2, dev)
    ns = a.hd // 2
    select = lambda: ops.qk_select(cq, ck, a.hd, mode, 1e-4, 1e-2)[0][:, :ns].contiguous()         # noqa: E731
    order = select()
    fmt = lambda ts: " / ".join("%.1f" % t for t in ts)                                            # noqa: E731
    t_plain = timed(lambda: ops.qk_rank_curve(cq, ck, mode, 0.0, 0.0, order, want_greedy=False, terms_ridges=(1e-4, 1e-2)), a.calls, a.runs)
    t_greedy = timed(lambda: ops.qk_rank_curve(cq, ck, mode, 0.0, 0.0, order, terms_ridges=(1e-4, 1e-2)), a.calls, a.runs)
    t_select = timed(select, a.calls, a.runs)
    t_both = timed(lambda: ops.qk_rank_curve(cq, ck, mode, 0.0, 0.0, select(), terms_ridges=(1e-4, 1e-2)), a.calls, a.runs)
    print("CALLS %d/%d hd=%d, microseconds per call over %d back-to-back calls, %d runs: curve %s; curve + greedy %s; order (qk_select at "
          "rank hd + slice) %s; per layer with the switch set (order + curve + greedy) %s" % (
              a.heads, a.kv, a.hd, a.calls, a.runs, fmt(t_plain), fmt(t_greedy), fmt(t_select), fmt(t_both)))
    out = ops.qk_rank_curve(cq, ck, mode, 0.0, 0.0, order, terms_ridges=(1e-4, 1e-2))
    m = ops.decode_qk_logit_error(out[0].cpu(), out[1].cpu(), 88, 2, terms=out[2].cpu(), scale=out[3].cpu(), greedy_curve=out[4].cpu())
    print("VALUES at rank 88:", {k: m[k] for k in m if k != "heads"})


if __name__ == "__main__":
    main()
