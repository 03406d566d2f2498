"""Cost of the greedy MLP selection (mdg_nystrom_greedy_select) at Llama-3-8B shapes, one GPU:

  1. the call alone for rounds in {8, 32, 128}: HIP events around 5 calls after a warm-up, inside an ops.DeferredStatus (no host
     round trip), median;
  2. the yardstick, in the same process: the flops the call executes, counted from its own GEMM shapes, at the rate ops.gemm reaches
     on one n x n x ceil(r / rounds) update and one d x n x ceil(r / rounds) update (beta = 1, as the call runs them);
  3. what the call replaces when the rank curve is off: ops.ridge_scores + ops.select_smallest_sorted;
  4. the workspace, and objective_over_total / greedy_over_ridge on this synthetic layer (two rank curves per setting).

    python scripts/probes/greedy_timing.py [--n 14336 --d 4096 --keep 0.7 --tokens 32768 --rounds 8 32 128 --runs 5]

Inputs: SiLU-gated activations silu(g) * u in bf16 (the generator of bench.py's value_gated leg), bf16 N(0, 0.02^2) weights."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import engine, ops  # noqa: E402


def timed(fn, runs):
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out, res


def call_flops(n, d, r, rounds):
    """The flops of one call from its GEMM shapes: B = W M, then per round the panel (2 m n |S|), the factorisation and the
    triangular inverse (m^3 / 3 each), Ynew = L^-1 Pt (m^2 n, triangular), Gt = L^-1 B[:, P]^T (m^2 d) and B -= Gt^T Ynew (2 d n m)."""
    total, off = 2.0 * d * n * n, 0
    for m in ops.greedy_partition(r, rounds):
        total += 2.0 * m * n * off + 2.0 * m ** 3 / 3 + m * m * n + m * m * d + 2.0 * d * n * m
        off += m
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=14336)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--keep", type=float, default=0.7)
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--rounds", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = dict(engine.SHAPES["llama-3-8b"], d=a.d, d_ff=a.n)
    n, d, r = a.n, a.d, int(a.n * a.keep)
    fmt = lambda ts: " / ".join("%.2f" % t for t in ts)          # noqa: E731
    lib = ops._lib.load()

    C = torch.zeros(n, n, dtype=torch.float64, device=dev)
    step = 8192
    for t0 in range(0, a.tokens, step):
        gen = torch.Generator(device=dev).manual_seed(4242 + t0)
        rows = min(step, a.tokens - t0)
        h = torch.nn.functional.silu(torch.randn(rows, n, generator=gen, device=dev, dtype=torch.float32))
        h.mul_(torch.randn(rows, n, generator=gen, device=dev, dtype=torch.float32))
        ops.cov_accum(C, h.to(torch.bfloat16))
        del h
    ops.cov_finalize(C, 1.0 / a.tokens)
    W = engine.make_layer_weights(shape, 1234, dev)["down"]

    # 3. the pair the call replaces
    ops.select_smallest_sorted(ops.ridge_scores(C, 1e-4), r)
    with ops.DeferredStatus(dev) as st:
        tr, scores = timed(lambda: ops.ridge_scores(C, 1e-4), a.runs)
        ts, idx = timed(lambda: ops.select_smallest_sorted(scores, r), a.runs)
    st.check()
    ridge_ms = statistics.median(tr) + statistics.median(ts)
    print("RIDGE PAIR n=%d r=%d: ridge_scores %s ms + select %s ms -> median %.2f ms" % (n, r, fmt(tr), fmt(ts), ridge_ms))
    ridge_order = torch.argsort(scores, stable=True)
    with ops.DeferredStatus(dev) as st:
        ridge_at_rank = float(ops.nystrom_rank_curve(C, ridge_order, W, eps=1e-6)[r])
    st.check()

    for rounds in a.rounds:
        m = -(-r // rounds)
        ws = lib.mdg_nystrom_greedy_ws_bytes(n, d, r, rounds)
        with ops.DeferredStatus(dev) as st:
            ops.nystrom_greedy_select(C, W, r, rounds)               # (warm-up)
            tc, out = timed(lambda: ops.nystrom_greedy_select(C, W, r, rounds), a.runs)
        st.check()
        call_ms = statistics.median(tc)
        # 2. the yardstick: the two updates at this round size, beta = 1
        X = torch.randn(n, m, dtype=torch.float64, device=dev)
        Y = torch.randn(m, n, dtype=torch.float64, device=dev)
        G = torch.randn(d, m, dtype=torch.float64, device=dev)
        Rn = torch.zeros(n, n, dtype=torch.float64, device=dev)
        Bn = torch.zeros(d, n, dtype=torch.float64, device=dev)
        ops.gemm(X, Y, Rn, alpha=-1.0, beta=1.0)
        ops.gemm(G, Y, Bn, alpha=-1.0, beta=1.0)
        t1, _ = timed(lambda: ops.gemm(X, Y, Rn, alpha=-1.0, beta=1.0), a.runs)
        t2, _ = timed(lambda: ops.gemm(G, Y, Bn, alpha=-1.0, beta=1.0), a.runs)
        del X, Y, G, Rn, Bn
        gemm_ms = statistics.median(t1) + statistics.median(t2)
        gemm_flops = 2.0 * n * n * m + 2.0 * d * n * m
        flops = call_flops(n, d, r, rounds)
        yard_ms = gemm_ms * flops / gemm_flops
        order, objective, cut, n_dead = out
        obj = objective.cpu().tolist()
        unselected = torch.ones(n, dtype=torch.int64, device=dev)
        unselected[order] = 0
        rest = ridge_order[torch.argsort(unselected[ridge_order], stable=True)][r:]
        with ops.DeferredStatus(dev) as st:
            greedy_at_rank = float(ops.nystrom_rank_curve(C, torch.cat((order, rest)), W, eps=1e-6)[r])
        st.check()
        rep = ops.decode_mlp_greedy(obj, cut.cpu().tolist(), int(n_dead.cpu()), r, ridge_at_rank=ridge_at_rank, greedy_at_rank=greedy_at_rank)
        print("CALL rounds=%d m=%d: %s ms -> median %.2f ms; %.3f TFLOP -> %.1f TF; yardstick %.2f ms (gemm pair %.2f ms at %.1f TF); "
              "call / yardstick %.2f; call - ridge pair %+.2f ms; workspace %.2f GB" % (
                  rounds, m, fmt(tc), call_ms, flops / 1e12, flops / call_ms / 1e9, yard_ms, gemm_ms, gemm_flops / gemm_ms / 1e9,
                  call_ms / yard_ms, call_ms - ridge_ms, ws / 1e9))
        print("RESULT " + json.dumps({"rounds": rounds, "call_ms": call_ms, "yardstick_ms": yard_ms, "ratio": call_ms / yard_ms,
                                      "ridge_pair_ms": ridge_ms, "workspace_bytes": ws, "tflop": flops / 1e12,
                                      "objective_over_total": rep["objective_over_total"], "greedy_over_ridge": rep["greedy_over_ridge"],
                                      "dead_picks": rep["dead_picks"], "min_cut_gap": rep["min_cut_gap"]}))
        del out, order, objective, cut, n_dead


if __name__ == "__main__":
    main()
