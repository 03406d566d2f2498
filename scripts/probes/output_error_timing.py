"""Cost of the realised MLP output error (mdg_mlp_output_error) at Llama-3-8B shapes, one GPU:

  1. the kernel alone, HIP events: one e call (the bf16 artefact subtracted, unorm2 requested) and one q call, 4 runs each;
  2. the same numbers by the route the tree offered before: a torch scatter that builds U in fp64, ops.gemm(U, C_full), a torch row
     dot -- times, workspace of both, and the largest difference of the two results relative to q_k;
  3. the MLP stage per layer through compress_nystrom with MODEGPT_OUTPUT_ERROR unset and set, alternating in one process.

    python scripts/probes/output_error_timing.py [--n 14336 --d 4096 --keep 0.7 --tokens 32768 --layers 6 --runs 3]

Inputs as in DESIGN.md section 7, "The error-versus-rank curve": Gaussian columns x log-uniform scales (engine.make_activation_batch),
bf16 N(0, 0.02^2) weights."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import engine, ops  # noqa: E402
from modegpt_amd.compression.compress_mlp import compress_nystrom  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=14336)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--keep", type=float, default=0.7)
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = dict(engine.SHAPES["llama-3-8b"], d=a.d, d_ff=a.n, n_layers=a.layers)
    n, d, r = a.n, a.d, int(a.n * a.keep)
    fmt = lambda ts: " / ".join("%.2f" % t for t in ts)          # noqa: E731

    C = torch.zeros(n, n, dtype=torch.float64, device=dev)
    step = 8192
    for t0 in range(0, a.tokens, step):
        ops.cov_accum(C, engine.make_activation_batch(shape, min(step, a.tokens - t0), seed=50 + t0, device=dev)["h"])
    ops.cov_finalize(C, 1.0 / a.tokens)
    W = engine.make_layer_weights(shape, 1234, dev)["down"]
    with ops.DeferredStatus(dev) as st:
        idx = ops.select_smallest_sorted(ops.ridge_scores(C, 1e-4), r)
        down = ops.nystrom_down(C, idx, W, eps=1e-6)
    st.check()

    # 1. the kernel alone
    ops.mlp_output_error(C, W, idx, down, want_unorm2=True)       # (warm-up: module load)
    te, (e, u2) = timed(lambda: ops.mlp_output_error(C, W, idx, down, want_unorm2=True), 4)
    tq, q = timed(lambda: ops.mlp_output_error(C, W, None, None), 4)
    ws = ops._lib.load().mdg_mlp_output_error_ws_bytes(n, d)
    flop = d * n * (n + 1)
    print("KERNEL n=%d d=%d r=%d: e call %s ms, q call %s ms; %.3f TFLOP per call -> %.1f TF at the fastest; workspace %.2f MB" % (
        n, d, r, fmt(te), fmt(tq), flop / 1e12, flop / min(te + tq) / 1e9, ws / 1e6))
    E, Q = float(e.sum()), float(q.sum())
    print("VALUES energy %.6e error %.6e relative %.3e objective %.6e; worst channel %.3e" % (
        Q, E, E / Q, E + 1e-6 * float(u2.sum()), float((e / q).max())))

    # 2. the materialising route
    def materialised():
        U = W.to(torch.float64)
        U[:, idx] -= down.to(torch.float64)
        P = torch.empty(d, n, dtype=torch.float64, device=dev)
        ops.gemm(U, C, P)                                         # C is full after cov_finalize (both triangles)
        return (P * U).sum(dim=1)
    materialised()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    tm, em = timed(materialised, 4)
    peak = torch.cuda.max_memory_allocated(dev) - base
    # (a statistic whose upper triangle was never mirrored would need a second copy of C on top of this: + 8 n^2 bytes)
    print("MATERIALISED U (torch scatter) + ops.gemm(U, C) + row dot: %s ms; peak extra memory %.2f GB (+ %.2f GB for a mirrored copy of C "
          "where only the lower triangle is valid); max |e - e'| / q_k = %.3e" % (
              fmt(tm), peak / 1e9, 8 * n * n / 1e9, float(((e - em).abs() / q).max())))
    del em

    # 3. the MLP stage through compress_nystrom, switch off / on alternating
    layers = list(range(a.layers))
    weights = {l: engine.make_layer_weights(shape, 1234 + l, dev) for l in layers}
    cov = [C] * a.layers
    keep = [a.keep] * a.layers
    res = {"off": [], "on": []}
    for run in range(a.runs + 1):                                 # (run 0 warms both settings up)
        for name in ("off", "on"):
            os.environ["MODEGPT_OUTPUT_ERROR"] = "1" if name == "on" else "0"
            adapter = engine.TensorAdapter(shape, weights)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            compress_nystrom(adapter, cov, keep, layers)
            if hasattr(adapter, "check_chains"):
                adapter.check_chains()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3 / a.layers
            if run:
                res[name].append(dt)
            if name == "on" and run == a.runs:
                rep = adapter.report_output_errors()
                print("REPORT layer 0:", rep.get(0))
    print("STAGE per layer through compress_nystrom (%d layers, wall clock, %d runs alternating): off %s ms, on %s ms" % (
        a.layers, a.runs, fmt(res["off"]), fmt(res["on"])))


if __name__ == "__main__":
    main()
