"""Cost of the V/O output error (mdg_vo_output_error) and of the V/O rank curve (mdg_vo_rank_curve) at Llama-3-8B shapes, one GPU:

  1. the calls alone, HIP events, 4 runs each: one e call (the bf16 artefact, dnorm2 requested), one q call, and vo_compress with and
     without the curve (the curve's time is the difference); workspace sizes; the flop count of the stacked-Gram route beside them;
  2. the V/O stage per layer through compress_vo with MODEGPT_VO_ERROR unset and set, alternating in one process.

    python scripts/probes/vo_error_timing.py [--d 4096 --heads 32 --kv 8 --hd 128 --rank 88 --tokens 32768 --layers 6 --runs 3]

Inputs: Gaussian columns x log-uniform scales (engine.make_activation_batch), bf16 N(0, 0.02^2) weights."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import engine, ops  # noqa: E402
from modegpt_amd.compression.compress_vo import compress_vo  # noqa: E402


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
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--rank", type=int, default=88)
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = dict(engine.SHAPES["llama-3-8b"], d=a.d, n_heads=a.heads, n_kv_heads=a.kv, head_dim=a.hd, n_layers=a.layers)
    d, nh, nkv, hd, r = a.d, a.heads, a.kv, a.hd, a.rank
    fmt = lambda ts: " / ".join("%.2f" % t for t in ts)          # noqa: E731

    C = torch.zeros(d, d, dtype=torch.float64, device=dev)
    step = 8192
    for t0 in range(0, a.tokens, step):
        ops.cov_accum(C, engine.make_activation_batch(shape, min(step, a.tokens - t0), seed=50 + t0, device=dev)["x"])
    ops.cov_finalize(C, 1.0 / a.tokens)
    w = engine.make_layer_weights(shape, 1234, dev)
    Wv, Wo = w["v"], w["o"]
    ridge = engine.RECIPE_RIDGES["ridge_vo"]

    # 1. the calls alone
    plain = lambda: ops.vo_compress(C, Wv, Wo, nh, nkv, hd, r, ridge)                       # noqa: E731
    curved = lambda: ops.vo_compress(C, Wv, Wo, nh, nkv, hd, r, ridge, want_curve=True)     # noqa: E731
    v, o, curve = curved()                                        # (warm-up: module load)
    ops.vo_output_error(C, Wv, Wo, nh, nkv, hd, r, v, o, want_dnorm2=True)
    te, (e, dn) = timed(lambda: ops.vo_output_error(C, Wv, Wo, nh, nkv, hd, r, v, o, want_dnorm2=True), 4)
    tq, q = timed(lambda: ops.vo_output_error(C, Wv, Wo, nh, nkv, hd, 0, None, None), 4)
    tp, _ = timed(plain, 4)
    tc, _ = timed(curved, 4)
    lib = ops._lib.load()
    n = hd + r
    flop_e = 2 * n * d * (nkv * d + nh * n) + 2 * nkv * n * n * d * 2
    flop_q = 2 * hd * d * (nkv * d + nh * hd) + 2 * nkv * hd * hd * d
    print("CALLS d=%d %d/%d hd=%d r=%d: e call %s ms (%.3f TFLOP), q call %s ms (%.3f TFLOP); vo_compress %s ms, with the curve %s ms" % (
        d, nh, nkv, hd, r, fmt(te), flop_e / 1e12, fmt(tq), flop_q / 1e12, fmt(tp), fmt(tc)))
    print("WORKSPACE e call %.2f MB, q call %.2f MB, curve %.2f MB (vo_compress itself %.2f MB)" % (
        lib.mdg_vo_output_error_ws_bytes(d, nh, nkv, hd, r) / 1e6, lib.mdg_vo_output_error_ws_bytes(d, nh, nkv, hd, 0) / 1e6,
        lib.mdg_vo_rank_curve_ws_bytes(d, nh, nkv, hd) / 1e6, lib.mdg_vo_compress_ws_bytes(d, nh, nkv, hd) / 1e6))
    m = ops.decode_vo_output_error(e.cpu(), q.cpu(), dn.cpu(), ridge, r, nkv, curve=curve.cpu())
    print("VALUES", {k: m[k] for k in m if k != "heads"})

    # 2. the V/O stage through compress_vo, switch off / on alternating
    layers = list(range(a.layers))
    weights = {l: engine.make_layer_weights(shape, 1234 + l, dev) for l in layers}
    cov = [C] * a.layers
    keep = [r / hd + 1e-9] * a.layers
    res = {"off": [], "on": []}
    for run in range(a.runs + 1):                                 # (run 0 warms both settings up)
        for name in ("off", "on"):
            os.environ["MODEGPT_VO_ERROR"] = "1" if name == "on" else "0"
            adapter = engine.TensorAdapter(shape, weights)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            compress_vo(adapter, cov, keep, target_layers=layers)
            if hasattr(adapter, "check_chains"):
                adapter.check_chains()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3 / a.layers
            if run:
                res[name].append(dt)
            if name == "on" and run == a.runs:
                rep = adapter.report_vo_errors()
                print("REPORT layer 0:", {k: rep[0][k] for k in rep[0] if k != "heads"})
    print("STAGE per layer through compress_vo (%d layers, wall clock, %d runs alternating): off %s ms, on %s ms" % (
        a.layers, a.runs, fmt(res["off"]), fmt(res["on"])))


if __name__ == "__main__":
    main()
