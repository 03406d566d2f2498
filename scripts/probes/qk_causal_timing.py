"""Cost of the causal Q/K statistic (MODEGPT_QK_CAUSAL=1) at Llama-3-8B shapes, one GPU.  HIP events around `--calls` back-to-back
calls per sample; the two sides of a comparison alternate (A B A B ...) after one warm-up round each, and the median with the spread
(min .. max) over `--rounds` samples is printed.  Steps, each a child process under its own `timeout`; the chain stops at the first
step that fails:

  compare  mdg_qk_causal_accum (pair and pair_raw) on the rotated rows of a calibration batch ([B*T, 32*128] and [B*T, 8*128] bf16)
           against the yardstick, ops.qk_pair_accum with both outputs on the same rows in the same process.  The yardstick executes
           2 Grams of 2 T hd^2 MFMA flops per (sequence, query head); the new call executes, per token and entry, four fused and
           three plain fp64 operations (qk_causal.hip: K, t, pair, pair_raw; qq r, m m) = 11 flops with an FMA as two.
           Budget: median(new) <= (flops(new) / flops(yardstick)) x 1.25 x median(yardstick)
  layer    the layer's existing statistic launches of the same batch (the four covariances, the post-RoPE pair and
           ops.qk_pair_accum), the part of a layer's calibration the switch adds one call to

    python scripts/probes/qk_causal_timing.py [--batch 16 --seq 2048 --heads 32 --kv 8 --hd 128 --d 4096 --ff 14336 --calls 10 --rounds 7]
    python scripts/probes/qk_causal_timing.py --step compare        (one step, in this process)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STEPS = (("compare", 300), ("layer", 300))
FLOPS_PER_ENTRY_TOKEN = 11          # 4 FMA + 3 plain operations per entry and token, with pair_raw


def sample(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls                       # microseconds per call


def alternating(fns, calls, rounds):
    """One warm-up sample of every side, then `rounds` samples of each in alternating order; {name: [microseconds]}."""
    for fn in fns.values():
        sample(fn, calls)
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            out[name].append(sample(fn, calls))
    return out


def show(ts):
    return "median %.1f (%.1f .. %.1f)" % (statistics.median(ts), min(ts), max(ts))


def run_step(a):
    import torch
    from modegpt_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("qk_causal_timing: no GPU")
    dev = torch.device("cuda:0")
    B, T, H, KV, hd = a.batch, a.seq, a.heads, a.kv, a.hd
    gen = torch.Generator(device=dev).manual_seed(3)
    rand = lambda *shape: torch.randn(*shape, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)                              # noqa: E731
    flops_yard = 2.0 * B * T * hd * hd * 2 * H
    flops_new = float(FLOPS_PER_ENTRY_TOKEN) * B * T * hd * hd * H
    rq, rk = rand(B * T, H * hd), rand(B * T, KV * hd)
    pair, raw, cau, cau_raw = zeros(H, hd, hd), zeros(H, hd, hd), zeros(H, hd, hd), zeros(H, hd, hd)
    if a.step == "layer":
        h, x, q, k = rand(B, T, a.ff), rand(B, T, a.d), rand(B, T, H * hd), rand(B, T, KV * hd)
        s_mlp, s_x, s_q, s_k, r_q, r_k = zeros(a.ff, a.ff), zeros(a.d, a.d), zeros(H, hd, hd), zeros(KV, hd, hd), zeros(H, hd, hd), zeros(KV, hd, hd)

        def layer():
            ops.cov_accum_multi([(s_mlp, h, 1), (s_x, x, 1), (s_q, q, H), (s_k, k, KV)])
            ops.cov_accum_multi([(r_q, rq, H), (r_k, rk, KV)])
            ops.qk_pair_accum(pair, raw, rq, rk, B, T, H, KV, hd)
        t = alternating({"layer": layer, "causal": lambda: ops.qk_causal_accum(cau, cau_raw, rq, rk, B, T, H, KV, hd)},
                        max(1, a.calls // 4), a.rounds)
        ml, mc = statistics.median(t["layer"]), statistics.median(t["causal"])
        print("LAYER the existing statistic launches of a batch of %d tokens (mode %s), microseconds: %s" % (B * T, ops.COV_MODE, show(t["layer"])))
        print("LAYER the causal call beside them: %s  = %.1f %% more per batch" % (show(t["causal"]), 100.0 * mc / ml))
        print(json.dumps({"step": "layer", "layer_us": t["layer"], "causal_us": t["causal"]}))
        return
    t = alternating({"yardstick": lambda: ops.qk_pair_accum(pair, raw, rq, rk, B, T, H, KV, hd),
                     "causal": lambda: ops.qk_causal_accum(cau, cau_raw, rq, rk, B, T, H, KV, hd)}, a.calls, a.rounds)
    my, mc = statistics.median(t["yardstick"]), statistics.median(t["causal"])
    budget = flops_new / flops_yard * 1.25 * my
    print("COMPARE [%d x %d, %d + %d heads of %d] bf16, microseconds per call over %d back-to-back calls, %d alternating rounds:"
          % (B, T, H, KV, hd, a.calls, a.rounds))
    print("  yardstick qk_pair_accum (pair and pair_raw):  %s  = %.1f TFLOP/s (%.3g MFMA flops)" % (show(t["yardstick"]), flops_yard / my / 1e6, flops_yard))
    print("  qk_causal_accum (pair and pair_raw):          %s  = %.1f TFLOP/s (%.3g vector flops)" % (show(t["causal"]), flops_new / mc / 1e6, flops_new))
    print("  budget (flop ratio %.2f x 1.25 x yardstick) %.1f: %s, call / budget = %.2f" % (flops_new / flops_yard, budget,
                                                                                          "met" if mc <= budget else "MISSED", mc / budget))
    print(json.dumps({"step": "compare", "yardstick_us": t["yardstick"], "causal_us": t["causal"], "budget_us": budget,
                      "causal_tflops": flops_new / mc / 1e6, "yardstick_tflops": flops_yard / my / 1e6}))


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("batch", 16), ("seq", 2048), ("heads", 32), ("kv", 8), ("hd", 128), ("d", 4096), ("ff", 14336), ("calls", 10),
                          ("rounds", 7)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step:
        return run_step(a)
    passed = [x for x in sys.argv[1:]]
    for step, limit in STEPS:                                    # a fresh child per step, each under its own time limit
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + passed).returncode
        if rc != 0:
            raise SystemExit("qk_causal_timing: step %s ended with status %d; the remaining steps are not started" % (step, rc))


if __name__ == "__main__":
    main()
