"""Cost of the within-sequence Q/K statistic (MODEGPT_QK_SEQ=1) at Llama-3-8B shapes, one GPU.  HIP events around `--calls`
back-to-back calls per sample; the two sides of a comparison alternate (A B A B ...) after one warm-up round each, and the median
with the spread (min .. max) over `--rounds` samples is printed.  Steps, each a child process under its own `timeout`; the chain
stops at the first step that fails:

  compare  mdg_qk_pair_accum on the rotated rows of a calibration batch ([B*T, 32*128] and [B*T, 8*128] bf16) against the
           yardstick, the fp64 launch ops.cov_accum_multi([(sigma_q', rq, H), (sigma_k', rk, KV)]) on the same rows: the yardstick
           multiplies H + KV Grams of 2 T hd^2 flops per sequence, the new call 2 H (G^k is recomputed per query head).
           Target: median(new) <= (2 H / (H + KV)) x 1.25 x median(yardstick)
  peak     the fp64 matrix rate ops.probe_mfma_f64 reports, and the fraction of it both calls reach
  layer    the layer's four existing statistic launches of the same batch, the part of a layer's calibration the switch adds to

    python scripts/probes/qk_pair_timing.py [--batch 16 --seq 2048 --heads 32 --kv 8 --hd 128 --d 4096 --ff 14336 --calls 10 --rounds 7]
    python scripts/probes/qk_pair_timing.py --step compare        (one step, in this process)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STEPS = (("compare", 240), ("peak", 120), ("layer", 240))


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
        raise SystemExit("qk_pair_timing: no GPU")
    dev = torch.device("cuda:0")
    B, T, H, KV, hd = a.batch, a.seq, a.heads, a.kv, a.hd
    gen = torch.Generator(device=dev).manual_seed(3)
    rand = lambda *shape: torch.randn(*shape, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731
    flops_pair, flops_yard = 2.0 * B * T * hd * hd * 2 * H, 2.0 * B * T * hd * hd * (H + KV)
    if a.step == "layer":
        h, x, q, k = rand(B, T, a.ff), rand(B, T, a.d), rand(B, T, H * hd), rand(B, T, KV * hd)
        zeros = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)                          # noqa: E731
        s_mlp, s_x, s_q, s_k = zeros(a.ff, a.ff), zeros(a.d, a.d), zeros(H, hd, hd), zeros(KV, hd, hd)
        t = alternating({"layer": lambda: ops.cov_accum_multi([(s_mlp, h, 1), (s_x, x, 1), (s_q, q, H), (s_k, k, KV)])},
                        max(1, a.calls // 4), a.rounds)["layer"]
        print("LAYER the four existing statistics of a batch of %d tokens (mode %s), microseconds: %s" % (B * T, ops.COV_MODE, show(t)))
        print(json.dumps({"step": "layer", "median_us": statistics.median(t)}))
        return
    if a.step == "peak":
        peak = ops.probe_mfma_f64()
        print("PEAK fp64 matrix rate reported by mdg_probe_mfma_f64: %.1f TFLOP/s" % (peak / 1e12 if peak > 1e6 else peak))
        print(json.dumps({"step": "peak", "value": peak}))
        return
    rq, rk = rand(B * T, H * hd), rand(B * T, KV * hd)
    pair = torch.zeros(H, hd, hd, dtype=torch.float64, device=dev)
    raw = torch.zeros_like(pair)
    sq, sk = torch.zeros_like(pair), torch.zeros(KV, hd, hd, dtype=torch.float64, device=dev)
    t = alternating({"yardstick": lambda: ops.cov_accum_multi([(sq, rq, H), (sk, rk, KV)]),
                     "pair": lambda: ops.qk_pair_accum(pair, raw, rq, rk, B, T, H, KV, hd)}, a.calls, a.rounds)
    my, mp = statistics.median(t["yardstick"]), statistics.median(t["pair"])
    target = flops_pair / flops_yard * 1.25 * my
    print("COMPARE [%d x %d, %d + %d heads of %d] bf16, microseconds per call over %d back-to-back calls, %d alternating rounds:"
          % (B, T, H, KV, hd, a.calls, a.rounds))
    print("  yardstick cov_accum_multi(sigma_q', sigma_k'): %s  = %.1f TFLOP/s" % (show(t["yardstick"]), flops_yard / my / 1e6))
    print("  qk_pair_accum (pair and pair_raw):             %s  = %.1f TFLOP/s" % (show(t["pair"]), flops_pair / mp / 1e6))
    print("  target (flop ratio %.2f x 1.25 x yardstick) %.1f: %s by %.1f %%" % (flops_pair / flops_yard, target,
                                                                               "met" if mp <= target else "MISSED", abs(mp / target - 1) * 100))
    print(json.dumps({"step": "compare", "yardstick_us": t["yardstick"], "pair_us": t["pair"], "target_us": target,
                      "pair_tflops": flops_pair / mp / 1e6, "yardstick_tflops": flops_yard / my / 1e6}))


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
            raise SystemExit("qk_pair_timing: step %s ended with status %d; the remaining steps are not started" % (step, rc))


if __name__ == "__main__":
    main()
