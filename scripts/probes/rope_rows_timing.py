"""Cost of the post-RoPE statistics (MODEGPT_QK_ROPE=1) at Llama-3-8B shapes, one GPU: HIP events around `--calls` back-to-back
calls, repeated `--runs` times after a warm-up, for

  1. mdg_rope_rows on the q and k projection outputs of a calibration batch ([B*T, 32*128] and [B*T, 8*128] bf16), beside
     mdg_rope_gather without a mask at the same shapes -- it moves the same bytes (read once, write once), so it is the yardstick --
     with the achieved TB/s of both (algorithmic bytes: 2 * B*T*heads*hd * 2),
  2. what the switch adds per layer and batch: the two rotations plus the one fp64 launch for sigma_q' and sigma_k',
  3. the layer's existing statistic launches of the same batch (sigma_mlp, sigma_x, sigma_q, sigma_k through ops.cov_accum_multi,
     as the Llama hooks send them), the part of a layer's calibration that 2. is compared with.

    python scripts/probes/rope_rows_timing.py [--batch 16 --seq 2048 --heads 32 --kv 8 --hd 128 --d 4096 --ff 14336 --calls 20 --runs 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import ops  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--ff", type=int, default=14336)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rope_rows_timing: no GPU")
    dev = torch.device("cuda:0")
    B, T, hd = a.batch, a.seq, a.hd
    gen = torch.Generator(device=dev).manual_seed(3)
    rand = lambda *shape: torch.randn(*shape, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731
    q, k = rand(B, T, a.heads * hd), rand(B, T, a.kv * hd)
    ang = torch.rand(1, T, hd // 2, device=dev, generator=gen) * 6.28
    emb = torch.cat((ang, ang), -1)
    cos, sin = emb.cos().to(torch.bfloat16), emb.sin().to(torch.bfloat16)
    fmt = lambda ts: " / ".join("%.1f" % t for t in ts)                                              # noqa: E731
    tbs = lambda x, ts: " / ".join("%.2f" % (2 * x.numel() * 2 / (t * 1e-6) / 1e12) for t in ts)     # noqa: E731

    # 1. the rotation against its yardstick
    oq, ok = torch.empty_like(q), torch.empty_like(k)
    gq = torch.empty(B, a.heads, T, hd, dtype=q.dtype, device=dev)
    gk = torch.empty(B, a.kv, T, hd, dtype=k.dtype, device=dev)
    for name, x, heads, n_kv, out, gout in (("q", q, a.heads, a.kv, oq, gq), ("k", k, a.kv, a.kv, ok, gk)):
        t_rows = timed(lambda: ops.rope_rows(x, cos, sin, heads, hd, out=out), a.calls, a.runs)
        t_gather = timed(lambda: ops.rope_gather(x, cos, sin, None, heads, n_kv, hd, out=gout), a.calls, a.runs)
        assert torch.equal(out.view(B, T, heads, hd).transpose(1, 2), gout), "the two kernels disagree"
        print("ROTATE %s [%d, %d x %d] bf16, microseconds per call over %d back-to-back calls, %d runs: rope_rows %s (%s TB/s); "
              "rope_gather without a mask %s (%s TB/s)" % (name, B * T, heads, hd, a.calls, a.runs, fmt(t_rows), tbs(x, t_rows),
                                                            fmt(t_gather), tbs(x, t_gather)))

    # 2. what the switch adds per layer and batch
    sq = torch.zeros(a.heads, hd, hd, dtype=torch.float64, device=dev)
    sk = torch.zeros(a.kv, hd, hd, dtype=torch.float64, device=dev)

    def added():
        rq = ops.rope_rows(q, cos, sin, a.heads, hd, out=ops.rope_scratch(q, "q"))
        rk = ops.rope_rows(k, cos, sin, a.kv, hd, out=ops.rope_scratch(k, "k"))
        ops.cov_accum_multi([(sq, rq, a.heads), (sk, rk, a.kv)])
    t_cov = timed(lambda: ops.cov_accum_multi([(sq, oq, a.heads), (sk, ok, a.kv)]), a.calls, a.runs)
    t_added = timed(added, a.calls, a.runs)

    # 3. the layer's existing statistic launches of the same batch
    h, x = rand(B, T, a.ff), rand(B, T, a.d)
    s_mlp = torch.zeros(a.ff, a.ff, dtype=torch.float64, device=dev)
    s_x = torch.zeros(a.d, a.d, dtype=torch.float64, device=dev)
    s_q, s_k = torch.zeros_like(sq), torch.zeros_like(sk)
    t_layer = timed(lambda: ops.cov_accum_multi([(s_mlp, h, 1), (s_x, x, 1), (s_q, q, a.heads), (s_k, k, a.kv)]), max(1, a.calls // 4), a.runs)
    print("SWITCH per layer and batch of %d tokens, microseconds, %d runs: the fp64 launch for sigma_q' + sigma_k' alone %s; two rotations "
          "+ that launch %s; the layer's four existing statistics (mode %s) %s; added / existing = %.3f" % (
              B * T, a.runs, fmt(t_cov), fmt(t_added), ops.COV_MODE, fmt(t_layer), min(t_added) / min(t_layer)))


if __name__ == "__main__":
    main()
