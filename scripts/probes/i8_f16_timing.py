"""Whole-call time of the int8 digit-plane covariance on fp16 activations against the fp64 route on the same tensors in the same
process, and the same values rounded to bf16 as the baseline for what the element type costs ("fp16
activations and ReLU on load").  HIP events around the whole ops call (split + route + lists + product + remainder), warm-up,
median and spread (max - min) of the same number of repeats for both routes.  Per data set: the route taken, which remainder
implementation the device picked, and the fill of the exact route's event lists (elements with a digit below plane 2, per column
and 2048-token segment, against the capacity of 128) computed here from the bits.

    python scripts/probes/i8_f16_timing.py [--reps 7] [--no-llama]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from modegpt_amd import ops  # noqa: E402


def make(kind, T, n, dev, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    c = torch.exp(torch.empty(n, device=dev).uniform_(math.log(0.05), math.log(2.0), generator=g))
    z = torch.randn(T, n, device=dev, generator=g)
    if kind in ("gaussian", "relu"):        # relu: pre-activations, the ReLU is applied on load (MDG_I8_RELU)
        return z * c
    a = torch.nn.functional.silu(z)
    return a.mul_(torch.randn(T, n, device=dev, generator=g)).mul_(c)


def list_fill(x, relu):
    """-> (largest, mean) number of listed elements per (column, 2048-token segment): elements whose 48-bit integer has a nonzero
    bit below 2^24 (F16Elem / Bf16Elem of csrc/cov_i8.hpp; the columns the route hands to the fp64 column kernel are not excluded)."""
    f16 = x.dtype == torch.float16
    mant, top, bias = (10, 35, 112) if f16 else (7, 38, 0)
    worst, total, segs = 0, 0, 0
    for c0 in range(0, x.shape[1], 1024):
        b = x[:, c0:c0 + 1024].contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        if relu:
            b = torch.where((b & 0x8000) != 0, torch.zeros_like(b), b)
        e, m = (b >> mant) & ((1 << (15 - mant)) - 1), b & ((1 << mant) - 1)
        sig = torch.where(e > 0, m | (1 << mant), m)
        ee = torch.where(e > 0, e, torch.ones_like(e)) + bias
        E = torch.where(sig != 0, ee, torch.zeros_like(ee)).max(dim=0).values
        low = top - (E[None, :] - ee)                                     # position of the significand's lowest bit
        tz = torch.log2((sig & -sig).clamp_min(1).float()).to(torch.int32)     # trailing zeros of the significand
        listed = (sig != 0) & (low + tz < 24)
        T = listed.shape[0]
        pad = (-T) % 2048
        if pad:
            listed = torch.cat([listed, torch.zeros(pad, listed.shape[1], dtype=torch.bool, device=x.device)])
        cnt = listed.view(-1, 2048, listed.shape[1]).sum(dim=1)
        worst, total, segs = max(worst, int(cnt.max())), total + int(cnt.sum()), segs + cnt.numel()
    return worst, total / segs


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), max(ms) - min(ms)


def measure(name, base, relu, reps):
    T, n = base.shape
    S = torch.zeros(n, n, dtype=torch.float64, device=base.device)
    for dtype in (torch.float16, torch.bfloat16):
        x = base.to(dtype)
        info = {}
        ops.cov_accum_i8(S, x, route_info=info, relu=relu)
        worst, mean = list_fill(x, relu)
        i8 = timed(lambda: ops.cov_accum_i8(S, x, report=False, relu=relu), reps)
        f64 = timed(lambda: ops.cov_accum(S, x, relu=relu), reps)
        wins = f64[0] - i8[0] > i8[1] + f64[1]
        print(f"{T}x{n} {name:14s} {str(dtype)[6:]:8s} relu={int(relu)} planes={info['planes']} exact={int(info['exact'])} "
              f"remainder={info['remainder']} columns_out={len(info['columns'])} bound={info['bound']:.2e} "
              f"list_fill max {worst}/128 mean {mean:.2f} | int8 {i8[0]:.2f} ms (spread {i8[1]:.2f}) | fp64 {f64[0]:.2f} ms "
              f"(spread {f64[1]:.2f}) | int8 faster beyond the spreads: {wins}", flush=True)
        del x
    del S
    torch.cuda.empty_cache()


def llama_activations(dev):
    """One calibration batch (16 x 2048 tokens) through a random-init fp16 Llama (d 2048, d_ff 8192, 16 / 4 heads of 128, 2 layers):
    what the down_proj pre-hook and the input_layernorm hook of layer 1 see."""
    import transformers
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(hidden_size=2048, intermediate_size=8192, num_hidden_layers=2, num_attention_heads=16,
                                   num_key_value_heads=4, head_dim=128, vocab_size=1024, max_position_embeddings=2048)
    model = transformers.LlamaForCausalLM(cfg).to(dev).to(torch.float16).eval()
    got = {}
    blk = model.model.layers[1]
    h1 = blk.mlp.down_proj.register_forward_pre_hook(lambda m, a: got.__setitem__("mlp", a[0].detach().reshape(-1, a[0].shape[-1]).clone()))
    h2 = blk.input_layernorm.register_forward_hook(lambda m, a, o: got.__setitem__("x", o.detach().reshape(-1, o.shape[-1]).clone()))
    with torch.no_grad():
        model(torch.randint(0, 1024, (16, 2048), device=dev, generator=torch.Generator(device=dev).manual_seed(3)))
    h1.remove()
    h2.remove()
    del model
    torch.cuda.empty_cache()
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-llama", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T = 32768
    for n, kinds in ((4096, ("gaussian", "silu_gated", "relu")), (14336, ("gaussian", "silu_gated", "relu")), (16384, ("relu",))):
        for kind in kinds:
            base = make(kind, T, n, dev)
            measure(kind, base, kind == "relu", args.reps)
            del base
            torch.cuda.empty_cache()
    if not args.no_llama:
        acts = llama_activations(dev)
        measure("llama_mlp_in", acts["mlp"].float(), False, args.reps)
        measure("llama_x", acts["x"].float(), False, args.reps)


if __name__ == "__main__":
    main()
