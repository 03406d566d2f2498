"""mdg_attn_fwd (MODEGPT_FUSED_ATTN=1) against HF's attention interface on the same tensors, at compressed Llama-3-8B shapes, one
GPU: 32 query heads, 8 kv heads, causal prefill T = S, bf16.  HIP events around `--calls` back-to-back calls, repeated `--runs`
times after a warm-up run (the minimum and the median are reported); peak memory of each path beyond its operands.

  kernel    ops.attn_fwd                                           [B, T, 32, r_vo] token-major, what o_proj reads
  sdpa      transformers' sdpa_attention_forward, no mask, is_causal: what the compressed forward calls with the switch off
  eager     the model family's eager_attention_forward with an additive causal mask (skipped where the score matrix alone
            exceeds --eager-gib)

Which sdpa back end served a shape is FOUND, not guessed: the call is repeated under torch.nn.attention.sdpa_kernel restricted to
one back end at a time; the back ends that accept the shape are listed with their own times, and the unrestricted call's time says
which of them torch chose.  TFLOP/s count the causal half: B * heads * T * S / 2 * 2 * (r_qk + r_vo), against the bf16 matrix peak.

    python scripts/probes/attn_fwd_timing.py [--shapes 1x2048,16x2048,1x8192,16x8192 --widths 90x90,90x77,128x128 --json out.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import ops  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0       # MI355X dense bf16 matrix peak


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
            out.append(a.elapsed_time(b) / calls)                 # milliseconds per call
    return out


def measure(fn, calls, runs):
    """(times in ms, peak bytes allocated beyond what was live before the call) or the error that refused the call."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        fn()
        torch.cuda.synchronize()
    except (RuntimeError, torch.OutOfMemoryError) as exc:
        return None, str(exc).splitlines()[0][:160]
    peak = torch.cuda.max_memory_allocated() - base
    return timed(fn, calls, runs), peak


class _Module(torch.nn.Module):
    """What HF's attention functions read from the attention module."""

    def __init__(self, groups):
        super().__init__()
        self.num_key_value_groups, self.is_causal = groups, True
        self.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x2048,16x2048,1x8192,16x8192", help="BxT list")
    ap.add_argument("--widths", default="90x90,90x77,128x128", help="r_qk x r_vo list")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--eager-gib", type=float, default=24.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_fwd_timing: no GPU")
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    from transformers.models.llama.modeling_llama import eager_attention_forward
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    mod = _Module(a.heads // a.kv)
    backends = {"flash": SDPBackend.FLASH_ATTENTION, "efficient": SDPBackend.EFFICIENT_ATTENTION, "math": SDPBackend.MATH}
    records = []
    for shape in a.shapes.split(","):
        B, T = (int(x) for x in shape.split("x"))
        for width in a.widths.split(","):
            r_qk, r_vo = (int(x) for x in width.split("x"))
            rand = lambda *s: torch.randn(*s, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731
            q, k, v = rand(B, a.heads, T, r_qk), rand(B, a.kv, T, r_qk), rand(B, a.kv, T, r_vo)
            scale = float(r_qk) ** -0.5
            flops = B * a.heads * T * T / 2 * 2 * (r_qk + r_vo)
            calls = max(1, a.calls if B * T <= 16 * 2048 else a.calls // 2)
            rec = dict(B=B, T=T, r_qk=r_qk, r_vo=r_vo, heads=a.heads, kv=a.kv, calls=calls, runs=a.runs, paths={})

            def put(name, res):
                times, extra = res
                if times is None:
                    rec["paths"][name] = dict(refused=extra)
                    print("  %-16s refused: %s" % (name, extra))
                    return
                best, med = min(times), statistics.median(times)
                rec["paths"][name] = dict(ms_min=best, ms_median=med, tflops=flops / (best * 1e-3) / 1e12, peak_bytes=extra)
                print("  %-16s %9.3f ms min / %9.3f median   %7.1f TFLOP/s (%4.1f %% of the bf16 peak)   peak +%.2f GiB"
                      % (name, best, med, flops / (best * 1e-3) / 1e12, 100 * flops / (best * 1e-3) / 1e12 / PEAK_BF16_TFLOPS,
                         extra / 2 ** 30))

            print("B=%d T=S=%d heads=%d kv=%d r_qk=%d r_vo=%d bf16 causal, %d calls x %d runs" % (B, T, a.heads, a.kv, r_qk, r_vo,
                                                                                                calls, a.runs))
            out = torch.empty(B, T, a.heads, r_vo, dtype=q.dtype, device=dev)
            put("kernel", measure(lambda: ops.attn_fwd(q, k, v, scale, causal=True, out=out), calls, a.runs))
            sdpa = lambda: sdpa_attention_forward(mod, q, k, v, None, dropout=0.0, scaling=scale, is_causal=True)  # noqa: E731
            math_gib = B * a.heads * T * T * 2 / 2 ** 30
            with torch.no_grad():
                put("sdpa", measure(sdpa, calls, a.runs))
                err = float("nan")
                if "ms_min" in rec["paths"]["sdpa"]:
                    err = float((sdpa()[0].float() - out.float()).abs().max())
                rec["max_abs_diff_vs_sdpa"] = err
                for name, be in backends.items():
                    if name == "math" and math_gib > a.eager_gib:
                        rec["paths"]["sdpa:math"] = dict(skipped="score matrix %.0f GiB" % math_gib)
                        print("  %-16s skipped: the score matrix alone is %.0f GiB" % ("sdpa:math", math_gib))
                        continue

                    def only(be=be):
                        with sdpa_kernel([be]):
                            return sdpa_attention_forward(mod, q, k, v, None, dropout=0.0, scaling=scale, is_causal=True)
                    put("sdpa:" + name, measure(only, calls, a.runs))
                if math_gib > a.eager_gib:
                    rec["paths"]["eager"] = dict(skipped="score matrix %.0f GiB" % math_gib)
                    print("  %-16s skipped: the score matrix alone is %.0f GiB" % ("eager", math_gib))
                else:
                    mask = torch.full((T, T), torch.finfo(q.dtype).min, dtype=q.dtype, device=dev).triu(1)[None, None]
                    put("eager", measure(lambda: eager_attention_forward(mod, q, k, v, mask, scaling=scale, dropout=0.0),
                                         max(1, calls // 2), a.runs))
                    del mask
            accepted = [n for n in backends if "ms_min" in rec["paths"].get("sdpa:" + n, {})]
            chosen = None
            if "ms_min" in rec["paths"]["sdpa"] and accepted:
                chosen = min(accepted, key=lambda n: abs(rec["paths"]["sdpa:" + n]["ms_min"] - rec["paths"]["sdpa"]["ms_min"]))
            rec["sdpa_backends_accepting"], rec["sdpa_backend_closest_to_unrestricted"] = accepted, chosen
            print("  sdpa back ends that accept the shape: %s; the unrestricted call's time matches: %s; max |kernel - sdpa| = %.3e"
                  % (accepted, chosen, err))
            records.append(rec)
            del q, k, v, out
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, records=records), f, indent=1)


if __name__ == "__main__":
    main()
