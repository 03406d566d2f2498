"""What a bool mask costs on the attention kernels (MODEGPT_FUSED_ATTN_MASK=1), one GPU: 32 query heads, 8 kv heads, bf16, the
mask Transformers builds for a left-padded batch (sdpa_mask: the causal rule ANDed with the padding columns, bool [B, 1, T, S]);
the pad counts of the B rows are spread evenly over 0 .. T / 4 (prefill) or 0 .. S / 4 (decode).

Per shape, on the same tensors:
  prefill (T = S)   masked     mdg_attn_mask_summary + mdg_attn_fwd_masked with causal = 0 (the mask alone decides), as _attend calls them
                    summary    mdg_attn_mask_summary alone
                    unmasked   mdg_attn_fwd with causal = 1 and no mask: the yardstick for what the mask costs (it ignores the padding)
                    sdpa       transformers' sdpa_attention_forward with the same mask: what the switch-off forward runs
  decode (T = 1)    masked     mdg_attn_decode_masked with causal = 0, the split rule of mdg_attn_decode_splits
                    unmasked   mdg_attn_decode with causal = 1
                    sdpa       as above
Decode is timed COLD: the calls rotate over enough distinct k / v buffers that their total exceeds --cold-mib (the Infinity Cache
is 256 MiB), the discipline of attn_decode_timing.py.  Prefill repeats one buffer set (its K / V are re-read many times per call
anyway).  HIP events around `calls` back-to-back calls, `--runs` repeats after a warm-up run; minimum and median per call.

    python scripts/probes/attn_mask_timing.py [--prefill 1x2048,16x8192 --decode 1x2048,16x8192 --widths 90x77,128x128 --json out.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import _lib, ops  # noqa: E402


def timed(fns, calls, runs):
    """ms per call, `runs` times: call i of a run is fns[i % len(fns)] (the rotation over the buffers)."""
    out = []
    for run in range(runs + 1):                                   # (run 0 warms up)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(calls):
            fns[i % len(fns)]()
        b.record()
        b.synchronize()
        if run:
            out.append(a.elapsed_time(b) / calls)
    return out


class _Module(torch.nn.Module):
    """What HF's attention functions read from the attention module."""

    def __init__(self, groups):
        super().__init__()
        self.num_key_value_groups, self.is_causal = groups, True
        self.eval()


def hf_mask(B, T, S, span, dev):
    """bool [B, 1, T, S]: j <= i + S - T and j >= pad_b, pad_b spread evenly over 0 .. span."""
    pads = torch.tensor([span * b // max(B - 1, 1) for b in range(B)], device=dev)
    i = torch.arange(T, device=dev)[None, :, None]
    j = torch.arange(S, device=dev)[None, None, :]
    return ((j <= i + (S - T)) & (j >= pads[:, None, None]))[:, None].contiguous(), pads.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefill", default="1x2048,1x8192,16x2048,16x8192", help="BxT list (S = T)")
    ap.add_argument("--decode", default="1x2048,1x8192,16x2048,16x8192", help="BxS list (T = 1)")
    ap.add_argument("--widths", default="90x77,128x128", help="r_qk x r_vo list")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4, help="prefill calls per run; decode: at least this many")
    ap.add_argument("--cold-mib", type=float, default=320.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_mask_timing: no GPU")
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    lib = _lib.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    mod = _Module(a.heads // a.kv)
    stream = torch.cuda.current_stream(dev).cuda_stream
    records = []
    H, KV = a.heads, a.kv
    print("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), flush=True)

    def measure(rec, name, fns, calls):
        try:
            rc = fns[0]()
            torch.cuda.synchronize()
            if isinstance(rc, int) and rc != 0:
                raise RuntimeError(_lib.last_error())
            times = timed(fns, calls, a.runs)
        except (RuntimeError, torch.OutOfMemoryError) as exc:
            rec["paths"][name] = dict(refused=str(exc).splitlines()[0][:160])
            print("  %-10s refused: %s" % (name, rec["paths"][name]["refused"]), flush=True)
            torch.cuda.empty_cache()
            return
        rec["paths"][name] = dict(us_min=round(min(times) * 1e3, 1), us_median=round(statistics.median(times) * 1e3, 1))
        print("  %-10s %11.1f us min / %11.1f us median" % (name, min(times) * 1e3, statistics.median(times) * 1e3), flush=True)

    def ratios(rec):
        p = rec["paths"]
        if all("us_min" in p.get(n, {}) for n in ("masked", "unmasked")):
            rec["masked_over_unmasked"] = round(p["masked"]["us_min"] / p["unmasked"]["us_min"], 3)
            print("  masked / unmasked = %.3f" % rec["masked_over_unmasked"], flush=True)
        if all("us_min" in p.get(n, {}) for n in ("masked", "sdpa")):
            rec["sdpa_over_masked"] = round(p["sdpa"]["us_min"] / p["masked"]["us_min"], 2)
            print("  sdpa / masked = %.2f" % rec["sdpa_over_masked"], flush=True)

    for width in a.widths.split(","):
        r_qk, r_vo = (int(x) for x in width.split("x"))
        scale = float(r_qk) ** -0.5
        rand = lambda *s: torch.randn(*s, device=dev, generator=gen).to(torch.bfloat16)              # noqa: E731
        for shape in [s for s in a.prefill.split(",") if s]:
            B, T = (int(x) for x in shape.split("x"))
            S = T
            q, k, v = rand(B, H, T, r_qk), rand(B, KV, S, r_qk), rand(B, KV, S, r_vo)
            out = torch.empty(B, T, H, r_vo, dtype=q.dtype, device=dev)
            mask, pads = hf_mask(B, T, S, T // 4, dev)
            n_sum = int(lib.mdg_attn_mask_summary_bytes(B, 1, T, S))
            summary = torch.empty(n_sum, dtype=torch.uint8, device=dev)
            st = (0 if B == 1 else mask.stride(0), 0, mask.stride(2))
            base = (q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.MDG_BF16, B, T, S, H, KV, r_qk, r_vo, k.stride(0), k.stride(1),
                    k.stride(2), v.stride(0), v.stride(1), v.stride(2), scale)
            sum_args = (mask.data_ptr(), B, 1, T, S, st[0], st[1], st[2], summary.data_ptr(), n_sum, stream)
            m_args = base + (0, out.data_ptr(), H * r_vo, stream, mask.data_ptr(), 1, st[0], st[1], st[2], summary.data_ptr(), n_sum)
            u_args = base + (1, out.data_ptr(), H * r_vo, stream)

            def masked():
                rc = lib.mdg_attn_mask_summary(*sum_args)
                return rc or lib.mdg_attn_fwd_masked(*m_args)

            rec = dict(kind="prefill", B=B, T=T, S=S, r_qk=r_qk, r_vo=r_vo, heads=H, kv=KV, pads=pads, paths={})
            print("prefill B=%d T=S=%d r_qk=%d r_vo=%d bf16, pads %s" % (B, T, r_qk, r_vo, pads if B <= 4 else "0 .. %d" % pads[-1]),
                  flush=True)
            measure(rec, "masked", [masked], a.calls)
            got = out.clone()
            measure(rec, "summary", [lambda: lib.mdg_attn_mask_summary(*sum_args)], a.calls)
            states = torch.bincount(summary.flatten().long(), minlength=3).tolist()
            rec["tiles_none_all_mixed"] = states
            print("  tiles: %d admit nothing, %d everything, %d mixed" % tuple(states[:3]), flush=True)
            measure(rec, "unmasked", [lambda: lib.mdg_attn_fwd(*u_args)], a.calls)
            with torch.no_grad():
                measure(rec, "sdpa", [lambda: sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale)], a.calls)
                if "us_min" in rec["paths"]["sdpa"]:
                    ref = sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale)[0]
                    ok = mask.any(dim=-1)[:, 0, :, None, None]                                    # rows with a key at all
                    rec["max_abs_diff_masked_vs_sdpa"] = float(((ref.float() - got.float()) * ok).abs().max())
                    print("  max |masked - sdpa| = %.3e" % rec["max_abs_diff_masked_vs_sdpa"], flush=True)
                    del ref
            ratios(rec)
            records.append(rec)
            del q, k, v, out, mask, summary, got
            torch.cuda.empty_cache()
        for shape in [s for s in a.decode.split(",") if s]:
            B, S = (int(x) for x in shape.split("x"))
            T = 1
            kv_bytes = B * KV * S * (r_qk + r_vo) * 2
            nbuf = max(2, int(a.cold_mib * 2 ** 20 // kv_bytes) + 1)
            calls = max(a.calls, nbuf)
            q = rand(B, H, T, r_qk)
            sets = [(rand(B, KV, S, r_qk), rand(B, KV, S, r_vo)) for _ in range(nbuf)]
            out = torch.empty(B, T, H, r_vo, dtype=q.dtype, device=dev)
            mask, pads = hf_mask(B, T, S, S // 4, dev)
            st = (0 if B == 1 else mask.stride(0), 0, 0)
            splits = ops.attn_decode_splits(B, KV, S, dev)
            ws = torch.empty(lib.mdg_attn_decode_ws_bytes(B, T, H, r_vo, splits) // 4, dtype=torch.float32, device=dev)

            def make(k, v, masked):
                base = (q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.MDG_BF16, B, T, S, H, KV, r_qk, r_vo, k.stride(0), k.stride(1),
                        k.stride(2), v.stride(0), v.stride(1), v.stride(2), scale, 0 if masked else 1, splits, ws.data_ptr(),
                        ws.numel() * 4, out.data_ptr(), H * r_vo, stream)
                if masked:
                    args = base + (mask.data_ptr(), 1, st[0], st[1], st[2])
                    return lambda: lib.mdg_attn_decode_masked(*args)
                return lambda: lib.mdg_attn_decode(*base)

            rec = dict(kind="decode", B=B, T=T, S=S, r_qk=r_qk, r_vo=r_vo, heads=H, kv=KV, kv_bytes=kv_bytes, buffers=nbuf, calls=calls,
                       splits=splits, paths={})
            print("decode B=%d T=1 S=%d r_qk=%d r_vo=%d bf16: K+V %.1f MB, %d buffers (cold), %d splits" % (B, S, r_qk, r_vo, kv_bytes / 1e6,
                                                                                                        nbuf, splits), flush=True)
            measure(rec, "masked", [make(k, v, True) for k, v in sets], calls)
            measure(rec, "unmasked", [make(k, v, False) for k, v in sets], calls)
            with torch.no_grad():
                measure(rec, "sdpa", [(lambda k=k, v=v: sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale))
                                      for k, v in sets], calls)
            ratios(rec)
            records.append(rec)
            del q, sets, out, ws, mask
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            f.write("{" + json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__))[1:-1] + ', "records": [\n')
            f.write(",\n".join(json.dumps(r) for r in records))
            f.write("\n]}\n")


if __name__ == "__main__":
    main()
