"""mdg_attn_decode_kv8 on an fp8 cache against mdg_attn_decode on a bf16 cache of the same shape, in the same run: the shapes, the
COLD protocol (calls rotate over enough distinct caches that their total exceeds --cold-mib, so no call finds its cache in the
256 MiB Infinity Cache) and the min / median / max of attn_decode_timing.py.  32 query heads, 8 kv heads, bf16 q, causal, T = 1,
the split rule of the device.  The figure of each side is ITS OWN K+V bytes (fp8: padded rows plus scales) over its time, as a share
of the 6.29 TB/s copy figure; the ratio of the two times is what the cache buys.

Beside them, per shape: mdg_kv8_append of one decode step (K and V of T = 1) and of a prefill (T = 2048) into the cache, and one
step's DynamicCache.update at the same S -- the torch.cat of the whole cache that the Fp8KVCache removes.

    python scripts/probes/attn_decode_kv8_timing.py [--shapes 1x1x2048,... --widths 90x77,... --json out.json]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from modegpt_amd import _lib, ops  # noqa: E402
from scripts.probes.attn_decode_timing import COPY_TBPS, timed, write_json  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x1x2048,1x1x8192,1x1x32768,16x1x2048,16x1x8192,16x1x32768", help="BxTxS list")
    ap.add_argument("--widths", default="90x77,90x90,128x128", help="r_qk x r_vo list")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-calls", type=int, default=8)
    ap.add_argument("--cold-mib", type=float, default=320.0, help="total cache bytes a rotation must exceed (Infinity Cache: 256)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_decode_kv8_timing: no GPU")
    from transformers.cache_utils import DynamicCache
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    gen = torch.Generator(device=dev).manual_seed(5)
    stream = torch.cuda.current_stream(dev).cuda_stream
    records = []
    print("device %s, %d CUs, torch %s; copy bandwidth taken as %.2f TB/s" % (torch.cuda.get_device_name(0), n_cu, torch.__version__,
                                                                            COPY_TBPS))
    for shape in a.shapes.split(","):
        B, T, S = (int(x) for x in shape.split("x"))
        for width in a.widths.split(","):
            r_qk, r_vo = (int(x) for x in width.split("x"))
            rand = lambda *s: torch.randn(*s, device=dev, generator=gen).to(torch.bfloat16)          # noqa: E731
            pk, pv = ops.kv8_pitch(r_qk), ops.kv8_pitch(r_vo)
            bytes16 = B * a.kv * S * (r_qk + r_vo) * 2
            bytes8 = B * a.kv * S * (pk + pv + 8)
            nbuf = max(2, int(a.cold_mib * 2 ** 20 // bytes8) + 1)               # the smaller cache sets the rotation for both
            calls = max(a.min_calls, nbuf)
            q = rand(B, a.heads, T, r_qk)
            scale = float(r_qk) ** -0.5
            out = torch.empty(B, T, a.heads, r_vo, dtype=q.dtype, device=dev)
            rule = ops.attn_decode_splits(B, a.kv, S, dev)
            ws = torch.empty(lib.mdg_attn_decode_ws_bytes(B, T, a.heads, r_vo, rule) // 4, dtype=torch.float32, device=dev)
            sets16, sets8 = [], []
            for _ in range(nbuf):
                k, v = rand(B, a.kv, S, r_qk), rand(B, a.kv, S, r_vo)
                planes = []
                for x, p in ((k, pk), (v, pv)):
                    data = torch.empty(B, a.kv, S, p, dtype=torch.uint8, device=dev)
                    sc = torch.empty(B, a.kv, S, dtype=torch.float32, device=dev)
                    ops.kv8_append(x, data, sc, 0)
                    planes += [data, sc]
                sets16.append((k, v))
                sets8.append(tuple(planes))
            rec = dict(B=B, T=T, S=S, r_qk=r_qk, r_vo=r_vo, heads=a.heads, kv=a.kv, bytes_bf16=bytes16, bytes_fp8=bytes8, buffers=nbuf,
                       calls=calls, runs=a.runs, splits=rule, paths={})
            print("B=%d T=%d S=%d r_qk=%d r_vo=%d: K+V bf16 %.1f MB, fp8 %.1f MB; %d caches each, %d calls x %d runs, %d splits"
                  % (B, T, S, r_qk, r_vo, bytes16 / 1e6, bytes8 / 1e6, nbuf, calls, a.runs, rule), flush=True)

            def bf16_fn(k, v):
                args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.MDG_BF16, B, T, S, a.heads, a.kv, r_qk, r_vo, k.stride(0),
                        k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), scale, 1, rule, ws.data_ptr(), ws.numel() * 4,
                        out.data_ptr(), a.heads * r_vo, stream)
                return lambda: lib.mdg_attn_decode(*args)

            def fp8_fn(kd, ks, vd, vs):
                args = (q.data_ptr(), kd.data_ptr(), ks.data_ptr(), vd.data_ptr(), vs.data_ptr(), _lib.MDG_BF16, B, T, S, a.heads, a.kv,
                        r_qk, r_vo, S, pk, pv, scale, 1, rule, ws.data_ptr(), ws.numel() * 4, out.data_ptr(), a.heads * r_vo, stream,
                        None, 0, 0, 0, 0)
                return lambda: lib.mdg_attn_decode_kv8(*args)

            def put(name, fns, nbytes, n_calls=calls):
                rc = fns[0]()
                torch.cuda.synchronize()
                if isinstance(rc, int) and rc != 0:
                    raise RuntimeError(_lib.last_error())
                times = timed(fns, n_calls, a.runs)
                best = min(times)
                e = dict(us_min=round(best * 1e3, 2), us_median=round(statistics.median(times) * 1e3, 2), us_max=round(max(times) * 1e3, 2),
                         mb=round(nbytes / 1e6, 2), of_copy=round(nbytes / (best * 1e-3) / 1e12 / COPY_TBPS, 4))
                rec["paths"][name] = e
                print("  %-22s cold %9.1f us min / %9.1f med / %9.1f max   %8.2f MB  (%4.1f %% of copy)"
                      % (name, e["us_min"], e["us_median"], e["us_max"], e["mb"], 100 * e["of_copy"]), flush=True)
                return best

            t16 = put("decode bf16", [bf16_fn(*s) for s in sets16], bytes16)
            t8 = put("decode fp8", [fp8_fn(*s) for s in sets8], bytes8)
            rec["fp8_over_bf16_time"] = round(t8 / t16, 4)
            print("  fp8 time / bf16 time = %.3f" % (t8 / t16), flush=True)
            # the append of one step and of a prefill into those caches (K and V: two launches), rotating over them
            for Ta in (1, 2048):
                if Ta > S:
                    continue
                kn, vn = rand(B, a.kv, Ta, r_qk), rand(B, Ta, a.kv, r_vo).transpose(1, 2)     # v: the projection's transposed view

                def append_fn(kd, ks, vd, vs):
                    def call():
                        ops.kv8_append(kn, kd, ks, S - Ta)
                        ops.kv8_append(vn, vd, vs, S - Ta)
                    return call
                put("kv8_append T=%d" % Ta, [append_fn(*s) for s in sets8], B * a.kv * Ta * ((r_qk + r_vo) * 2 + pk + pv + 8))
            # what DynamicCache.update costs one decode step at this S: a torch.cat of the whole bf16 cache (read + write)
            k1, v1 = rand(B, a.kv, 1, r_qk), rand(B, a.kv, 1, r_vo)

            def cat_fn(k, v):
                def call():
                    c = DynamicCache()
                    c.update(k[:, :, :S - 1], v[:, :, :S - 1], 0)
                    c.update(k1, v1, 0)
                return call

            def seed_fn(k, v):
                def call():
                    DynamicCache().update(k[:, :, :S - 1], v[:, :, :S - 1], 0)
                return call
            both = put("DynamicCache seed+step", [cat_fn(*s) for s in sets16], 2 * bytes16)
            seed = put("DynamicCache seed", [seed_fn(*s) for s in sets16], bytes16)
            rec["dynamic_cache_step_us"] = round((both - seed) * 1e3, 2)
            print("  one step's DynamicCache.update (difference of the two): %.1f us" % ((both - seed) * 1e3), flush=True)
            records.append(rec)
            del q, sets16, sets8, out, ws
            torch.cuda.empty_cache()
    if a.json:
        write_json(a.json, dict(device=torch.cuda.get_device_name(0), n_cu=n_cu, torch=torch.__version__, copy_tbps=COPY_TBPS), records)


if __name__ == "__main__":
    main()
