"""What one mdg_vo_bias call costs at Llama-3-8B attention shapes (d = 4096, 32 query / 8 kv heads of 128, rank 88, bf16 weights):
HIP events around CALLS back-to-back calls on one stream, five runs after a warm-up, both forms (b_o given: the fold into o_proj's
bias; b_o NULL: the projected v bias).  A call is three launches: one workgroup per kv head (P b_v, (I - Q P) b_v), the pass over
W_o (32 MiB, the only HBM traffic that matters), one workgroup for the two norms.  Prints one JSON line per form.

    python scripts/probes/vo_bias_timing.py            ("Projection biases", quotes the result)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from modegpt_amd import _lib  # noqa: E402

CALLS, RUNS = 20, 5
D, N_HEADS, N_KV, HD, RANK = 4096, 32, 8, 128, 88


def main():
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(8192, D, device=dev, generator=g, dtype=torch.float64)
    cov = (x.T @ x) / 8192
    Wv = (torch.randn(N_KV * HD, D, device=dev, generator=g) * D ** -0.5).to(torch.bfloat16)
    Wo = (torch.randn(D, N_HEADS * HD, device=dev, generator=g) * D ** -0.5).to(torch.bfloat16)
    b_v = (torch.randn(N_KV * HD, device=dev, generator=g) * 0.15).to(torch.bfloat16)
    b_o = (torch.randn(D, device=dev, generator=g) * 0.15).to(torch.bfloat16)
    nbytes = lib.mdg_vo_compress_ws_bytes(D, N_HEADS, N_KV, HD)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    v_out = torch.empty(N_KV * RANK, D, dtype=torch.bfloat16, device=dev)
    o_out = torch.empty(D, N_HEADS * RANK, dtype=torch.bfloat16, device=dev)
    o_bias = torch.empty(D, dtype=torch.float64, device=dev)
    v_bias = torch.empty(N_KV * RANK, dtype=torch.float64, device=dev)
    resid = torch.empty(2, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.mdg_vo_compress(cov.data_ptr(), D, D, Wv.data_ptr(), D, Wo.data_ptr(), N_HEADS * HD, _lib.MDG_BF16, N_HEADS, N_KV, HD,
                                   RANK, 1e-5, v_out.data_ptr(), D, o_out.data_ptr(), N_HEADS * RANK, None, None, ws.data_ptr(), nbytes, st),
               "mdg_vo_compress")

    def call(bo):
        _lib.check(lib.mdg_vo_bias(ws.data_ptr(), nbytes, Wo.data_ptr(), N_HEADS * HD, _lib.MDG_BF16, D, b_v.data_ptr(),
                                   None if bo is None else bo.data_ptr(), _lib.MDG_BF16, N_HEADS, N_KV, HD, RANK, o_bias.data_ptr(),
                                   v_bias.data_ptr(), resid.data_ptr(), st), "mdg_vo_bias")

    for form, bo in (("fold", b_o), ("project", None)):
        for _ in range(CALLS):
            call(bo)
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(RUNS):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(CALLS):
                call(bo)
            stop.record()
            torch.cuda.synchronize(dev)
            times.append(start.elapsed_time(stop) * 1e3 / CALLS)
        times.sort()
        print(json.dumps({"probe": "vo_bias_timing", "form": form, "d": D, "n_heads": N_HEADS, "n_kv": N_KV, "hd": HD, "rank": RANK,
                          "calls_per_run": CALLS, "us_per_call": [round(t, 2) for t in times], "median_us": round(times[RUNS // 2], 2),
                          "w_o_mib": Wo.numel() * 2 / 2 ** 20, "resid": [float(v) for v in resid.cpu()]}))


if __name__ == "__main__":
    main()
