"""VO compression: SVD of sqrt(C) W_v^T per kv head (reference: src/compression/compress_vo.py)."""
from __future__ import annotations

import logging
from typing import List, Optional

import torch
from torch import Tensor

from .. import ops
from ..adapters.model_adapter import ModelAdapter
from ..model_utils import dtype_p, local_device
from ._window import over_layers
from .compress_qk import attention_error_eps

logger = logging.getLogger("MoDeGPT")


def vo_rank_rule(head_dim: int, keep_ratio: float, arch: str) -> int:
    """compress_vo.py:35-41 (no upper clamp upstream; capped at head_dim here because a head has no more
    singular directions than that)."""
    r = max(1, int(head_dim * keep_ratio))
    if arch == "llama" or "qwen" in arch:
        r = r - (r % 2)
        r = max(2, r)
    return min(r, head_dim)


def _regularised_cov(sqrt_C: Tensor) -> Tensor:
    """The per-head functions of the reference receive sqrt(C + ridge I) (and its inverse) from their caller; the kernel
    works from C + ridge I itself: one fp64-MFMA product recovers it."""
    S = sqrt_C.to(device=local_device(), dtype=dtype_p).contiguous()
    C = torch.empty_like(S)
    ops.gemm(S, S, C)
    return C


@torch.no_grad()
def compress_head_grouped(kv_head_idx: int, kv_head_ratio: int, head_dim: int, rank: int, W_v: Tensor, W_o: Tensor,
                          sqrt_C: Tensor, inv_sqrt_C: Tensor, new_heads_V: list, new_heads_O: list, slice_dims=True,
                          arch="opt"):
    """One kv head of a GQA layer (compress_vo.py:112-159): thin SVD of sqrt(C) W_v,h^T = U S Vh; appends
    W_v' = (C^-1/2 U_r)^T  [rank, d] and, for every query head j of the group, W_o'[j] = (S_r Vh_r W_o[:, j]^T)^T
    [d, rank], fp64 (factors are unique up to a sign per component).  `inv_sqrt_C` is accepted for signature
    compatibility; the Gram route does not need it."""
    if kv_head_ratio < 2:
        raise NotImplementedError("a group of one query head is the MHA case: use compress_head")
    r0, c0 = kv_head_idx * head_dim, kv_head_idx * kv_head_ratio * head_dim
    Wv_h = W_v[r0:r0 + head_dim, :].detach().to(local_device())
    Wo_g = W_o[:, c0:c0 + kv_head_ratio * head_dim].detach().to(local_device())
    _, _, v64, o64 = ops.vo_compress(_regularised_cov(sqrt_C), Wv_h, Wo_g, kv_head_ratio, 1, head_dim, rank, 0.0,
                                     want_f64=True)
    if slice_dims:
        new_heads_V.append(v64)
        for j in range(kv_head_ratio):
            new_heads_O.append(o64[:, j * rank:(j + 1) * rank])
        return
    # upstream's slice_dims=False branch writes the zero-padded V through W_v[:, kv_start:kv_end] (compress_vo.py:135),
    # a column slice of a [n_kv*hd, d] matrix -- shape-inconsistent as written; the row slice is what is meant
    Vp = torch.zeros(head_dim, W_v.shape[1], dtype=W_v.dtype, device=W_v.device)
    Vp[:rank] = v64.to(dtype=W_v.dtype, device=W_v.device)
    W_v[r0:r0 + head_dim, :].data.copy_(Vp)
    for j in range(kv_head_ratio):
        Op = torch.zeros(W_o.shape[0], head_dim, dtype=W_o.dtype, device=W_o.device)
        Op[:, :rank] = o64[:, j * rank:(j + 1) * rank].to(dtype=W_o.dtype, device=W_o.device)
        W_o[:, c0 + j * head_dim:c0 + (j + 1) * head_dim].data.copy_(Op)


@torch.no_grad()
def compress_head(head_idx: int, head_dim: int, rank_i: int, W_v: Tensor, W_o: Tensor, sqrt_C: Tensor, inv_sqrt_C: Tensor,
                  new_heads_V: list, new_heads_O: list, slice_dims=True, arch="opt"):
    """One head of an MHA layer (compress_vo.py:162-223): the two-SVD variant; appends W_v' [rank, d] and W_o' [d, rank]
    (fp64), or with slice_dims=False writes them zero-padded into W_v / W_o in place."""
    s0 = head_idx * head_dim
    Wv_h = W_v[s0:s0 + head_dim, :].detach().to(local_device())
    Wo_h = W_o[:, s0:s0 + head_dim].detach().to(local_device())
    _, _, v64, o64 = ops.vo_compress(_regularised_cov(sqrt_C), Wv_h, Wo_h, 1, 1, head_dim, rank_i, 0.0, want_f64=True)
    if slice_dims:
        new_heads_V.append(v64)
        new_heads_O.append(o64)
        return
    Vp = torch.zeros(head_dim, W_v.shape[1], dtype=W_v.dtype, device=W_v.device)
    Vp[:rank_i] = v64.to(dtype=W_v.dtype, device=W_v.device)
    Op = torch.zeros(W_o.shape[0], head_dim, dtype=W_o.dtype, device=W_o.device)
    Op[:, :rank_i] = o64.to(dtype=W_o.dtype, device=W_o.device)
    W_v[s0:s0 + head_dim, :].data.copy_(Vp)
    W_o[:, s0:s0 + head_dim].data.copy_(Op)


@torch.no_grad()
def compress_vo(adapter: ModelAdapter, cov: List[Tensor], keep_ratios=None, slice_dims=True,
                target_layers: Optional[List[int]] = None):
    """compress_vo.py:13-109.  Grouped (GQA) and two-SVD (MHA) variants are chosen by n_kv_heads != n_heads, as
    upstream; both run inside mdg_vo_compress on the head-sized Gram matrix.  Saves {"v_proj": [n_kv*r, d],
    "o_proj": [d, n_heads*r]} bf16 -- and, with the biases carried (ops.keep_bias_enabled), "o_bias" [d] (b_o + sum_h W_o,h b_v,kv(h):
    v_proj becomes bias-free) or, where o_proj has no bias, "v_bias" [n_kv*r] (P_g b_v,g), in the bias's own dtype.
    With MODEGPT_VO_INTERCEPT=1 (not upstream; DESIGN.md section 7, "The V/O intercept") the truncation is taken on the centred
    statistic S = C - mu mu^T, mu = adapter.x_means[layer], and "o_bias" [d] = b_o + delta is saved for every layer (ops.vo_intercept
    on the stored bf16 factors; b_v / b_o enter only where the biases are carried) and no "v_bias".  The spectrum report's Weyl bound
    still reads the diagonal of the UNCENTRED C: |E_ab| <= eps sqrt(c_aa c_bb) bounds the error of S as well, up to the fp64
    rounding of mu, so the bound stays a bound; the output-error report and the rank curve are evaluated on S."""
    if target_layers is None:
        target_layers = list(range(adapter.n_layers))
    n_heads, head_dim, arch, n_kv = adapter.n_heads, adapter.head_dim, adapter.arch, adapter.n_kv_heads
    ranks = {}

    def enqueue(layer):
        ranks[layer] = rank_i = vo_rank_rule(head_dim, keep_ratios[layer], arch)
        C = cov[layer].to(device=local_device(), dtype=dtype_p)
        try:
            comps = adapter.get_attn_components(layer)
            W_v, W_o = comps.v_proj.weight, comps.o_proj.weight
        except Exception as e:  # same tolerance as compress_vo.py:47-53
            logger.warning(f"[VO] Layer {layer}: cannot access v_proj/o_proj: {e}")
            return None
        # (the eigensolver's convergence flag is read once per layer, by the adapter: over_layers)
        record = getattr(adapter, "attention_margin", None)       # (a duck-typed adapter without it: no spectrum report)
        record_error = getattr(adapter, "vo_error", None) if ops.vo_error_enabled() else None       # (... without this: no output error)
        Wv_d, Wo_d = W_v.detach().to(local_device()), W_o.detach().to(local_device())
        # sigma_r against sigma_r+1 of the spectrum just truncated: stays on the device until report_attention_margins
        eps = attention_error_eps(adapter) if record is not None else None
        # the biases (MODEGPT_KEEP_BIAS=1, or Qwen2; DESIGN.md section 7, "Projection biases"): a v bias passes through the softmax
        # unchanged, so it is folded into o_proj's bias where there is one (exact at every rank) and projected by P_g where there is none
        b_v = b_o = None
        if ops.keep_bias_enabled(arch):
            b_v, b_o = getattr(comps.v_proj, "bias", None), getattr(comps.o_proj, "bias", None)
            b_v = None if b_v is None else b_v.detach().to(local_device())
            b_o = None if b_o is None else b_o.detach().to(local_device())
        # the mean-aware truncation (MODEGPT_VO_INTERCEPT=1; DESIGN.md section 7, "The V/O intercept"): the statistic is centred, the
        # factorisation runs on S unchanged (the ridge acts on S), and the mean -- v bias included -- goes into o_bias for exactly the
        # bf16 tensors that are stored.  The spectrum's Weyl bound keeps reading the diagonal of the uncentred C (ops.vo_compress)
        mu, more = None, {"bias": None if b_v is None else (b_v, b_o)}
        if ops.vo_intercept_enabled():
            means = getattr(adapter, "x_means", None)
            if means is None or means[layer] is None:
                raise RuntimeError(f"MODEGPT_VO_INTERCEPT=1 but layer {layer} has no input mean (adapter.x_means): "
                                   "the statistics were collected without the switch")
            mu = means[layer].to(device=local_device(), dtype=dtype_p)
            more = {"spectrum_cov": C}
            C = ops.cov_center(C, mu)                            # S: from here on the statistic of x - mu (cov[layer] is not modified)
        out = ops.vo_compress(C, Wv_d, Wo_d, n_heads, n_kv, head_dim, rank_i, adapter.config.ridge_vo, want_spectrum=record is not None,
                              spectrum_eps=eps, want_curve=record_error is not None, **more)
        biases = {}
        if mu is not None:
            # b_o + delta, in o_proj's bias dtype where it has one (and biases are carried), else the weight's; no v_bias: the v bias
            # is part of a_g and folded exactly at every rank, so mdg_vo_bias is not called and nothing is left for vo_bias_residual
            o_bias, _, norms = ops.vo_intercept(Wv_d, Wo_d, out[0], out[1], mu, n_heads, n_kv, head_dim, rank_i, b_v=b_v, b_o=b_o)
            biases["o_bias"] = o_bias
            record_intercept = getattr(adapter, "vo_intercept", None)
            if callable(record_intercept):
                record_intercept(layer, norms)                   # stays on the device until report_vo_intercepts
        elif b_v is not None:
            (o_bias, v_bias, resid), out = out[-1], out[:-1]
            if o_bias is not None:
                biases["o_bias"] = o_bias.to(b_o.dtype)          # (one rounding of the fp64 sum)
            else:
                biases["v_bias"] = v_bias.to(b_v.dtype)
                record_resid = getattr(adapter, "vo_bias_residual", None)
                if record_resid is not None:
                    record_resid(layer, resid)                   # stays on the device until report_vo_bias_residuals
        elif b_o is not None:
            biases["o_bias"] = b_o.clone()
        V_heads, O_heads = out[0], out[1]
        if record is not None:
            record(layer, "vo", out[2], eps)
        if record_error is not None:
            # what the bf16 tensors about to be saved lose of the attention output, beside the curve of the fp64 truncation: enqueued
            # only, read by report_vo_errors
            q = ops.vo_output_error(C, Wv_d, Wo_d, n_heads, n_kv, head_dim, 0, None, None)
            e, dnorm2 = ops.vo_output_error(C, Wv_d, Wo_d, n_heads, n_kv, head_dim, rank_i, V_heads, O_heads, want_dnorm2=True)
            # (with the intercept C is S here: report and curve are the affine map's, and sum(e + rho dnorm2) = curve[r] holds on S)
            record_error(layer, (q, e, dnorm2, out[-1]), rank_i, **({"centred": True} if mu is not None else {}))
        return V_heads, O_heads, biases

    def retire(layer, result):
        if result is None:
            return
        V_heads, O_heads, biases = result
        adapter.save_layer(output_dir=adapter.config.temp_storage_dir, suffix="vo",
                           weights={"v_proj": V_heads, "o_proj": O_heads, **biases}, layer_idx=layer)
        logger.info(f"[VO] Compressed layer {layer} to rank {ranks[layer]} per head")

    over_layers(adapter, list(target_layers), enqueue, retire)
