"""QK compression: CR column selection in RoPE-pair units (reference: src/compression/compress_qk.py:152-476)."""
from __future__ import annotations

import logging
from typing import List, Optional

import torch
from torch import Tensor

from .. import _lib, calib_stats, ops
from ..calib_stats import layer_value
from ..adapters.model_adapter import ModelAdapter
from ..model_utils import dtype_p, local_device
from .compress_mlp import I8_GUARANTEED_EPS

logger = logging.getLogger("MoDeGPT")

_SQRT_M_DEFAULT_RIDGE = 1e-4  # sqrt_M's default ridge_lambda (compression_utils.py:16)

# What the reference's route to a squared column norm -- eigh -> sqrt -> V diag V^T -> column norm (compression_utils.py:15-55) --
# can differ by from the identity C_jj + rho this engine scores with, relative to ||C||_inf + rho: the `eps_abs` of the QK
# certificate (mdg_qk_select_margin).  The one figure of the certificate that is measured, not derived; measured against the CPU
# oracle's sqrt_M (torch.linalg.eigh on LAPACK), never against this engine:
#     worst over the family of  | ||col_j(sqrt_M(C, rho))||^2 - (C_jj + rho) | / (||C||_inf + rho)  =  EIGH_ROUTE_MEASURED_ULPS * 2^-53
# over every sigma_q / sigma_k head of tests/golden/ (rho in {1e-4, 1e-2}) and 96 seeded synthetic matrices (hd in {64, 128},
# C = X^T X / T with column scales spread over 0, 2, 4, 6 decades and mild mixing, rho in {1e-4, 1e-2}, 6 seeds each;
# tests/test_attn_certificate_host.py builds the family and re-measures it).  Times EIGH_ROUTE_SAFETY = 4, because the reference
# runs torch.linalg.eigh on whatever backend its user has -- LAPACK builds, thread counts and the GPU solvers round differently --
# and a certificate has to cover those too.
EIGH_ROUTE_MEASURED_ULPS = 41.04     # (at tests/golden tiny_mha sigma_k[2], rho = 1e-4; the synthetic part of the family: 24 .. 39 depending on LAPACK threads)
EIGH_ROUTE_SAFETY = 4
EIGH_ROUTE_EPS_ABS = EIGH_ROUTE_SAFETY * EIGH_ROUTE_MEASURED_ULPS * 2.0 ** -53

# ops.qk_select_statistic()'s name of an optional Q/K statistic -> (its record in calib_stats.STATS, what metrics["qk_selection"]
# calls a selection scored on it).  MODEGPT_<switch>_SELECT=1 selects on it; the refusal when the layer has none names the
# record's switch, and the switch of the statistic it needs, as the remedy.
SELECT_STATS = {"rope": ("qk_rope", "post_rope"), "seq": ("qk_pair", "within_sequence"), "causal": ("qk_causal", "within_sequence_causal")}


def attention_error_eps(adapter) -> float:
    """The entry-wise relative error bound eps of the sigma_q / sigma_k / sigma_x this run accumulated, |sigma_ij - exact| <= eps
    sqrt(sigma_ii sigma_jj), for the attention certificates.  `adapter.cov_error_eps` when the caller states it.  Otherwise: which
    route each of these statistics took is not recorded separately, so the larger of the int8 route's guarantee (1.1e-11 x the
    tolerance factor + one fp64 rounding per fold) and the worst case of fp64 accumulation over the calibration tokens,
    (tokens / 4 + 4) 2^-53 -- whatever the model's dtype or width."""
    stated = getattr(adapter, "cov_error_eps", None)
    if stated is not None:
        return float(stated)
    tokens = int(getattr(adapter, "calib_tokens", 0) or getattr(adapter.config, "calib_size", 32) * 2048)
    return max(I8_GUARANTEED_EPS * ops.i8_tolerance() + 64 * 2.0 ** -53, (tokens / 4 + 4) * 2.0 ** -53)


def qk_rank_rule(head_dim: int, keep_ratio: float, arch: str, rank: Optional[int] = None) -> int:
    """compress_qk.py:176-182."""
    r = int(head_dim * keep_ratio) if rank is None else rank
    r = max(1, min(r, head_dim))
    if arch == "llama" or "qwen" in arch:
        r = r - (r % 2)
        r = max(2, min(r, head_dim))
    return r


def qk_mode_and_ridges(arch: str, grouped: bool, ridge_qk: float):
    """Which scoring variant compress_layer dispatches to, with the ridges each one really uses:
    GQA: K gets config.ridge_qk, Q gets sqrt_M's default; MHA llama / OPT: defaults for both."""
    if (arch == "llama" or "qwen" in arch) and grouped:
        return _lib.MDG_QK_ROPE_GROUPED, _SQRT_M_DEFAULT_RIDGE, ridge_qk
    if arch in ("llama", "qwen2"):       # (qwen2 is not upstream's: its MHA checkpoints, Qwen1.5, are Llama blocks with q/k/v biases)
        return _lib.MDG_QK_ROPE_MHA, _SQRT_M_DEFAULT_RIDGE, _SQRT_M_DEFAULT_RIDGE
    if arch == "opt":
        return _lib.MDG_QK_OPT, _SQRT_M_DEFAULT_RIDGE, _SQRT_M_DEFAULT_RIDGE
    raise NotImplementedError("Most likely have to implement it compression for this model.")


@torch.no_grad()
def compress_layer(adapter: ModelAdapter, layer_idx: int, rank: int, cov_q_list: Tensor, cov_k_list: Tensor,
                   rotary_masks: List[Tensor], slice_dims=True, bias=True):
    """One layer (compress_qk.py:208-308): score, select (score-descending order, NOT sorted), gather the rows
    of W_q (all heads of the group) and W_k, append the [n_kv, rank] int64 rotary mask, save {"q_proj","k_proj"}."""
    n_heads, head_dim, arch, n_kv = adapter.n_heads, adapter.head_dim, adapter.arch, adapter.n_kv_heads
    comps = adapter.get_qk_components(layer_idx=layer_idx)
    mode, ridge_q, ridge_k = qk_mode_and_ridges(arch, n_kv != n_heads, adapter.config.ridge_qk)
    cq = cov_q_list.to(device=local_device(), dtype=dtype_p)
    ck = cov_k_list.to(device=local_device(), dtype=dtype_p)
    # Which statistic the selection is scored on (two select switches set together are refused here, before anything else).
    # MODEGPT_QK_ROPE_SELECT=1: the selection, its certificate and the report's order take (sigma_q', sigma_k') instead of the
    # reference's pre-RoPE pair, same mode and ridges.  MODEGPT_QK_SEQ_SELECT=1 / MODEGPT_QK_CAUSAL_SELECT=1: they take (P, ones) /
    # (P^c, ones) with ridges 0 -- a unit's score is then the diagonal of the objective 1^T P[D,D] 1, summed over the group.  No
    # certificate: mdg_qk_select_margin's error model does not cover the cancellation in the centring.  Everything downstream of
    # the mask is unchanged.
    statistic = ops.qk_select_statistic()
    by_rope = statistic == "rope"
    # the layer's optional Q/K statistics (their switch at calibration or in the loaded record), or None: the post-RoPE pair
    # (sigma_q', sigma_k'), the within-sequence (P, P_raw), the causal (P^c, P^c_raw)
    stats = {}
    for select, (name, _) in SELECT_STATS.items():
        value = layer_value(adapter, name, layer_idx)
        stats[select] = None if value is None else tuple(t.to(device=local_device(), dtype=dtype_p) for t in value)
    rope = stats["rope"]
    if statistic in stats and stats[statistic] is None:
        stat = calib_stats.BY_NAME[SELECT_STATS[statistic][0]]
        switches = " and ".join(f"{s.switch}=1" for s in (stat,) + ((calib_stats.BY_NAME[stat.needs],) if stat.needs else ()))
        raise RuntimeError(f"{stat.switch}_SELECT=1 but layer {layer_idx} has no {stat.noun} (adapter.{stat.stats_attr}): "
                           f"calibrate, or load a record saved, with {switches} on a Llama / Qwen2 model")
    sequence = {select: value for select, value in stats.items() if select != "rope" and value is not None}
    ones = torch.ones(n_kv, head_dim, head_dim, dtype=dtype_p, device=local_device()) if sequence else None
    if statistic in sequence:
        sq, sk, sel_ridges = sequence[statistic][0], ones, (0.0, 0.0)
    else:
        (sq, sk), sel_ridges = (rope if by_rope else (cq, ck)), (ridge_q, ridge_k)
    mask, q_rows, k_rows = ops.qk_select(sq, sk, rank, mode, *sel_ridges)
    record = getattr(adapter, "attention_margin", None)           # (a duck-typed adapter without it: no certificate)
    if statistic in sequence:
        note = getattr(adapter, "qk_selection_statistic", None)
        if note is not None:                          # (report_attention_margins writes the entry, with the certificate's absence)
            note(layer_idx, SELECT_STATS[statistic][1])
    elif record is not None:
        # the selection's certificate stays on the device until the adapter next waits for the stream (report_attention_margins)
        eps_rel = attention_error_eps(adapter)
        record(layer_idx, "qk", ops.qk_select_margin(sq, sk, rank, mode, ridge_q, ridge_k, mask, eps_rel, EIGH_ROUTE_EPS_ABS),
               eps_rel, EIGH_ROUTE_EPS_ABS)
        note = getattr(adapter, "qk_selection_statistic", None)
        if rope is not None and note is not None:     # (a run without post-RoPE statistics: the entry is what it always was)
            note(layer_idx, SELECT_STATS["rope"][1] if by_rope else "pre_rope")
    record_error = getattr(adapter, "qk_error", None) if ops.qk_error_enabled() else None      # (... without this: no logit error)
    if record_error is not None:
        # what the selection loses of the logits, at every rank: the order of ALL units from one more scoring call (the mask above is
        # its prefix), then the curves on the RAW statistics (ridges 0: the stored rows are bit copies, so this is the artefact's
        # error) with the diagonal terms under the ridges the scores really use.  Enqueued only, read by report_qk_errors.
        ns, _ = ops.qk_units(mode, head_dim)
        order = ops.qk_select(sq, sk, head_dim, mode, *sel_ridges)[0][:, :ns].contiguous()
        record_error(layer_idx, ops.qk_rank_curve(cq, ck, mode, 0.0, 0.0, order, terms_ridges=(ridge_q, ridge_k)) + (order,), rank)
        record_rope = getattr(adapter, "qk_error_rope", None)
        if rope is not None and record_rope is not None:
            # the same curves along the SAME order on (sigma_q', sigma_k'): for a rotary model the exact mean-square logit change
            record_rope(layer_idx, ops.qk_rank_curve(rope[0], rope[1], mode, 0.0, 0.0, order, terms_ridges=(ridge_q, ridge_k)) + (order,),
                        rank)
        for select in ("seq", "causal"):
            # ... and on the within-sequence statistic: cov_q = P (then P_raw), cov_k = ones -- a product with 1.0 is exact, so the
            # curve is 1^T P[D,D] 1 over the dropped columns D, the part of the logit change softmax can see (then the whole of it);
            # and on the causal statistic, the same way: 1^T P^c[D,D] 1 is the variance of the logit change over the keys each
            # query can see, summed over the queries (then, on P^c_raw, the mean square over them)
            record_seq = getattr(adapter, "qk_error_" + select, None)
            if select in sequence and record_seq is not None:
                centred, raw = sequence[select]
                curves = ops.qk_rank_curve(centred, ones, mode, 0.0, 0.0, order)
                raw_curve = ops.qk_rank_curve(raw, ones, mode, 0.0, 0.0, order, want_greedy=False)[1]
                record_seq(layer_idx, curves + (order, raw_curve), rank)
    W_q = comps.query_proj.weight.detach().to(device=local_device(), dtype=torch.bfloat16)
    W_k = comps.key_proj.weight.detach().to(device=local_device(), dtype=torch.bfloat16)
    Q_heads = ops.gather_rows(W_q, q_rows)   # [n_heads*rank, d]
    K_heads = ops.gather_rows(W_k, k_rows)   # [n_kv*rank, d]
    if (arch == "llama" or "qwen" in arch) and slice_dims:
        rotary_masks.append(mask)
    weights = {"q_proj": Q_heads, "k_proj": K_heads}
    if bias and ops.keep_bias_enabled(arch):         # (MODEGPT_KEEP_BIAS=1, or Qwen2)
        # the bias entries at exactly the rows gathered above, in their order (compress_head_opt gathers them the same way,
        # compress_qk.py:439-476; the save_layer route upstream drops them): bit copies in the bias's own dtype
        for name, proj, rows in (("q_bias", comps.query_proj, q_rows), ("k_bias", comps.key_proj, k_rows)):
            b = getattr(proj, "bias", None)
            if b is not None:
                weights[name] = torch.index_select(b.detach().to(local_device()), 0, rows)
    adapter.save_layer(output_dir=adapter.config.temp_storage_dir, suffix="qk", weights=weights, layer_idx=layer_idx)
    return mask


def _kept_rows(head: Tensor, rows: Tensor, slice_dims: bool) -> Tensor:
    """head[rows] when slicing; otherwise a zero matrix of the head's shape with those rows copied (the reference's
    slice_dims=False convention: same shape, dropped rows zeroed)."""
    if slice_dims:
        return head[rows]
    out = torch.zeros_like(head)
    out[rows] = head[rows]
    return out


@torch.no_grad()
def compress_head_llama_grouped(kv_head_idx: int, kv_head_ratio: int, cov_q_layer, cov_k_layer, Wq_heads: Tensor,
                                Wk_heads: Tensor, Q_heads_out: list, K_heads_out: list, layer_rotary_mask: list, rank: int,
                                slice_dims=True, ridge_lambda=1e-4):
    """One kv head of a GQA layer (compress_qk.py:320-382): score the RoPE pairs over the group's query heads
    (K statistics with `ridge_lambda`, Q with sqrt_M's default), keep rank/2 pairs in score order, append the kept
    rows of K and of every query head of the group, and the mask.  Same kernel as compress_layer, one head at a time."""
    q0 = kv_head_idx * kv_head_ratio
    cq = torch.stack([c.to(device=local_device(), dtype=dtype_p) for c in cov_q_layer[q0:q0 + kv_head_ratio]])
    ck = cov_k_layer[kv_head_idx].to(device=local_device(), dtype=dtype_p)[None]
    mask, _, _ = ops.qk_select(cq, ck, rank, _lib.MDG_QK_ROPE_GROUPED, _SQRT_M_DEFAULT_RIDGE, ridge_lambda)
    rows = mask[0]
    K_heads_out.append(_kept_rows(Wk_heads[kv_head_idx], rows.to(Wk_heads.device), slice_dims))
    for Q_head in Wq_heads[q0:q0 + kv_head_ratio]:
        Q_heads_out.append(_kept_rows(Q_head, rows.to(Q_head.device), slice_dims))
    layer_rotary_mask.append(rows)


@torch.no_grad()
def compress_head_llama(C_q: Tensor, C_k: Tensor, Q_head: Tensor, K_head: Tensor, Q_heads_out: list, K_heads_out: list,
                        layer_rotary_mask: list, rank: int, slice_dims=True):
    """One head of an MHA Llama layer (compress_qk.py:387-436): default ridges for both statistics; the kept rows go
    to the lists as CPU bf16 tensors, as upstream."""
    cq = C_q.to(device=local_device(), dtype=dtype_p)[None]
    ck = C_k.to(device=local_device(), dtype=dtype_p)[None]
    mask, _, _ = ops.qk_select(cq, ck, rank, _lib.MDG_QK_ROPE_MHA, _SQRT_M_DEFAULT_RIDGE, _SQRT_M_DEFAULT_RIDGE)
    rows = mask[0]
    Q_heads_out.append(_kept_rows(Q_head, rows.to(Q_head.device), slice_dims).to(device="cpu", dtype=torch.bfloat16))
    K_heads_out.append(_kept_rows(K_head, rows.to(K_head.device), slice_dims).to(device="cpu", dtype=torch.bfloat16))
    layer_rotary_mask.append(rows)


@torch.no_grad()
def compress_head_opt(C_q: Tensor, C_k: Tensor, Q_head: Tensor, K_head: Tensor, bias_Q_head: Tensor, bias_K_head: Tensor,
                      out_Q_heads: list, out_K_heads: list, out_Q_bias: list, out_K_bias: list, rank: int):
    """One OPT head (compress_qk.py:439-476): score_j = |sqrt(Cq)[:, j]| * |sqrt(Ck)[:, j]|, top-`rank` columns in score
    order; rows (to the CPU, as upstream) and the matching bias entries are appended."""
    cq = C_q.to(device=local_device(), dtype=dtype_p)[None]
    ck = C_k.to(device=local_device(), dtype=dtype_p)[None]
    mask, _, _ = ops.qk_select(cq, ck, rank, _lib.MDG_QK_OPT, _SQRT_M_DEFAULT_RIDGE, _SQRT_M_DEFAULT_RIDGE)
    rows = mask[0]
    out_Q_heads.append(Q_head[rows.to(Q_head.device)].to(device="cpu"))
    out_K_heads.append(K_head[rows.to(K_head.device)].to(device="cpu"))
    out_Q_bias.append(bias_Q_head[rows.to(bias_Q_head.device)])
    out_K_bias.append(bias_K_head[rows.to(bias_K_head.device)])


def compress_qk_svd(adapter, cov_x, keep_ratios, rank=None, ridge_lambda=1, slice_dims=True):
    """Present upstream (compress_qk.py:16-150) but unreachable there: nothing calls it and its body ends in a call to
    an undefined name (`slice_QK_dims`), so it cannot run.  Not reproduced."""
    raise NotImplementedError("compress_qk_svd is dead code in the reference (calls the undefined slice_QK_dims); "
                              "use compress_qk")


@torch.no_grad()
def compress_qk(adapter: ModelAdapter, cov, keep_ratios, rank=None, slice_dims=True,
                target_layers: Optional[List[int]] = None):
    """compress_qk.py:152-201.  Returns the list of per-layer rotary masks (None when slice_dims is False)."""
    if target_layers is None:
        target_layers = list(range(adapter.n_layers))
    cov_q_list, cov_k_list = cov
    rotary_masks: List[Tensor] = []
    for i in target_layers:
        rank_i = qk_rank_rule(adapter.head_dim, keep_ratios[i], adapter.arch, rank)
        compress_layer(adapter, i, rank_i, cov_q_list=cov_q_list[i], cov_k_list=cov_k_list[i],
                       rotary_masks=rotary_masks, slice_dims=slice_dims)
        logger.info(f"[QK] Layer {i}: compressed to rank {rank_i} per head (CR-score + interpolation)")
    return rotary_masks if slice_dims else None
