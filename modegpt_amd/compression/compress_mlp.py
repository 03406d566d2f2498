"""MLP compression: ridge-leverage column selection + Nystrom refit of down_proj
(reference: src/compression/compress_mlp.py)."""
from __future__ import annotations

import logging

import torch
from torch import Tensor

from .. import ops
from ..adapters.model_adapter import MLPComponents, ModelAdapter
from ..model_utils import dtype_p, local_device
from ._window import over_layers

logger = logging.getLogger("MoDeGPT")


def _fl32(x: float) -> float:
    """The reference adds `ridge * torch.eye(n)` with a float32 eye (compress_mlp.py:18): the value that reaches
    the fp64 matrix is the fp32 rounding of lambda."""
    return float(torch.tensor(x, dtype=torch.float32).to(torch.float64))


def get_ridge_scores(C: Tensor, layer_idx: int, ridge_lambda=1e-2) -> Tensor:
    """diag((C + fl32(lambda) I)^-1)  (compress_mlp.py:13-25) -- blocked Cholesky + triangular inverse on the
    fp64 MFMA, column norms of L^-1 instead of forming the inverse."""
    C = C.to(dtype=dtype_p, device=local_device())
    return ops.ridge_scores(C, _fl32(ridge_lambda))


I8_GUARANTEED_EPS = 1.1e-11      # mdg_cov_accum_i8: entry-wise over sqrt(sigma_ii sigma_jj), for any input, at tolerance factor 1


def covariance_error_eps(adapter, n_features: int) -> float:
    """The entry-wise relative error bound eps of the sigma_mlp this run accumulated, |sigma_ij - exact| <= eps sqrt(sigma_ii sigma_jj)
    -- what the selection certificate is taken against.  `adapter.cov_error_eps` when the caller states it; else from the route
    the statistics TOOK -- `adapter.cov_routes`, the device's own counts (ops.i8_route_counts) that calibration leaves there:
    no statistic on the int8 digit planes (an fp32 model, a narrow one, OPT's fc1 statistic below 4096 features, MODEGPT_COV_MODE=f64)
    -> the worst case of an fp64 sum of exact products over the calibration tokens, (tokens / 4 + 4) 2^-53 (v_mfma_f64_16x16x4 adds
    four products per step; typical errors are ~sqrt of that count: 6e-14 at 10^6 tokens); some on them -> the route's guarantee
    1.1e-11 x the tolerance factor (+ one fp64 rounding per fold); a mix -- a statistic or single columns fell back to fp64 -- the
    larger of the two.  A statistic of a width the int8 route never takes is on fp64 whatever the counts say.  Without counts (no
    calibration ran on this adapter) the route is predicted from the mode, the width and the hook the architecture uses."""
    stated = getattr(adapter, "cov_error_eps", None)
    if stated is not None:
        return float(stated)
    tokens = int(getattr(adapter, "calib_tokens", 0) or getattr(adapter.config, "calib_size", 32) * 2048)
    eps_f64 = (tokens / 4 + 4) * 2.0 ** -53
    eps_i8 = I8_GUARANTEED_EPS * ops.i8_tolerance() + 64 * 2.0 ** -53
    if not ops.takes_i8_planes(n_features):
        return eps_f64
    # (OPT's fc1 statistic goes through ops.cov_accum_fc_relu, ReLU on load: the int8 planes from ops.FC_I8_MIN_FEATURES features only)
    takes_i8 = ops.takes_i8_planes(n_features, relu=getattr(adapter, "arch", None) == "opt")
    routes = getattr(adapter, "cov_routes", None)
    if routes is None:
        return eps_i8 if ops.COV_MODE == "i8" and takes_i8 else eps_f64
    if routes.get("i8_5", 0) + routes.get("i8_6", 0) == 0:
        return eps_f64
    if not takes_i8:
        return max(eps_i8, eps_f64)      # (the counts are another statistic's, sigma_x's: OPT's fc1 statistic of this width ran on fp64)
    return max(eps_i8, eps_f64) if routes.get("fallback_f64", 0) or routes.get("fp64_columns", 0) else eps_i8


@torch.no_grad()
def compress_weights(comps: MLPComponents, C: Tensor, keep_ratio: float, layer_idx: int, ridge_lambda: float,
                     margin_eps: float = None, margin_out: list = None, curve_out: list = None, error_out: list = None,
                     bias_out: dict = None, intercept: Tensor = None, intercept_out: list = None, carry_bias: bool = True,
                     greedy_out: list = None):
    """compress_mlp.py:28-64.  Returns (W_u'^T [d, r], W_d' [r, d], W_g'^T [d, r] or None, rank), bf16 --
    the same orientation the reference returns (transposed views of the saved layout).
    margin_eps / margin_out (not upstream): with both given, the certificate of the rank selection against an entry-wise relative
    error margin_eps of C (ops.select_margin: 8 numbers on the device) is appended to margin_out -- two more passes over the
    triangular inverse the scores come from, nothing else changes.
    curve_out (not upstream): a list, with MODEGPT_RANK_CURVE=1 -- the layer's error-versus-rank curve (ops.nystrom_rank_curve, n + 1
    numbers on the device) is appended to it, enqueued behind the refit; the outputs are the same bits with or without it.
    error_out (not upstream): a list, with MODEGPT_OUTPUT_ERROR=1 -- (q, e, unorm2), d numbers each on the device
    (ops.mlp_output_error: the output energy of the uncompressed weights, the output error and the squared residual norm per channel
    of the bf16 tensor this call RETURNS, not of the fp64 solution) are appended to it; the outputs are the same bits either way.
    bias_out (not upstream's save route, which drops every bias; its in-place slice_gate_dims keeps these three): a dict -- the biases
    the projections have go into it as "up_bias" / "gate_bias" (the entries at the selected columns, in their order) and "down_bias"
    (unchanged without `intercept`: the linear refit has none), bit copies in the bias's own dtype; the weights are the same bits
    either way.  carry_bias=False: bias_out receives nothing but the intercept below (the caller does not carry biases).
    intercept (not upstream; DESIGN.md section 7, "The MLP intercept"): mu = E[h] [n] fp64, normalised as C is -- the refit is taken
    on the centred statistic S = C - mu mu^T (ops.cov_center into a buffer of its own; C is not modified) and
    bias_out["down_bias"] = b_d + W_d mu - D^ mu_k for the bf16 tensor D^ this call RETURNS (ops.nystrom_intercept; b_d = the
    projection's bias with carry_bias, else 0; in the bias's dtype, else the weight's), so bias_out is required.  Scores, idx, up and
    gate still come from C and are the same bits with and without it; the curve and the output error are taken on S, where they
    are the affine map's.  intercept_out: a list -- the two norms (||delta||^2, ||W_d mu||^2, on the device) are appended to it.
    MODEGPT_MLP_GREEDY=T (not upstream; DESIGN.md section 7, "Greedy MLP selection"): idx = the sorted picks of T rounds of
    block-greedy descent on the refit's objective (ops.nystrom_greedy_select on the uncentred C, eps = 1e-6) instead of the ridge
    rule; up, gate, the refit, the biases and the intercept run on that idx as before.  The ridge scores are then computed only
    for the rank curve, which runs along the greedy order followed by the unselected columns in ridge-score order; no certificate
    is computed (margin_out stays empty).  greedy_out: a list -- (objective, cut, n_dead, ridge_at_rank, greedy_at_rank), on the
    device, are appended to it; the last two are the ridge order's and this order's curve at `rank`, None without the curve."""
    C = C.to(dtype=dtype_p, device=local_device())
    if intercept is not None and bias_out is None:
        raise ValueError("compress_weights: intercept= needs bias_out= to leave the down_bias in")
    rank = int(C.shape[0] * keep_ratio)
    greedy_rounds = ops.mlp_greedy_rounds()                           # (MODEGPT_MLP_GREEDY: 0 = off, the reference's rule below)
    scores = greedy = None
    if greedy_rounds:
        # block-greedy descent on the refit's own objective, on the uncentred C with the refit's eps; no ridge scores, no certificate
        W_sel = comps.down_proj.weight.detach().to(device=local_device())
        greedy = ops.nystrom_greedy_select(C, W_sel, rank, greedy_rounds, eps=1e-6)
        idx = torch.sort(greedy[0]).values
    elif margin_out is not None and margin_eps is not None:
        scores, sens = ops.ridge_scores(C, _fl32(ridge_lambda), want_sens=True)
        idx = ops.select_smallest_sorted(scores, rank)
        margin_out.append(ops.select_margin(scores, sens, idx, margin_eps))
    else:
        scores = get_ridge_scores(C, layer_idx=layer_idx, ridge_lambda=ridge_lambda)
        idx = ops.select_smallest_sorted(scores, rank)                # topk(largest=False) + sort  (:45-47)
    W_u = comps.up_proj.weight.detach().to(device=local_device(), dtype=torch.bfloat16)
    up = ops.gather_rows(W_u, idx)                                    # W_u[topk, :]               (:49)
    gate = None
    if comps.gate_proj is not None:
        W_g = comps.gate_proj.weight.detach().to(device=local_device(), dtype=torch.bfloat16)
        gate = ops.gather_rows(W_g, idx)                              # W_g[topk, :]               (:50)
    W_d = comps.down_proj.weight.detach().to(device=local_device())              # bf16 as is; fp16/fp32 widen exactly to fp64
    C_sel = C                                                         # (the statistic every selection is taken on)
    if intercept is not None:
        mu = intercept.to(dtype=dtype_p, device=local_device())
        C = ops.cov_center(C, mu)                                    # S: from here on the statistic of h - mu (selection is done)
    down = ops.nystrom_down(C, idx, W_d, eps=1e-6)                    # [d, r] bf16                (:52-62)
    at_rank = (None, None)
    if curve_out is not None and ops.rank_curve_enabled():
        # the selection is a prefix of the ridge-score order (ties: lower index first, NaN last, as select_smallest_sorted ranks them),
        # so the factor of sigma_mlp in that order holds the refit's residual energy at every rank, this layer's included
        if scores is None:                                            # (the greedy selection skipped them)
            scores = get_ridge_scores(C_sel, layer_idx=layer_idx, ridge_lambda=ridge_lambda)
        order = torch.argsort(scores, stable=True)
        if greedy is not None:
            # the curve runs along the greedy order, then the unselected columns in ridge-score order (a stable sort on "unselected"
            # keeps that order: no host round trip); the curve along the plain ridge order gives the rule's value at this rank
            ridge_curve = ops.nystrom_rank_curve(C, order, W_d, eps=1e-6)
            unselected = torch.ones(C.shape[0], dtype=torch.int64, device=C.device)
            unselected[greedy[0]] = 0
            rest = order[torch.argsort(unselected[order], stable=True)][rank:]
            order = torch.cat((greedy[0], rest))
        curve_out.append(ops.nystrom_rank_curve(C, order, W_d, eps=1e-6))
        if greedy is not None:
            at_rank = (ridge_curve[rank], curve_out[-1][rank])
    if greedy is not None and greedy_out is not None:
        greedy_out.append(greedy[1:] + at_rank)                      # (objective, cut, n_dead, ridge_at_rank, greedy_at_rank)
    if error_out is not None and ops.output_error_enabled():
        q = ops.mlp_output_error(C, W_d, None, None)                  # the channel's energy: nothing subtracted
        e, unorm2 = ops.mlp_output_error(C, W_d, idx, down, want_unorm2=True)     # ... and what the tensor that is saved loses of it
        error_out.extend((q, e, unorm2))
    if bias_out is not None and carry_bias:
        for name, proj, rows in (("up_bias", comps.up_proj, idx), ("gate_bias", comps.gate_proj, idx), ("down_bias", comps.down_proj, None)):
            b = getattr(proj, "bias", None)
            if b is not None:
                b = b.detach().to(local_device())
                bias_out[name] = b.clone() if rows is None else torch.index_select(b, 0, rows.to(torch.int64))
    if intercept is not None:
        b_d = getattr(comps.down_proj, "bias", None) if carry_bias else None
        b_d = None if b_d is None else b_d.detach().to(local_device())
        bias, _, norms = ops.nystrom_intercept(W_d, down, idx, mu, b_d=b_d)
        bias_out["down_bias"] = bias
        if intercept_out is not None:
            intercept_out.append(norms)
    return up.T, down.T, (None if gate is None else gate.T), rank


@torch.no_grad()
def compress_nystrom(adapter: ModelAdapter, cov, keep_ratios, target_layers, ridge_lambda=1e-4):
    """Per-layer driver (compress_mlp.py:67-117).  As upstream, the ridge actually used is
    adapter.config.nystrom_ridge; the `ridge_lambda` argument is ignored."""
    def enqueue(layer_idx):
        # the layer's whole chain (two Cholesky factorisations, selection, gathers, Nystrom solve) enqueues without a host round
        # trip; the not-positive-definite status of both factorisations is read once (adapter.chain_status)
        comps = adapter.get_mlp_components(layer_idx)
        record = getattr(adapter, "selection_margin", None)          # (a duck-typed adapter without it: no certificate)
        record_curve = getattr(adapter, "rank_curve", None)          # (... and without this: no error-versus-rank curve)
        curve = [] if callable(record_curve) else None               # (filled only with MODEGPT_RANK_CURVE=1)
        record_error = getattr(adapter, "output_error", None)        # (... and without this: no realised output error)
        error = [] if callable(record_error) else None               # (filled only with MODEGPT_OUTPUT_ERROR=1)
        carry = ops.keep_bias_enabled(getattr(adapter, "arch", None))                      # (MODEGPT_KEEP_BIAS=1, or Qwen2)
        more = {}
        if ops.mlp_intercept_enabled():                                                     # (MODEGPT_MLP_INTERCEPT=1)
            means = getattr(adapter, "mlp_means", None)
            if means is None or means[layer_idx] is None:
                raise RuntimeError(f"MODEGPT_MLP_INTERCEPT=1 but layer {layer_idx} has no activation mean (adapter.mlp_means): "
                                   "the statistics were collected without the switch")
            more = {"intercept": means[layer_idx], "intercept_out": [], "carry_bias": carry}
        biases = {} if carry or more else None
        record_greedy = getattr(adapter, "mlp_greedy", None)         # (... and without this: the greedy selection reports nothing)
        if ops.mlp_greedy_rounds():                                  # (MODEGPT_MLP_GREEDY=T; unset: no list, nothing recorded)
            more["greedy_out"] = []
        if record is None:
            result = compress_weights(comps, cov[layer_idx], keep_ratios[layer_idx], layer_idx=layer_idx,
                                      ridge_lambda=adapter.config.nystrom_ridge, curve_out=curve, error_out=error, bias_out=biases,
                                      **more)
        else:
            eps, margin = covariance_error_eps(adapter, cov[layer_idx].shape[0]), []
            result = compress_weights(comps, cov[layer_idx], keep_ratios[layer_idx], layer_idx=layer_idx,
                                      ridge_lambda=adapter.config.nystrom_ridge, margin_eps=eps, margin_out=margin, curve_out=curve,
                                      error_out=error, bias_out=biases, **more)
            # the selection's certificate stays on the device until the adapter next waits for the chain (report_selection_margins)
            if margin:                                               # (empty under the greedy selection: it has no certificate)
                record(layer_idx, margin[0], eps)
        if more.get("greedy_out") and callable(record_greedy):
            record_greedy(layer_idx, more["greedy_out"][0], result[3])       # ... and the descent's numbers (report_mlp_greedy)
        if curve:
            record_curve(layer_idx, curve[0], result[3])             # ... and so does the curve (report_rank_curves)
        if error:
            record_error(layer_idx, tuple(error), result[3])         # ... and the stored tensor's output error (report_output_errors)
        record_intercept = getattr(adapter, "mlp_intercept", None)
        if more.get("intercept_out") and callable(record_intercept):
            record_intercept(layer_idx, more["intercept_out"][0])    # ... and the intercept's two norms (report_mlp_intercepts)
        return result + (biases or {},)

    def retire(layer_idx, result):
        up_T, down_T, gate_T, rank, biases = result
        logger.info(f"[MLP] Layer {layer_idx}  compressed to rank {rank}")
        weights = {"up": up_T.T, "down": down_T.T}
        if gate_T is not None:
            weights["gate"] = gate_T.T
        weights.update(biases)
        adapter.save_layer(output_dir=adapter.config.temp_storage_dir, suffix="mlp", weights=weights,
                           layer_idx=layer_idx)

    over_layers(adapter, list(target_layers), enqueue, retire)      # (CHAIN_WIDTH layers' chains in flight, artefacts in layer order)
