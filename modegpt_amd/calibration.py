"""Calibration pass: one sweep of the model over the calibration batches during which adapter hooks stream every
target layer's activations into the HIP covariance kernel, plus Block-Influence scores from the hidden states.

Public entry point and return contract follow the reference (src/calibration.py:18-36):
    load_calibs(adapter, n_samples, batch_size, dataset, load_calibs_from, calibs_save_path, target_layers)
        -> (cov_mlp, cov_q, cov_k, cov_x, bi_scores)
each cov_* a list with one fp64 device tensor per layer (None outside target_layers), bi_scores a list of floats
for ALL layers.  Internals differ: sigma buffers are lower-triangular until one fused mirror+normalise pass at the
end, and the BI running sums stay on the device (one host sync per calibration, not one per layer per batch).
"""
from __future__ import annotations

import logging
import random
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .adapters.model_adapter import ModelAdapter
from .model_utils import dtype_p, local_device

logger = logging.getLogger("MoDeGPT")

np.random.seed(1234)
random.seed(1234)

# The normaliser is n_texts * 2048 whatever the real sequence length is (src/calibration.py:141).
TOKENS_PER_TEXT_NORMALISER = 2048


QK_ROPE_ARCHS = ("llama", "qwen2")      # rotary models whose compressed attention keeps the dropped-column identity


def qk_rope_collected(adapter: ModelAdapter, log=None) -> bool:
    """Whether this run collects (or loads) the post-RoPE statistics sigma_q', sigma_k': MODEGPT_QK_ROPE=1 on a Llama / Qwen2
    adapter.  With the switch on any other architecture nothing is collected and, given a logger, one line says why."""
    if not ops.qk_rope_enabled():
        return False
    arch = adapter.arch
    if arch in QK_ROPE_ARCHS:
        return True
    if log is not None:
        if "qwen" in arch:
            log.warning(f"MODEGPT_QK_ROPE=1 ignored for {arch}: the compressed model renormalises q / k over the kept columns (masked "
                        "RMSNorm), so the dropped-column identity of the post-RoPE statistic does not hold; nothing is collected")
        else:
            log.info(f"MODEGPT_QK_ROPE=1: {arch} has no rotary embedding, the pre-RoPE statistic is already the exact one; nothing "
                     "more is collected")
    return False


def qk_seq_collected(adapter: ModelAdapter, log=None) -> bool:
    """Whether this run collects (or loads) the within-sequence Q/K statistic P, P_raw: MODEGPT_QK_SEQ=1 on a Llama / Qwen2 adapter
    that collects the post-RoPE statistics too -- the statistic is taken on the rotated rows the post-RoPE flush produces, so
    MODEGPT_QK_SEQ=1 without MODEGPT_QK_ROPE=1 raises there.  On any other architecture nothing is collected and, given a logger,
    one line says why."""
    if not ops.qk_seq_enabled():
        return False
    arch = adapter.arch
    if arch in QK_ROPE_ARCHS:
        if not ops.qk_rope_enabled():
            raise RuntimeError("MODEGPT_QK_SEQ=1 needs MODEGPT_QK_ROPE=1: the within-sequence Q/K statistic is accumulated from the "
                               "post-RoPE rows, which are only produced when the post-RoPE statistics are collected")
        if adapter.head_dim > 128:
            raise RuntimeError(f"MODEGPT_QK_SEQ=1: head_dim {adapter.head_dim} > 128 is not supported by mdg_qk_pair_accum")
        return True
    if log is not None:
        if "qwen" in arch:
            log.warning(f"MODEGPT_QK_SEQ=1 ignored for {arch}: the compressed model renormalises q / k over the kept columns (masked "
                        "RMSNorm), so the dropped-column identity of the within-sequence statistic does not hold; nothing is collected")
        else:
            log.info(f"MODEGPT_QK_SEQ=1: {arch} has no rotary embedding and separate q / k hooks; the within-sequence statistic is "
                     "not collected for it")
    return False


def qk_causal_collected(adapter: ModelAdapter, log=None) -> bool:
    """Whether this run collects (or loads) the causal Q/K statistic P^c, P^c_raw: MODEGPT_QK_CAUSAL=1 on a Llama / Qwen2 adapter
    that collects the post-RoPE statistics too -- the statistic is taken on the rotated rows the post-RoPE flush produces, so
    MODEGPT_QK_CAUSAL=1 without MODEGPT_QK_ROPE=1 raises there.  Independent of MODEGPT_QK_SEQ.  On any other architecture nothing
    is collected and, given a logger, one line says why."""
    if not ops.qk_causal_enabled():
        return False
    arch = adapter.arch
    if arch in QK_ROPE_ARCHS:
        if not ops.qk_rope_enabled():
            raise RuntimeError("MODEGPT_QK_CAUSAL=1 needs MODEGPT_QK_ROPE=1: the causal Q/K statistic is accumulated from the "
                               "post-RoPE rows, which are only produced when the post-RoPE statistics are collected")
        if adapter.head_dim > 128:
            raise RuntimeError(f"MODEGPT_QK_CAUSAL=1: head_dim {adapter.head_dim} > 128 is not supported by mdg_qk_causal_accum")
        return True
    if log is not None:
        if "qwen" in arch:
            log.warning(f"MODEGPT_QK_CAUSAL=1 ignored for {arch}: the compressed model renormalises q / k over the kept columns (masked "
                        "RMSNorm), so the dropped-column identity of the causal statistic does not hold; nothing is collected")
        else:
            log.info(f"MODEGPT_QK_CAUSAL=1: {arch} has no rotary embedding and separate q / k hooks; the causal statistic is "
                     "not collected for it")
    return False


class SigmaBuffers:
    """The four statistic families of the target layers (shapes: src/calibration.py:82-96)."""

    KINDS = ("mlp", "q", "k", "x")
    ROPE_KINDS = ("q_rope", "k_rope")

    def __init__(self, adapter: ModelAdapter, target_layers: Sequence[int], device=None):
        L = adapter.n_layers
        hd, d, f = adapter.head_dim, adapter.d_model, adapter.get_n_inner()
        shapes = {"mlp": (f, f), "q": (adapter.n_heads, hd, hd), "k": (adapter.n_kv_heads, hd, hd), "x": (d, d)}
        self.lists: Dict[str, List[Optional[torch.Tensor]]] = {k: [None] * L for k in self.KINDS}
        self.layers = list(target_layers)
        device = device or local_device()          # this rank's own GPU (calib_device upstream: src/calibration.py:83)
        for i in self.layers:
            for kind, shp in shapes.items():
                self.lists[kind][i] = torch.zeros(*shp, dtype=dtype_p, device=device)
        # the column sums of the sigma_mlp activation (MODEGPT_MLP_INTERCEPT=1: the means of the mean-aware refit); None without it
        self.mlp_sums: Optional[List[Optional[torch.Tensor]]] = None
        if ops.mlp_intercept_enabled():
            self.mlp_sums = [None] * L
            for i in self.layers:
                self.mlp_sums[i] = torch.zeros(f, dtype=dtype_p, device=device)
        # ... and of x, the post-norm hidden state (MODEGPT_VO_INTERCEPT=1: the means of the mean-aware V/O truncation); None without it
        self.x_sums: Optional[List[Optional[torch.Tensor]]] = None
        if ops.vo_intercept_enabled():
            self.x_sums = [None] * L
            for i in self.layers:
                self.x_sums[i] = torch.zeros(d, dtype=dtype_p, device=device)
        # the per-head Grams of the post-RoPE rows q', k' (MODEGPT_QK_ROPE=1 on a rotary model): the shapes of q / k; None without it
        self.q_rope: Optional[List[Optional[torch.Tensor]]] = None
        self.k_rope: Optional[List[Optional[torch.Tensor]]] = None
        if qk_rope_collected(adapter, logger):
            self.q_rope, self.k_rope = [None] * L, [None] * L
            for i in self.layers:
                self.q_rope[i] = torch.zeros(*shapes["q"], dtype=dtype_p, device=device)
                self.k_rope[i] = torch.zeros(*shapes["k"], dtype=dtype_p, device=device)

        # the within-sequence Q/K statistic and its uncentred twin (MODEGPT_QK_SEQ=1 beside MODEGPT_QK_ROPE=1 on a rotary model): per
        # layer [n_heads, hd, hd], both triangles; None without it
        self.qk_pair: Optional[List[Optional[torch.Tensor]]] = None
        self.qk_pair_raw: Optional[List[Optional[torch.Tensor]]] = None
        if qk_seq_collected(adapter, logger):
            self.qk_pair, self.qk_pair_raw = [None] * L, [None] * L
            for i in self.layers:
                self.qk_pair[i] = torch.zeros(*shapes["q"], dtype=dtype_p, device=device)
                self.qk_pair_raw[i] = torch.zeros(*shapes["q"], dtype=dtype_p, device=device)

        # the causal Q/K statistic and its uncentred twin (MODEGPT_QK_CAUSAL=1 beside MODEGPT_QK_ROPE=1 on a rotary model): per layer
        # [n_heads, hd, hd], both triangles; None without it
        self.qk_causal: Optional[List[Optional[torch.Tensor]]] = None
        self.qk_causal_raw: Optional[List[Optional[torch.Tensor]]] = None
        if qk_causal_collected(adapter, logger):
            self.qk_causal, self.qk_causal_raw = [None] * L, [None] * L
            for i in self.layers:
                self.qk_causal[i] = torch.zeros(*shapes["q"], dtype=dtype_p, device=device)
                self.qk_causal_raw[i] = torch.zeros(*shapes["q"], dtype=dtype_p, device=device)

    @property
    def qk_causals(self):
        """(qk_causal, qk_causal_raw), or None without the switch."""
        return None if self.qk_causal is None else (self.qk_causal, self.qk_causal_raw)

    @property
    def qk_pairs(self):
        """(qk_pair, qk_pair_raw), or None without the switch."""
        return None if self.qk_pair is None else (self.qk_pair, self.qk_pair_raw)

    @property
    def qk_rope(self):
        """(q_rope, k_rope), or None without the switch."""
        return None if self.q_rope is None else (self.q_rope, self.k_rope)

    def finalize(self, n_texts: int) -> None:
        """sigma <- sigma / (n_texts * 2048), lower triangle mirrored into the upper (src/calibration.py:141-146)."""
        scale = 1.0 / (n_texts * TOKENS_PER_TEXT_NORMALISER)
        for i in self.layers:
            for kind in self.KINDS:
                ops.cov_finalize(self.lists[kind][i], scale)
            if self.mlp_sums is not None:
                self.mlp_sums[i].mul_(scale)                 # mu = E[h] under the normaliser sigma_mlp gets: one rounding per entry
            if self.x_sums is not None:
                self.x_sums[i].mul_(scale)                   # mu = E[x] under sigma_x's normaliser, likewise
            if self.q_rope is not None:
                ops.cov_finalize(self.q_rope[i], scale)      # the same mirror + normaliser as sigma_q / sigma_k
                ops.cov_finalize(self.k_rope[i], scale)
            if self.qk_pair is not None:
                # the token normaliser squared: the mean over the within-sequence pairs in the unit of <sigma_q', sigma_k'> (one
                # rounding per entry, the same for both triangles)
                pair_scale = 1.0 / (n_texts * TOKENS_PER_TEXT_NORMALISER ** 2)
                self.qk_pair[i].mul_(pair_scale)
                self.qk_pair_raw[i].mul_(pair_scale)
            if self.qk_causal is not None:
                # every query row carries a mean over its keys already, so ONE token normaliser: the mean over the queries of the
                # variance over the keys each can see, in the unit of the within-sequence figure (one rounding per entry)
                causal_scale = 1.0 / (n_texts * TOKENS_PER_TEXT_NORMALISER)
                self.qk_causal[i].mul_(causal_scale)
                self.qk_causal_raw[i].mul_(causal_scale)


class BlockInfluence:
    """bi[l] = (1/n_texts) * sum over batches of mean_T sum_B (1 - cos(h_l, h_{l+1}))  (src/calibration.py:118-136)."""

    def __init__(self, n_layers: int, device=None):
        self.n_layers = n_layers
        device = device or local_device()
        self.acc = torch.zeros(n_layers, dtype=torch.float64, device=device)

    def add_batch(self, hidden_states) -> None:
        T = hidden_states[0].shape[1]
        step = torch.zeros_like(self.acc)
        for l in range(self.n_layers):
            ops.bi_accum(step[l:l + 1], hidden_states[l], hidden_states[l + 1])
        self.acc += step / T

    def scores(self, n_texts: int) -> List[float]:
        return [v / n_texts for v in self.acc.cpu().tolist()]


class StopForward(Exception):
    """Raised by a forward hook behind the last layer a rank owns: the rest of the model forward is not needed there."""


def _stop_forward(module, args, output):
    raise StopForward()


def load_calibs(adapter: ModelAdapter, n_samples: int, batch_size: int, dataset: str = "wikitext",
                load_calibs_from="", calibs_save_path="", target_layers: List[int] = []):
    """load_calibs_from / calibs_save_path (declared and never read upstream, src/calibration.py:23-24): a directory of per-layer
    statistic records (calib_cache.py).  With calibs_save_path the target layers' statistics are written there after calibration;
    with load_calibs_from they are read from there and the model is not run at all; with both, loaded and written again (a copy or
    a subset).  The return value is the same five-tuple in every case."""
    if not load_calibs_from and not calibs_save_path:
        return _calibrate_model(adapter, n_samples=n_samples, batch_size=batch_size, dataset=dataset,
                                target_layers=target_layers)
    from . import calib_cache
    loaded = None
    if load_calibs_from:
        calibs, loaded = calib_cache.load(adapter, load_calibs_from, n_samples, batch_size, dataset, target_layers)
    else:
        calibs = _calibrate_model(adapter, n_samples=n_samples, batch_size=batch_size, dataset=dataset,
                                  target_layers=target_layers)
    if calibs_save_path:
        calib_cache.save(adapter, calibs_save_path, calibs, n_samples, batch_size, dataset, target_layers, loaded)
    return calibs


@torch.no_grad()
def _calibrate_model(adapter: ModelAdapter, n_samples: int, batch_size: int, target_layers: List[int] = [],
                     dataset="wikitext"):
    model = adapter.model
    targets = list(target_layers) if target_layers else list(range(adapter.n_layers))
    if getattr(adapter, "calib_no_hooks", False):      # a sharded rank that owns no layer of this chunk (BI only, or nothing)
        targets = []
    if adapter.calibs is None:
        from .eval import load_calibration_texts
        adapter.calibs = load_calibration_texts(calib_size=n_samples, model=model, tokenizer=adapter.tokenizer,
                                                batch_size=batch_size, dataset=dataset)
    logger.info(f"Detected architecture: {adapter.arch}")
    logger.info(f"target_layers = {targets}")
    logger.info("Calibrating model")

    sig = SigmaBuffers(adapter, targets)
    bi = BlockInfluence(adapter.n_layers)
    blocks = adapter.get_transformer_blocks()
    handles: list = []
    adapter.mlp_sums = sig.mlp_sums                      # (read by register_hooks; None without MODEGPT_MLP_INTERCEPT=1)
    adapter.x_sums = sig.x_sums                          # (likewise; None without MODEGPT_VO_INTERCEPT=1)
    adapter.qk_rope_sums = sig.qk_rope                   # (likewise; None without MODEGPT_QK_ROPE=1 on a rotary model)
    adapter.qk_pair_sums = sig.qk_pairs                  # (likewise; None without MODEGPT_QK_SEQ=1 beside it)
    adapter.qk_causal_sums = sig.qk_causals              # (likewise; None without MODEGPT_QK_CAUSAL=1 beside it)
    for i in targets:
        adapter.register_hooks(i, blocks[i], cov_mlp_list=sig.lists["mlp"], cov_q_list=sig.lists["q"],
                               cov_k_list=sig.lists["k"], cov_x_list=sig.lists["x"], handles=handles, logger=logger)
    # A sharded run (run_modegpt.compress_chunk) sets two attributes on the adapter: calib_stop_after = the last layer this rank
    # needs activations of -- the forward is cut right behind it -- and calib_want_bi = whether this rank is the one that
    # computes the BI scores (they need every layer's hidden state, i.e. the full forward; the others receive them).
    stop_after = getattr(adapter, "calib_stop_after", None)
    want_bi = getattr(adapter, "calib_want_bi", True)
    if want_bi:
        stop_after = None
    if stop_after is not None:
        handles.append(blocks[stop_after].register_forward_hook(_stop_forward))
    hidden_states_before = getattr(model.config, "output_hidden_states", False)
    model.config.output_hidden_states = bool(want_bi)
    model.eval()
    n_texts = n_tokens = 0
    try:
        for batch in adapter.calibs:
            n_texts += len(batch)
            n_tokens += int(batch.numel()) if hasattr(batch, "numel") else 0
            try:
                out = model(batch, output_hidden_states=bool(want_bi))
            except StopForward:
                continue
            if want_bi:
                bi.add_batch(out.hidden_states)
            del out
    finally:
        for h in handles:
            h.remove()
        model.config.output_hidden_states = hidden_states_before     # (the caller's model goes back as it came)
    bi_scores = bi.scores(n_texts) if want_bi else None
    adapter.bi_scores = bi_scores
    adapter.calib_tokens = n_tokens       # (how many tokens each statistic summed over: the fp64 route's rounding bound scales with it)
    sig.finalize(n_texts)
    adapter.mlp_sums = None
    adapter.mlp_means = sig.mlp_sums                     # per target layer mu = E[h] (None without the switch): compress_nystrom reads it
    adapter.x_sums = None
    adapter.x_means = sig.x_sums                         # per target layer mu = E[x] (None without the switch): compress_vo reads it
    adapter.qk_rope_sums = None
    adapter.qk_rope_stats = sig.qk_rope                  # (sigma_q', sigma_k') lists (None without the switch): compress_qk reads them
    adapter.qk_pair_sums = None
    adapter.qk_pair_stats = sig.qk_pairs                 # (P, P_raw) lists (None without the switch): compress_qk reads them
    adapter.qk_causal_sums = None
    adapter.qk_causal_stats = sig.qk_causals             # (P^c, P^c_raw) lists (None without the switch): compress_qk reads them
    adapter.cov_routes = None  # (counts of an earlier calibration do not describe this one)
    if ops.COV_MODE == "i8":   # the route of every large-statistic launch was picked on the device; read the tally once
        if ops.I8_ROWS:        # (before the reset below, which clears this counter too)
            adapter.cov_rows_left = ops.i8_rows_left()
            logger.info(f"token rows handed to the fp64 row kernel (MODEGPT_I8_ROWS): {adapter.cov_rows_left}")
        adapter.cov_routes = ops.i8_route_counts(reset=True)
        logger.info(f"covariance routes (int8 five planes / six planes / fp64 fallback): {adapter.cov_routes}")
    logger.info("Finished calibration and computed BI scores.")
    return sig.lists["mlp"], sig.lists["q"], sig.lists["k"], sig.lists["x"], bi_scores


__calibrate_model = _calibrate_model  # the reference's (name-mangled) spelling
