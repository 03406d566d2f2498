"""The model-adapter plug-in surface (reference: src/adapters/model_adapter.py).

Same class / method / property names and argument meanings, so adapters written against the reference ABC
drop in.  What differs is underneath: the statistic hooks hand the activation's device pointer to the HIP
covariance kernel (ops.cov_accum -> mdg_cov_accum) instead of upcasting to fp64 and calling torch matmul.
Between hook calls a sigma buffer holds only its LOWER triangle; `load_calibs` mirrors and normalises it
once at the end (mdg_cov_finalize).
"""
from __future__ import annotations

import logging
import math
import os
from abc import ABC, abstractmethod
from typing import Any, List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .. import ops
from . import metrics as _metrics
from .CompressionConfig import CompressionConfig
from .components import (AttentionComponents, MLPComponents, MLPTensors, QKComponents, QKTensors,  # noqa: F401
                         VOComponents, VOTensors)


def build_metrics(_all_metrics: dict) -> dict:
    """Kept for callers of the reference's helper; the store itself lives in adapters/metrics.py."""
    m = _metrics.new_run()
    _all_metrics[m["RunName"]] = m
    return m


def _show(v) -> str:
    return "n/a" if v is None else f"{v:.3e}"


def _shift_share(m: dict) -> str:
    return f"({_show(m['relative_error'])} of its energy); {_show(m['shift_share'])} of the uncentred change is invisible to softmax"


# What report_qk_errors reads, in this order: (pending record, attribute the host copies are kept under, metrics key, decoder in ops,
# the entry's "statistic", whether entry 7 of the record -- the curve on the uncentred statistic -- goes to the decoder, the log line
# behind "[QK] Layer l: rank r: " from the entry and the layer's pre-RoPE relative error).  The pre-RoPE row comes first: the post-RoPE
# entries quote its figure; the causal row comes behind the within-sequence one: its decoder takes that entry as seq=.
_QK_REPORTS = (
    ("_qk_errors", "qk_errors", "qk_logit_error", "decode_qk_logit_error", None, False,
     lambda m, pre: f"the kept columns lose {m['relative_error']:.3e} of the logit energy"
     + ("" if m["diagonal_ratio"] is None else f"; the diagonal rule's estimate is {m['diagonal_ratio']:.3g} x that")
     + ("" if m["greedy_relative_error"] is None else f"; a greedy order on the full objective loses {m['greedy_relative_error']:.3e}")
     + ("; NOT monotone in the rank" if m["non_monotone"] else "")),
    ("_qk_errors_rope", "qk_errors_rope", "qk_logit_error_rope", "decode_qk_logit_error", "post_rope", False,
     lambda m, pre: f"of the post-RoPE logit energy the kept columns lose {_show(m['relative_error'])} (exact for a rotary model); "
     f"the pre-RoPE statistic said {_show(pre)}"),
    ("_qk_errors_seq", "qk_errors_seq", "qk_logit_error_seq", "decode_qk_seq_error", "within_sequence", True,
     lambda m, pre: f"within-sequence, shift-invariant logit error {_show(m['error'])} " + _shift_share(m)),
    ("_qk_errors_causal", "qk_errors_causal", "qk_logit_error_causal", "decode_qk_causal_error", "within_sequence_causal", True,
     lambda m, pre: f"causal within-sequence logit error {_show(m['error'])} " + _shift_share(m)
     + (f"; {_show(m['over_full'])} x the figure without the causal mask" if "over_full" in m else "")),
)


class ModelAdapter(ABC):
    _metrics: dict = {}

    def __init__(self, model: nn.Module, tokenizer=None):
        self.model = model
        self.model_config = model.config
        self.config: CompressionConfig = CompressionConfig()
        self.tokenizer = tokenizer
        self.calibs = None
        ModelAdapter.load_metrics()
        self.metrics = _metrics.new_run()

    # ---- construction (model_adapter.py:118-135) ----
    @staticmethod
    def from_model(model: nn.Module, tokenizer) -> "ModelAdapter":
        from .LlamaAdapter import LlamaAdapter
        from .OPTAdapter import OPTAdapter
        from .QwenAdapter import QwenAdapter
        inner = getattr(model, "model", None)
        if inner is not None and hasattr(inner, "decoder"):
            return OPTAdapter(model, tokenizer=tokenizer)
        if inner is not None and hasattr(inner, "layers"):
            model_type = getattr(model.config, "model_type", None) or ""
            if "qwen3" in model_type:
                return QwenAdapter(model, tokenizer=tokenizer)
            if model_type == "qwen2":      # (Qwen2 / Qwen2.5: a Llama block with q/k/v biases, which are always carried)
                from .QwenAdapter import Qwen2Adapter
                return Qwen2Adapter(model, tokenizer=tokenizer)
            return LlamaAdapter(model, tokenizer=tokenizer)
        raise RuntimeError("Unsupported model architecture")

    # ---- metrics: thin delegates to adapters/metrics.py ----
    @staticmethod
    def load_metrics(path="./metrics/metrics.json"):
        _metrics.load(path)
        ModelAdapter._metrics = _metrics.ALL_RUNS

    @staticmethod
    def save_metrics_static(path="./metrics/metrics.json", backup_dir="./metrics/backups/",
                            jsons_path="./metrics/jsons/", run_metrics: Optional[dict] = None):
        _metrics.save(path, backup_dir, jsons_path, run_metrics)

    def save_metrics(self, path="./metrics/metrics.json", backup_dir="./metrics/backups/"):
        _metrics.save(path=path, backup_dir=backup_dir, run_metrics=self.metrics)

    def chain_status(self, status) -> None:
        """Called by compress_nystrom / compress_vo with the ops.DeferredStatus of a layer's kernel chain, right before the
        layer's artefact is saved: the default reads it now -- the save waits for the stream anyway, so this is the chain's one
        host round trip (upstream raises from inside torch.linalg.cholesky at the same point, compress_mlp.py:20,56).  An adapter
        that keeps results on the device (engine.TensorAdapter) collects the statuses and checks them later."""
        status.check()

    # ---- the plumbing of the opt-in reports below: a compressor records device tensors per layer, report_xxx reads them ----
    def _record(self, name: str, key, payload) -> None:
        self.__dict__.setdefault(name, {})[key] = payload

    def _take(self, name: str) -> dict:
        return self.__dict__.pop(name, {})

    def _merge_metrics(self, key: str, report: dict) -> None:
        """metrics[key][str(layer)] = report[layer]; nothing for an empty report."""
        if report:
            if not isinstance(getattr(self, "metrics", None), dict):
                self.metrics = {}
            self.metrics.setdefault(key, {}).update({str(k): v for k, v in report.items()})

    def _report_pairs(self, name: str, key: str, fields, prefix: str, sentence: str, log=None) -> dict:
        """The reports of two squared norms per layer (MLP / V/O intercept, v-bias residual): reads the pairs (a, b) recorded under
        `name` (16 bytes per layer) and writes metrics[key][str(layer)] = {fields[0]: a, fields[1]: b, "relative": a / b} -- both
        None when either is not finite, the ratio only for b > 0.  Logs "[prefix] Layer l: " + sentence.format(a, b) per layer."""
        log = log or logging.getLogger("MoDeGPT")
        pending = self._take(name)
        report = {}
        for layer in sorted(pending):
            a, b = (float(x) for x in pending[layer].cpu().tolist())
            ok = math.isfinite(a) and math.isfinite(b)
            report[layer] = {fields[0]: a if ok else None, fields[1]: b if ok else None, "relative": a / b if ok and b > 0 else None}
            log.info(f"[{prefix}] Layer {layer}: " + sentence.format(a, b))
        self._merge_metrics(key, report)
        return report

    # ---- the certificate of the MLP rank selections (not upstream; north_star: "rank selections bit-identical") ----
    def selection_margin(self, layer_idx: int, out8, eps: float) -> None:
        """compress_nystrom hands over ops.select_margin's 8 numbers (still on the device) for layer `layer_idx`."""
        self._record("_selection_margins", int(layer_idx), (out8, float(eps)))

    def report_selection_margins(self, log=None) -> dict:
        """Reads the recorded certificates (one 64-byte copy per layer; call it where the host waits for the chains anyway), writes
        them to metrics["mlp_selection"] = {layer: {"margin", "score_bound", "eps", "eps_certifiable", "scores_at_risk", "certified"}}
        and WARNS for every layer whose selection the covariance error bound cannot certify: there the k-th and (k+1)-th ridge
        scores sit closer than the bound on what the route's sigma error can do to them, and another accumulation order / route /
        the reference's CPU arithmetic may select a different column set (compress_mlp.py:45-47)."""
        log = log or logging.getLogger("MoDeGPT")
        pending = self._take("_selection_margins")
        report = {}
        for layer in sorted(pending):
            out8, eps = pending[layer]
            m = ops.decode_margin(out8.cpu().tolist(), eps)
            report[layer] = {k: m[k] for k in ("margin", "score_bound", "eps", "eps_certifiable", "scores_at_risk", "certified")}
            if not m["certified"]:
                log.warning(f"[MLP] Layer {layer}: rank selection NOT certified -- threshold margin {m['margin']:.3e} against a score "
                            f"perturbation bound {m['score_bound']:.3e} (covariance error bound eps = {eps:.2e}); "
                            f"{m['scores_at_risk']} scores within reach of the threshold")
        self._merge_metrics("mlp_selection", report)
        return report

    # ---- what the MLP compression costs, at every rank (not upstream; MODEGPT_RANK_CURVE=1) ----
    def rank_curve(self, layer_idx: int, curve, rank: int) -> None:
        """compress_nystrom hands over ops.nystrom_rank_curve's n + 1 numbers (still on the device) for layer `layer_idx`, which it
        compressed to `rank`."""
        self._record("_rank_curves", int(layer_idx), (curve, int(rank)))

    def report_rank_curves(self, log=None) -> dict:
        """Reads the recorded curves (8 (n + 1) bytes per layer; call it where the host waits for the chains anyway), keeps them as
        CPU tensors in self.rank_curves[layer] and writes metrics["mlp_rank_curve"][str(layer)] = ops.decode_rank_curve(...): the
        relative output error of the layer's MLP at the rank it got, at the keep ratios 0.05 .. 1.00, and the smallest rank that
        reaches 1e-1 / 1e-2 / 1e-3 -- under sigma_mlp + eps I and for the fp64 refit ("The error-versus-rank
        curve", says what that is not).  Logs one line per layer and the energy-weighted mean over the layers read by this call."""
        log = log or logging.getLogger("MoDeGPT")
        pending = self._take("_rank_curves")
        report = {}
        for layer in sorted(pending):
            curve, rank = pending[layer]
            host = curve.detach().cpu()
            self._record("rank_curves", layer, host)
            m = report[layer] = ops.decode_rank_curve(host.tolist(), rank)
            if m["rel_error"] is None:
                log.warning(f"[MLP] Layer {layer}: rank curve has no usable energy (curve[0] = {m['energy']!r})")
                continue
            log.info(f"[MLP] Layer {layer}: rank {rank} of {m['n']}: relative output error {m['rel_error']:.3e}; "
                     f"rank for 1e-2: {m['rank_for_rel_error']['0.01']}")
        if report:
            # (a NaN / Inf energy would be written as the non-standard NaN / Infinity by json.dump: None there, as the relative fields)
            finite = lambda m: m if math.isfinite(m["energy"]) else {**m, "energy": None}      # noqa: E731
            self._merge_metrics("mlp_rank_curve", {k: finite(v) for k, v in report.items()})
            usable = [m for m in report.values() if m["rel_error"] is not None]
            energy = sum(m["energy"] for m in usable)
            if usable and energy > 0:
                mean = sum(m["energy"] * m["rel_error"] for m in usable) / energy
                log.info(f"[MLP] rank curves of {len(usable)} layers: energy-weighted mean relative output error {mean:.3e}")
        return report

    # ---- the greedy MLP selection's own numbers (not upstream; MODEGPT_MLP_GREEDY=T) ----
    def mlp_greedy(self, layer_idx: int, tensors, rank: int) -> None:
        """compress_nystrom hands over (objective, cut, n_dead, ridge_at_rank, greedy_at_rank) of the layer's greedy selection --
        ops.nystrom_greedy_select's outputs and, with MODEGPT_RANK_CURVE=1, the two rank curves' values at `rank` (else None) --
        still on the device."""
        self._record("_mlp_greedy", int(layer_idx), (tuple(tensors), int(rank)))

    def report_mlp_greedy(self, log=None) -> dict:
        """Reads the recorded tensors (8 (3 rounds + 4) bytes per layer; call it where the host waits for the chains anyway) and
        writes metrics["mlp_greedy"][str(layer)] = ops.decode_mlp_greedy(...): the objective before the first round and after
        each, its last value over the first, the dead picks, the narrowest cut, and the ridge rule's residual energy at the same
        rank beside this selection's where the rank curve ran.  metrics["mlp_selection"][str(layer)] says that the selection
        carries no certificate.  WARNS once per layer where the ridge rule's value is the smaller one: more rounds are needed
        ("Greedy MLP selection")."""
        log = log or logging.getLogger("MoDeGPT")
        pending = self._take("_mlp_greedy")
        report, selection = {}, {}
        for layer in sorted(pending):
            tensors, rank = pending[layer]
            objective, cut, n_dead, ridge, greedy = (None if t is None else t.detach().cpu() for t in tensors)
            m = report[layer] = ops.decode_mlp_greedy(objective.tolist(), cut.tolist(), int(n_dead), rank,
                                                      ridge_at_rank=None if ridge is None else float(ridge),
                                                      greedy_at_rank=None if greedy is None else float(greedy))
            selection[layer] = {"statistic": "greedy", "certificate": None, "certified": None,
                                "reason": "no certificate is issued for a selection by greedy descent on the refit's objective"}
            show = lambda v: "n/a" if v is None else f"{v:.3e}"      # noqa: E731
            log.info(f"[MLP] Layer {layer}: greedy selection, {m['rounds']} rounds to rank {rank}: objective over total "
                     f"{show(m['objective_over_total'])}, {m['dead_picks']} dead picks, narrowest cut {show(m['min_cut_gap'])}"
                     + ("" if m.get("greedy_over_ridge") is None else f"; {m['greedy_over_ridge']:.3g} x the ridge rule's residual"))
            over = m.get("greedy_over_ridge")
            if over is not None and over > 1.0:
                log.warning(f"[MLP] Layer {layer}: the ridge rule's residual energy {m['ridge_at_rank']:.3e} is below the greedy "
                            f"selection's {m['greedy_at_rank']:.3e} at rank {rank}: {m['rounds']} rounds take correlated columns "
                            f"together -- more rounds are needed (MODEGPT_MLP_GREEDY)")
        self._merge_metrics("mlp_greedy", report)
        self._merge_metrics("mlp_selection", selection)
        return report

    # ---- what the STORED MLP weights lose of the layer's output (not upstream; MODEGPT_OUTPUT_ERROR=1) ----
    def output_error(self, layer_idx: int, tensors, rank: int) -> None:
        """compress_nystrom hands over (q, e, unorm2) of ops.mlp_output_error (d numbers each, still on the device) for layer
        `layer_idx`, which it compressed to `rank`."""
        self._record("_output_errors", int(layer_idx), (tuple(tensors), int(rank)))

    def report_output_errors(self, log=None) -> dict:
        """Reads the recorded tensors (24 d bytes per layer; call it where the host waits for the chains anyway), keeps them as CPU
        tensors in self.output_errors[layer] = (q, e, unorm2) and writes metrics["mlp_output_error"][str(layer)] =
        ops.decode_output_error(...): the energy the layer's output carries on the calibration statistic, how much of it the bf16
        tensor that was saved loses, the worst output channel -- and, where report_rank_curves has read the layer's curve before,
        the distance from the best possible refit ("The realised output error of the stored MLP weights", says
        what that is not).  Logs one line per layer."""
        log = log or logging.getLogger("MoDeGPT")
        pending = self._take("_output_errors")
        curves = self.__dict__.get("rank_curves", {})
        report = {}
        for layer in sorted(pending):
            (q, e, unorm2), rank = pending[layer]
            host = tuple(t.detach().cpu() for t in (q, e, unorm2))
            self._record("output_errors", layer, host)
            curve = curves.get(layer)
            m = report[layer] = ops.decode_output_error(host[1].tolist(), host[0].tolist(), host[2].tolist(), ops.NYSTROM_EPS, rank,
                                                        curve=None if curve is None else curve.tolist())
            if m["relative_error"] is None:
                log.warning(f"[MLP] Layer {layer}: output error has no usable energy (energy {m['energy']!r}, error {m['error']!r})")
                continue
            excess = m.get("excess_over_optimum")
            log.info(f"[MLP] Layer {layer}: rank {rank}: stored weights lose {m['relative_error']:.3e} of the output energy; "
                     f"worst channel {m['worst_channel']} loses {m['worst_channel_relative_error']:.3e}"
                     + ("" if excess is None else f"; {excess:.3e} of the energy above the best refit"))
        self._merge_metrics("mlp_output_error", report)
        return report

    # ---- what the STORED v_proj / o_proj lose of the attention output (not upstream; MODEGPT_VO_ERROR=1) ----
    def vo_error(self, layer_idx: int, tensors, rank: int, centred: bool = False) -> None:
        """compress_vo hands over (q, e, dnorm2, curve) -- ops.vo_output_error's [n_heads, d] tensors and
        ops.vo_compress(want_curve=True)'s [n_kv, hd + 1], still on the device -- for layer `layer_idx`, truncated to `rank` per head.
        centred: they were taken on S = C - mu mu^T (MODEGPT_VO_INTERCEPT=1); the layer's entry then says "centred": true."""
        self._record("_vo_errors", int(layer_idx), (tuple(tensors), int(rank), bool(centred)))

    def report_vo_errors(self, log=None) -> dict:
        """Reads the recorded tensors (24 n_heads d + 8 n_kv (hd + 1) bytes per layer; call it where the host waits for the chains
        anyway), keeps them as CPU tensors in self.vo_errors[layer] = (q, e, dnorm2, curve) and writes
        metrics["vo_output_error"][str(layer)] = ops.decode_vo_output_error(...): the energy the attention output carries on the
        calibration statistic, how much of it the bf16 v_proj / o_proj that were saved lose, per kv head and for the layer, the worst
        head and channel, and the distance from the fp64 truncation's curve ("The realised output error of the
        stored V/O factors", says what that is not).  Logs one line per layer."""
        log = log or logging.getLogger("MoDeGPT")
        pending = self._take("_vo_errors")
        report = {}
        for layer in sorted(pending):
            tensors, rank, centred = pending[layer]
            host = tuple(t.detach().cpu() for t in tensors)
            self._record("vo_errors", layer, host)
            q, e, dnorm2, curve = host
            m = report[layer] = ops.decode_vo_output_error(e.tolist(), q.tolist(), dnorm2.tolist(), self.config.ridge_vo, rank,
                                                           curve.shape[0], curve=curve.tolist())
            if centred:
                m["centred"] = True                   # (the figures are the affine map's: the statistic was S = C - mu mu^T)
            if m["relative_error"] is None:
                log.warning(f"[VO] Layer {layer}: output error has no usable energy (energy {m['energy']!r}, error {m['error']!r})")
                continue
            excess = m.get("excess_over_curve")
            log.info(f"[VO] Layer {layer}: rank {rank}: stored factors lose {m['relative_error']:.3e} of the output energy; "
                     f"worst head {m['worst_head']} loses {m['worst_head_relative_error']:.3e}"
                     + ("" if excess is None else f"; {excess:.3e} of the energy above the fp64 truncation"))
        # (decode_vo_output_error maps every non-finite sum to None, so json.dump never meets a NaN)
        self._merge_metrics("vo_output_error", report)
        return report

    # ---- what the Q/K pair selection loses of the attention logits (not upstream; MODEGPT_QK_ERROR=1) ----
    def qk_error(self, layer_idx: int, tensors, rank: int) -> None:
        """compress_qk hands over ops.qk_rank_curve's (curve_h, curve, terms, scale, greedy_curve, greedy_order) and the order they
        were taken along, still on the device, for layer `layer_idx`, whose heads keep `rank` columns."""
        self._record("_qk_errors", int(layer_idx), (tuple(tensors), int(rank)))

    def report_qk_errors(self, log=None) -> dict:
        """Reads the recorded tensors (about 8 (n_heads + 4 n_kv) (ns + 1) bytes per layer; call it where the host waits for the
        chains anyway), keeps them as CPU tensors in self.qk_errors[layer] = (curve_h, curve, terms, scale, greedy_curve,
        greedy_order, order) and writes metrics["qk_logit_error"][str(layer)] = ops.decode_qk_logit_error(...): the mean-square
        logit the layer's heads carry on the calibration statistic, how much of it the kept columns lose, per kv head and for the
        layer, what the diagonal rule believed it would lose, and what a greedy order on the full objective loses at the same rank
        ("What the Q/K selection costs the attention logits", says what that is not).  The same curves on the post-RoPE
        (MODEGPT_QK_ROPE=1), within-sequence (MODEGPT_QK_SEQ=1) and causal (MODEGPT_QK_CAUSAL=1) statistics, where compress_qk had
        them, go the same way through the rows of _QK_REPORTS: to self.qk_errors_rope / _seq / _causal and metrics["qk_logit_error_rope"]
        (with the pre-RoPE figure beside it) / ["qk_logit_error_seq"] (with the error on the uncentred statistic and the share of it
        softmax cannot see) / ["qk_logit_error_causal"] (the seq entry's fields plus over_full against the layer's seq entry where
        there is one).  Logs one line per layer and statistic; returns the pre-RoPE report."""
        log = log or logging.getLogger("MoDeGPT")
        reports = {}
        for name, attr, key, decoder, statistic, with_raw, line in _QK_REPORTS:
            pending = self._take(name)
            report = reports[key] = {}
            for layer in sorted(pending):
                tensors, rank = pending[layer]
                host = tuple(None if t is None else t.detach().cpu() for t in tensors)
                self._record(attr, layer, host)
                curve_h, curve, terms, scale, g_curve = host[:5]
                cols = max(1, self.head_dim // max(1, curve.shape[1] - 1))
                more = {"seq": reports["qk_logit_error_seq"].get(layer)} if key == "qk_logit_error_causal" else {}
                m = report[layer] = getattr(ops, decoder)(curve_h.tolist(), curve.tolist(), *((host[7].tolist(),) if with_raw else ()), rank,
                                                          cols, terms=terms.tolist(), scale=scale.tolist(),
                                                          greedy_curve=None if g_curve is None else g_curve.tolist(), **more)
                pre = reports["qk_logit_error"].get(layer, {}).get("relative_error")
                if statistic is None and m["relative_error"] is None:
                    log.warning(f"[QK] Layer {layer}: logit error has no usable energy (energy {m['energy']!r}, error {m['error']!r})")
                    continue
                if statistic is not None:
                    m["statistic"] = statistic
                if statistic == "post_rope":
                    m["pre_rope_relative_error"] = pre
                log.info(f"[QK] Layer {layer}: rank {rank}: " + line(m, pre))
            # (the decoders map every non-finite figure to None, so json.dump never meets a NaN)
            self._merge_metrics(key, report)
        return reports["qk_logit_error"]

    def qk_error_causal(self, layer_idx: int, tensors, rank: int) -> None:
        """compress_qk hands over ops.qk_rank_curve's outputs on the causal statistic (P^c, ones), the order -- the one of qk_error's
        tensors -- and the kv-head curve on the uncentred P^c_raw, for layer `layer_idx`; report_qk_errors reads them into
        metrics["qk_logit_error_causal"]."""
        self._record("_qk_errors_causal", int(layer_idx), (tuple(tensors), int(rank)))

    def qk_error_seq(self, layer_idx: int, tensors, rank: int) -> None:
        """compress_qk hands over ops.qk_rank_curve's outputs on the within-sequence statistic (P, ones), the order -- the one of
        qk_error's tensors -- and the kv-head curve on the uncentred P_raw, for layer `layer_idx`; report_qk_errors reads them into
        metrics["qk_logit_error_seq"]."""
        self._record("_qk_errors_seq", int(layer_idx), (tuple(tensors), int(rank)))

    def qk_error_rope(self, layer_idx: int, tensors, rank: int) -> None:
        """compress_qk hands over ops.qk_rank_curve's outputs on the post-RoPE statistics (sigma_q', sigma_k') and the order -- the one
        of qk_error's tensors -- for layer `layer_idx`; report_qk_errors reads them into metrics["qk_logit_error_rope"]."""
        self._record("_qk_errors_rope", int(layer_idx), (tuple(tensors), int(rank)))

    def qk_selection_statistic(self, layer_idx: int, statistic: str) -> None:
        """compress_qk says which statistic the layer's pair selection was scored on ("pre_rope" / "post_rope") when the run carries
        post-RoPE statistics, "within_sequence" under MODEGPT_QK_SEQ_SELECT=1 or "within_sequence_causal" under
        MODEGPT_QK_CAUSAL_SELECT=1; report_attention_margins writes it to
        metrics["qk_selection"][layer]["statistic"]."""
        self._record("_qk_selection_statistics", int(layer_idx), str(statistic))

    # ---- the certificates of the attention half: QK pair selection, VO spectral gap (not upstream) ----
    def attention_margin(self, layer_idx: int, kind: str, tensor, *eps: float) -> None:
        """compress_qk (kind "qk": ops.qk_select_margin's [n_kv, 8], eps = (eps_rel, eps_abs)) and compress_vo (kind "vo":
        ops.vo_compress(want_spectrum=True)'s [n_kv, 8], eps = (eps,)) hand their device tensors over for layer `layer_idx`."""
        if kind not in ("qk", "vo"):
            raise ValueError(f"attention_margin: kind must be 'qk' or 'vo', got {kind!r}")
        self._record("_attention_margins", (kind, int(layer_idx)), (tensor, tuple(float(e) for e in eps)))

    def report_attention_margins(self, log=None) -> dict:
        """Reads the recorded attention certificates (64 bytes per kv head; call it where the host waits for the chains anyway) and
        returns {"qk": {layer: ops.decode_qk_margin(...)}, "vo": {layer: ops.decode_vo_spectrum(...)}}; the same goes to
        metrics["qk_selection"] / metrics["vo_spectrum"] under str(layer).  WARNS once per layer whose QK pair selection is not
        certified -- some head's weakest selected and strongest unselected pair sit closer than the covariance route's error bound
        and the rounding of the reference's eigh route can move them, so the reference may keep another pair set there
        (compress_qk.py:366-367) -- and once per grouped VO layer in which some head's sigma_r and sigma_r+1 are not separated
        (compress_vo.py:130-146: the kept subspace is then not determined by the data)."""
        log = log or logging.getLogger("MoDeGPT")
        pending = self._take("_attention_margins")
        statistics = self._take("_qk_selection_statistics")
        report = {"qk": {}, "vo": {}}
        for kind, layer in sorted(pending):
            tensor, eps = pending[(kind, layer)]
            rows = tensor.cpu().tolist()
            if kind == "qk":
                m = ops.decode_qk_margin(rows, *eps)
                if layer in statistics:               # (only a run that carries post-RoPE statistics says which one it scored on)
                    m["statistic"] = statistics[layer]
                if not m["certified"]:
                    flagged = [i for i, h in enumerate(m["heads"]) if not h["certified"]]
                    log.warning(f"[QK] Layer {layer}: pair selection NOT certified -- kv head {m['weakest_head']}: threshold margin "
                                f"{m['margin']:.3e} against a score half-width {m['score_halfwidth']:.3e} (eps_rel = {eps[0]:.2e}, "
                                f"eps_abs = {eps[1]:.2e}); {m['heads'][m['weakest_head']]['units_at_risk']} pairs within reach of the "
                                f"threshold; uncertified kv heads: {flagged}")
            else:
                m = ops.decode_vo_spectrum(rows, *eps)
                if m["separated"] is False:
                    flagged = [i for i, h in enumerate(m["heads"]) if h["separated"] is False]
                    worst = min(flagged, key=lambda i: m["heads"][i]["gap"])
                    w = m["heads"][worst]
                    log.warning(f"[VO] Layer {layer}: kept subspace NOT separated -- kv head {worst}: relative gap "
                                f"{w['gap']:.3e} between sigma_r and sigma_r+1 (lambda_r - lambda_r+1 = "
                                f"{w['lambda_r'] - w['lambda_next']:.3e} against twice the bound {w['bound']:.3e}, eps = {eps[0]:.2e})")
            report[kind][layer] = m
        for layer in sorted(statistics):
            if statistics[layer] == "within_sequence" and layer not in report["qk"]:
                # MODEGPT_QK_SEQ_SELECT=1: no certificate is computed for this selection; the entry says so instead of carrying one
                # computed on an error model that does not cover the centring's cancellation
                report["qk"][layer] = {"statistic": "within_sequence", "certificate": None, "certified": None, "order_certified": None,
                                       "reason": "no certificate is issued for a selection on the within-sequence statistic"}
            elif statistics[layer] == "within_sequence_causal" and layer not in report["qk"]:         # MODEGPT_QK_CAUSAL_SELECT=1: likewise
                report["qk"][layer] = {"statistic": "within_sequence_causal", "certificate": None, "certified": None,
                                       "order_certified": None,
                                       "reason": "no certificate is issued for a selection on the causal within-sequence statistic"}
        for kind, key in (("qk", "qk_selection"), ("vo", "vo_spectrum")):       # (only the non-empty kinds)
            self._merge_metrics(key, report[kind])
        return report

    # ---- reconstruction: per-(layer, stage) artefacts and the final swap (model_adapter.py:184-237) ----
    def save_layer(self, output_dir: str, suffix: str, weights: dict, layer_idx):
        """torch.save({name: bf16 tensor}) to <output_dir>/layer_<i>_<suffix>; env vars in the path expand.  The file is in
        place when this returns -- unless the run switched the background writer on (async_artifacts(True): run_modegpt does),
        in which case it is in place after flush_artifacts(), which every reader of the directory here calls first."""
        output_dir = os.path.expandvars(output_dir)
        os.makedirs(output_dir, exist_ok=True)
        path = os.path.join(output_dir, f"layer_{layer_idx}_{suffix}")
        held = getattr(self, "_held_artifacts", None)
        if held is not None:                     # a sharded run: the gather packs its send buffer from these, not from the files
            held.setdefault(int(layer_idx), {}).update(weights)
        writer = getattr(self, "_artifact_writer", None)
        if writer is not None:
            writer.submit(path, weights)
        else:
            torch.save(weights, path)

    def hold_artifacts(self, enable: bool = True) -> None:
        """Keep a reference to every tensor handed to save_layer (on its device) until take_held_artifacts(layer) collects it:
        sharding.gather_layer_artifacts packs the all-gather's send buffer from them instead of reading the files back.  ~0.3 GB
        per layer at Llama-3-8B / 30 %, for the layers of one chunk a rank owns."""
        self._held_artifacts = {} if enable else None

    def take_held_artifacts(self, layer_idx: int) -> dict:
        held = getattr(self, "_held_artifacts", None)
        return {} if held is None else held.pop(int(layer_idx), {})

    def async_artifacts(self, enable: bool = True) -> None:
        """Layer artefacts through a background writer (artifact_io.ArtifactWriter): save_layer enqueues the device-to-host copy
        and returns, the next layer's kernels run meanwhile.  Off by default: a caller that reads a file right after save_layer
        finds it."""
        self.flush_artifacts()
        if enable and os.environ.get("MODEGPT_ASYNC_SAVE", "1") != "0":
            from ..artifact_io import ArtifactWriter
            self._artifact_writer = ArtifactWriter()
        else:
            self._artifact_writer = None

    def flush_artifacts(self) -> None:
        writer = getattr(self, "_artifact_writer", None)
        if writer is not None:
            writer.flush()

    @torch.no_grad()
    def convert_model(self, saved_layers_dir: str = "./compressed_output/layers/", suffixes=("mlp", "qk", "vo"),
                      device: str = "cuda"):
        """Swap every layer's Linears for bf16 Linears built from the saved artefacts: bias-free (model_adapter.py:199-208), except
        where the artefact carries a bias (`<name>_bias`: the compressors write them with MODEGPT_KEEP_BIAS=1 and for Qwen2; down_bias
        also with MODEGPT_MLP_INTERCEPT=1, the refit's intercept, and o_bias with MODEGPT_VO_INTERCEPT=1, the truncation's -- keys the
        reference's LlamaRebuild does not know)."""
        saved_layers_dir = os.path.expandvars(saved_layers_dir)
        self.flush_artifacts()

        def linear_of(w: Tensor, b: Optional[Tensor] = None) -> nn.Linear:
            lin = nn.Linear(w.shape[1], w.shape[0], bias=b is not None, device=device, dtype=torch.bfloat16)
            lin.weight.data.copy_(w.to(torch.bfloat16))
            if b is not None:
                lin.bias.data.copy_(b.to(torch.bfloat16))
            return lin

        for suffix in suffixes:
            for i in range(self.n_layers):
                art = torch.load(os.path.join(saved_layers_dir, f"layer_{i}_{suffix}"), map_location=device)
                if suffix == "mlp":
                    gate = art.get("gate")
                    down_bias = art.get("down_bias")
                    if down_bias is None and ops.mlp_intercept_enabled():
                        # MODEGPT_MLP_INTERCEPT=1: the refitted layers store an intercept as down_bias; a layer whose artefact has
                        # none (outside the target layers, or written without the switch) gets an exact zero, so that
                        # projection_biases() is uniform over the layers and the checkpoint loads strictly
                        down_bias = torch.zeros(art["down"].shape[0], dtype=torch.bfloat16, device=device)
                    self.replace_mlp_layers(i, new_up=linear_of(art["up"], art.get("up_bias")),
                                            new_down=linear_of(art["down"], down_bias),
                                            new_gate=None if gate is None else linear_of(gate, art.get("gate_bias")))
                elif suffix == "qk":
                    self.replace_attn_layers(i, new_q=linear_of(art["q_proj"], art.get("q_bias")),
                                             new_k=linear_of(art["k_proj"], art.get("k_bias")), new_v=None, new_o=None)
                elif suffix == "vo":
                    o_bias = art.get("o_bias")
                    if ops.vo_intercept_enabled():
                        # MODEGPT_VO_INTERCEPT=1: the truncated layers store an intercept as o_bias and no v_bias (the v bias is part
                        # of the intercept); a layer whose artefact has no o_bias (outside the target layers, or written without the
                        # switch) gets an exact zero, as down_bias above.  A v_bias cannot stand beside it: projection_biases() would
                        # differ between the layers and the checkpoint would not load strictly
                        if art.get("v_bias") is not None:
                            raise RuntimeError(f"MODEGPT_VO_INTERCEPT=1 but the vo artefact of layer {i} carries a v_bias: it was written "
                                               "without the switch (MODEGPT_KEEP_BIAS=1 / Qwen2); compress the layer again with the switch on")
                        if o_bias is None:
                            o_bias = torch.zeros(art["o_proj"].shape[0], dtype=torch.bfloat16, device=device)
                    self.replace_attn_layers(i, new_q=None, new_k=None, new_v=linear_of(art["v_proj"], art.get("v_bias")),
                                             new_o=linear_of(art["o_proj"], o_bias))

    # ---- which projections of the converted model carry a bias (not upstream; patch_config records it) ----
    BIAS_SLOTS = ("up", "gate", "down", "q", "k", "v", "o")

    def projection_biases(self) -> list:
        """Names out of BIAS_SLOTS whose Linear carries a bias in the model as it stands (uniform over the layers: they come from one
        architecture and one switch); a model with layers that disagree is refused rather than written as a checkpoint that cannot
        be loaded strictly."""
        found = None
        for i in range(self.n_layers):
            mlp, attn = self.get_mlp_components(i), self.get_attn_components(i)
            mods = {"up": mlp.up_proj, "gate": mlp.gate_proj, "down": mlp.down_proj, "q": attn.q_proj, "k": attn.k_proj,
                    "v": attn.v_proj, "o": attn.o_proj}
            here = [n for n in self.BIAS_SLOTS if mods[n] is not None and getattr(mods[n], "bias", None) is not None]
            if found is not None and here != found:
                raise RuntimeError(f"layer {i} carries biases on {here}, earlier layers on {found}")
            found = here
        return found or []

    # ---- the intercept of the mean-aware MLP refit (not upstream; MODEGPT_MLP_INTERCEPT=1) ----
    def mlp_intercept(self, layer_idx: int, norms) -> None:
        """compress_nystrom hands over ops.nystrom_intercept's norms (2 numbers, still on the device) for layer `layer_idx`."""
        self._record("_mlp_intercepts", int(layer_idx), norms)

    def report_mlp_intercepts(self, log=None) -> dict:
        """Reads the recorded pairs (16 bytes per layer; call it where the host waits for the chains anyway) and writes
        metrics["mlp_intercept"][str(layer)] = {"offset_norm2": ||delta||^2, "mean_output_norm2": ||W_d mu||^2, "relative": their
        ratio}: delta = W_d mu - D^ mu_k is what the stored down_bias adds to the projection's own bias, W_d mu the mean output of the
        uncompressed projection ("The MLP intercept").  Non-finite figures become None."""
        return self._report_pairs("_mlp_intercepts", "mlp_intercept", ("offset_norm2", "mean_output_norm2"), "MLP",
                                  "the intercept carries {:.3e} of the mean output {:.3e} (squared norms)", log)

    # ---- the intercept of the mean-aware V/O truncation (not upstream; MODEGPT_VO_INTERCEPT=1) ----
    def vo_intercept(self, layer_idx: int, norms) -> None:
        """compress_vo hands over ops.vo_intercept's norms (2 numbers, still on the device) for layer `layer_idx`."""
        self._record("_vo_intercepts", int(layer_idx), norms)

    def report_vo_intercepts(self, log=None) -> dict:
        """Reads the recorded pairs (16 bytes per layer; call it where the host waits for the chains anyway) and writes
        metrics["vo_intercept"][str(layer)] = {"offset_norm2": ||delta||^2, "mean_output_norm2": ||sum_h W_o,h a_kv(h)||^2, "relative":
        their ratio}: a_g = W_v,g mu + b_v,g, the second figure is the constant the uncompressed attention adds to its output, delta what
        the stored o_bias adds to the projection's own bias -- the part of that constant the stored factors do not carry (DESIGN.md
        section 7, "The V/O intercept").  Non-finite figures become None."""
        return self._report_pairs("_vo_intercepts", "vo_intercept", ("offset_norm2", "mean_output_norm2"), "VO",
                                  "the intercept carries {:.3e} of the mean output {:.3e} (squared norms)", log)

    # ---- what the truncated v_proj cannot carry of a v bias where o_proj has no bias to fold it into (not upstream) ----
    def vo_bias_residual(self, layer_idx: int, resid) -> None:
        """compress_vo hands over ops.vo_bias's resid (2 numbers, still on the device) for layer `layer_idx`."""
        self._record("_vo_bias_residuals", int(layer_idx), resid)

    def report_vo_bias_residuals(self, log=None) -> dict:
        """Reads the recorded pairs (16 bytes per layer; call it where the host waits for the chains anyway) and writes
        metrics["vo_bias_residual"][str(layer)] = {"residual_norm2": ||rho||^2, "constant_norm2": ||sum_h W_o,h b_v||^2,
        "relative": their ratio}: rho = sum_h W_o,h (I - Pi_g) b_v,kv(h) is the part of the constant a v bias adds to the attention
        output that the rank-r v_proj cannot represent ("Projection biases").  Non-finite figures become None."""
        return self._report_pairs("_vo_bias_residuals", "vo_bias_residual", ("residual_norm2", "constant_norm2"), "VO",
                                  "the truncated v_proj loses {:.3e} of the v bias's output constant {:.3e} (squared norms)", log)

    # ---- in-place slicing (model_adapter.py:394-542; upstream's call sites are commented out in favour of the
    #      save_layer -> convert_model route, the methods stay part of the adapter surface) ----
    @staticmethod
    def _swap_in(weight: Tensor, bias_from=None, bias_values: Optional[Tensor] = None) -> nn.Linear:
        """bf16 Linear on the GPU holding `weight` [out, in]; carries a bias only when `bias_from` (the module it
        replaces) has one, initialised from `bias_values` when given."""
        has_bias = bias_from is not None and getattr(bias_from, "bias", None) is not None
        lin = nn.Linear(weight.shape[1], weight.shape[0], bias=has_bias, device="cuda", dtype=torch.bfloat16)
        lin.weight.data.copy_(weight.to(torch.bfloat16))
        if has_bias and bias_values is not None:
            lin.bias.data.copy_(bias_values)
        return lin

    @torch.no_grad()
    def slice_gate_dims(self, layer_idx: int, up_weights: Tensor, down_weights: Tensor, gate_weights: Optional[Tensor],
                        new_bias_u: Optional[Tensor], new_bias_g: Optional[Tensor], bias: bool = True,
                        expert_idx: Optional[int] = None):
        """Put compressed MLP weights ([out, in] each) straight into the block.  up/gate biases come from the caller
        (they were sliced with the kept rows), down keeps the module's own bias."""
        comps = self.get_mlp_components(layer_idx, expert_idx=expert_idx)
        keep = (lambda m: m) if bias else (lambda m: None)
        up = self._swap_in(up_weights, keep(comps.up_proj), new_bias_u)
        gate = None if gate_weights is None else self._swap_in(gate_weights, keep(comps.gate_proj), new_bias_g)
        down_bias = None if comps.down_proj.bias is None else comps.down_proj.bias.data
        down = self._swap_in(down_weights, keep(comps.down_proj), down_bias)
        self.replace_mlp_layers(layer_idx, up, down, gate, expert_idx=expert_idx)

    @torch.no_grad()
    def slice_qk_dims(self, layer_idx: int, new_heads_Q: List[Tensor], new_heads_K: List[Tensor],
                      new_bias_Q: List[Tensor] = [], new_bias_K: List[Tensor] = [], bias: bool = True):
        """Per-head row blocks -> one q_proj / k_proj; a bias survives only if the original had one, `bias` is set and
        per-head biases were passed."""
        comps = self.get_attn_components(layer_idx)
        bq = torch.cat(list(new_bias_Q), dim=0) if len(new_bias_Q) > 0 else None
        bk = torch.cat(list(new_bias_K), dim=0) if len(new_bias_K) > 0 else None
        q = self._swap_in(torch.cat(list(new_heads_Q), dim=0), comps.q_proj if (bias and bq is not None) else None, bq)
        k = self._swap_in(torch.cat(list(new_heads_K), dim=0), comps.k_proj if (bias and bk is not None) else None, bk)
        self.replace_attn_layers(layer_idx, new_q=q, new_k=k, new_v=None, new_o=None)

    @torch.no_grad()
    def slice_vo_dims(self, layer_idx: int, new_heads_V: List[Tensor], new_heads_O: List[Tensor], bias: bool):
        """Per-head V row blocks / O column blocks -> v_proj (never biased) and o_proj (keeps the original bias)."""
        comps = self.get_attn_components(layer_idx)
        v = self._swap_in(torch.cat(list(new_heads_V), dim=0))
        o_bias = None if comps.o_proj.bias is None else comps.o_proj.bias.data
        o = self._swap_in(torch.cat(list(new_heads_O), dim=1), comps.o_proj if bias else None, o_bias)
        self.replace_attn_layers(layer_idx, new_q=None, new_k=None, new_v=v, new_o=o)

    # ---- shape properties (model_adapter.py:253-307) ----
    @property
    def arch(self) -> str:
        return self.model_config.model_type

    @property
    def n_layers(self) -> int:
        c = self.model_config
        return getattr(c, "n_layer", None) or getattr(c, "num_hidden_layers", None) or getattr(c, "num_layers", None)

    @property
    def n_heads(self) -> int:
        c = self.model_config
        return getattr(c, "n_head", None) or getattr(c, "num_attention_heads", None)

    @property
    def d_model(self) -> int:
        c = self.model_config
        return getattr(c, "hidden_size", None) or getattr(c, "dim", None)

    @property
    def d_int(self) -> int:
        return getattr(self.model_config, "intermediate_size", None)

    @property
    def head_dim(self) -> int:
        hd = getattr(self.model_config, "head_dim", None)
        return hd if hd else self.d_model // self.n_heads  # OPTConfig carries no head_dim

    @property
    def n_experts(self) -> int:
        if self.arch == "deepseek":
            return getattr(self.model_config, "n_routed_experts", 0)
        return getattr(self.model_config, "num_local_experts", 0)

    @property
    def n_kv_heads(self) -> int:
        return getattr(self.model_config, "num_key_value_heads", self.n_heads)

    def get_n_inner(self) -> int:
        return self.model_config.intermediate_size

    # ---- what an adapter must provide (model_adapter.py:249-392) ----
    @abstractmethod
    def compute_layer_energy(self, layer_idx: int, Ca: Optional[Tensor] = None) -> MLPTensors: ...

    @abstractmethod
    def calibrate_model(self, n_samples: int, batch_size: int, target_layers: List[int], dataset="wikitext"): ...

    @abstractmethod
    def get_transformer_blocks(self) -> nn.ModuleList: ...

    @abstractmethod
    def register_hooks(self, layer_idx: int, block: nn.Module, cov_mlp_list: List[Tensor], cov_q_list: List[Tensor],
                       cov_k_list: List[Tensor], cov_x_list: List[Tensor], handles: List[Any],
                       logger: logging.Logger): ...

    def on_batch_end_step(self, layer_idx: int, x_in: Tensor, cov_x_list: List[Tensor]):
        pass

    @abstractmethod
    def get_mlp_components(self, layer_idx: int, expert_idx: Optional[int] = None) -> MLPComponents: ...

    @abstractmethod
    def get_mlp_tensors(self, layer_idx: int, expert_idx: Optional[int] = None) -> MLPTensors: ...

    @abstractmethod
    def get_vo_components(self, layer_idx: int, expert_idx: Optional[int] = None) -> VOComponents: ...

    @abstractmethod
    def get_vo_tensors(self, layer_idx: int, expert_idx: Optional[int] = None) -> VOTensors: ...

    @abstractmethod
    def get_qk_components(self, layer_idx: int, expert_idx: Optional[int] = None) -> QKComponents: ...

    @abstractmethod
    def get_qk_tensors(self, layer_idx: int, expert_idx: Optional[int] = None) -> QKTensors: ...

    @abstractmethod
    def replace_mlp_layers(self, layer_idx: int, new_up: nn.Module, new_down: nn.Module,
                           new_gate: Optional[nn.Module] = None, expert_idx: Optional[int] = None) -> None: ...

    @abstractmethod
    def get_attn_components(self, layer_idx: int) -> AttentionComponents: ...

    @abstractmethod
    def replace_attn_layers(self, layer_idx: int, new_q: Optional[nn.Module], new_k: Optional[nn.Module],
                            new_v: Optional[nn.Module], new_o: Optional[nn.Module]) -> None: ...

    @abstractmethod
    def get_qk_weights(self, layer_idx: int) -> Tuple[Tensor, Tensor]: ...

    @abstractmethod
    def get_vo_weights(self, layer_idx: int) -> Tuple[Tensor, Tensor]: ...

    # ---- statistic hooks shared by adapters (model_adapter.py:546-567) ----
    @staticmethod
    def _make_fc_hook(layer_idx, cov_mlp_list, sum_list=None):
        """sigma_mlp += ReLU(fc1 out)^T ReLU(fc1 out) -- ReLU fused into the kernel's load.  bf16 / fp16 activations of at least
        ops.FC_I8_MIN_FEATURES features (a multiple of 128) take the int8 digit planes with ReLU on load; everything else the fp64
        kernel, as before (ops.cov_accum_fc_relu).  sum_list (not upstream): one fp64 vector per layer -- the column sums of
        ReLU(fc1 out) are added to sum_list[layer_idx] as well (ops.col_sum_accum, ReLU on load)."""
        @torch.no_grad()
        def hook(module, inp, out):
            ops.cov_accum_fc_relu(cov_mlp_list[layer_idx], out)
            if sum_list is not None and sum_list[layer_idx] is not None:
                ops.col_sum_accum(sum_list[layer_idx], out, relu=True)
        return hook

    @staticmethod
    def _make_proj_hook(layer_idx, cov_list, n_heads, head_dim, d_model=None):
        """sigma[h] += P_h^T P_h for every head, read in place from the [tokens, n_heads*head_dim] output."""
        @torch.no_grad()
        def hook(module, inp, out):
            ops.cov_accum(cov_list[layer_idx], out, n_heads=n_heads)
        return hook
