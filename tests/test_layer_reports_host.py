"""Host (no GPU): what ModelAdapter's per-layer reports write, return, keep and log, end to end on recorded payloads -- the three
two-number reports (MLP intercept, V/O intercept, v-bias residual), report_qk_errors on all four Q/K statistics -- and the order in
which run_modegpt.compress_chunk calls the report_* methods of an adapter that has only some of them.

CPU tensors pass through .cpu() unchanged, so the payloads are recorded as the compressors record them.  The expected figures are
written out by hand for the two-number reports; for the Q/K reports they are the decoders of modegpt_amd/reports.py (which have tests
of their own: test_reports_host.py, test_qk_error_host.py, test_qk_causal_model_host.py) applied to the recorded curves, plus the
fields the report adds.  The curves come from the host model of tests/qk_error_model.py."""
import json
import logging
import types

import numpy as np
import pytest
import torch

from tests import qk_error_model as QK

F64 = torch.float64
NAN = float("nan")
HD, N_HEADS, N_KV, RANK = 8, 4, 2, 4                          # RoPE: ns = 4 units of 2 columns, 2 kept


def adapter():
    from modegpt_amd import engine
    return engine.TensorAdapter(dict(engine.SHAPES["tiny"], head_dim=HD, n_heads=N_HEADS, n_kv_heads=N_KV), {})


def messages(caplog):
    return [(r.levelname, r.getMessage()) for r in caplog.records if r.name == "MoDeGPT"]


# ------------------------------------------------------------------ the two-number reports
PAIRS = {3: (2.0, 8.0), 0: (0.5, 0.0), 7: (NAN, 4.0), 5: (1e-3, 2.5e-1)}      # a zero denominator (0), a NaN (7)
TWO = [  # (recorder, report, metrics key, the two fields, log line)
    ("mlp_intercept", "report_mlp_intercepts", "mlp_intercept", ("offset_norm2", "mean_output_norm2"),
     "[MLP] Layer {}: the intercept carries {:.3e} of the mean output {:.3e} (squared norms)"),
    ("vo_intercept", "report_vo_intercepts", "vo_intercept", ("offset_norm2", "mean_output_norm2"),
     "[VO] Layer {}: the intercept carries {:.3e} of the mean output {:.3e} (squared norms)"),
    ("vo_bias_residual", "report_vo_bias_residuals", "vo_bias_residual", ("residual_norm2", "constant_norm2"),
     "[VO] Layer {}: the truncated v_proj loses {:.3e} of the v bias's output constant {:.3e} (squared norms)"),
]


@pytest.mark.parametrize("recorder,report,key,fields,line", TWO, ids=[t[0] for t in TWO])
def test_two_number_reports(caplog, recorder, report, key, fields, line):
    ad = adapter()
    for layer, pair in PAIRS.items():
        getattr(ad, recorder)(layer, torch.tensor(pair, dtype=F64))
    a, b = fields
    want = {0: {a: 0.5, b: 0.0, "relative": None}, 3: {a: 2.0, b: 8.0, "relative": 0.25}, 5: {a: 1e-3, b: 2.5e-1, "relative": 1e-3 / 2.5e-1},
            7: {a: None, b: None, "relative": None}}
    with caplog.at_level(logging.INFO, logger="MoDeGPT"):
        got = getattr(ad, report)()
    assert got == want and list(got) == [0, 3, 5, 7]
    assert ad.metrics == {key: {str(k): v for k, v in want.items()}}
    assert messages(caplog) == [("INFO", line.format(layer, *PAIRS[layer])) for layer in (0, 3, 5, 7)]
    json.dumps(ad.metrics)                                                       # (no NaN reaches the metrics file)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="MoDeGPT"):
        assert getattr(ad, report)() == {}                                       # read once
    assert messages(caplog) == [] and ad.metrics == {key: {str(k): v for k, v in want.items()}}
    # a later layer merges into the same key
    getattr(ad, recorder)(9, torch.tensor((1.0, 4.0), dtype=F64))
    assert getattr(ad, report)(logging.getLogger("MoDeGPT")) == {9: {a: 1.0, b: 4.0, "relative": 0.25}}
    assert sorted(ad.metrics[key]) == ["0", "3", "5", "7", "9"]


# ------------------------------------------------------------------ report_qk_errors
def curves(seed, zero=False, raw_seed=None):
    """qk_rank_curve's (curve_h, curve, terms, scale, greedy_curve, greedy_order) + (order,) [+ (raw_curve,)] as CPU tensors."""
    cov_q, cov_k = QK.full_rank(N_HEADS, HD, seed), QK.full_rank(N_KV, HD, seed + 1)
    if zero:
        cov_q, cov_k = cov_q * 0, cov_k * 0
    ns = HD // 2
    order = np.stack([np.random.default_rng(seed + kv).permutation(ns) for kv in range(N_KV)])
    g_order = np.ascontiguousarray(order[:, ::-1])
    m = QK.model(cov_q, cov_k, QK.ROPE_GROUPED, 0.0, 0.0, order, dtype=np.float64)
    greedy = QK.model(cov_q, cov_k, QK.ROPE_GROUPED, 0.0, 0.0, g_order, dtype=np.float64)["curve"]
    terms = QK.terms(cov_q, cov_k, QK.ROPE_GROUPED, 1e-4, 1e-2, order).astype(np.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                                              # noqa: E731
    out = (t(m["curve_h"]), t(m["curve"]), t(terms), t(m["A"][:, 0]), t(greedy), t(g_order), t(order))
    if raw_seed is not None:
        rq, rk = QK.full_rank(N_HEADS, HD, raw_seed) * 3, QK.full_rank(N_KV, HD, raw_seed + 1)
        out += (t(QK.model(rq, rk, QK.ROPE_GROUPED, 0.0, 0.0, order, dtype=np.float64)["curve"]),)
    return out


def decoded(decoder, tensors, **more):
    from modegpt_amd import ops
    ch, cv, terms, scale, greedy = tensors[:5]
    raw = (tensors[7].tolist(),) if len(tensors) > 7 else ()
    return getattr(ops, decoder)(ch.tolist(), cv.tolist(), *raw, RANK, 2, terms=terms.tolist(), scale=scale.tolist(),
                                 greedy_curve=greedy.tolist(), **more)


def show(v):
    return "n/a" if v is None else f"{v:.3e}"


def test_report_qk_errors_on_all_four_statistics(caplog):
    ad = adapter()
    pre = {2: curves(10), 5: curves(20, zero=True)}              # layer 5: no usable energy
    rope = {2: curves(30), 5: curves(40)}
    seq = {2: curves(50, raw_seed=60)}                           # (layer 5 has the causal statistic alone)
    causal = {5: curves(90, raw_seed=100), 2: curves(70, raw_seed=80)}
    for layer, t in pre.items():
        ad.qk_error(layer, t, RANK)
    for layer, t in rope.items():
        ad.qk_error_rope(layer, list(t), RANK)
    for layer, t in seq.items():
        ad.qk_error_seq(layer, t, RANK)
    for layer, t in causal.items():
        ad.qk_error_causal(layer, t, RANK)

    want_pre = {layer: decoded("decode_qk_logit_error", pre[layer]) for layer in (2, 5)}
    assert want_pre[5]["relative_error"] is None and want_pre[2]["relative_error"] is not None
    want_rope = {layer: dict(decoded("decode_qk_logit_error", rope[layer]), statistic="post_rope",
                             pre_rope_relative_error=want_pre[layer]["relative_error"]) for layer in (2, 5)}
    want_seq = {2: dict(decoded("decode_qk_seq_error", seq[2]), statistic="within_sequence")}
    want_causal = {layer: dict(decoded("decode_qk_causal_error", causal[layer], seq=want_seq.get(layer)), statistic="within_sequence_causal")
                   for layer in (2, 5)}
    assert "over_full" in want_causal[2] and "over_full" not in want_causal[5]

    with caplog.at_level(logging.INFO, logger="MoDeGPT"):
        got = ad.report_qk_errors()
    assert got == want_pre and list(got) == [2, 5]
    assert ad.metrics == {"qk_logit_error": {str(k): v for k, v in want_pre.items()},
                          "qk_logit_error_rope": {str(k): v for k, v in want_rope.items()},
                          "qk_logit_error_seq": {str(k): v for k, v in want_seq.items()},
                          "qk_logit_error_causal": {str(k): v for k, v in want_causal.items()}}
    assert list(ad.metrics) == ["qk_logit_error", "qk_logit_error_rope", "qk_logit_error_seq", "qk_logit_error_causal"]
    json.dumps(ad.metrics)

    m = want_pre[2]
    lines = [("INFO", f"[QK] Layer 2: rank {RANK}: the kept columns lose {m['relative_error']:.3e} of the logit energy"
              f"; the diagonal rule's estimate is {m['diagonal_ratio']:.3g} x that"
              f"; a greedy order on the full objective loses {m['greedy_relative_error']:.3e}"
              + ("; NOT monotone in the rank" if m["non_monotone"] else "")),
             ("WARNING", f"[QK] Layer 5: logit error has no usable energy (energy {want_pre[5]['energy']!r}, error {want_pre[5]['error']!r})")]
    for layer in (2, 5):
        m = want_rope[layer]
        lines.append(("INFO", f"[QK] Layer {layer}: rank {RANK}: of the post-RoPE logit energy the kept columns lose {show(m['relative_error'])} "
                      f"(exact for a rotary model); the pre-RoPE statistic said {show(want_pre[layer]['relative_error'])}"))
    m = want_seq[2]
    lines.append(("INFO", f"[QK] Layer 2: rank {RANK}: within-sequence, shift-invariant logit error {show(m['error'])} "
                  f"({show(m['relative_error'])} of its energy); {show(m['shift_share'])} of the uncentred change is invisible to softmax"))
    for layer in (2, 5):
        m = want_causal[layer]
        lines.append(("INFO", f"[QK] Layer {layer}: rank {RANK}: causal within-sequence logit error {show(m['error'])} "
                      f"({show(m['relative_error'])} of its energy); {show(m['shift_share'])} of the uncentred change is invisible to softmax"
                      + (f"; {show(m['over_full'])} x the figure without the causal mask" if layer == 2 else "")))
    assert "n/a" in lines[3][1]                                  # (layer 5's pre-RoPE figure beside its post-RoPE one)
    assert messages(caplog) == lines

    # the host copies: every recorded tensor, in the order recorded, under the public attribute
    for name, recorded in (("qk_errors", pre), ("qk_errors_rope", rope), ("qk_errors_seq", seq), ("qk_errors_causal", causal)):
        kept = getattr(ad, name)
        assert sorted(kept) == sorted(recorded), name
        for layer, tensors in recorded.items():
            assert isinstance(kept[layer], tuple) and len(kept[layer]) == len(tensors), (name, layer)
            assert all(k.device.type == "cpu" and torch.equal(k, t) for k, t in zip(kept[layer], tensors)), (name, layer)

    before = json.dumps(ad.metrics, sort_keys=True)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="MoDeGPT"):
        assert ad.report_qk_errors() == {}                       # read once
    assert messages(caplog) == [] and json.dumps(ad.metrics, sort_keys=True) == before
    # a statistic recorded without the pre-RoPE one still reports; the return value stays the (empty) pre-RoPE report
    ad.qk_error_causal(6, causal[5], RANK)
    assert ad.report_qk_errors() == {}
    assert ad.metrics["qk_logit_error_causal"]["6"] == want_causal[5] and sorted(ad.metrics["qk_logit_error_causal"]) == ["2", "5", "6"]
    assert sorted(ad.qk_errors_causal) == [2, 5, 6]


def test_a_missing_greedy_curve_is_passed_as_none():
    ad = adapter()
    t = curves(10)
    ad.qk_error(1, t[:4] + (None, None) + t[6:], RANK)
    got = ad.report_qk_errors()
    assert got[1]["greedy_relative_error"] is None and got[1]["heads"][0]["rank_for_rel_error"]["greedy"] is None
    assert ad.qk_errors[1][4] is None and ad.qk_errors[1][5] is None and torch.equal(ad.qk_errors[1][6], t[6])


# ------------------------------------------------------------------ the order run_modegpt calls the reports in
ALL_REPORTS = ["report_selection_margins", "report_mlp_greedy", "report_rank_curves", "report_output_errors", "report_mlp_intercepts",
               "report_vo_intercepts", "report_vo_errors", "report_qk_errors", "report_vo_bias_residuals", "report_attention_margins"]


@pytest.mark.parametrize("have", [ALL_REPORTS, ALL_REPORTS[2::2] + ALL_REPORTS[3:4], []], ids=["all", "half", "none"])
def test_compress_chunk_calls_the_reports_an_adapter_has_in_order(monkeypatch, have):
    from modegpt_amd import run_modegpt as R
    calls = []

    class Stub:
        n_layers = 4

    stub = Stub()
    for name in have:
        setattr(stub, name, lambda log, name=name: calls.append((name, log)))
    monkeypatch.setattr(R, "load_calibs", lambda **kw: (None, None, None, None, [0.0] * 4))
    monkeypatch.setattr(R, "allocate_global_sparsity", lambda *a, **kw: None)
    monkeypatch.setattr(R, "_free", lambda: None)
    monkeypatch.setattr(R.sharding, "gather_layer_artifacts", lambda adapter, chunk, mine, masks, rank, world: ("gathered", list(chunk), masks))
    monkeypatch.delenv("MODEGPT_CALIBS_SAVE", raising=False)
    monkeypatch.delenv("MODEGPT_CALIBS_LOAD", raising=False)
    config = types.SimpleNamespace(calib_size=1, calibs_batch_size=1, dataset="none", compression_ratio=0.5, sparsity_smoothing=0.0,
                                   max_sparsity=0.9, order="nothing")
    assert R.compress_chunk(stub, config, [0, 1], 0, 1) == ("gathered", [0, 1], [])
    assert [c[0] for c in calls] == [name for name in ALL_REPORTS if name in have]
    assert all(c[1] is R.logger for c in calls)
    assert ALL_REPORTS.index("report_rank_curves") < ALL_REPORTS.index("report_output_errors") and ALL_REPORTS[-1] == "report_attention_margins"
