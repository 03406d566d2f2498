"""CPU: the host models of the causal Q/K statistic (tests/qk_causal_model.py) against the explicit masked sums they stand for, the
switches, the finalisation scale, the decoder of over_full / shift_share, the cache metadata of the qk_causal / qk_causal_raw files, and
the case on which the causal and the full within-sequence rule select differently."""
import copy
import json

import numpy as np
import pytest
import torch

from modegpt_amd import calib_cache as cc
from modegpt_amd import reports
from tests import qk_causal_model as C
from tests import qk_pair_model as M

HD, G, B, T = 8, 2, 3, 40
KV = 2
H = KV * G


def rows(seed=0, offset=3):
    return M.lattice_rows(B, T, H, HD, seed), M.lattice_rows(B, T, KV, HD, seed + 1, offset=offset)


def test_identity_against_the_explicit_masked_sum():
    """1^T P[D,D] 1 = sum_s sum_i Var_{j<=i}(e_ij) and 1^T P_raw[D,D] 1 = sum_s sum_i mean_{j<=i}(e_ij^2), hd 8, g 2, B 3, T 40, random
    column sets D and all columns.  Both sides divide by n_i, so they agree to long-double rounding: under B T (T + hd^2) < 2^13
    roundings of 2^-64 on either side, relative to sums no larger than the raw one."""
    q, k = rows()
    P, R, A = C.longdouble_causal(q, k, B, T, H, KV, HD)
    gen = np.random.default_rng(3)
    for trial in range(4):
        D = sorted(gen.choice(HD, size=int(gen.integers(1, HD + 1)), replace=False).tolist()) if trial else list(range(HD))
        var, ms = C.brute_force_causal(q, k, B, T, H, KV, HD, D)
        for h in range(H):
            assert abs(P[h][np.ix_(D, D)].sum() - var[h]) <= 2.0 ** -48 * ms[h]
            assert abs(R[h][np.ix_(D, D)].sum() - ms[h]) <= 2.0 ** -48 * ms[h]
            assert 0 <= var[h] <= ms[h]
    slack = M.LD(1) + M.LD(2) ** -50                                                   # (the scale's square roots round)
    assert (np.abs(P) <= A * slack).all() and (np.abs(R) <= A * slack).all()


def test_a_constant_key_offset_moves_raw_but_not_the_centred_statistic():
    """k_j -> k_j + c changes e_ij by q_iD . c, a function of i alone: every row's variance over its keys stays."""
    q, k0 = rows(offset=0)
    k3 = (k0.float() + 3.0).to(torch.bfloat16)
    P0, R0, _ = C.longdouble_causal(q, k0, B, T, H, KV, HD)
    P3, R3, A3 = C.longdouble_causal(q, k3, B, T, H, KV, HD)
    assert (np.abs(P0 - P3) <= 2.0 ** -48 * A3).all() and (np.abs(R0 - R3).max() > 1e-3 * np.abs(R3).max())


def test_one_token_gives_exactly_zero_and_p_is_psd():
    q, k = M.lattice_rows(B, 1, H, HD, 3), M.lattice_rows(B, 1, KV, HD, 4, offset=3)
    P, R, _ = C.longdouble_causal(q, k, B, 1, H, KV, HD)
    assert (P == 0).all() and R.max() > 0
    q, k = rows(seed=7)
    P, R, _ = C.longdouble_causal(q, k, B, T, H, KV, HD)
    for Mx in (P, R):
        S = Mx.astype(np.float64)
        assert np.array_equal(S, S.transpose(0, 2, 1))
        assert (np.linalg.eigvalsh(S) >= -1e-9 * np.abs(S).max()).all()


def test_rational_model_is_the_rounded_long_double_model_and_its_own_fractions():
    """exact_causal against the token-by-token Fraction recurrence (bit for bit) and against the long-double model (whose error is
    far below one fp64 ulp of the scale)."""
    b, t, h, kv, hd = 2, 7, 2, 1, 4
    q, k = M.lattice_rows(b, t, h, hd, 5), M.lattice_rows(b, t, kv, hd, 6, offset=3)
    Pe, Re = C.exact_causal(q, k, b, t, h, kv, hd)
    Pf, Rf = C.exact_causal_fractions(q, k, b, t, h, kv, hd)
    assert torch.equal(Pe.view(torch.int64), Pf.view(torch.int64)) and torch.equal(Re.view(torch.int64), Rf.view(torch.int64))
    P, R, A = C.longdouble_causal(q, k, b, t, h, kv, hd)
    assert (np.abs(Pe.numpy().astype(M.LD) - P) <= 2.0 ** -52 * A).all() and (np.abs(Re.numpy().astype(M.LD) - R) <= 2.0 ** -52 * A).all()
    # n = 1, 2 only: every division is by a power of two and the values are dyadic -- exact in fp64, equal to the long double ones
    q2, k2 = M.lattice_rows(3, 2, h, hd, 8), M.lattice_rows(3, 2, kv, hd, 9, offset=3)
    P2e, R2e = C.exact_causal(q2, k2, 3, 2, h, kv, hd)
    P2, R2, _ = C.longdouble_causal(q2, k2, 3, 2, h, kv, hd)
    assert np.array_equal(P2e.numpy().astype(M.LD), P2) and np.array_equal(R2e.numpy().astype(M.LD), R2)


def test_bound_is_the_headers_formula():
    A = np.full((1, 2, 2), 8.0, dtype=M.LD)
    assert float(C.bound(A, 5, 100)[0, 0, 0]) == (4 * 100 + 5 + 8) * 2.0 ** -53 * 8.0


# ---------------------------------------------------------------- switches, finalisation
SELECTS = ("MODEGPT_QK_CAUSAL_SELECT", "MODEGPT_QK_SEQ_SELECT", "MODEGPT_QK_ROPE_SELECT")


def test_switches_are_read_when_asked_and_the_select_switches_exclude_each_other(monkeypatch):
    for name, fn in (("MODEGPT_QK_CAUSAL", reports.qk_causal_enabled), ("MODEGPT_QK_CAUSAL_SELECT", reports.qk_causal_select_enabled)):
        monkeypatch.delenv(name, raising=False)
        assert fn() is False
        monkeypatch.setenv(name, "1")
        assert fn() is True
        monkeypatch.setenv(name, "0")
        assert fn() is False
    from modegpt_amd import ops
    assert ops.qk_causal_enabled is reports.qk_causal_enabled and ops.qk_causal_select_enabled is reports.qk_causal_select_enabled
    assert ops.decode_qk_causal_error is reports.decode_qk_causal_error
    for name in SELECTS:
        monkeypatch.delenv(name, raising=False)
    assert reports.qk_select_statistic() == "default"
    for name, kind in zip(SELECTS, ("causal", "seq", "rope")):
        monkeypatch.setenv(name, "1")
        assert reports.qk_select_statistic() == kind
        monkeypatch.delenv(name)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        monkeypatch.setenv(SELECTS[a], "1")
        monkeypatch.setenv(SELECTS[b], "1")
        with pytest.raises(RuntimeError, match=f"{SELECTS[a]}=1 and {SELECTS[b]}=1 are both set: the pair selection takes one statistic"):
            reports.qk_select_statistic()
        monkeypatch.delenv(SELECTS[a])
        monkeypatch.delenv(SELECTS[b])
    for name in SELECTS:
        monkeypatch.setenv(name, "1")
    with pytest.raises(RuntimeError, match="are all set"):
        reports.qk_select_statistic()


def test_collected_rules(monkeypatch, caplog):
    import logging
    from types import SimpleNamespace
    from modegpt_amd import calibration
    log = logging.getLogger("test_qk_causal")
    for name in ("MODEGPT_QK_CAUSAL", "MODEGPT_QK_ROPE", "MODEGPT_QK_SEQ"):
        monkeypatch.delenv(name, raising=False)
    llama = SimpleNamespace(arch="llama", head_dim=64)
    assert calibration.qk_causal_collected(llama) is False
    monkeypatch.setenv("MODEGPT_QK_CAUSAL", "1")
    with pytest.raises(RuntimeError, match="MODEGPT_QK_CAUSAL=1 needs MODEGPT_QK_ROPE=1"):
        calibration.qk_causal_collected(llama)
    monkeypatch.setenv("MODEGPT_QK_ROPE", "1")
    assert calibration.qk_causal_collected(llama) is True and calibration.qk_seq_collected(llama) is False     # independent of QK_SEQ
    assert calibration.qk_causal_collected(SimpleNamespace(arch="qwen2", head_dim=128)) is True
    with pytest.raises(RuntimeError, match="head_dim 256 > 128"):
        calibration.qk_causal_collected(SimpleNamespace(arch="llama", head_dim=256))
    for arch, level in (("qwen3", logging.WARNING), ("opt", logging.INFO)):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="test_qk_causal"):
            assert calibration.qk_causal_collected(SimpleNamespace(arch=arch, head_dim=64), log) is False
        said = [r for r in caplog.records if "MODEGPT_QK_CAUSAL=1" in r.getMessage()]
        assert len(said) == 1 and said[0].levelno == level


def test_finalisation_scale():
    """finalize multiplies the causal sums by 1 / (n_texts TOKENS_PER_TEXT_NORMALISER): ONE token normaliser, every query row being
    a mean over its keys already; the full within-sequence statistic beside it takes the square."""
    from modegpt_amd import calibration
    sig = calibration.SigmaBuffers.__new__(calibration.SigmaBuffers)
    one = lambda: [torch.full((2, 4, 4), 3.0, dtype=torch.float64)]          # noqa: E731
    sig.layers, sig.lists = [0], {k: [torch.zeros(2, 2, dtype=torch.float64)] for k in ("mlp", "x", "q", "k")}
    sig.extra = {kind: one() for kind in ("qk_pair", "qk_pair_raw", "qk_causal", "qk_causal_raw")}      # (the means and the post-RoPE pair: absent)
    import modegpt_amd.ops as ops
    real = ops.cov_finalize
    ops.cov_finalize = lambda *a, **kw: None                                 # (the four device statistics are not this test's)
    try:
        sig.finalize(5)
    finally:
        ops.cov_finalize = real
    n = calibration.TOKENS_PER_TEXT_NORMALISER
    assert bool((sig.extra["qk_causal"][0] == 3.0 * (1.0 / (5 * n))).all()) and bool((sig.extra["qk_causal_raw"][0] == 3.0 * (1.0 / (5 * n))).all())
    assert bool((sig.extra["qk_pair"][0] == 3.0 * (1.0 / (5 * n ** 2))).all()) and bool((sig.extra["qk_pair_raw"][0] == 3.0 * (1.0 / (5 * n ** 2))).all())
    assert sig.value("qk_causal")[0] is sig.extra["qk_causal"] and sig.value("qk_causal")[1] is sig.extra["qk_causal_raw"]
    assert sig.value("qk_rope") is None and sig.value("mlp_mean") is None and sig.value("x_mean") is None     # absent: skipped
    del sig.extra["qk_causal"], sig.extra["qk_causal_raw"]
    assert sig.value("qk_causal") is None


# ---------------------------------------------------------------- the decoder
def test_decode_of_over_full_and_shift_share():
    curve_h = [[10.0, 4.0, 1.0, 0.0], [6.0, 2.0, 1.0, 0.0], [8.0, 3.0, 0.5, 0.0], [8.0, 1.0, 0.5, 0.0]]
    curve = [[16.0, 6.0, 2.0, 0.0], [16.0, 4.0, 1.0, 0.0]]
    raw = [[64.0, 24.0, 16.0, 0.0], [32.0, 4.0, 2.0, 0.0]]
    seq = reports.decode_qk_seq_error(curve_h, [[32.0, 12.0, 2.0, 0.0], [16.0, 16.0, 1.0, 0.0]], raw, 2, 2)
    base = reports.decode_qk_seq_error(curve_h, curve, raw, 2, 2)
    out = reports.decode_qk_causal_error(curve_h, curve, raw, 2, 2, seq=seq)
    assert [h["raw_error"] for h in out["heads"]] == [24.0, 4.0]
    assert [h["shift_share"] for h in out["heads"]] == [1.0 - 6.0 / 24.0, 0.0]
    assert [h["over_full"] for h in out["heads"]] == [6.0 / 12.0, 4.0 / 16.0]
    assert out["over_full"] == 10.0 / 28.0 and out["shift_share"] == 1.0 - 10.0 / 28.0
    for key in base:
        if key != "heads":
            assert out[key] == base[key]
    for hb, ho in zip(base["heads"], out["heads"]):
        assert {k: ho[k] for k in hb} == hb
    json.dumps(out, allow_nan=False)
    # without a seq entry: the seq decoder's fields and no over_full
    alone = reports.decode_qk_causal_error(curve_h, curve, raw, 2, 2)
    assert alone == base and "over_full" not in alone
    # a seq error that is zero or not finite -> None, never NaN or a division by zero
    bad = copy.deepcopy(seq)
    bad["heads"][0]["error"], bad["error"] = 0.0, None
    nan = reports.decode_qk_causal_error(curve_h, curve, raw, 2, 2, seq=bad)
    assert nan["heads"][0]["over_full"] is None and nan["over_full"] is None and nan["heads"][1]["over_full"] == 0.25
    json.dumps(nan, allow_nan=False)
    with pytest.raises(ValueError, match="same rank"):
        reports.decode_qk_causal_error(curve_h, curve, raw, 4, 2, seq=seq)


# ---------------------------------------------------------------- cache metadata
ARCH = {"arch": "llama", "d_model": 6, "n_inner": 9, "n_heads": 2, "n_kv_heads": 1, "head_dim": 3, "n_layers": 4,
        "dtype": "torch.bfloat16"}


def test_cache_metadata_round_trip_and_refusals(tmp_path):
    d = str(tmp_path)
    g = np.random.default_rng(1)
    files, values = {}, {}
    assert tuple(cc.CAUSAL_KINDS) == ("qk_causal", "qk_causal_raw") and tuple(cc.PAIR_KINDS) == ("qk_pair", "qk_pair_raw")
    for kind in ("q",) + tuple(cc.CAUSAL_KINDS):
        n, batch = cc.stat_shapes(ARCH)[cc.EXTRA_KINDS.get(kind, kind)]
        values[kind] = g.standard_normal(batch * n * n)
        files[kind] = cc.write_data_file(d, 1, kind, values[kind], n, batch)
    assert files["qk_causal"]["file"] == "layer_1_qk_causal.f64" and files["qk_causal_raw"]["file"] == "layer_1_qk_causal_raw.f64"
    meta = {"files": files}
    for kind in cc.CAUSAL_KINDS:
        entry = cc.validate_extra_entry(meta, ARCH, 1, kind)
        assert {k: entry[k] for k in ("n", "batch", "bytes", "layout")} == {k: files["q"][k] for k in ("n", "batch", "bytes", "layout")}
        out = np.empty(values[kind].size)
        cc.read_data_file(d, 1, kind, entry, out)
        assert np.array_equal(out.view(np.int64), values[kind].view(np.int64))
    with pytest.raises(ValueError, match=r"layer 1\b.*files\.qk_causal_raw is missing.*MODEGPT_QK_CAUSAL=1"):
        cc.validate_extra_entry({"files": {k: v for k, v in files.items() if k != "qk_causal_raw"}}, ARCH, 1, "qk_causal_raw")
    with pytest.raises(ValueError, match=r"layer 1\b.*files\.qk_pair is missing.*MODEGPT_QK_SEQ=1"):
        cc.validate_extra_entry(meta, ARCH, 1, "qk_pair")
    for field, value in (("n", 4), ("batch", 1), ("bytes", 8), ("layout", "packed_lower")):
        broken = copy.deepcopy(meta)
        broken["files"]["qk_causal"][field] = value
        with pytest.raises(ValueError, match=rf"layer 1\b.*files\.qk_causal\.{field}\b"):
            cc.validate_extra_entry(broken, ARCH, 1, "qk_causal")
    broken = copy.deepcopy(meta)
    broken["files"]["qk_causal"]["trace_bits"] += 1
    with pytest.raises(ValueError, match=r"layer 1\b.*qk_causal"):
        cc.read_data_file(d, 1, "qk_causal", broken["files"]["qk_causal"], np.empty(values["qk_causal"].size))


# ---------------------------------------------------------------- the two rules disagree where they should
def disagreement(where, amplitude, T=0):
    d = C.DIS
    T = T or d["T"]
    q, k = C.disagreement_rows(where, amplitude, T=T)
    Pc = C.longdouble_causal(q, k, d["B"], T, d["H"], d["KV"], d["hd"])[0]
    Pf = M.longdouble_pair(q, k, d["B"], T, d["H"], d["KV"], d["hd"])[0]
    keep = d["hd"] // 4                                                       # rank hd / 2 = hd / 4 rotary units
    return C.margins(C.unit_scores(Pc, d["KV"])[0], d["special"], keep), C.margins(C.unit_scores(Pf, d["KV"])[0], d["special"], keep), keep


def test_a_late_component_is_kept_by_the_full_rule_and_dropped_by_the_causal_rule():
    """Key amplitude 24 on the last two tokens of each sequence only: every query sees it in the full statistic, two queries per
    sequence under the mask.  In long double (B 2, T 24, 2 / 1 heads of 16, seed 5): the full rule ranks the unit FIRST with
    2.75 x the score of the best dropped unit; the causal rule ranks it LAST with 0.30 x the score of the weakest kept unit."""
    (c_rank, c_ratio), (f_rank, f_ratio), keep = disagreement("late", 24.0)
    print("LATE: full rank %d ratio %.3f, causal rank %d ratio %.3f" % (f_rank, f_ratio, c_rank, c_ratio))
    assert f_rank < keep and f_ratio >= 2.0
    assert c_rank >= keep and c_ratio <= 0.5


MIRROR_T = 512


def test_a_first_token_component_is_kept_by_the_causal_rule_and_dropped_by_the_full_rule():
    """The mirror: a key amplitude on token 0 only (an attention sink), margins of 2 on both sides as above.  With independent unit
    queries the unit's score over the other units' is A^2 S_1 / (sigma^2 S_2) under the mask, S_1 = sum_n (1/n - 1/n^2),
    S_2 = sum_n (1 - 1/n), and A^2 / (T sigma^2) without it: the two ratios differ by the factor T S_1 / S_2 whatever the amplitudes --
    2.58 at T = 24, where margins of 2 on both sides (a factor of 4) are therefore out of reach, and growing like ln T.  So the
    mirror case alone runs at T = 512 (factor 5.2), amplitude 60.  In long double (B 2, 2 / 1 heads of 16, seed 5): the causal rule
    ranks the unit FIRST with 2.35 x the score of the best dropped unit, the full rule LAST with 0.447 x the weakest kept unit's."""
    (c_rank, c_ratio), (f_rank, f_ratio), keep = disagreement("first", 60.0, T=MIRROR_T)
    print("FIRST: causal rank %d ratio %.3f, full rank %d ratio %.3f" % (c_rank, c_ratio, f_rank, f_ratio))
    assert c_rank < keep and c_ratio >= 2.0
    assert f_rank >= keep and f_ratio <= 0.5
