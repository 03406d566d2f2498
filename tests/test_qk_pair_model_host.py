"""CPU: the host models of the within-sequence Q/K statistic (tests/qk_pair_model.py) against the explicit sums they stand for, the
decoder of shift_share, and the cache metadata of the qk_pair / qk_pair_raw files."""
import copy
import json

import numpy as np
import pytest
import torch

from modegpt_amd import calib_cache as cc
from modegpt_amd import reports
from tests import qk_pair_model as M

HD, G, B, T = 8, 2, 3, 40
KV = 2
H = KV * G


def rows(seed=0, offset=3):
    return M.lattice_rows(B, T, H, HD, seed), M.lattice_rows(B, T, KV, HD, seed + 1, offset=offset)


def test_identity_against_the_explicit_double_sum():
    """1^T P[D,D] 1 = sum_s sum_i sum_j (e_ij - mean_j e_ij)^2 and 1^T P_raw[D,D] 1 = sum e_ij^2: integer rows, so the long-double
    raw sums are exact and EQUAL; the centred ones divide by T = 40 and agree to long-double rounding.  Random column sets D and all columns."""
    q, k = rows()
    P, R, scale = M.longdouble_pair(q, k, B, T, H, KV, HD)
    gen = np.random.default_rng(3)
    for trial in range(4):
        D = sorted(gen.choice(HD, size=int(gen.integers(1, HD + 1)), replace=False).tolist()) if trial else list(range(HD))
        var, ms = M.brute_force(q, k, B, T, H, KV, HD, D)
        for h in range(H):
            # (long double: under B T^2 + hd^2 < 2^13 roundings of 2^-64 on either side, relative to sums no larger than ms)
            assert abs(P[h][np.ix_(D, D)].sum() - var[h]) <= 2.0 ** -48 * ms[h]
            assert R[h][np.ix_(D, D)].sum() == ms[h]
            assert var[h] <= ms[h]
    slack = M.LD(1) + M.LD(2) ** -60                                                   # (the scale's square roots round)
    assert (np.abs(P) <= scale * slack).all() and (np.abs(R) <= scale * slack).all()


def test_p_is_positive_semidefinite_and_symmetric():
    q, k = rows(seed=7)
    P, R, _ = M.longdouble_pair(q, k, B, T, H, KV, HD)
    for Mx in (P, R):
        A = Mx.astype(np.float64)
        assert np.array_equal(A, A.transpose(0, 2, 1))
        assert (np.linalg.eigvalsh(A) >= -1e-9 * np.abs(A).max()).all()


def test_rational_model_equals_the_long_double_model_on_the_lattice():
    """T = 40 is no power of two: the rational model holds T P in Python ints; T P equals T x the long-double P exactly
    (40 P is an integer below 2^64)."""
    q, k = rows(seed=11)
    P, R, _ = M.longdouble_pair(q, k, B, T, H, KV, HD)
    with pytest.raises(AssertionError, match="not exact"):
        M.exact_pair(q, k, B, T, H, KV, HD)                                   # m m^T / 40 is not a dyadic rational
    q2, k2 = M.lattice_rows(B, 16, H, HD, 5), M.lattice_rows(B, 16, KV, HD, 6, offset=3)
    Pe, Re = M.exact_pair(q2, k2, B, 16, H, KV, HD)
    P2, R2, _ = M.longdouble_pair(q2, k2, B, 16, H, KV, HD)
    assert np.array_equal(Pe.numpy().astype(M.LD), P2) and np.array_equal(Re.numpy().astype(M.LD), R2)
    assert R.max() > 0 and P.shape == (H, HD, HD)


def test_one_sequence_raw_is_the_hadamard_product_of_the_grams():
    q, k = M.lattice_rows(1, T, H, HD, 21), M.lattice_rows(1, T, KV, HD, 22, offset=3)
    _, R, _ = M.longdouble_pair(q, k, 1, T, H, KV, HD)
    Q = q.double().numpy().reshape(T, H, HD)
    K = k.double().numpy().reshape(T, KV, HD)
    for h in range(H):
        want = (Q[:, h].T @ Q[:, h]) * (K[:, h // G].T @ K[:, h // G])
        assert np.array_equal(R[h].astype(np.float64), want)


def test_a_constant_key_offset_moves_raw_but_not_the_centred_statistic():
    """The shift invariance itself: k_j -> k_j + c changes e_ij by q_iD . c, a function of i alone."""
    q, k0 = rows(offset=0)
    k3 = (k0.float() + 3.0).to(torch.bfloat16)
    P0, R0, _ = M.longdouble_pair(q, k0, B, T, H, KV, HD)
    P3, R3, scale3 = M.longdouble_pair(q, k3, B, T, H, KV, HD)
    assert (np.abs(P0 - P3) <= 2.0 ** -48 * scale3).all() and (np.abs(R0 - R3).max() > 1e-3 * np.abs(R3).max())


def test_bound_is_the_headers_formula():
    scale = np.full((1, 2, 2), 8.0, dtype=M.LD)
    assert float(M.bound(scale, 5, 100)[0, 0, 0]) == (4 * 100 + 5 + 8) * 2.0 ** -53 * 8.0


# ---------------------------------------------------------------- the decoder
def test_decode_of_shift_share():
    curve_h = [[10.0, 4.0, 1.0, 0.0], [6.0, 2.0, 1.0, 0.0], [8.0, 3.0, 0.5, 0.0], [8.0, 1.0, 0.5, 0.0]]
    curve = [[16.0, 6.0, 2.0, 0.0], [16.0, 4.0, 1.0, 0.0]]
    raw = [[64.0, 24.0, 16.0, 0.0], [32.0, 4.0, 2.0, 0.0]]
    base = reports.decode_qk_logit_error(curve_h, curve, 2, 2)
    out = reports.decode_qk_seq_error(curve_h, curve, raw, 2, 2)
    assert out["units_kept"] == 1
    assert [h["raw_error"] for h in out["heads"]] == [24.0, 4.0]
    assert [h["shift_share"] for h in out["heads"]] == [1.0 - 6.0 / 24.0, 0.0]
    assert out["raw_error"] == 28.0 and out["shift_share"] == 1.0 - 10.0 / 28.0
    for key in base:
        if key != "heads":
            assert out[key] == base[key]
    for hb, ho in zip(base["heads"], out["heads"]):
        assert {k: ho[k] for k in hb} == hb
    json.dumps(out, allow_nan=False)
    # at full rank nothing is dropped: raw_error 0 -> no share; a non-finite raw figure -> None, never NaN in the JSON
    full = reports.decode_qk_seq_error(curve_h, curve, raw, 6, 2)
    assert full["raw_error"] == 0.0 and full["shift_share"] is None and all(h["shift_share"] is None for h in full["heads"])
    bad = copy.deepcopy(raw)
    bad[0][1] = float("nan")
    nan = reports.decode_qk_seq_error(curve_h, curve, bad, 2, 2)
    assert nan["heads"][0]["raw_error"] is None and nan["heads"][0]["shift_share"] is None and nan["shift_share"] is None
    assert nan["heads"][1]["shift_share"] == 0.0
    json.dumps(nan, allow_nan=False)
    with pytest.raises(ValueError, match="raw_curve"):
        reports.decode_qk_seq_error(curve_h, curve, [r[:-1] for r in raw], 2, 2)


def test_switches_are_read_when_asked(monkeypatch):
    for name, fn in (("MODEGPT_QK_SEQ", reports.qk_seq_enabled), ("MODEGPT_QK_SEQ_SELECT", reports.qk_seq_select_enabled)):
        monkeypatch.delenv(name, raising=False)
        assert fn() is False
        monkeypatch.setenv(name, "1")
        assert fn() is True
        monkeypatch.setenv(name, "0")
        assert fn() is False
    from modegpt_amd import ops
    assert ops.qk_seq_enabled is reports.qk_seq_enabled and ops.qk_seq_select_enabled is reports.qk_seq_select_enabled


# ---------------------------------------------------------------- cache metadata
ARCH = {"arch": "llama", "d_model": 6, "n_inner": 9, "n_heads": 2, "n_kv_heads": 1, "head_dim": 3, "n_layers": 4,
        "dtype": "torch.bfloat16"}


def test_cache_metadata_round_trip_and_refusals(tmp_path):
    d = str(tmp_path)
    g = np.random.default_rng(1)
    files, values = {}, {}
    for kind in ("q",) + tuple(cc.PAIR_KINDS):
        n, batch = cc.stat_shapes(ARCH)[cc.EXTRA_KINDS.get(kind, kind)]
        values[kind] = g.standard_normal(batch * n * n)
        files[kind] = cc.write_data_file(d, 1, kind, values[kind], n, batch)
    assert files["qk_pair"]["file"] == "layer_1_qk_pair.f64" and files["qk_pair_raw"]["file"] == "layer_1_qk_pair_raw.f64"
    meta = {"files": files}
    for kind in cc.PAIR_KINDS:
        entry = cc.validate_extra_entry(meta, ARCH, 1, kind)
        assert {k: entry[k] for k in ("n", "batch", "bytes", "layout")} == {k: files["q"][k] for k in ("n", "batch", "bytes", "layout")}
        out = np.empty(values[kind].size)
        cc.read_data_file(d, 1, kind, entry, out)
        assert np.array_equal(out.view(np.int64), values[kind].view(np.int64))
    # a record without the entry: refused on metadata alone, naming the layer, the field and the switch
    with pytest.raises(ValueError, match=r"layer 1\b.*files\.qk_pair_raw is missing.*MODEGPT_QK_SEQ=1"):
        cc.validate_extra_entry({"files": {k: v for k, v in files.items() if k != "qk_pair_raw"}}, ARCH, 1, "qk_pair_raw")
    with pytest.raises(ValueError, match=r"layer 1\b.*files\.q_rope is missing.*MODEGPT_QK_ROPE=1"):
        cc.validate_extra_entry(meta, ARCH, 1, "q_rope")
    for field, value in (("n", 4), ("batch", 1), ("bytes", 8), ("layout", "packed_lower")):
        broken = copy.deepcopy(meta)
        broken["files"]["qk_pair"][field] = value
        with pytest.raises(ValueError, match=rf"layer 1\b.*files\.qk_pair\.{field}\b"):
            cc.validate_extra_entry(broken, ARCH, 1, "qk_pair")
    broken = copy.deepcopy(meta)
    broken["files"]["qk_pair"]["trace_bits"] += 1
    with pytest.raises(ValueError, match=r"layer 1\b.*qk_pair"):
        cc.read_data_file(d, 1, "qk_pair", broken["files"]["qk_pair"], np.empty(values["qk_pair"].size))
