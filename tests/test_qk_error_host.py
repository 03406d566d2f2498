"""Host (no GPU): the identity behind the Q/K logit error, E(D) = mean over token pairs of (sum_{c in D} q_ic k_jc)^2 =
<C_q[D, D], C_k[D, D]>_F, against an explicit T x T sum; the long-double model (tests/qk_error_model.py) against the same route in
plain fp64 within the a-priori bound of include/modegpt_hip.h; and ops.decode_qk_logit_error / ops.qk_error_enabled, which read lists."""
import json
import math

import numpy as np
import pytest
import torch

from tests import qk_error_model as QK

LD, U = QK.LD, QK.U


def test_identity_against_the_explicit_token_pair_sum():
    hd, g, T = 16, 2, 400
    rng = np.random.default_rng(5)
    mix = lambda: np.eye(hd) + 0.3 * rng.standard_normal((hd, hd))            # noqa: E731
    Xq = [(rng.standard_normal((T, hd)) @ mix()).astype(LD) for _ in range(g)]
    Xk = (rng.standard_normal((T, hd)) @ mix()).astype(LD)
    cov_q = np.stack([x.T @ x / T for x in Xq])                              # long double: the identity itself, no fp64 rounding of sigma
    cov_k = (Xk.T @ Xk / T)[None]
    ns = hd // 2
    order = rng.permutation(ns)[None]
    curve, A = QK.objective(cov_q, cov_k, QK.ROPE_GROUPED, 0.0, 0.0, order)
    worst = 0.0
    for m in range(ns + 1):
        D = np.concatenate([order[0][m:], order[0][m:] + ns]).astype(np.int64)
        explicit = sum(((x[:, D] @ Xk[:, D].T) ** 2).mean() for x in Xq)     # the T x T logit changes of every head of the group
        assert abs(curve[0][m] - explicit) <= T * U * abs(explicit), (m, curve[0][m], explicit)
        worst = max(worst, float(abs(curve[0][m] - explicit) / explicit) if explicit else 0.0)
    assert curve[0][ns] == 0 and curve[0][0] > 0
    print("IDENTITY worst relative difference %.2e (allowed %.2e)" % (worst, T * U))


def test_non_monotone_example_is_reported_raw():
    from modegpt_amd import ops
    P = np.array([[1.0, -0.81], [-0.81, 1.0]])
    curve = [float(P.sum()), float(P[1, 1]), 0.0]                            # both columns dropped, one, none
    assert abs(curve[0] - 0.38) < 1e-15 and curve[1] == 1.0
    m = ops.decode_qk_logit_error([curve], [curve], 1, 1, scale=[float(np.abs(P).sum())])
    assert m["non_monotone"] is True and m["heads"][0]["non_monotone"] is True
    assert m["error"] == 1.0 and m["energy"] == curve[0]
    assert m["relative_error"] == 1.0 / curve[0] > 1.0                       # raw: never clamped to the energy
    assert m["heads"][0]["rank_for_rel_error"]["selection"] == {"0.1": 2, "0.01": 2, "0.001": 2}
    mono = ops.decode_qk_logit_error([[2.0, 1.0, 0.0]], [[2.0, 1.0, 0.0]], 1, 1, scale=[2.0])
    assert mono["non_monotone"] is False


@pytest.mark.parametrize("hd", [8, 64, 128])
def test_plain_fp64_stays_within_the_a_priori_bound(hd):
    g, n_kv = 2, 2
    for name, build in QK.BUILDERS.items():
        cov_q, cov_k = build(g * n_kv, hd, seed=hd), build(n_kv, hd, seed=hd + 1)
        for mode, (rq, rk) in ((QK.ROPE_GROUPED, (1e-4, 1e-2)), (QK.ROPE_GROUPED, (0.0, 0.0))):
            ns, _ = QK.units(mode, hd)
            order = np.stack([np.random.default_rng(kv).permutation(ns) for kv in range(n_kv)])
            ref = QK.model(cov_q, cov_k, mode, rq, rk, order)
            f64 = QK.model(cov_q, cov_k, mode, rq, rk, order, dtype=np.float64)
            for key, scale, terms_ in (("curve_h", "A_h", hd * hd + 2), ("curve", "A", g * hd * hd + 2)):
                bound = terms_ * U * ref[scale]
                err = np.abs(f64[key].astype(LD) - ref[key])
                assert bool((err <= bound).all()), (name, key, float((err / np.maximum(bound, 1e-300)).max()))
                live = bound > 0
                print("FP64 hd=%d %s %s rho=(%g, %g): largest error / bound %.2e" % (hd, name, key, rq, rk, float((err[live] / bound[live]).max())))
            assert bool((ref["curve"] >= -g * hd * hd * U * ref["A"]).all())         # PSD by Schur: never below zero beyond rounding


CH = [[4.0, 1.0, 0.2, 0.0], [6.0, 3.0, 0.3, 0.0], [1.0, 0.5, 0.25, 0.0], [3.0, 0.5, 0.002, 0.0]]      # 4 heads, 2 kv heads, ns = 3
CV = [[10.0, 4.0, 0.5, 0.0], [4.0, 1.0, 0.252, 0.0]]
TERMS = [[5.0, 2.0, 1.0], [2.0, 0.5, 0.25]]
SCALE = [20.0, 8.0]
GREEDY = [[10.0, 2.0, 0.05, 0.0], [4.0, 1.0, 0.002, 0.0]]


def test_decode_on_hand_made_lists():
    from modegpt_amd import ops
    m = ops.decode_qk_logit_error(CH, CV, 2, 2, terms=TERMS, scale=SCALE, greedy_curve=GREEDY)        # RoPE: 2 columns = 1 unit kept
    assert m["rank"] == 2 and m["units_kept"] == 1 and m["n_kv"] == 2 and m["head_dim"] == 6
    h0, h1 = m["heads"]
    assert h0["energy"] == 10.0 and h0["error"] == 4.0 and h0["relative_error"] == 0.4
    assert h0["diagonal_estimate"] == 3.0 and h0["diagonal_ratio"] == 0.75
    assert h0["greedy_relative_error"] == 0.2 and h0["head_relative_error"] == [0.25, 0.5]
    assert h0["rank_for_rel_error"] == {"selection": {"0.1": 4, "0.01": 6, "0.001": 6}, "greedy": {"0.1": 4, "0.01": 4, "0.001": 6}}
    assert h1["rank_for_rel_error"]["greedy"] == {"0.1": 4, "0.01": 4, "0.001": 4}
    unit = (2 * 36 + 2) * 2.0 ** -53
    assert h0["noise_floor"] == unit * 20.0 / 10.0 and h0["non_monotone"] is False
    assert m["energy"] == 14.0 and m["error"] == 5.0 and m["relative_error"] == 5.0 / 14.0
    assert m["diagonal_estimate"] == 3.75 and m["greedy_relative_error"] == 3.0 / 14.0
    assert m["noise_floor"] == math.fsum([unit * 20.0, unit * 8.0]) / 14.0 and m["non_monotone"] is False
    full = ops.decode_qk_logit_error(CH, CV, 6, 2, terms=TERMS, scale=SCALE, greedy_curve=GREEDY)
    assert full["error"] == 0.0 and full["relative_error"] == 0.0 and full["diagonal_estimate"] == 0.0 and full["diagonal_ratio"] is None
    bare = ops.decode_qk_logit_error(CH, CV, 2, 2)
    assert bare["relative_error"] == m["relative_error"] and bare["noise_floor"] is None and bare["greedy_relative_error"] is None
    assert bare["heads"][0]["rank_for_rel_error"]["greedy"] is None
    t = lambda x: torch.tensor(x, dtype=torch.float64)                      # noqa: E731
    assert ops.decode_qk_logit_error(t(CH), t(CV), 2, 2, terms=t(TERMS), scale=t(SCALE), greedy_curve=t(GREEDY)) == m
    json.dumps(m, allow_nan=False)


def test_decode_maps_non_finite_figures_to_none():
    from modegpt_amd import ops
    nan, inf = float("nan"), float("inf")
    cv = [[nan, nan, 0.5, 0.0], CV[1]]
    ch = [[nan, nan, 0.2, 0.0]] + CH[1:]
    m = ops.decode_qk_logit_error(ch, cv, 2, 2, terms=[[inf, 2.0, 1.0], TERMS[1]], scale=[nan, 8.0], greedy_curve=[[nan] * 3 + [0.0], GREEDY[1]])
    h0, h1 = m["heads"]
    assert h0["energy"] is None and h0["error"] is None and h0["relative_error"] is None and h0["noise_floor"] is None
    assert h0["diagonal_estimate"] == 3.0 and h0["diagonal_ratio"] is None and h0["greedy_relative_error"] is None
    assert h0["head_relative_error"] == [None, 0.5] and h0["non_monotone"] is None
    assert set(h0["rank_for_rel_error"]["selection"].values()) == {None}
    assert h1 == ops.decode_qk_logit_error(CH, CV, 2, 2, terms=TERMS, scale=SCALE, greedy_curve=GREEDY)["heads"][1]      # the clean head: untouched
    assert m["energy"] is None and m["relative_error"] is None and m["non_monotone"] is None and m["noise_floor"] is None
    json.dumps(m, allow_nan=False)
    zero = ops.decode_qk_logit_error([[0.0, 0.0]], [[0.0, 0.0]], 0, 1, terms=[[0.0]], scale=[0.0])
    assert zero["relative_error"] is None and zero["error"] == 0.0
    json.dumps(zero, allow_nan=False)


def test_decode_refuses_wrong_shapes():
    from modegpt_amd import ops
    for bad in (dict(curve_h=CH[:3]), dict(curve=[CV[0], CV[1][:3]]), dict(rank=3), dict(rank=8), dict(rank=-2), dict(cols_per_unit=3),
                dict(terms=TERMS[:1]), dict(terms=[[1.0] * 4] * 2), dict(scale=[1.0]), dict(greedy_curve=[[1.0] * 3] * 2), dict(curve=[])):
        kw = dict(curve_h=CH, curve=CV, rank=2, cols_per_unit=2, terms=TERMS, scale=SCALE, greedy_curve=GREEDY)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.decode_qk_logit_error(**kw)


def test_qk_error_enabled(monkeypatch):
    from modegpt_amd import ops
    monkeypatch.delenv("MODEGPT_QK_ERROR", raising=False)
    assert ops.qk_error_enabled() is False
    for v in ("1", "on", "TRUE"):
        monkeypatch.setenv("MODEGPT_QK_ERROR", v)
        assert ops.qk_error_enabled() is True
    for v in ("0", "off", ""):
        monkeypatch.setenv("MODEGPT_QK_ERROR", v)
        assert ops.qk_error_enabled() is False


def test_null_pointers_are_refused_without_a_device():
    from modegpt_amd import _lib
    lib = _lib.load()
    rc = lib.mdg_qk_rank_curve(None, None, 4, 2, 16, 0.0, 0.0, _lib.MDG_QK_ROPE_GROUPED, None, 0.0, 0.0, None, None, None, None, None, None, None)
    assert rc == _lib.MDG_ERR_BAD_ARG and b"null" in lib.mdg_last_error()
