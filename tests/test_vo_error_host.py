"""Host (no GPU): the long-double model of the V/O output error and rank curve (tests/vo_error_model.py) against an independent dense
product, the identity objective == curve that ties the two together -- and ops.decode_vo_output_error / ops.vo_error_enabled, which
are pure host code, and the workspace size queries."""
import math

import numpy as np
import pytest
import torch

from modegpt_amd import ops
from tests import vo_error_model as VO
from tests.output_error_model import LD, wide

U64 = 2.0 ** -64                     # the unit roundoff of x87 long double (ppc / aarch64 quad is finer still)
RIDGE = 1e-5


def small_case(d, n_heads, n_kv, hd, r, seed, wdt=torch.bfloat16):
    C = VO.covariance(d, seed)
    Wv, Wo = VO.weights(d, n_heads, n_kv, hd, wdt, seed)
    gen = torch.Generator().manual_seed(seed + 5)
    vn = (torch.randn(n_kv * r, d, generator=gen) * 0.05).to(torch.bfloat16)
    on = (torch.randn(d, n_heads * r, generator=gen) * 0.05).to(torch.bfloat16)
    return C, Wv, Wo, vn, on


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("d,n_heads,n_kv,hd,r", [(1, 1, 1, 2, 1), (7, 2, 2, 4, 3), (24, 4, 2, 8, 5), (24, 3, 1, 6, 6), (24, 4, 2, 8, 0)])
def test_model_against_the_dense_product(d, n_heads, n_kv, hd, r):
    """e and dnorm2 from delta formed directly against y G y^T with the dense stacked Grams, both in long double: two routes to the same
    number whose roundings are each bounded by (2 d + 2 (hd + r)) 2^-64 a (three nested sums of products) -- 8 (d + hd + r) 2^-64 a."""
    C, Wv, Wo, vn, on = small_case(d, n_heads, n_kv, hd, r, seed=100 * d + r)
    e, dn, a, an = VO.errors(C, Wv, Wo, n_heads, n_kv, hd, r, vn, on)
    assert e.shape == dn.shape == a.shape == an.shape == (n_heads, d)
    bound = 8 * (d + hd + r) * U64
    for h in range(n_heads):
        wv, wo, v1, o1 = VO.head_blocks(Wv, Wo, vn, on, n_heads, n_kv, hd, r, h)
        V, y = np.concatenate([wv, -v1]), np.concatenate([wo, o1], axis=1)
        dense = np.einsum("ki,ij,kj->k", y, V @ wide(C) @ V.T, y)
        dense_n = np.einsum("ki,ij,kj->k", y, V @ V.T, y)
        worst = float((np.abs(e[h] - dense) / a[h]).max())
        print("DENSE d=%d hd=%d r=%d head %d: max |e - dense| / a = %.3e (bound %.3e)" % (d, hd, r, h, worst, bound))
        assert worst <= bound and float((np.abs(dn[h] - dense_n) / an[h]).max()) <= bound
    assert bool((a >= np.abs(e)).all()) and bool((an >= dn).all()) and bool((dn >= 0).all())
    # the fp64 restatement is the same quantity by the kernel's route
    e64, dn64 = VO.errors_fp64(C, Wv, Wo, n_heads, n_kv, hd, r, vn, on)
    assert float((np.abs(wide(e64) - e) / a).max()) <= 64 * (d + hd + r) * 2.0 ** -53
    assert float((np.abs(wide(dn64) - dn) / an).max()) <= 64 * (d + hd + r) * 2.0 ** -53
    # rank 0 and absent factors are the same thing: q
    q = VO.errors(C, Wv, Wo, n_heads, n_kv, hd, 0, vn, on)
    q2 = VO.errors(C, Wv, Wo, n_heads, n_kv, hd, r, None, None)
    assert all(np.array_equal(x, y) for x, y in zip(q, q2)) and bool((q[0] >= 0).all())


# ---------------------------------------------------------------- the identity: objective == curve, every rank, both variants
@pytest.mark.parametrize("n_heads,n_kv", [(4, 2), (3, 1), (2, 2)], ids=["gqa4-2", "gqa3-1", "mha2"])
def test_identity_objective_equals_curve(n_heads, n_kv):
    """For the factors of rank r built from the model's own eigenvectors, sum_{h in g} sum_k (e + rho dnorm2) = curve[g][r] in exact
    arithmetic.  In long double both sides carry (d + hd) 2^-64 of curve[g][0]; the MHA factors hold S^-1, which multiplies that by
    cond = lambda_1 / lambda_hd of the first spectrum.  Allowed: 64 (d + hd + r) 2^-64 max(1, cond) curve[g][0]."""
    d, hd = 24, 8
    C = VO.covariance(d, 3)
    Wv, Wo = VO.weights(d, n_heads, n_kv, hd, torch.bfloat16, seed=3)
    spec = VO.spectra(C, RIDGE, Wv, Wo, n_heads, n_kv, hd)
    cv = VO.curve(C, RIDGE, Wv, Wo, n_heads, n_kv, hd, spec=spec)
    assert cv.shape == (n_kv, hd + 1) and bool((cv[:, hd] == 0).all()) and bool((np.diff(cv, axis=1) <= 0).all())
    rho, group = LD(np.float64(RIDGE)), n_heads // n_kv
    worst = 0.0
    for r in range(hd + 1):
        vn, on = VO.factors(spec, Wv, Wo, n_heads, n_kv, hd, r) if r else (None, None)
        e, dn, _, _ = VO.errors(C, Wv, Wo, n_heads, n_kv, hd, r, vn, on)
        for g in range(n_kv):
            lam = spec[g][0]
            cond = float(lam[0] / lam[-1]) if n_kv == n_heads else 1.0
            objective = (e[g * group:(g + 1) * group] + rho * dn[g * group:(g + 1) * group]).sum()
            diff = float(abs(objective - cv[g, r]) / cv[g, 0])
            worst = max(worst, diff / max(1.0, cond))
            assert diff <= 64 * (d + hd + r) * U64 * max(1.0, cond), (r, g, diff, cond)
    print("IDENTITY %d/%d heads: max |objective - curve[r]| / (curve[0] max(1, cond)) = %.3e" % (n_heads, n_kv, worst))


def test_grouped_curve_is_not_the_value_stream_energy():
    """Field 3 of mdg_vo_spectrum is the lambda share; the output error weighs every dropped direction by ||W_o,h v_i||^2: the two
    part (the issue's numpy check: 9.17e-2 against 8.35e-2 at d = 96, hd = 16, g = 4, r = 11)."""
    d, hd, n_heads, n_kv, r = 96, 16, 4, 1, 11
    C = VO.covariance(d, 1)
    Wv, Wo = VO.weights(d, n_heads, n_kv, hd, torch.float64, seed=1)
    spec = VO.spectra(C, RIDGE, Wv, Wo, n_heads, n_kv, hd)
    cv = VO.curve(C, RIDGE, Wv, Wo, n_heads, n_kv, hd, spec=spec)
    lam = spec[0][0]
    out_err, tail = float(cv[0, r] / cv[0, 0]), float(lam[r:].sum() / lam.sum())
    print("GROUPED r=%d: output error %.4e, lambda-tail share %.4e" % (r, out_err, tail))
    assert 0 < out_err < 1 and 0 < tail < 1 and abs(out_err - tail) > 1e-3 * tail


# ---------------------------------------------------------------- ops.decode_vo_output_error
E4 = [[0.1, 0.2], [0.0, 0.1], [0.3, 0.1], [0.2, 0.2]]
Q4 = [[1.0, 2.0], [1.0, 1.0], [3.0, 1.0], [2.0, 2.0]]
N4 = [[1.0, 1.0]] * 4
LAYER_KEYS = {"rank", "n_kv", "energy", "error", "relative_error", "objective", "noise_floor", "heads", "worst_head",
              "worst_head_relative_error", "worst_channel", "worst_channel_relative_error"}


def test_decode_every_field():
    m = ops.decode_vo_output_error(E4, Q4, N4, 1e-3, 1, 2, hd=2)
    assert set(m) == LAYER_KEYS
    assert m["rank"] == 1 and m["n_kv"] == 2 and m["energy"] == 13.0 and m["error"] == math.fsum([0.1, 0.2, 0.1, 0.3, 0.1, 0.2, 0.2])
    assert m["relative_error"] == m["error"] / 13.0 and m["objective"] == m["error"] + 1e-3 * 8.0
    assert m["noise_floor"] == 64.0 * (2 + 2 + 1) * 2.0 ** -53 * 13.0
    assert len(m["heads"]) == 2
    h0, h1 = m["heads"]
    assert h0["energy"] == 5.0 and h0["error"] == math.fsum([0.1, 0.2, 0.0, 0.1]) and h0["relative_error"] == h0["error"] / 5.0
    assert h1["energy"] == 8.0 and h1["objective"] == math.fsum([0.3, 0.1, 0.2, 0.2]) + 1e-3 * 4.0
    assert set(h0) == {"energy", "error", "relative_error", "objective", "noise_floor"}
    # query heads: 0.3/3, 0.1/2, 0.4/4, 0.4/4 -- head 0 is largest by rounding or the first of a tie; its channels 0.1 and 0.1
    assert m["worst_head"] in (0, 2, 3) and abs(m["worst_head_relative_error"] - 0.1) < 1e-15
    assert m["worst_channel"] in (0, 1)
    m2 = ops.decode_vo_output_error([[0.5, 0.0], [0.1, 0.3]], [[1.0, 0.0], [1.0, 1.0]], [[0.0, 0.0]] * 2, 0.0, 2, 1)
    assert m2["worst_head"] == 0 and m2["worst_head_relative_error"] == 0.5 and m2["worst_channel"] == 0      # (q = 0: no part)
    assert m2["noise_floor"] == 64.0 * (2 + 2 + 2) * 2.0 ** -53 * 3.0                                      # hd unknown: rank
    t = lambda v: torch.tensor(v, dtype=torch.float64)                                                     # noqa: E731
    assert ops.decode_vo_output_error(t(E4), t(Q4), t(N4), 1e-3, 1, 2, hd=2) == m
    for bad in (dict(n_kv=3), dict(n_kv=0)):
        with pytest.raises(ValueError):
            ops.decode_vo_output_error(E4, Q4, N4, 1e-3, 1, **bad)
    with pytest.raises(ValueError):
        ops.decode_vo_output_error(E4, Q4[:3], N4, 1e-3, 1, 2)


def test_decode_with_a_curve():
    curve = [[5.0, 1.0, 0.0], [8.0, 2.0, 0.0]]
    m = ops.decode_vo_output_error(E4, Q4, N4, 1e-3, 1, 2, curve=curve)
    h0, h1 = m["heads"]
    assert h0["predicted_objective"] == 1.0 and h1["predicted_objective"] == 2.0 and m["predicted_objective"] == 3.0
    assert h0["excess_over_curve"] == (h0["objective"] - 1.0) / 5.0 and m["excess_over_curve"] == (m["objective"] - 3.0) / 13.0
    assert h0["relative_curve"] == [1.0, 0.2, 0.0] and h1["relative_curve"] == [1.0, 0.25, 0.0]
    assert h0["rank_for_rel_error"] == {"0.1": 2, "0.01": 2, "0.001": 2}
    assert m["noise_floor"] == 64.0 * (2 + 2 + 1) * 2.0 ** -53 * 13.0                                      # hd from the curve
    big = ops.decode_vo_output_error(E4, Q4, N4, 0.0, 1, 2, curve=[[1.0, 0.05, 0.0], [1.0, 0.5, 1e-4]])
    assert big["heads"][0]["rank_for_rel_error"] == {"0.1": 1, "0.01": 2, "0.001": 2}
    assert big["heads"][1]["rank_for_rel_error"] == {"0.1": 2, "0.01": 2, "0.001": 2}
    with pytest.raises(ValueError):
        ops.decode_vo_output_error(E4, Q4, N4, 1e-3, 3, 2, curve=curve)
    with pytest.raises(ValueError):
        ops.decode_vo_output_error(E4, Q4, N4, 1e-3, 1, 2, curve=curve[:1])
    nan = ops.decode_vo_output_error(E4, Q4, N4, 1e-3, 1, 2, curve=[[float("nan"), 1.0, 0.0], [8.0, 2.0, 0.0]])
    assert nan["heads"][0]["predicted_objective"] is None and nan["heads"][0]["relative_curve"] is None
    assert nan["heads"][1]["predicted_objective"] == 2.0 and nan["predicted_objective"] is None and nan["error"] == m["error"]


def test_decode_rank_equals_head_dim():
    """rank = hd with fp64 factors: e is rounding noise of either sign, returned raw; the floor says so."""
    e = [[1e-18, -2e-18], [-1e-18, 1e-18]]
    m = ops.decode_vo_output_error(e, [[1.0, 2.0], [1.0, 1.0]], [[0.0, 0.0]] * 2, 1e-5, 2, 1, curve=[[5.0, 1.0, 0.0]])
    assert m["error"] == math.fsum([1e-18, -2e-18, -1e-18, 1e-18]) and m["error"] < 0
    assert abs(m["error"]) < m["noise_floor"] == 64.0 * (2 + 2 + 2) * 2.0 ** -53 * 5.0
    assert m["heads"][0]["predicted_objective"] == 0.0 and m["heads"][0]["excess_over_curve"] == m["objective"] / 5.0


def test_decode_zero_energy():
    z = [[0.0, 0.0]] * 2
    m = ops.decode_vo_output_error(z, z, z, 1e-6, 0, 2, curve=[[0.0, 0.0, 0.0]] * 2)
    assert m["energy"] == 0.0 and m["error"] == 0.0 and m["relative_error"] is None and m["noise_floor"] is None
    assert m["worst_head"] is None and m["worst_channel"] is None and m["predicted_objective"] is None
    assert m["heads"][0]["relative_curve"] is None and m["heads"][0]["rank_for_rel_error"] == {"0.1": None, "0.01": None, "0.001": None}


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["e", "q", "dnorm2"])
def test_decode_non_finite(bad, where):
    v = {"e": [list(r) for r in E4], "q": [list(r) for r in Q4], "dnorm2": [list(r) for r in N4]}
    v[where][3][1] = bad                                           # kv head 1 only
    m = ops.decode_vo_output_error(v["e"], v["q"], v["dnorm2"], 1e-3, 1, 2, curve=[[5.0, 1.0, 0.0], [8.0, 2.0, 0.0]])
    clean = ops.decode_vo_output_error(E4, Q4, N4, 1e-3, 1, 2, curve=[[5.0, 1.0, 0.0], [8.0, 2.0, 0.0]])
    assert m["heads"][0] == clean["heads"][0]                      # the other kv head keeps its numbers
    h1 = m["heads"][1]
    assert (h1["error"] is None) == (where == "e") and (h1["energy"] is None) == (where == "q")
    assert (h1["objective"] is None) == (where != "q") and (h1["excess_over_curve"] is None) == (where != "q")
    assert (h1["relative_error"] is None) == (where != "dnorm2") and (m["relative_error"] is None) == (where != "dnorm2")
    assert h1["predicted_objective"] == 2.0

    def finite(x):
        if isinstance(x, dict):
            return all(finite(y) for y in x.values())
        if isinstance(x, list):
            return all(finite(y) for y in x)
        return x is None or isinstance(x, int) or math.isfinite(x)
    assert finite(m)                                                # json.dump never meets a NaN


# ---------------------------------------------------------------- the switch and the size queries
def test_vo_error_enabled(monkeypatch):
    monkeypatch.delenv("MODEGPT_VO_ERROR", raising=False)
    assert ops.vo_error_enabled() is False
    for v in ("1", "on", "true", "TRUE", "On"):
        monkeypatch.setenv("MODEGPT_VO_ERROR", v)
        assert ops.vo_error_enabled() is True
    for v in ("0", "", "off", "no", "2"):
        monkeypatch.setenv("MODEGPT_VO_ERROR", v)
        assert ops.vo_error_enabled() is False
    monkeypatch.setenv("MODEGPT_VO_ERROR", "1")
    monkeypatch.delenv("MODEGPT_OUTPUT_ERROR", raising=False)
    assert ops.output_error_enabled() is False                      # the switches are independent


def test_workspace_size_queries_need_no_gpu():
    from modegpt_amd import _lib
    lib = _lib.load()
    for d, nh, nkv, hd, r in [(1, 1, 1, 2, 1), (70, 4, 2, 16, 11), (257, 3, 1, 128, 1), (4096, 32, 8, 128, 88), (4096, 32, 8, 128, 0)]:
        n = hd + r
        assert lib.mdg_vo_output_error_ws_bytes(d, nh, nkv, hd, r) == 8 * (nkv * n * d + 2 * nkv * n * n + 2 * ((n + 127) // 128) * nh * d)
        grouped = 8 * nh * hd * (d + (d + 255) // 256)
        assert lib.mdg_vo_rank_curve_ws_bytes(d, nh, nkv, hd) == (grouped if nh != nkv else 0)
    assert lib.mdg_vo_output_error_ws_bytes(4096, 32, 8, 128, 88) < 80e6
    for bad in [(0, 4, 2, 16, 1), (70, 4, 3, 16, 1), (70, 4, 2, 15, 1), (70, 4, 2, 130, 1), (70, 4, 2, 16, 17), (70, 4, 2, 16, -1)]:
        assert lib.mdg_vo_output_error_ws_bytes(*bad) == 0
    assert lib.mdg_vo_rank_curve_ws_bytes(0, 4, 2, 16) == 0 and lib.mdg_vo_rank_curve_ws_bytes(70, 4, 3, 16) == 0
    rc = lib.mdg_vo_output_error(None, 8, 8, None, 8, None, 8, _lib.MDG_BF16, 2, 1, 4, 0, None, 0, None, 0, _lib.MDG_BF16, None, None,
                                 None, 0, None)
    assert rc == _lib.MDG_ERR_BAD_ARG and b"null pointer" in lib.mdg_last_error()
    rc = lib.mdg_vo_rank_curve(None, 0, None, 8, _lib.MDG_BF16, 8, 2, 1, 4, None, None, 0, None)
    assert rc == _lib.MDG_ERR_BAD_ARG and b"null pointer" in lib.mdg_last_error()
