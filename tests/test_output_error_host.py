"""Host (no GPU): the long-double model of the realised MLP output error (tests/output_error_model.py) against an independent dense
product, the sandwich that ties it to the rank curve, the bf16 artefact's objective against the curve (the minimum over all
refits) -- and ops.decode_output_error / ops.output_error_enabled, which are pure host code, and the workspace size query."""
import math

import numpy as np
import pytest
import torch

from modegpt_amd import ops
from tests import chol_ref as R
from tests import output_error_model as OE
from tests import rank_curve_model as RC
from tests.test_rank_curve_host import EPS, case


def small_case(n, d, r, seed):
    gen = torch.Generator().manual_seed(seed)
    C = RC.covariance(RC.gated_acts(3 * n, n, seed=seed))
    W = (torch.randn(d, n, generator=gen) * 0.05).to(torch.bfloat16)
    idx = torch.sort(torch.randperm(n, generator=gen)[:r]).values.numpy()
    down = (torch.randn(d, r, generator=gen) * 0.05).to(torch.bfloat16)
    return C, W, idx, down


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("n,d,r", [(1, 1, 0), (1, 1, 1), (7, 3, 4), (48, 7, 33), (48, 7, 48), (48, 7, 0)])
def test_model_against_the_dense_product(n, d, r):
    """e_k against diag(U C_full U^T) with C_full the mirrored lower triangle, both in long double: two summation orders of the same
    numbers, n 2^-64 a_k apart at most -- 1e-17 a_k is a decade above that at n = 48 and four below fp64 noise."""
    C, W, idx, down = small_case(n, d, r, seed=100 * n + r)
    e, a = OE.errors(C, W, idx, down if r else None)
    U = OE.residual(W, idx, down if r else None)
    Cf = np.tril(R.ld(C)) + np.tril(R.ld(C), -1).T
    dense = np.einsum("ki,ij,kj->k", U, Cf, U)
    assert e.shape == a.shape == (d,)
    worst = float((np.abs(e - dense) / a).max())
    print("DENSE n=%d d=%d r=%d max |e - dense| / a = %.3e" % (n, d, r, worst))
    assert worst <= 1e-17
    assert bool((a >= np.abs(e)).all())
    # the fp64 restatement is the same algorithm
    assert float((np.abs(R.ld(OE.errors_fp64(C, W, idx, down if r else None)) - e) / a).max()) <= 64 * n * 2.0 ** -53
    # nothing above the diagonal is read
    Cn = np.array(C, dtype=np.float64)
    Cn[np.triu_indices(n, 1)] = np.nan
    e2, a2 = OE.errors(Cn, W, idx, down if r else None)
    assert np.array_equal(e2, e) and np.array_equal(a2, a)
    assert np.array_equal(OE.unorm2(W, idx, down if r else None), (U * U).sum(axis=1))


def test_model_index_rule():
    """clamped; the highest position of a repeated index is the one subtracted"""
    assert OE.inverse_map([3, 1, 3, -5, 99], 6).tolist() == [3, 1, -1, 2, -1, 4]
    C, W, idx, down = small_case(7, 3, 4, seed=5)
    idx = np.array([2, 5, 2, 9])
    U = OE.residual(W, idx, down)
    Wl, Dl = OE.wide(W), OE.wide(down)
    want = Wl.copy()
    want[:, 2] -= Dl[:, 2]
    want[:, 5] -= Dl[:, 1]
    want[:, 6] -= Dl[:, 3]
    assert np.array_equal(U, want)


# ---------------------------------------------------------------- the sandwich and the curve as the minimum
@pytest.mark.parametrize("keep", [0.5, 0.7, 0.9])
@pytest.mark.parametrize("n,d,tokens", [(385, 70, 300), (384, 96, 1024)])
def test_sandwich_and_the_rounded_refit(n, d, tokens, keep):
    """E_D + eps ||U||^2 - eps ||W_S||^2 <= curve[r] <= E_D + eps ||U||^2 with E_D = sum_k e_k and ||U||^2 = sum_k unorm2_k from THIS
    model, D the refit of chol_ref.nystrom; and objective(bf16(D)) >= curve[r]: the curve is the minimum over all refits.  Slack:
    the rounding of the long-double routes, 1e-12 of curve[0], as tests/test_rank_curve_host.py allows."""
    C, W, order = case(n, d, tokens)
    r = int(n * keep)
    idx = np.sort(order[:r])
    D = R.nystrom(torch.from_numpy(C), idx, W, EPS)              # [r, d] long double
    cv = RC.curve(C, order, W, EPS)
    q, eps = cv[0], R.LD(np.float64(EPS))
    e, _ = OE.errors(C, W, idx, D.T)
    hi = e.sum() + eps * OE.unorm2(W, idx, D.T).sum()
    ws = R.ld(W)[:, idx]
    lo = hi - eps * (ws * ws).sum()
    lo_rc, hi_rc = RC.sandwich(C, W, idx, D, EPS)
    assert abs(hi - hi_rc) <= 1e-15 * q and abs(lo - lo_rc) <= 1e-15 * q          # the two models state the same ends
    assert lo - 1e-12 * q <= cv[r] <= hi + 1e-12 * q
    Db = torch.from_numpy(D.T.astype(np.float64)).to(torch.bfloat16)              # [d, r]: what the engine stores
    eb, _ = OE.errors(C, W, idx, Db)
    objective = eb.sum() + eps * OE.unorm2(W, idx, Db).sum()
    print("ROUNDED n=%d keep=%.1f (objective(bf16 D) - curve[r]) / q = %.3e, (objective(D) - curve[r]) / q = %.3e" % (
        n, keep, float((objective - cv[r]) / q), float((hi - cv[r]) / q)))
    assert objective >= cv[r] - 1e-12 * q
    assert bool((e >= -1e-12 * q).all()) and bool((eb >= -1e-12 * q).all())       # C is positive semidefinite
    assert e.sum() < OE.errors(C, W, None, None)[0].sum()                        # ... and the refit loses less than everything


# ---------------------------------------------------------------- ops.decode_output_error
def test_decode_every_field():
    e, q, u2 = [1.0, 2.0, 0.5, 0.0], [10.0, 4.0, 1000.0, 0.0], [0.5, 0.25, 0.125, 0.0]
    m = ops.decode_output_error(e, q, u2, 1e-3, 7)
    assert set(m) == {"rank", "energy", "error", "relative_error", "objective", "worst_channel", "worst_channel_relative_error",
                      "channels_above"}
    assert m["rank"] == 7 and m["energy"] == 1014.0 and m["error"] == 3.5
    assert m["relative_error"] == 3.5 / 1014.0
    assert m["objective"] == 3.5 + 1e-3 * 0.875
    assert m["worst_channel"] == 1 and m["worst_channel_relative_error"] == 0.5   # channel 3 (q = 0) takes no part
    assert m["channels_above"] == {"0.1": 1, "0.01": 2, "0.001": 2}               # 0.1, 0.5, 5e-4: strictly above
    # CPU tensors are accepted as well
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    assert ops.decode_output_error(t(e), t(q), t(u2), 1e-3, 7) == m
    with pytest.raises(ValueError):
        ops.decode_output_error(e, q[:3], u2, 1e-3, 7)


def test_decode_with_a_curve():
    e, q, u2 = [1.0, 2.0], [10.0, 4.0], [0.5, 0.25]
    curve = [16.0, 8.0, 2.5, 0.0]
    m = ops.decode_output_error(e, q, u2, 1e-2, 2, curve=curve)
    assert m["predicted_objective"] == 2.5
    assert m["excess_over_optimum"] == (3.0 + 1e-2 * 0.75 - 2.5) / 16.0
    assert "predicted_objective" not in ops.decode_output_error(e, q, u2, 1e-2, 2)
    with pytest.raises(ValueError):
        ops.decode_output_error(e, q, u2, 1e-2, 4, curve=curve)
    nan = ops.decode_output_error(e, q, u2, 1e-2, 2, curve=[float("nan"), 1.0, 1.0, 0.0])
    assert nan["predicted_objective"] is None and nan["excess_over_optimum"] is None and nan["error"] == 3.0


def test_decode_zero_energy_channels_only():
    m = ops.decode_output_error([0.0, 0.0], [0.0, 0.0], [0.0, 0.0], 1e-6, 0)
    assert m["energy"] == 0.0 and m["error"] == 0.0 and m["relative_error"] is None
    assert m["worst_channel"] is None and m["worst_channel_relative_error"] is None
    assert m["channels_above"] == {"0.1": None, "0.01": None, "0.001": None}


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["e", "q", "unorm2"])
def test_decode_non_finite(bad, where):
    v = {"e": [1.0, 2.0], "q": [10.0, 4.0], "unorm2": [0.5, 0.25]}
    v[where] = [v[where][0], bad]
    m = ops.decode_output_error(v["e"], v["q"], v["unorm2"], 1e-6, 1, curve=[16.0, 2.0, 0.0])
    assert m["rank"] == 1
    assert m["objective"] is None if where != "q" else m["objective"] is not None
    assert (m["error"] is None) == (where == "e") and (m["energy"] is None) == (where == "q")
    if where in ("e", "q"):
        assert m["relative_error"] is None and m["worst_channel"] is None and m["worst_channel_relative_error"] is None
        assert m["channels_above"] == {"0.1": None, "0.01": None, "0.001": None}
    else:
        assert m["relative_error"] == 3.0 / 14.0 and m["worst_channel"] == 1
    assert (m["excess_over_optimum"] is None) == (where != "q")
    assert m["predicted_objective"] == 2.0
    assert all(x is None or isinstance(x, (int, dict)) or math.isfinite(x) for x in m.values())


# ---------------------------------------------------------------- the switch and the size query
def test_output_error_enabled(monkeypatch):
    monkeypatch.delenv("MODEGPT_OUTPUT_ERROR", raising=False)
    assert ops.output_error_enabled() is False
    for v in ("1", "on", "true", "TRUE", "On"):
        monkeypatch.setenv("MODEGPT_OUTPUT_ERROR", v)
        assert ops.output_error_enabled() is True
    for v in ("0", "", "off", "no", "2"):
        monkeypatch.setenv("MODEGPT_OUTPUT_ERROR", v)
        assert ops.output_error_enabled() is False
    monkeypatch.setenv("MODEGPT_OUTPUT_ERROR", "1")
    monkeypatch.delenv("MODEGPT_RANK_CURVE", raising=False)
    assert ops.rank_curve_enabled() is False                        # the two switches are independent


def test_workspace_size_query_needs_no_gpu():
    from modegpt_amd import _lib
    lib = _lib.load()
    assert lib.mdg_mlp_output_error_ws_bytes(0, 5) == 0 and lib.mdg_mlp_output_error_ws_bytes(5, 0) == 0
    for n, d in [(1, 1), (129, 257), (14336, 4096)]:
        tiles = (n + 127) // 128
        want = (4 * n + 15) // 16 * 16 + 16 * d * tiles           # the inverse map + two planes of partials
        assert lib.mdg_mlp_output_error_ws_bytes(n, d) == want
    assert lib.mdg_mlp_output_error_ws_bytes(14336, 4096) < 2.6e9 / 100          # far below the materialising route's workspace
    rc = lib.mdg_mlp_output_error(None, 10, 10, None, 4, 10, _lib.MDG_BF16, None, 0, None, 0, 0, _lib.MDG_BF16, None, None, None, 0, None)
    assert rc == _lib.MDG_ERR_BAD_ARG and b"null pointer" in lib.mdg_last_error()
