"""CPU: the identities the mean-aware V/O truncation stands on, in the long double model of tests/vo_mean_model.py, on a token matrix
whose channel means are up to 8 x the channel spread (512 tokens, d = 64).

  * with the intercept delta the layer's summed per-head linear maps have NO mean output error over the tokens; without it the mean
    error is delta -- for any factors, optimal or not (softmax rows sum to one: the constant needs no rank);
  * MHA, two-SVD variant, ridge 0, exact factors: centring + intercept cannot lose against the reference's route, which is the optimal
    rank-r LINEAR map per head; the optimal affine map is at least as good;
  * grouped: the reference's subspace ignores W_o, so the same inequality holds on the VALUE stream: the tail eigenvalue sums of
    G_S = W_v S W_v^T are at most those of G_C = G_S + a a^T, a = W_v mu.
Both premises were checked here before the GPU tests were written to rely on them; they hold on the prescribed inputs."""
import numpy as np
import pytest

from tests import vo_mean_model as V

LD = V.LD
TOKENS, D = 512, 64
LAYOUTS = [(4, 2, 16, 10), (4, 4, 16, 10), (2, 1, 8, 8), (2, 2, 8, 2)]      # (n_heads, n_kv, hd, rank)


def _case(layout, seed=0):
    n_heads, n_kv, hd, rank = layout
    X = V.make_tokens(TOKENS, D, seed=seed)
    w = V.make_weights(n_heads, n_kv, hd, D, seed=seed, rank=rank)
    C, mu = V.moments(X)
    return X, w, C, mu


def test_the_inputs_carry_a_mean_of_several_spreads():
    X = V.make_tokens(TOKENS, D)
    ratio = np.abs(X.mean(axis=0)) / X.std(axis=0)
    assert ratio.max() > 4 and np.median(ratio) > 1


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("factors", ["arbitrary", "centred", "uncentred"])
def test_intercept_leaves_no_mean_error_and_without_it_the_error_is_delta(layout, factors):
    n_heads, n_kv, hd, rank = layout
    X, w, C, mu = _case(layout)
    if factors == "arbitrary":
        v_hat, o_hat = w["v_hat"], w["o_hat"]
    else:
        stat = C - np.outer(mu, mu) if factors == "centred" else C
        v_hat, o_hat, _ = V.truncate(stat, w["W_v"], w["W_o"], n_heads, n_kv, hd, rank)
    dl, const = V.delta(w["W_v"], w["W_o"], v_hat, o_hat, mu, n_heads, n_kv, hd, rank)
    Dh = V.head_maps(w["W_v"], w["W_o"], v_hat, o_hat, n_heads, n_kv, hd, rank)
    scale = V.magnitude(w["W_v"], w["W_o"], v_hat, o_hat, mu, n_heads, n_kv, hd, rank)
    eps = LD(np.finfo(LD).eps)
    tol = (TOKENS + D + n_heads * (hd + rank) + 8) * eps * scale * 8       # (the token sums add |x| <= 8 |mu|-sized terms)
    mean_on, _ = V.output_errors(X, Dh, bias=dl)
    mean_off, _ = V.output_errors(X, Dh)
    assert np.all(np.abs(mean_on) <= tol)
    assert np.all(np.abs(mean_off - dl) <= tol)
    if rank < hd or factors == "arbitrary":                                 # (a full-rank truncation loses nothing: delta = 0)
        assert np.abs(dl).max() > 1e3 * tol.max()                           # ... and delta is not itself rounding noise
    # the v bias rides along: it enters a_g and nothing else
    dl_b, const_b = V.delta(w["W_v"], w["W_o"], v_hat, o_hat, mu, n_heads, n_kv, hd, rank, b_v=w["b_v"])
    fold = V.ld(w["W_o"]) @ np.repeat(V.ld(w["b_v"]).reshape(n_kv, hd), n_heads // n_kv, axis=0).reshape(-1)
    assert np.all(np.abs((dl_b - dl) - fold) <= tol) and np.all(np.abs((const_b - const) - fold) <= tol)


@pytest.mark.parametrize("layout", [l for l in LAYOUTS if l[0] == l[1]])
def test_mha_centred_truncation_with_intercept_cannot_lose(layout):
    n_heads, n_kv, hd, rank = layout
    X, w, C, mu = _case(layout)
    S = C - np.outer(mu, mu)
    v_c, o_c, _ = V.truncate(S, w["W_v"], w["W_o"], n_heads, n_kv, hd, rank)
    v_u, o_u, _ = V.truncate(C, w["W_v"], w["W_o"], n_heads, n_kv, hd, rank)
    dl, _ = V.delta(w["W_v"], w["W_o"], v_c, o_c, mu, n_heads, n_kv, hd, rank)
    _, sq_on = V.output_errors(X, V.head_maps(w["W_v"], w["W_o"], v_c, o_c, n_heads, n_kv, hd, rank), bias=dl)
    _, sq_off = V.output_errors(X, V.head_maps(w["W_v"], w["W_o"], v_u, o_u, n_heads, n_kv, hd, rank))
    print(f"{layout}: summed squared output error, centred + intercept {float(sq_on):.6e}, reference route {float(sq_off):.6e}")
    assert sq_on <= sq_off
    if rank < hd:
        assert sq_on < sq_off * (1 - 1e-6)                                   # with means of several spreads the gain is not marginal


@pytest.mark.parametrize("layout", [l for l in LAYOUTS if l[0] != l[1]])
def test_grouped_value_stream_inequality(layout):
    n_heads, n_kv, hd, rank = layout
    X, w, C, mu = _case(layout)
    S = C - np.outer(mu, mu)
    _, _, Pi_c = V.truncate(S, w["W_v"], w["W_o"], n_heads, n_kv, hd, rank)
    _, _, Pi_u = V.truncate(C, w["W_v"], w["W_o"], n_heads, n_kv, hd, rank)
    a, _ = V.head_vectors(w["W_v"], None, mu, n_kv, hd, 0)
    on = V.value_stream_error(X, w["W_v"], Pi_c, n_kv, hd, a=a)
    off = V.value_stream_error(X, w["W_v"], Pi_u, n_kv, hd)
    print(f"{layout}: value stream error, centred {float(on):.6e}, uncentred {float(off):.6e}")
    assert on <= off + 64 * float(np.finfo(LD).eps) * off                    # (rank == hd: both are rounding noise around 0)
    # the same thing as eigenvalue sums: tail of G_S against tail of G_S + a a^T, per kv head
    for k in range(n_kv):
        Wk = V.ld(w["W_v"])[k * hd:(k + 1) * hd]
        lam_s, _ = V._eigh(Wk @ S @ Wk.T)
        lam_c, _ = V._eigh(Wk @ C @ Wk.T)
        assert lam_s[rank:].sum() <= lam_c[rank:].sum() * (1 + 1e-12) + 1e-15


def test_norms_and_bound_of_the_model_are_consistent():
    layout = LAYOUTS[0]
    n_heads, n_kv, hd, rank = layout
    X, w, C, mu = _case(layout)
    bias, n0, n1 = V.intercept(w["W_v"], w["W_o"], w["v_hat"], w["o_hat"], mu, n_heads, n_kv, hd, rank, b_v=w["b_v"], b_o=w["b_o"])
    dl, const = V.delta(w["W_v"], w["W_o"], w["v_hat"], w["o_hat"], mu, n_heads, n_kv, hd, rank, b_v=w["b_v"])
    assert np.array_equal(bias, V.ld(w["b_o"]) + dl) and n0 == (dl * dl).sum() and n1 == (const * const).sum()
    # rank 0: the factors are not read and delta is the whole constant
    d0, c0 = V.delta(w["W_v"], w["W_o"], None, None, mu, n_heads, n_kv, hd, 0, b_v=w["b_v"])
    assert np.array_equal(d0, c0) and np.array_equal(c0, const)
    # the fp64 evaluation of the same sums sits inside the bound
    a64 = (w["W_v"] @ np.asarray(mu, dtype=np.float64)).reshape(n_kv, hd) + w["b_v"].reshape(n_kv, hd)
    a264 = (w["v_hat"] @ np.asarray(mu, dtype=np.float64)).reshape(n_kv, rank)
    g = n_heads // n_kv
    d64 = w["W_o"] @ np.repeat(a64, g, axis=0).reshape(-1) - w["o_hat"] @ np.repeat(a264, g, axis=0).reshape(-1)
    bound = V.delta_bound(w["W_v"], w["W_o"], w["v_hat"], w["o_hat"], np.asarray(mu, dtype=np.float64), n_heads, n_kv, hd, rank, b_v=w["b_v"])
    ref = V.delta(w["W_v"], w["W_o"], w["v_hat"], w["o_hat"], np.asarray(mu, dtype=np.float64), n_heads, n_kv, hd, rank, b_v=w["b_v"])[0]
    assert np.all(np.abs(V.ld(d64) - ref) <= bound)
