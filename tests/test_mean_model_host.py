"""CPU: the arithmetic of the mean-aware MLP refit on the long double model of tests/mean_model.py.

  * the centred fit D = W_d S[:,k] (S_kk + eps I)^-1 with b' = b_d + W_d mu - D mu_k IS the ridge least-squares fit on the augmented
    feature [h_k; 1] (Sherman-Morrison), at condition numbers 10^3 .. 10^9 of S with eps = 10^-6;
  * the error of the affine map with the optimal intercept is u S u^T per channel, at most the linear map's u C u^T;
  * r = n with eps = 0 returns D = W_d and b' = b_d.

Both fits solve the same system in long double (w = 2^-64), so they differ by rounding alone: the forming of S = C - mu mu^T costs
w ||C|| per entry against a smallest eigenvalue lambda_min(S_kk) + eps, every solve another n w cond.  The bound asserted is
64 n 2^-63 ||C||_2 / (lambda_min(S_kk) + eps), relative, in the Frobenius norm."""
import numpy as np
import pytest

from tests import chol_ref as R
from tests import mean_model as M

EPS = 1e-6
N, RANK, D_OUT = 48, 33, 12


def _case(p, seed):
    rng = np.random.default_rng(100 + seed)
    S0 = R.spd_matrix(N, p, seed=seed).numpy()
    mu = np.abs(rng.standard_normal(N)) + 0.5                      # means of the order of the largest standard deviation
    C = S0 + np.outer(mu, mu)
    C = np.tril(C) + np.tril(C, -1).T
    W = rng.standard_normal((D_OUT, N))
    b_d = rng.standard_normal(D_OUT)
    idx = np.sort(rng.permutation(N)[:RANK])
    return C, mu, W, b_d, idx


def _rel(a, b):
    return float(np.linalg.norm((a - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


@pytest.mark.parametrize("p", [3, 5, 7, 9])
def test_centred_fit_is_the_augmented_least_squares_fit(p):
    C, mu, W, b_d, idx = _case(p, seed=p)
    D1, b1 = M.centred_fit(C, mu, idx, W, EPS, b_d)
    D2, b2 = M.augmented_fit(C, mu, idx, W, EPS, b_d)
    S = M.center(C, mu).astype(np.float64)
    lam = np.linalg.eigvalsh(S[np.ix_(idx, idx)])
    assert 10.0 ** (p - 0.5) < M.cond(S) < 10.0 ** (p + 0.5)       # the statistic has the condition number asked for
    tol = 64 * N * 2.0 ** -63 * np.linalg.norm(C, 2) / (max(lam[0], 0.0) + EPS)
    print(f"p={p}: D rel {_rel(D1, D2):.3e}  b' rel {_rel(b1, b2):.3e}  tol {tol:.3e}")
    assert _rel(D1, D2) <= tol
    # b' = rhs - mu_k D: the error of D enters times |mu_k|
    scale = np.linalg.norm(D2.astype(np.float64)) * np.linalg.norm(mu[idx]) / np.linalg.norm(b2.astype(np.float64))
    assert _rel(b1, b2) <= tol * max(scale, 1.0)


@pytest.mark.parametrize("p", [3, 6])
def test_affine_error_is_the_centred_quadratic_form_and_never_larger(p):
    C, mu, W, b_d, idx = _case(p, seed=10 + p)
    S = M.center(C, mu)
    D, _ = M.centred_fit(C, mu, idx, W, EPS, b_d)
    u = M.residual(W, idx, D)
    affine, linear = M.quad(u, S), M.quad(u, C)
    # E|u h + b_d - b'|^2 with b' - b_d = u mu is E|u (h - mu)|^2 = u C u^T - (u mu)^2, directly:
    direct = linear - (u @ M.ld(mu)) ** 2
    assert np.all(np.abs(affine - direct) <= 64 * N * 2.0 ** -63 * M.quad(np.abs(u), np.abs(M.ld(C))))
    assert np.all(affine <= linear)
    # ... and b' is optimal for this D: any other intercept adds its squared distance
    other = linear - 2 * (u @ M.ld(mu)) * 0.9 * (u @ M.ld(mu)) + (0.9 * (u @ M.ld(mu))) ** 2
    assert np.all(other >= affine)


def test_full_rank_without_ridge_returns_the_weights_and_the_bias():
    C, mu, W, b_d, _ = _case(3, seed=3)
    idx = np.arange(N)
    D, bp = M.centred_fit(C, mu, idx, W, 0.0, b_d)
    assert _rel(D, M.ld(W)) <= 64 * N * 2.0 ** -63 * M.cond(M.center(C, mu))
    # with the stored tensor equal to W_d the intercept is b_d exactly
    b, d2, w2 = M.intercept(W, W, idx, mu, b_d)
    assert np.array_equal(b, M.ld(b_d)) and d2 == 0 and w2 > 0


def test_stored_intercept_zeroes_the_mean_error_of_any_stored_tensor():
    """b' is taken for the tensor that is STORED: with D^ = bf16(D) the per-channel mean of y - y' over the tokens is zero in exact
    arithmetic, while the linear refit on C leaves a mean of the order of delta."""
    case = M.make_case(40, 28, 8, tokens=256, seed=1)
    H, W, C, mu, idx, b_d = (case[k] for k in ("H", "W", "C", "mu", "idx", "b_d"))
    S = M.center(C, mu).astype(np.float64)
    D_hat = M.bf16_round(M.refit(S, idx, W, EPS).astype(np.float64))
    mu_exact = M.col_sums(H) / M.LD(H.shape[0])
    b, _, _ = M.intercept(W, D_hat, idx, mu_exact, b_d)
    mean_on, sq_on = M.token_errors(H, W, idx, D_hat, bias=b, b_d=b_d)
    assert np.all(np.abs(mean_on) <= 4 * M.bias_bound(W, D_hat, idx, mu_exact, b_d))
    D_lin = M.bf16_round(M.refit(C, idx, W, EPS).astype(np.float64))
    mean_off, sq_off = M.token_errors(H, W, idx, D_lin, bias=b_d, b_d=b_d)
    assert sq_on < sq_off and np.abs(mean_off).max() > 1e3 * np.abs(mean_on).max()


# ---- the case builders of tests/test_gpu_intercept_kernel.py: why that file may assert equality to the bit
@pytest.mark.parametrize("name,repeat", [(k, False) for k in M.INTERCEPT_SHAPES] + [("E", True), ("F", True)])
def test_lattice_case_is_exact_in_fp64_in_any_order(name, repeat):
    d, n, r = M.INTERCEPT_SHAPES[name]
    assert n <= 6144 and d <= 531
    c = M.lattice_case(d, n, r, seed=1, repeat=repeat)
    W, D, mu, idx, b_d = (c[k] for k in ("W", "D", "mu", "idx", "b_d"))
    assert W.shape == (d, n) and D.shape == (d, r) and mu.shape == (n,) and idx.shape == (r,) and b_d.shape == (d,)
    for a, lim in ((W, 8), (D, 8), (mu, 16), (b_d, 64)):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= lim
    assert np.array_equal(M.bf16_round(W), W) and np.array_equal(M.bf16_round(D), D)
    assert idx.min() >= 0 and idx.max() < n
    distinct = len(np.unique(idx))
    assert distinct == (r - min(5, r // 2) if repeat else r)
    if r > 8:
        assert not np.array_equal(idx, np.sort(idx))                              # shuffled
    assert M.lattice_is_exact(c)
    for b in (b_d, None):
        ref = M.intercept(W, D, idx, mu, b)
        want = tuple(np.asarray(v).astype(np.float64) for v in ref)
        assert all(np.array_equal(M.ld(w), np.asarray(v)) for w, v in zip(want, ref))     # the model's values ARE fp64 numbers
        for order in ("ascending", "chunks_reversed"):
            got = M.intercept_fp64(W, D, idx, mu, b, order=order)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), order
    assert want[1] < 2 ** 48 and want[2] < 2 ** 48


def test_generic_case_fp64_evaluation_stays_inside_the_bias_bound():
    d, n, r = M.INTERCEPT_SHAPES["E"]
    c = M.generic_case(d, n, r, seed=1)
    W, D, mu, idx, b_d = (c[k] for k in ("W", "D", "mu", "idx", "b_d"))
    assert np.array_equal(M.bf16_round(W), W) and np.array_equal(M.bf16_round(D), D) and np.array_equal(M.bf16_round(b_d), b_d)
    assert mu.min() > 0 and len(np.unique(idx)) == r and not np.array_equal(idx, np.sort(idx))
    for b in (b_d, None):
        ref, _, _ = M.intercept(W, D, idx, mu, b)
        bound = M.bias_bound(W, D, idx, mu, b)
        for order in ("ascending", "chunks_reversed"):
            got, _, _ = M.intercept_fp64(W, D, idx, mu, b, order=order)
            ratio = float((np.abs(M.ld(got) - ref) / bound).max())
            print(f"generic E, {order}, b_d {'given' if b is not None else 'none'}: err / bound max {ratio:.3e}")
            assert ratio <= 1


# ---- the saved activation mean (calib_cache: layer_<i>_mlp_mean.f64 and its sidecar entry), host half only
def test_mean_file_reads_back_with_numpy_alone_and_every_refusal_fires_on_metadata(tmp_path):
    import json
    import math
    import struct

    from modegpt_amd import calib_cache as CC
    rng = np.random.default_rng(5)
    n, layer = 37, 3
    mu = np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-3, 4, size=n)
    entry = CC.write_mean_file(str(tmp_path), layer, mu, n)
    path = tmp_path / f"layer_{layer}_mlp_mean.f64"
    assert entry == {"file": path.name, "layout": "vector", "n": n, "bytes": 8 * n,
                     "sum_bits": struct.unpack("<q", struct.pack("<d", math.fsum(mu.tolist())))[0]}
    assert not [p for p in tmp_path.iterdir() if ".tmp" in p.name]            # temporary name, then os.replace
    back = np.fromfile(path, "<f8")                                           # numpy alone
    assert back.tobytes() == mu.astype("<f8").tobytes()
    json.dumps(entry)                                                         # plain JSON types
    meta = {"files": {"mlp_mean": dict(entry)}}
    assert CC.validate_extra_entry(meta, {"n_inner": n}, layer, "mlp_mean") == entry
    assert np.array_equal(CC.read_mean_file(str(tmp_path), layer, entry), mu)
    # refusals on metadata alone (the data file is not opened: it is deleted first)
    path.rename(tmp_path / "moved")
    with pytest.raises(ValueError, match=r"layer 3: field files\.mlp_mean is missing"):
        CC.validate_extra_entry({"files": {}}, {"n_inner": n}, layer, "mlp_mean")
    for field, bad in (("n", n + 1), ("bytes", 8 * n + 8), ("layout", "packed_lower"), ("sum_bits", "x"), ("sum_bits", None)):
        broken = {"files": {"mlp_mean": dict(entry, **{field: bad})}}
        with pytest.raises(ValueError, match=rf"layer 3: field files\.mlp_mean\.{field}"):
            CC.validate_extra_entry(broken, {"n_inner": n}, layer, "mlp_mean")
    with pytest.raises(ValueError, match=r"files\.mlp_mean\.n"):
        CC.validate_extra_entry(meta, {"n_inner": n + 2}, layer, "mlp_mean")                  # this run's width differs
    with pytest.raises(FileNotFoundError, match=r"layer 3.*files\.mlp_mean\.file"):
        CC.read_mean_file(str(tmp_path), layer, entry)
    # ... and on the data: a truncated file, a flipped bit
    (tmp_path / "moved").rename(path)
    raw = path.read_bytes()
    path.write_bytes(raw[:-8])
    with pytest.raises(ValueError, match=r"layer 3: field files\.mlp_mean\.bytes"):
        CC.read_mean_file(str(tmp_path), layer, entry)
    path.write_bytes(raw[:5] + bytes([raw[5] ^ 1]) + raw[6:])
    with pytest.raises(ValueError, match=r"layer 3: field files\.mlp_mean\.sum_bits"):
        CC.read_mean_file(str(tmp_path), layer, entry)
    with pytest.raises(ValueError, match="n_inner"):
        CC.write_mean_file(str(tmp_path), layer, mu[:-1], n)
