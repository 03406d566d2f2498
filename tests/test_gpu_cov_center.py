"""GPU: mdg_cov_center, S_ij = fma(-mu_i, mu_j, C_ij), through the raw C ABI.

Integer inputs (|C_ij| < 2^20, |mu_i| < 2^10) make the fused result exact: torch.equal against the long double model.  Generic data is
held entry-wise to one rounding, 2^-53 (|C_ij| + |mu_i mu_j|).  S equals its transpose bit for bit in every case -- also when the upper
triangle of C holds NaN, which is never read.  Sizes sit around the 64 x 64 tile; C and S have different padded leading dimensions
and the pads, NaN-filled, stay untouched."""
import numpy as np
import pytest
import torch

from tests import mean_model as M

pytestmark = pytest.mark.gpu
TILE = 64                         # ops.COV_CENTER_TILE, asserted below
SIZES = [1, TILE - 1, TILE + 1, 3 * TILE + 5]


def _run(C, mu, pad_c=3, pad_s=5, poison_upper=False):
    from modegpt_amd import _lib, ops
    assert ops.COV_CENTER_TILE == TILE
    lib = _lib.load()
    dev = torch.device("cuda")
    n = C.shape[0]
    ldc, lds = n + pad_c, n + pad_s
    Cb = torch.full((n, ldc), float("nan"), dtype=torch.float64, device=dev)
    Cb[:, :n] = torch.from_numpy(C).to(dev)
    if poison_upper:
        Cb[:, :n] = torch.where(torch.triu(torch.ones(n, n, dtype=torch.bool, device=dev), 1), torch.full_like(Cb[:, :n], float("nan")),
                                Cb[:, :n])
    before = Cb.clone()
    Sb = torch.full((n + 2, lds), float("nan"), dtype=torch.float64, device=dev)      # (two guard rows behind the matrix)
    mu_d = torch.from_numpy(mu).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.mdg_cov_center(Cb.data_ptr(), n, ldc, mu_d.data_ptr(), Sb.data_ptr(), lds, st), "mdg_cov_center")
    torch.cuda.synchronize(dev)
    assert torch.equal(Cb.view(torch.int64), before.view(torch.int64)), "C was modified"
    host = Sb.cpu()
    assert bool(torch.isnan(host[:n, n:]).all()) and bool(torch.isnan(host[n:]).all()), "a pad of S was written"
    S = host[:n, :n].contiguous()
    assert torch.equal(S, S.T.contiguous()), "S is not symmetric bit for bit"
    return S.numpy()


def _sym(A):
    return np.tril(A) + np.tril(A, -1).T


@pytest.mark.parametrize("n", SIZES)
def test_integer_inputs_are_exact(n):
    rng = np.random.default_rng(n)
    C = _sym(rng.integers(-2 ** 20, 2 ** 20, size=(n, n)).astype(np.float64))
    mu = rng.integers(-2 ** 10, 2 ** 10, size=n).astype(np.float64)
    ref = M.center(C, mu).astype(np.float64)
    assert np.array_equal(ref.astype(M.LD), M.center(C, mu))
    assert np.array_equal(_run(C, mu), ref)
    assert np.array_equal(_run(C, mu, poison_upper=True), ref)      # nothing above the diagonal of C is read


@pytest.mark.parametrize("n", SIZES)
def test_generic_data_within_one_rounding(n):
    rng = np.random.default_rng(100 + n)
    H = np.abs(rng.standard_normal((2 * n + 8, n))) * 2.0 ** rng.integers(-3, 4, size=n)
    C = _sym(H.T @ H / H.shape[0])
    mu = H.mean(axis=0)
    S = _run(C, mu, pad_c=0, pad_s=7)
    ref = M.center(C, mu)
    bound = M.LD(2.0 ** -53) * (np.abs(M.ld(C)) + np.abs(np.outer(M.ld(mu), M.ld(mu))))
    err = np.abs(M.ld(S) - ref)
    print(f"n={n}: max err / bound = {float((err / bound).max()):.3e}")
    assert np.all(err <= bound)


def test_ops_front_end_and_refusals():
    from modegpt_amd import ops
    dev = torch.device("cuda")
    rng = np.random.default_rng(5)
    n = 70
    C = _sym(rng.integers(-1000, 1000, size=(n, n)).astype(np.float64))
    mu = rng.integers(-30, 30, size=n).astype(np.float64)
    Cd, mud = torch.from_numpy(C).to(dev), torch.from_numpy(mu).to(dev)
    S = ops.cov_center(Cd, mud)
    assert np.array_equal(S.cpu().numpy(), M.center(C, mu).astype(np.float64)) and np.array_equal(Cd.cpu().numpy(), C)
    big = torch.zeros(n, n + 9, dtype=torch.float64, device=dev)
    out = ops.cov_center(Cd, mud, out=big[:, :n])
    assert out.data_ptr() == big.data_ptr() and torch.equal(big[:, :n], S) and not bool(big[:, n:].any())
    with pytest.raises(ValueError):
        ops.cov_center(Cd, mud[:-1])
    with pytest.raises(ValueError):
        ops.cov_center(Cd.to(torch.float32), mud)
