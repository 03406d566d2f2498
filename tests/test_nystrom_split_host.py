"""The identity behind the split Nystrom refit, in fp64 torch against the long-double solve of tests/chol_ref.py:

    (C_kk + eps I)^-1 C[k,:] W^T  =  W[:,k]^T + M^-1 (C[k,k'] W[:,k']^T - eps_p W[:,k]^T),      M = C_kk + eps I

Both sides are the same backward-stable solve with M, so the split form's error may not exceed 2 x the full form's (the factor 2 is
the margin over the reference form) plus a floor of n 2^-53 relative to the column's largest entry (one rounding per term of a sum
of n).  Also the Python model of the complement list and the compaction that the GPU tests compare against."""
import numpy as np
import pytest
import torch

from tests import chol_ref as R
from tests import nystrom_split_ref as S

N = 160


@pytest.mark.parametrize("eps", [1e-6, 0.5])
@pytest.mark.parametrize("keep", [0.7, 0.3, 1.0])
@pytest.mark.parametrize("kind", ["well", "lowrank"])
def test_split_form_is_no_worse_than_the_full_product(kind, keep, eps):
    C = S.statistic(kind, N)
    r = int(keep * N)
    idx = S.selection(N, r, seed=17 + r)
    W = (torch.randn(33, N, generator=torch.Generator().manual_seed(r), dtype=torch.float64) * 0.05).to(torch.bfloat16)
    ref = R.nystrom(C, idx.numpy(), W.double(), eps)
    e_full = S.column_error(S.full_form(C, idx, W, eps), ref)
    e_split = S.column_error(S.split_form(C, idx, W, eps), ref)
    print("IDENTITY %s keep %.1f eps %g: full %.3e split %.3e ratio %.3f" % (kind, keep, eps, e_full, e_split, e_split / e_full))
    assert e_split <= 2 * e_full + N * S.U


def test_a_wrong_sign_of_the_ridge_term_is_seen_at_eps_half():
    """What the eps = 0.5 cases are for: with the ridge term's sign flipped the split form is wrong by O(1), not by rounding."""
    C = S.statistic("well", N)
    idx = S.selection(N, 112, seed=3)
    W = torch.randn(5, N, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    ref = R.nystrom(C, idx.numpy(), W, 0.5)
    comp = torch.from_numpy(S.complement(idx.numpy(), N))
    Wk = W[:, idx].T
    wrong = Wk + torch.cholesky_solve(C[idx][:, comp] @ W[:, comp].T + 0.5 * Wk, S.ridge_factor(C, idx, 0.5))
    assert S.column_error(wrong, ref) > 1e-2


def test_complement_model():
    assert S.complement([3, 0, 5], 6).tolist() == [1, 2, 4]
    assert S.complement([5, 3, 0], 6).tolist() == [1, 2, 4]                 # the order of idx does not matter
    assert S.complement(np.arange(6), 6).tolist() == []
    assert S.complement([2], 3).tolist() == [0, 1]
    assert S.complement([-1, 7, 1], 3).tolist() == [0, 2]                   # out of range: names nothing
    gen = np.random.default_rng(0)
    for n, r in ((1, 1), (129, 1), (384, 269), (384, 383)):
        idx = gen.permutation(n)[:r]
        comp = S.complement(idx, n)
        assert len(comp) == n - r and (np.diff(comp) > 0).all()
        assert sorted(comp.tolist() + idx.tolist()) == list(range(n))


def test_compaction_model_pads_with_zeros():
    A = np.arange(30, dtype=np.float64).reshape(5, 6)
    comp = S.complement([4, 1], 6)
    out = S.compacted(A, [4, 1], comp, 16)
    assert out.shape == (2, 16) and (out[:, 4:] == 0).all()
    assert out[:, :4].tolist() == [[24, 26, 27, 29], [6, 8, 9, 11]]
    assert S.compacted(A, None, comp, 16)[:, :4].tolist() == A[:, [0, 2, 3, 5]].tolist()
