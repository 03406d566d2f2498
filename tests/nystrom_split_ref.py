"""Host pieces shared by the tests of the split Nystrom refit: the statistics, the fp64 torch evaluation of both forms

    full :  X = M^-1 (C[k,:] W^T)                                          (compress_mlp.py:52-57, what the oracle evaluates)
    split:  X = W[:,k]^T + M^-1 (C[k,k'] W[:,k']^T - eps_p W[:,k]^T)       (what mdg_nystrom_down evaluates)

with M = C_kk + eps I as fp64 forms it (eps_p = fl(c_pp + eps) - c_pp), a model of the complement list, and the error metric.
The long-double reference is tests/chol_ref.py's `nystrom`."""
import functools

import numpy as np
import torch

from tests import chol_ref as R

F64 = torch.float64
U = 2.0 ** -53


def complement(idx, n):
    """The indices of 0 .. n-1 that idx does not name, ascending; entries of idx outside 0 .. n-1 name nothing."""
    marks = np.zeros(n, dtype=bool)
    idx = np.asarray(idx)
    marks[idx[(idx >= 0) & (idx < n)]] = True
    return np.flatnonzero(~marks)


def compacted(A, rows, comp, pitch):
    """A[rows][:, comp] in a zero-padded [len(rows), pitch] array (rows=None: every row)."""
    A = np.asarray(A)
    sub = A[:, comp] if rows is None else A[np.asarray(rows)][:, comp]
    out = np.zeros((sub.shape[0], pitch), dtype=A.dtype)
    out[:, :len(comp)] = sub
    return out


def ridge_factor(C, idx, eps):
    Ckk = C[idx][:, idx].clone()
    Ckk.diagonal().add_(eps)
    return torch.linalg.cholesky(Ckk)


def full_form(C, idx, W, eps):
    """[r, d] fp64: the reference expression with the ridge as an argument (oracle.modegpt_oracle.nystrom_down fixes it at 1e-6)."""
    C, W = C.to(F64), W.to(F64)
    return torch.cholesky_solve(C[idx, :] @ W.T, ridge_factor(C, idx, eps))


def split_form(C, idx, W, eps):
    C, W = C.to(F64), W.to(F64)
    n = C.shape[0]
    comp = torch.from_numpy(complement(idx.numpy(), n))
    c = C.diagonal()[idx]
    eps_p = (c + eps) - c
    Wk = W[:, idx].T
    rhs = C[idx][:, comp] @ W[:, comp].T - eps_p[:, None] * Wk
    return Wk + torch.cholesky_solve(rhs, ridge_factor(C, idx, eps))


def column_error(X, ref):
    """max over entries of |x - ref| relative to the largest |ref| of the entry's column (a column is one right-hand side)."""
    return float((np.abs(R.ld(X) - ref).max(axis=0) / np.abs(ref).max(axis=0)).max())


def unit_diagonal(C):
    s = C.diagonal().rsqrt()
    C = torch.tril(C * s[:, None] * s[None, :])
    C = C + torch.tril(C, -1).T
    C.diagonal().fill_(1.0)
    return C


@functools.lru_cache(maxsize=None)
def statistic(kind, n):
    """'well': unit diagonal, condition ~1e3.  'lowrank': unit-scale, rank n / 4 plus 1e-9 of a full-rank part -- C_kk is singular to
    1e-9 and the ridge decides the solve."""
    if kind == "well":
        return unit_diagonal(R.spd_matrix(n, 3.0, seed=5))
    gen = torch.Generator().manual_seed(31 * n)
    G = torch.randn(n, n // 4, generator=gen, dtype=F64)
    C = G @ G.T / (n // 4) + 1e-9 * R.spd_matrix(n, 1.0, seed=6)
    C = torch.tril(C)
    return C + torch.tril(C, -1).T


def selection(n, r, seed, shuffled=False):
    gen = torch.Generator().manual_seed(seed)
    idx = torch.sort(torch.randperm(n, generator=gen)[:r]).values
    return idx[torch.randperm(r, generator=gen)] if shuffled else idx
