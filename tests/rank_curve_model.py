"""Long-double host model of the MLP error-versus-rank curve (mdg_nystrom_rank_curve), built on tests/chol_ref.py.

    M = C + eps I (eps added in fp64, one rounding per diagonal entry, as the kernel adds it),  pi = `order`,
    M[pi, pi] = L L^T,  Z = W[:, pi] L,  c_j = ||Z[:, j]||^2,  curve[r] = sum_{j >= r} c_j,  r = 0 .. n.

Why the suffix sums are Nystrom residuals: split pi at r, M[pi, pi] = [[A, B^T], [B, D]] and L = [[L11, 0], [L21, L22]]; then
L22 L22^T = D - B A^-1 B^T, the Schur complement of A = M_SS (S = pi[:r]), and M - M[:, S] M_SS^-1 M[S, :] is zero outside the
rows and columns pi[r:], where it equals that Schur complement.  So tr(W (M - M[:, S] M_SS^-1 M[S, :]) W^T) =
||W[:, pi[r:]] L22||_F^2 = sum_{j >= r} ||Z[:, j]||^2: columns j >= r of Z = W[:, pi] L only involve L[r:, r:] = L22.

Nothing here imports the package or needs a GPU."""
import numpy as np

from tests import chol_ref as R

LD = R.LD


def f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu()
        a = a.double().numpy() if a.dtype.is_floating_point else a.numpy()
    return np.asarray(a, dtype=np.float64)


def argsort_stable(scores):
    """Ascending, ties by index, NaN last: torch.argsort(scores, stable=True) -- numpy's stable sort ranks NaN last too."""
    return np.argsort(f64(scores), kind="stable")


def smallest_sorted(scores, r):
    """What mdg_select_smallest_sorted states, written out without a sort of the scores: the ascending indices of the r smallest
    under "ties: lower index first, NaN largest" -- index j is selected when fewer than r entries rank before it."""
    s = f64(scores)
    n = s.shape[0]
    key = np.where(np.isnan(s), np.inf, s)
    nan = np.isnan(s)
    before = np.empty(n, dtype=np.int64)
    for j in range(n):
        lt = (key < key[j]) | ((key == key[j]) & (nan < nan[j]))          # (a NaN ranks behind +inf)
        tie = (key == key[j]) & (nan == nan[j]) & (np.arange(n) < j)
        before[j] = int(lt.sum() + tie.sum())
    return np.flatnonzero(before < r)


def gathered(C, order, eps):
    """M[pi, pi] in fp64 with the ridge added in fp64: the matrix every route factorises."""
    C64 = f64(C)
    C64 = np.tril(C64) + np.tril(C64, -1).T                  # the lower triangle is authoritative
    order = np.asarray(order, dtype=np.int64)
    M = C64[np.ix_(order, order)].copy()
    M[np.diag_indices_from(M)] += np.float64(eps)
    return M


def suffix_sums(c):
    out = np.zeros(c.shape[0] + 1, dtype=c.dtype)
    out[:-1] = np.cumsum(c[::-1])[::-1]
    return out


def curve(C, order, W, eps=1e-6):
    """The curve in long double: [n + 1]."""
    order = np.asarray(order, dtype=np.int64)
    L = R.cholesky(gathered(C, order, eps))
    Z = R.ld(f64(W))[:, order] @ L
    return suffix_sums((Z * Z).sum(axis=0))


def curve_fp64(C, order, W, eps=1e-6):
    """The same algorithm in plain fp64 numpy / LAPACK (the e_cpu of the forward criterion)."""
    order = np.asarray(order, dtype=np.int64)
    L = np.linalg.cholesky(gathered(C, order, eps))
    Z = f64(W)[:, order] @ L
    return suffix_sums((Z * Z).sum(axis=0))


def schur_trace(C, order, W, eps, r):
    """tr(W (M - M[:, S] M_SS^-1 M[S, :]) W^T), S = order[:r], computed directly (a solve with M_SS), in long double."""
    order = np.asarray(order, dtype=np.int64)
    n = order.shape[0]
    M = R.ld(gathered(C, np.arange(n), eps))
    Wl = R.ld(f64(W))
    if r == 0:
        res = M
    else:
        S = order[:r]
        Mss = gathered(C, S, eps)
        res = M - M[:, S] @ R.cholesky_solve(R.cholesky(Mss), M[S, :])
    return ((Wl @ res) * Wl).sum()


def sandwich(C, W, idx, D, eps=1e-6):
    """(lo, hi) of  E_D + eps ||U||^2 - eps ||W[:, S]||^2 <= curve[r] <= E_D + eps ||U||^2  in long double, for the refit D [r, d]
    (mdg_nystrom_down's down_f64) at the columns S = idx:  U = W with D^T subtracted at the columns S, E_D = sum_k u_k^T C u_k.
    Upper end: curve[r] = min over refits of sum_k u_k^T M u_k, and D is one refit.  Lower end: the minimiser is
    D* = M_SS^-1 M[S, :] W^T = D + eps M_SS^-1 W[:, S]^T (M[S, :] = C[S, :] + eps I[S, :]), and the objective, quadratic with Hessian
    M_SS, exceeds its minimum by tr((D - D*)^T M_SS (D - D*)) = eps^2 tr(W_S M_SS^-1 W_S^T) <= eps ||W_S||_F^2 since M_SS >= eps I."""
    C64 = f64(C)
    Cl = R.ld(np.tril(C64) + np.tril(C64, -1).T)
    idx = np.asarray(idx, dtype=np.int64)
    U = R.ld(f64(W)).copy()
    U[:, idx] -= R.ld(f64(D)).T
    e_d = ((U @ Cl) * U).sum()
    e = LD(np.float64(eps))
    hi = e_d + e * (U * U).sum()
    ws = R.ld(f64(W))[:, idx]
    return hi - e * (ws * ws).sum(), hi


def gated_acts(tokens, n, seed):
    """bf16 SiLU-gated activations silu(g) * u with column scales over 1.5 decades, as a float64 array [tokens, n] of the bf16
    values -- what an MLP's down_proj sees."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    g, u = torch.randn(tokens, n, generator=gen), torch.randn(tokens, n, generator=gen)
    scale = torch.logspace(0, -1.5, n)[torch.randperm(n, generator=gen)]
    return (torch.nn.functional.silu(g) * u * scale).to(torch.bfloat16).double().numpy()


def covariance(X):
    X = f64(X)
    C = np.tril(X.T @ X / X.shape[0])
    return C + np.tril(C, -1).T


def ridge_scores_fp64(C, ridge):
    return np.diag(np.linalg.inv(f64(C) + ridge * np.eye(C.shape[0])))
