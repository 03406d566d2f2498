"""Long-double host model of the realised MLP output error (mdg_mlp_output_error), built on the helpers of tests/chol_ref.py.

    U [d, n]: column j = W[:, j] where j is not kept, W[:, j] - down[:, pos(j)] where j = idx[pos(j)]
    e_k = u_k C u_k^T = sum_i C_ii u_ki^2 + 2 sum_{i > j} C_ij u_ki u_kj          (the lower triangle of C alone)
    a_k = |u_k| |C| |u_k|^T, the same form on absolute values: what the rounding analysis of a sum of products is relative to.

The index rule is the kernel's: entries outside 0 .. n-1 are clamped, and where an index occurs more than once its highest position
is the one subtracted.  Nothing here imports the package or needs a GPU."""
import numpy as np

from tests import chol_ref as R

LD = R.LD


def wide(a, dtype=LD):
    """Exact widening of a torch tensor (bf16 included) or numpy array."""
    if hasattr(a, "detach"):
        a = a.detach().cpu()
        a = a.double().numpy() if a.dtype.is_floating_point else a.numpy()
    return np.asarray(a).astype(dtype)


def inverse_map(idx, n):
    """pos[j] = the highest position p with clamp(idx[p]) == j, -1 where there is none."""
    pos = np.full(n, -1, dtype=np.int64)
    for p, v in enumerate(np.asarray(wide(idx, np.int64)).reshape(-1)):
        pos[min(max(int(v), 0), n - 1)] = p                      # ascending p: the highest one stays
    return pos


def residual(W, idx, down, dtype=LD):
    """U in `dtype` (down: [d, r], or None for U = W); the subtraction happens in `dtype`."""
    U = wide(W, dtype).copy()
    if down is not None and idx is not None and len(idx):
        D = wide(down, dtype)
        pos = inverse_map(idx, U.shape[1])
        kept = np.flatnonzero(pos >= 0)
        U[:, kept] -= D[:, pos[kept]]
    return U


def _forms(C, U, dtype):
    Cl = np.tril(wide(C, dtype))
    diag = Cl.diagonal().copy()
    P = U @ np.tril(Cl, -1)                                      # P_kj = sum_{i > j} u_ki C_ij
    return (U * (2 * P + U * diag)).sum(axis=1)


def errors(C, W, idx, down):
    """(e, a) in long double: [d] each."""
    U = residual(W, idx, down)
    return _forms(C, U, LD), _forms(np.abs(wide(C)), np.abs(U), LD)


def errors_fp64(C, W, idx, down):
    """e by the same algorithm in plain numpy fp64 (the e_cpu of the forward criterion)."""
    return _forms(C, residual(W, idx, down, np.float64), np.float64)


def unorm2(W, idx, down, dtype=LD):
    U = residual(W, idx, down, dtype)
    return (U * U).sum(axis=1)
