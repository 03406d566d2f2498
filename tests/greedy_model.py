"""Host model of the block-greedy MLP column selection (mdg_nystrom_greedy_select), in long double on tests/chol_ref.py and in plain
fp64 numpy / LAPACK, and the seeded cases the host and the GPU tests share.

The algorithm (include/modegpt_hip.h states the same contract):
    M = C + eps I (the lower triangle of C is authoritative; eps added in fp64, one rounding per diagonal entry),
    S = {}, R = M, B = W R, J = sum B o W = tr(W R W^T).
    Round t = 0 .. T-1 (T = min(rounds, r)) takes m_t = floor(r (t + 1) / T) - floor(r t / T) columns:
      gain g_j = (sum_i B_ij^2) / R_jj;  j is eligible if j is not in S, R_jj > n 2^-52 M_jj and g_j is finite;
      the m_t eligible columns of largest gain are picked, ties to the lower index; if fewer are eligible the round is filled with
      unselected ineligible columns in ascending index order (dead picks: they join S with no downdate and are counted);
      with the eligible picks P: K = R[P, P], X = K^-1 R[P, :] by Cholesky of K, R -= R[:, P] X, B -= B[:, P] X;
      objective[t + 1] = sum B o W.
    order: round by round, ascending index within a round; cut[t] = (smallest picked gain, largest eligible gain not picked), NaN
    where there is none; the rounds beyond r take nothing: they repeat the objective and their cut is (NaN, NaN).

Unlike the device, which never forms R (it keeps Yt with R = M - Yt^T Yt and downdates diag(R) and B), the model is the plain
right-looking statement above.  Nothing here imports the package or needs a GPU."""
import functools

import numpy as np

from tests import chol_ref as R
from tests import rank_curve_model as RC

LD = R.LD
EPS = 1e-6
U = 2.0 ** -53
SHAPES = [(48, 8), (130, 40), (300, 136)]           # n off the 16 pitch, across one 128 boundary, across two
RIDGE = float(np.float32(1e-4))                    # the ridge of the rule the selection is compared with


def partition(r, rounds):
    """m_t for t = 0 .. rounds-1."""
    T = min(rounds, r)
    return [r * (t + 1) // T - r * t // T for t in range(T)] + [0] * (rounds - T)


def ranks(n):
    return [1, int(0.7 * n), n - 1, n]


def rounds_for(r):
    """T in {1, 3, 8, r} (without the repeats a small r makes)."""
    return sorted({1, 3, 8, r})


def symmetric(C):
    C64 = RC.f64(C)
    return np.tril(C64) + np.tril(C64, -1).T


def ridged(C, eps):
    M = symmetric(C).copy()
    M[np.diag_indices_from(M)] += np.float64(eps)
    return M


def _solve_spd(K, rhs, dt):
    if dt is LD:
        return R.cholesky_solve(R.cholesky(K), rhs)
    L = np.linalg.cholesky(K)
    return np.linalg.solve(L.T, np.linalg.solve(L, rhs))


def greedy(C, W, r, rounds, eps=EPS, dt=LD):
    """(order int64 [r], objective [rounds + 1], cut [rounds, 2], n_dead, gaps) in the arithmetic `dt` (LD or np.float64); gaps: per
    round that has both sides of its cut, (picked - unpicked) / picked."""
    M = ridged(C, eps).astype(dt)
    Wl = RC.f64(W).astype(dt)
    n = M.shape[0]
    Rm, dM = M.copy(), np.diag(M).copy()
    B = Wl @ Rm
    taken = np.zeros(n, dtype=bool)
    order, objective, cut, gaps, n_dead = [], [(B * Wl).sum()], [], [], 0
    nan = dt(np.nan)
    for m in partition(r, rounds):
        if m == 0:
            objective.append(objective[-1])
            cut.append([nan, nan])
            continue
        dR = np.diag(Rm)
        with np.errstate(all="ignore"):
            g = (B * B).sum(axis=0) / dR
            elig = ~taken & (dR > dt(n) * dt(2.0 ** -52) * dM) & np.isfinite(g)
        cand = np.flatnonzero(elig)
        cand = cand[np.lexsort((cand, -g[cand]))]              # gain descending, ties to the lower index
        picks, left = cand[:m], cand[m:]
        dead = np.flatnonzero(~taken & ~elig)[:m - len(picks)]
        n_dead += len(dead)
        lo = g[picks].min() if len(picks) else nan
        hi = g[left[0]] if len(left) else nan
        cut.append([lo, hi])
        if len(picks) and len(left):
            gaps.append(float((lo - hi) / lo))
        P = np.sort(picks)
        if len(P):
            X = _solve_spd(Rm[np.ix_(P, P)], Rm[P, :], dt)
            Rm = Rm - Rm[:, P] @ X
            B = B - B[:, P] @ X
        chosen = np.sort(np.concatenate((picks, dead)))
        taken[chosen] = True
        order.extend(int(j) for j in chosen)
        objective.append((B * Wl).sum())
    return (np.asarray(order, dtype=np.int64), np.asarray(objective, dtype=dt), np.asarray(cut, dtype=dt).reshape(rounds, 2), n_dead,
            gaps)


def objective_of(C, W, S, eps=EPS):
    """J(S) = tr(W (M - M[:, S] M_SS^-1 M[S, :]) W^T) from scratch, in long double."""
    S = np.asarray(S, dtype=np.int64)
    M, Wl = R.ld(ridged(C, eps)), R.ld(RC.f64(W))
    res = M if len(S) == 0 else M - M[:, S] @ R.cholesky_solve(R.cholesky(M[np.ix_(S, S)]), M[S, :])
    return ((Wl @ res) * Wl).sum()


def scale_A(C, W, eps=EPS):
    """A = sum_i (|W| |M| |W|^T)_ii: what the errors of objective and cut are relative to."""
    Wa = np.abs(RC.f64(W))
    return float(((Wa @ np.abs(ridged(C, eps))) * Wa).sum())


def order_with_rest(order, scores):
    """order ++ the unselected columns in ascending ridge-score order: a permutation the rank curve can run along."""
    order = np.asarray(order, dtype=np.int64)
    by_score = RC.argsort_stable(scores)
    return np.concatenate((order, by_score[~np.isin(by_score, order)]))


# ---------------------------------------------------------------- the shared cases
def _bf16(a):
    import torch
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def case(n, d, kind="mixed", seed=0):
    """(C fp64 [n, n] symmetric, W bf16 torch [d, n]) of a seeded case.  SiLU-gated activations silu(g) * u over 4 n tokens with
    column scales over three decades in random order; kind "mixed": the columns are then mixed by 0.01 I + a rank-n/8 matrix, so
    that they are strongly correlated; "iid": not mixed.  W holds bf16 values, so that the bf16 and the fp64 call see the same numbers."""
    rng = np.random.default_rng(1000003 * n + 101 * d + seed)
    tokens = 4 * n
    g, u = rng.standard_normal((tokens, n)), rng.standard_normal((tokens, n))
    scale = np.logspace(0, -3, n)[rng.permutation(n)]
    X = g / (1 + np.exp(-g)) * u * scale
    if kind == "mixed":
        k = max(2, n // 8)
        X = X @ (0.01 * np.eye(n) + rng.standard_normal((n, k)) @ rng.standard_normal((k, n)) / np.sqrt(k))
    C = RC.covariance(X)
    W = _bf16(rng.standard_normal((d, n)) * 0.05)
    return C, W


def kind_of(n):
    return "iid" if n == 48 else "mixed"


def shared_case(n, d):
    return case(n, d, kind_of(n), SEEDS[(n, d)])


SEEDS = {(48, 8): 0, (130, 40): 0, (300, 136): 0}


def gpu_cases():
    """(n, d, r, rounds) of the model comparison: every shape with r in {1, floor(0.7 n), n - 1, n} and T in {1, 3, 8, r}."""
    return [(n, d, r, T) for n, d in SHAPES for r in ranks(n) for T in rounds_for(r)]


@functools.lru_cache(maxsize=None)
def reference(n, d, r, rounds):
    """The long-double model of a shared case, computed once."""
    C, W = shared_case(n, d)
    return greedy(C, W, r, rounds, EPS, LD)


@functools.lru_cache(maxsize=None)
def reference_fp64(n, d, r, rounds):
    C, W = shared_case(n, d)
    return greedy(C, W, r, rounds, EPS, np.float64)


def duplicate_case():
    """Integer data with exact duplicate columns, for eps = 0: (C [n, n], W bf16 [d, n], the duplicates {copy: original}).  Every
    entry of C is a small integer and every product of the first downdate of a copy is exact, so a copy's R_jj is exactly 0 once its
    original is in S: it is dead."""
    rng = np.random.default_rng(7)
    n, d, tokens = 24, 5, 64
    X = rng.integers(-3, 4, size=(tokens, n)).astype(np.float64)
    dup = {5: 2, 17: 11, 23: 0}
    for c, o in dup.items():
        X[:, c] = X[:, o]
    C = np.tril(X.T @ X)
    C = C + np.tril(C, -1).T
    W = _bf16(rng.integers(-4, 5, size=(d, n)).astype(np.float64))
    for c, o in dup.items():
        W[:, c] = W[:, o]
    return C, W, dup
