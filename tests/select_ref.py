"""Plain fp64 references of the index kernels (modegpt_amd/csrc/select.hip), restated from the words of include/modegpt_hip.h and
not from the kernels: the k-smallest selection, its eight-number certificate, the Q/K unit selection and the fp64 -> bf16 cast.
NumPy / torch on the CPU; tests/test_select_ref_host.py checks them, tests/test_gpu_select.py compares the kernels with them."""
import numpy as np
import torch

INF = float("inf")
ROPE_GROUPED, ROPE_MHA, OPT = 0, 1, 2


def smallest_sorted(s, k):
    """Indices of the k smallest of s, ascending.  Total order: (is-NaN, value, index) ascending -- NaN ranks as largest, ties go to
    the lower index, -0.0 == +0.0."""
    s = np.asarray(s, dtype=np.float64).ravel()
    nan = np.isnan(s)
    order = np.lexsort((np.arange(s.size), np.where(nan, 0.0, s), nan))          # (last key is the primary one)
    return np.sort(order[:k]).astype(np.int64)


def rank_count_select(s, k):
    """The same by brute force: element i is taken iff fewer than k elements come before it in the total order."""
    s = np.asarray(s, dtype=np.float64).ravel()
    n = s.size
    taken = []
    for i in range(n):
        before = 0
        for j in range(n):
            a, b = s[j], s[i]
            if np.isnan(a) or np.isnan(b):
                before += (not np.isnan(a) and np.isnan(b)) or (np.isnan(a) and np.isnan(b) and j < i)
            else:
                before += a < b or (a == b and j < i)
        if before < k:
            taken.append(i)
    return np.asarray(taken, dtype=np.int64)


def margin8(s, sens, idx, n, k, eps):
    """The eight numbers of mdg_select_margin for the selection idx [k] (ascending) of the scores s [n]:
    [0] largest selected score, [1] smallest unselected score, [2] max over selected of s + eps sens, [3] min over unselected of
    s - eps sens, [4] / [5] largest sens among the selected / unselected (0 when there is none), [6] how many scores' intervals
    [s - eps sens, s + eps sens] reach across the midpoint of [0] and [1], [7] 1.0 if [2] < [3].  NaN scores take no part.  An
    empty side leaves its sentinels (-inf for the maxima, +inf for the minima), nothing is counted and the selection is certified."""
    s = np.asarray(s, dtype=np.float64).ravel()[:n]
    sens = np.asarray(sens, dtype=np.float64).ravel()[:n]
    sel = np.zeros(n, dtype=bool)
    sel[np.asarray(idx, dtype=np.int64).ravel()[:k]] = True
    live = ~np.isnan(s)
    a, b = sel & live, ~sel & live
    w = eps * sens
    out = np.empty(8, dtype=np.float64)
    out[0] = s[a].max() if a.any() else -INF
    out[1] = s[b].min() if b.any() else INF
    out[2] = (s[a] + w[a]).max() if a.any() else -INF
    out[3] = (s[b] - w[b]).min() if b.any() else INF
    out[4] = sens[a].max() if a.any() else 0.0
    out[5] = sens[b].max() if b.any() else 0.0
    if a.any() and b.any():
        mid = 0.5 * (out[0] + out[1])
        out[6] = int((live & (s - w <= mid) & (mid <= s + w)).sum())
    else:
        out[6] = 0
    out[7] = 1.0 if out[2] < out[3] else 0.0
    return out


def qk_scores(cov_q, cov_k, n_heads, n_kv, hd, rq, rk, mode):
    """[n_kv, ns] scores of mdg_qk_select from the diagonals alone: a squared column norm is max(C_jj + rho, 0) (NaN stays NaN).
    OPT: sqrt(nq_j) sqrt(nk_j) per column; rotary: sum over the group's query heads of nq_j nk_j + nq_j' nk_j', j' = j + hd/2,
    square-rooted in the grouped mode."""
    cq = np.asarray(cov_q, dtype=np.float64).reshape(n_heads, hd, hd)
    ck = np.asarray(cov_k, dtype=np.float64).reshape(n_kv, hd, hd)

    def norm2(Cm, rho):
        v = np.diagonal(Cm, axis1=1, axis2=2) + rho
        return np.where(np.isnan(v), v, np.maximum(v, 0.0))
    nq, nk = norm2(cq, rq), norm2(ck, rk)
    if mode == OPT:
        return np.sqrt(nq) * np.sqrt(nk)
    g, half = n_heads // n_kv, hd // 2
    out = np.zeros((n_kv, half))
    for h in range(n_kv):
        for q in range(h * g, (h + 1) * g):
            out[h] = out[h] + (nq[q, :half] * nk[h, :half] + nq[q, half:] * nk[h, half:])
    return np.sqrt(out) if mode == ROPE_GROUPED else out


def qk_select_ref(cov_q, cov_k, n_heads, n_kv, hd, rq, rk, rank, mode):
    """(mask [n_kv, rank], q_rows [n_heads * rank], k_rows [n_kv * rank]) of mdg_qk_select, int64.  Units in score-descending order,
    NaN first, ties to the lower index; the rotary modes keep rank / 2 units and list them as cat(units, units + hd / 2); the row
    lists are head * hd + mask entry, every query head of a group with its kv head's mask."""
    sc = qk_scores(cov_q, cov_k, n_heads, n_kv, hd, rq, rk, mode)
    ns = sc.shape[1]
    take = rank if mode == OPT else rank // 2
    g = n_heads // n_kv
    mask = np.empty((n_kv, rank), dtype=np.int64)
    for h in range(n_kv):
        nan = np.isnan(sc[h])
        order = np.lexsort((np.arange(ns), -np.where(nan, 0.0, sc[h]), ~nan))[:take]
        mask[h] = order if mode == OPT else np.concatenate((order, order + hd // 2))
    k_rows = (np.arange(n_kv)[:, None] * hd + mask).reshape(-1)
    q_rows = (np.arange(n_heads)[:, None] * hd + np.repeat(mask, g, axis=0)).reshape(-1)
    return mask, q_rows.astype(np.int64), k_rows.astype(np.int64)


def to_bf16_via_float(x):
    """What the library's fp64 -> bf16 conversion is documented to be: double -> float, then float -> bf16, both round-to-nearest-even."""
    return x.double().float().bfloat16()


def to_bf16_single_rounding(x):
    """One correct round-to-nearest-even of the fp64 value to bf16 (finite values inside the float range), for contrast: the float
    nearest below is truncated to bf16, and the exact remainder decides."""
    x = x.double()
    lo = (x.float().view(torch.int32) & ~0xffff).view(torch.float32)            # candidate toward zero (x.float() never crosses it)
    lo = torch.where(lo.double().abs() > x.abs(), ((lo.view(torch.int32) - 0x10000).view(torch.float32)), lo)
    hi = (lo.view(torch.int32) + 0x10000).view(torch.float32)                   # next bf16 away from zero
    dl, dh = (x - lo.double()).abs(), (hi.double() - x).abs()                   # (exact: both differences fit in fp64)
    odd = ((lo.view(torch.int32) >> 16) & 1).bool()
    up = (dh < dl) | ((dh == dl) & odd)
    return torch.where(up, hi, lo).bfloat16()


def double_rounding_set():
    """fp64 values on which double -> float -> bf16 and a single rounding disagree.  A float whose low 16 bits are 0x8000 is an exact
    bf16 tie; widened and multiplied by 1 + 2^-40 it lies just ABOVE the tie (single rounding: up), but the first rounding to float
    lands ON the tie, which then goes to even -- down wherever the kept bf16 is even.  Bases over the normal and subnormal float
    range, both signs, even and odd kept bits (on the odd ones the two roundings agree)."""
    bases = [1.0, 1.5 * 2.0 ** -126, 3.0, 1.0078125, 1.0234375, 0.3671875, 2.0 ** 100, 1.0078125 * 2.0 ** -120, 2.0 ** -130, 96.0,
             1.75 * 2.0 ** -127, 1.625 * 2.0 ** -129]
    f = torch.tensor(bases + [-b for b in bases], dtype=torch.float32)
    tie = ((f.view(torch.int32) & ~0xffff) | 0x8000).view(torch.float32)
    return tie.double() * (1.0 + 2.0 ** -40)
