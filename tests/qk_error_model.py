"""Long-double host model of the Q/K logit error at every rank (mdg_qk_rank_curve), in the style of tests/vo_error_model.py.

    P_h = (sigma_q,h + rho_q I) (.) (sigma_k,kv(h) + rho_k I)              entry-wise, [hd, hd] per query head
    unit u: columns {u, u + hd/2} (RoPE modes, ns = hd/2) or {u} (OPT, ns = hd)
    curve_h[h][m] = sum_{a, b in cols(D_m)} P_h[a][b],  D_m = {order[i] : i >= m};   A_h the same with |P_h|
    curve[kv][m] = sum_{h in group} curve_h[h][m],  A likewise
    terms[kv][i] = sum_{h in group} sum_{a in cols(order[i])} max(Cq_aa + rho_q, 0) max(Ck_aa + rho_k, 0)
    B = the group's unit-block sums of sum_h P_h; a greedy step's increment Delta_u = B[u][u] + sum_{v in D} (B[u][v] + B[v][u])

and the input builders: sigma = X^T X / T from Gaussian columns mixed by I + 0.3 N and scaled over four decades.
Nothing here imports the package or needs a GPU."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
ROPE_GROUPED, ROPE_MHA, OPT = 0, 1, 2          # include/modegpt_hip.h: MDG_QK_ROPE_GROUPED / _ROPE_MHA / _OPT


def units(mode, hd):
    """(ns, columns per unit)."""
    return (hd, 1) if mode == OPT else (hd // 2, 2)


def sigma(n, hd, T, seed):
    """[n, hd, hd] fp64: X^T X / T per head, X = (T Gaussian rows) (I + 0.3 N) diag(scales), scales spread over four decades."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, hd, hd))
    for i in range(n):
        X = rng.standard_normal((T, hd)) @ (np.eye(hd) + 0.3 * rng.standard_normal((hd, hd)))
        X = X * 10.0 ** rng.uniform(-2.0, 2.0, hd)
        out[i] = X.T @ X / T
    return out


def full_rank(n, hd, seed):
    return sigma(n, hd, 3 * hd, seed)


def rank_deficient(n, hd, seed):
    return sigma(n, hd, max(1, hd // 2), seed)


BUILDERS = {"full": full_rank, "deficient": rank_deficient}


def product(cq, ck, rq, rk, dtype=LD):
    """P of one query head."""
    hd = cq.shape[-1]
    eye = np.eye(hd, dtype=dtype)
    return (cq.astype(dtype) + dtype(rq) * eye) * (ck.astype(dtype) + dtype(rk) * eye)


def unit_blocks(P, mode):
    """[ns, ns]: the sums of P over cols(u) x cols(v)."""
    ns, w = units(mode, P.shape[0])
    if w == 1:
        return P.copy()
    return P[:ns, :ns] + P[:ns, ns:2 * ns] + P[ns:2 * ns, :ns] + P[ns:2 * ns, ns:2 * ns]


def along(Ub, order):
    """[ns + 1]: sum of Ub over D_m x D_m for every m, D_m = order[m:]; [ns] = 0."""
    o = np.asarray(order, dtype=np.int64)
    M = Ub[np.ix_(o, o)][::-1, ::-1]
    S = np.cumsum(np.cumsum(M, axis=0), axis=1)                     # S[i][j] = sum of the last i+1 x j+1 block
    return np.concatenate([S.diagonal()[::-1], np.zeros(1, Ub.dtype)])


def model(cov_q, cov_k, mode, rq, rk, order, dtype=LD):
    """{"curve_h", "A_h": [n_heads, ns + 1]; "curve", "A": [n_kv, ns + 1]} in `dtype` (LD: the reference; float64: the same route in
    plain fp64, for the a-priori bound's own test)."""
    n_heads, n_kv = cov_q.shape[0], cov_k.shape[0]
    g = n_heads // n_kv
    ch, ah = [], []
    for h in range(n_heads):
        P = product(cov_q[h], cov_k[h // g], rq, rk, dtype)
        ch.append(along(unit_blocks(P, mode), order[h // g]))
        ah.append(along(unit_blocks(np.abs(P), mode), order[h // g]))
    ch, ah = np.stack(ch), np.stack(ah)
    group = lambda t: np.stack([sum(t[kv * g + q] for q in range(g)) for kv in range(n_kv)])      # noqa: E731
    return {"curve_h": ch, "A_h": ah, "curve": group(ch), "A": group(ah)}


def objective(cov_q, cov_k, mode, rq, rk, order):
    """(curve, A) of the kv groups along ANY order [n_kv][ns], long double."""
    m = model(cov_q, cov_k, mode, rq, rk, order)
    return m["curve"], m["A"]


def terms(cov_q, cov_k, mode, rq, rk, order):
    """[n_kv, ns] long double."""
    n_heads, n_kv, hd = cov_q.shape[0], cov_k.shape[0], cov_q.shape[-1]
    g = n_heads // n_kv
    ns, w = units(mode, hd)
    out = np.zeros((n_kv, ns), LD)
    for kv in range(n_kv):
        dk = np.maximum(np.diagonal(cov_k[kv]).astype(LD) + LD(rk), 0)
        for q in range(g):
            dq = np.maximum(np.diagonal(cov_q[kv * g + q]).astype(LD) + LD(rq), 0)
            d = dq * dk
            per_unit = d[:ns] + d[ns:2 * ns] if w == 2 else d
            out[kv] += per_unit[np.asarray(order[kv], dtype=np.int64)]
    return out


def group_blocks(cov_q, cov_k, mode, rq, rk, kv):
    """(B, |B|) [ns, ns] of kv group `kv`: unit-block sums of sum_h P_h and of sum_h |P_h|, long double."""
    g = cov_q.shape[0] // cov_k.shape[0]
    Ps = [product(cov_q[kv * g + q], cov_k[kv], rq, rk) for q in range(g)]
    return sum(unit_blocks(P, mode) for P in Ps), sum(unit_blocks(np.abs(P), mode) for P in Ps)


def greedy_increments(B, dropped):
    """Delta_u for every unit u given the dropped set (a list): B[u][u] + sum_{v in D} (B[u][v] + B[v][u])."""
    d = np.asarray(dropped, dtype=np.int64)
    return B.diagonal() + (B[:, d].sum(axis=1) + B[d, :].sum(axis=0) if len(d) else 0)
