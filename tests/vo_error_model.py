"""Long-double host model of the V/O output error (mdg_vo_output_error) and of the V/O rank curve (mdg_vo_rank_curve), in the style of
tests/output_error_model.py.

    delta_{h,k} = W_o,h[k, :] W_v,g - o'_h[k, :] v'_g        formed DIRECTLY here, [d, d] per query head
    e[h][k] = delta C delta^T,  dnorm2[h][k] = ||delta||^2,  q = e with nothing subtracted
    a[h][k] = (|y| |V_g|) |C| (|y| |V_g|)^T,  y = [W_o,h[k, :], o'_h[k, :]],  V_g = [W_v,g ; -v'_g]: the scale the stacked-Gram route's
    rounding is relative to (an[h][k] = || |y| |V_g| ||^2 for dnorm2).

errors_fp64 restates the kernel's route -- T = V_g C, the Grams, their lower triangles with the factor 2 -- in plain fp64.
curve: the eigen-decomposition of G_g = W_v,g (C + rho I) W_v,g^T by tests/eig_ref.jacobi_eigh (long double, or fp64 for the e_cpu of
the criterion), grouped c_i = max(lambda_i, 0) sum_h ||W_o,h v_i||^2, MHA c_i = max(lambda2_i, 0) from the second decomposition.
whitening_error, head_map_error, signed_factor_error, mha_gram_error, weyl_bound: the metrics tests/test_gpu_vo_factors.py holds the
device's own factors and mdg_vo_spectrum's bound to, against `factors(spectra(...))` in long double.
Nothing here imports the package or needs a GPU."""
import numpy as np

from tests import eig_ref as E
from tests.output_error_model import LD, wide


def head_blocks(Wv, Wo, vn, on, n_heads, n_kv, hd, r, h, dtype=LD):
    """(W_v,g [hd, d], W_o,h [d, hd], v'_g [r, d], o'_h [d, r]) of query head h, widened exactly; r = 0 or vn None: empty factors."""
    g = h // (n_heads // n_kv)
    Wv, Wo = wide(Wv, dtype), wide(Wo, dtype)
    d = Wv.shape[1]
    if vn is None or on is None or r == 0:
        return Wv[g * hd:(g + 1) * hd], Wo[:, h * hd:(h + 1) * hd], np.zeros((0, d), dtype), np.zeros((d, 0), dtype)
    return Wv[g * hd:(g + 1) * hd], Wo[:, h * hd:(h + 1) * hd], wide(vn, dtype)[g * r:(g + 1) * r], wide(on, dtype)[:, h * r:(h + 1) * r]


def errors(C, Wv, Wo, n_heads, n_kv, hd, r, vn, on):
    """(e, dnorm2, a, an) in long double, [n_heads, d] each, from delta formed directly."""
    Cl = wide(C)
    out = [[], [], [], []]
    for h in range(n_heads):
        wv, wo, v1, o1 = head_blocks(Wv, Wo, vn, on, n_heads, n_kv, hd, r, h)
        delta = wo @ wv - o1 @ v1
        B = np.abs(wo) @ np.abs(wv) + np.abs(o1) @ np.abs(v1)             # |y| |V_g|
        out[0].append(((delta @ Cl) * delta).sum(axis=1))
        out[1].append((delta * delta).sum(axis=1))
        out[2].append(((B @ np.abs(Cl)) * B).sum(axis=1))
        out[3].append((B * B).sum(axis=1))
    return tuple(np.stack(t) for t in out)


def _lower_form(y, G):
    P = y @ np.tril(G, -1)                                                # P_kj = sum_{i > j} y_ki G_ij
    return (y * (2 * P + y * G.diagonal())).sum(axis=1)


def errors_fp64(C, Wv, Wo, n_heads, n_kv, hd, r, vn, on, dtype=np.float64):
    """(e, dnorm2) by the stacked-Gram route in plain numpy fp64 (the e_cpu of the forward criterion)."""
    Cl = wide(C, dtype)
    e, dn = [], []
    for h in range(n_heads):
        wv, wo, v1, o1 = head_blocks(Wv, Wo, vn, on, n_heads, n_kv, hd, r, h, dtype)
        V = np.concatenate([wv, -v1])
        y = np.concatenate([wo, o1], axis=1)
        e.append(_lower_form(y, (V @ Cl) @ V.T))
        dn.append(_lower_form(y, V @ V.T))
    return np.stack(e), np.stack(dn)


def spectra(C, ridge, Wv, Wo, n_heads, n_kv, hd, dtype=LD):
    """Per kv head: (lam [hd] descending, V [hd, hd] eigenvectors in columns, lam2, Up) -- lam2 / Up of the second decomposition
    B B^T, B = S V^T W_o,h^T, for the MHA variant (None, None for the grouped one).  M = C + ridge I, the ridge added in `dtype`."""
    M = wide(C, dtype) + dtype(np.float64(ridge)) * np.eye(C.shape[0], dtype=dtype)
    Wvl, Wol = wide(Wv, dtype), wide(Wo, dtype)
    out = []
    for g in range(n_kv):
        wv = Wvl[g * hd:(g + 1) * hd]
        lam, V, _ = E.jacobi_eigh(wv @ M @ wv.T, dtype=dtype)
        lam2 = Up = None
        if n_kv == n_heads:
            wo = Wol[:, g * hd:(g + 1) * hd]
            Y = (V * np.sqrt(np.maximum(lam, 0))).T                        # Y[a][k] = S_a V[k][a]
            lam2, Up, _ = E.jacobi_eigh(Y @ (wo.T @ wo) @ Y.T, dtype=dtype)
        out.append((lam, V, lam2, Up))
    return out


def curve(C, ridge, Wv, Wo, n_heads, n_kv, hd, dtype=LD, spec=None):
    """curve [n_kv, hd + 1] in `dtype`: the suffix sums of c_i, accumulated from the tail."""
    spec = spectra(C, ridge, Wv, Wo, n_heads, n_kv, hd, dtype) if spec is None else spec
    Wol = wide(Wo, dtype)
    group = n_heads // n_kv
    out = np.zeros((n_kv, hd + 1), dtype=dtype)
    for g, (lam, V, lam2, _) in enumerate(spec):
        if lam2 is not None:
            c = np.maximum(lam2, 0)
        else:
            w = np.zeros(hd, dtype=dtype)
            for h in range(g * group, (g + 1) * group):
                Z = Wol[:, h * hd:(h + 1) * hd] @ V
                w += (Z * Z).sum(axis=0)
            c = np.maximum(lam, 0) * w
        for i in range(hd - 1, -1, -1):
            out[g, i] = out[g, i + 1] + c[i]
    return out


def factors(spec, Wv, Wo, n_heads, n_kv, hd, r, dtype=LD):
    """(v_new [n_kv r, d], o_new [d, n_heads r]) of rank r in `dtype` from the model's own eigenvectors, as vo.hip forms them:
    grouped v' = S_r^-1 V_r^T W_v,g, o'_h = W_o,h V_r S_r; MHA v' = Up_r^T S^-1 V^T W_v, o' = W_o V S Up_r."""
    Wvl, Wol = wide(Wv, dtype), wide(Wo, dtype)
    group = n_heads // n_kv
    vs, os_ = [], [None] * n_heads
    for g, (lam, V, lam2, Up) in enumerate(spec):
        S = np.sqrt(np.maximum(lam, 0))
        VoverS = np.divide(V, S, out=np.zeros_like(V), where=S > 0)          # (a zero eigenvalue's component is dropped, as in vo.hip)
        if lam2 is None:
            P, Q = VoverS[:, :r].T, V[:, :r] * S[:r]
        else:
            P, Q = Up[:, :r].T @ VoverS.T, (V * S) @ Up[:, :r]
        vs.append(P @ Wvl[g * hd:(g + 1) * hd])
        for h in range(g * group, (g + 1) * group):
            os_[h] = Wol[:, h * hd:(h + 1) * hd] @ Q
    return np.concatenate(vs), np.concatenate(os_, axis=1)


def min_relative_gap(lam):
    """min_i (lam_i - lam_i+1) / lam_i of a descending positive spectrum."""
    lam = np.asarray(lam)
    return float(((lam[:-1] - lam[1:]) / lam[:-1]).min())


# ---------------------------------------------------------------- the metrics of the factors themselves (tests/test_gpu_vo_factors.py)
def _heads(v, o, n_heads, n_kv, r):
    """[(g, h, v_g [r, d], o_h [d, r])] in long double."""
    v, o = wide(v), wide(o)
    group = n_heads // n_kv
    return [(h // group, h, v[h // group * r:(h // group + 1) * r], o[:, h * r:(h + 1) * r]) for h in range(n_heads)]


def whitening_error(C, ridge, v, n_kv, r, keep=None):
    """W: max_g max |v_g M v_g^T - I|, M = C + ridge I in long double.  keep: the components (of every kv head) that count."""
    M = wide(C) + LD(np.float64(ridge)) * np.eye(C.shape[0], dtype=LD)
    v = wide(v)
    keep = np.arange(r) if keep is None else np.asarray(keep)
    worst = 0.0
    for g in range(n_kv):
        vg = v[g * r:(g + 1) * r][keep]
        worst = max(worst, float(np.abs(vg @ M @ vg.T - np.eye(len(keep), dtype=LD)).max()))
    return worst


def head_map_error(v, o, tv, to, n_heads, n_kv, r):
    """P: max_h max |o_h v_g - to_h tv_g| / max |to_h tv_g|: the per-head map, which no choice of signs or of a basis inside the kept
    subspace changes."""
    worst = 0.0
    for (g, h, vg, oh), (_, _, tvg, toh) in zip(_heads(v, o, n_heads, n_kv, r), _heads(tv, to, n_heads, n_kv, r)):
        want = toh @ tvg
        worst = max(worst, float(np.abs(oh @ vg - want).max() / np.abs(want).max()))
    return worst


def signed_factor_error(v, o, tv, to, n_heads, n_kv, r):
    """F: component a of kv head g gets the sign of <v_g[a], tv_g[a]>, the same sign on column a of every o_h of the group; then
    max_a max |s_a v_g[a] - tv_g[a]| / max |tv_g[a]| over the rows of v and likewise over the columns of o."""
    worst = 0.0
    for (g, h, vg, oh), (_, _, tvg, toh) in zip(_heads(v, o, n_heads, n_kv, r), _heads(tv, to, n_heads, n_kv, r)):
        sgn = np.sign((vg * tvg).sum(axis=1))
        sgn[sgn == 0] = 1
        ev = np.abs(sgn[:, None] * vg - tvg).max(axis=1) / np.abs(tvg).max(axis=1)
        eo = np.abs(oh * sgn - toh).max(axis=0) / np.abs(toh).max(axis=0)
        worst = max(worst, float(ev.max()), float(eo.max()))
    return worst


def mha_gram_error(o, spec, n_heads, r):
    """L (MHA): max_h max |o_h^T o_h - diag(lam2[:r])| / lam2[0]."""
    o, worst = wide(o), 0.0
    for h in range(n_heads):
        oh, lam2 = o[:, h * r:(h + 1) * r], spec[h][2]
        worst = max(worst, float(np.abs(oh.T @ oh - np.diag(lam2[:r])).max() / lam2[0]))
    return worst


def relative_gap_at(lam, r):
    """(lam_r - lam_r+1) / lam_r, 1-based; r = len(lam) needs no gap: inf."""
    return float("inf") if r >= len(lam) else float((lam[r - 1] - lam[r]) / lam[r - 1])


def weyl_bound(C, Wv, n_kv, hd, eps):
    """mdg_vo_spectrum's out[4] per kv head in long double: eps || |W_v,g| sqrt(diag C) ||_2^2."""
    s = np.sqrt(np.maximum(np.diagonal(wide(C)), 0))
    W = np.abs(wide(Wv))
    return np.array([LD(np.float64(eps)) * (((W[g * hd:(g + 1) * hd] @ s) ** 2).sum()) for g in range(n_kv)], dtype=LD)


def weights(d, n_heads, n_kv, hd, wdt, seed=0, grade=1.0):
    """(W_v [n_kv hd, d], W_o [d, n_heads hd]) as torch tensors of dtype wdt, N(0, 0.05^2); grade < 1 scales row i of every kv head's
    W_v by grade^i, which spreads the spectrum of G (the curve's tests need its eigenvalues apart)."""
    import torch
    gen = torch.Generator().manual_seed(100003 * seed + 1009 * d + 31 * n_heads + hd)
    Wv = torch.randn(n_kv * hd, d, generator=gen, dtype=torch.float64) * 0.05
    Wo = torch.randn(d, n_heads * hd, generator=gen, dtype=torch.float64) * 0.05
    Wv = Wv * (float(grade) ** (torch.arange(n_kv * hd) % hd).double())[:, None]
    return Wv.to(wdt), Wo.to(wdt)


def covariance(d, seed=0):
    """A dense positive semidefinite [d, d] fp64 statistic, exactly symmetric."""
    rng = np.random.default_rng(77 + 13 * d + seed)
    X = rng.standard_normal((3 * d + 2, d)) * (1.0 + 3.0 * rng.random(d))
    C = np.tril(X.T @ X / X.shape[0])
    return C + np.tril(C, -1).T
