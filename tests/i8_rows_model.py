"""Host model of the row selection of the int8 covariance (MDG_I8_ROWS; modegpt_amd/csrc/cov_i8_rows.hip): which token rows leave
the int8 path for the fp64 row kernel.  A function of the exponent fields of x alone:

    E_j  = max effective exponent of the nonzero elements of column j, over all rows
    v_t  = #{ j : x_tj != 0 and ee(x_tj) >= E_j - WINDOW }
    row t is dominant  <=>  v_t >= n / SHARE
    the dominant rows leave  <=>  1 <= #dominant <= MAX_ROWS and #dominant * MINORITY <= T       (else: nothing leaves)

Test infrastructure, beside tests/i8_model.py (the route of what is left: `route_after`).
"""
import numpy as np

from tests import i8_model as M

WINDOW, SHARE, MAX_ROWS, MINORITY = 4, 8, 64, 8          # cov_i8_rows.hip: ROW_WINDOW, ROW_SHARE; MDG_I8_MAX_ROWS; ROW_MINORITY


def votes(X, relu=False, window=WINDOW):
    """torch bf16 [T, n] -> v [T] int64."""
    sig, ee = M.bf16_parts(X)
    if relu:
        sig = np.where(sig < 0, 0, sig)
    nz = sig != 0
    E = np.where(nz, ee, 1).max(axis=0)
    return (nz & (ee >= E[None, :] - window)).sum(axis=1)


def dominant_rows(X, relu=False, window=WINDOW, share=SHARE):
    v = votes(X, relu, window)
    return [int(t) for t in np.nonzero(v * share >= X.shape[1])[0]]


def choose_rows(X, relu=False, window=WINDOW, share=SHARE):
    """-> the token rows that leave, ascending ([]: nothing leaves)."""
    dom = dominant_rows(X, relu, window, share)
    return dom if 1 <= len(dom) <= MAX_ROWS and len(dom) * MINORITY <= X.shape[0] else []


def without_rows(X, rows):
    """X as the int8 path sees it: the rows that left read as +0."""
    Y = X.clone()
    if rows:
        Y[rows] = 0
    return Y


def route_after(X, **kw):
    """(rows that leave, i8_model.route_of of what stays)."""
    rows = choose_rows(X)
    return rows, M.route_of(without_rows(X, rows), **kw)
