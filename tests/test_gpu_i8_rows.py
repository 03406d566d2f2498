"""Outlier token rows on the int8 digit-plane covariance (MDG_I8_ROWS; csrc/cov_i8_rows.hip, host model tests/i8_rows_model.py):
a handful of tokens far larger than the rest leave for the fp64 row kernel and the statistic stays on the int8 path -- checked
against exact integer arithmetic --, nothing changes on ordinary data, too many outliers change nothing, the layouts the masked
kernels and the row kernel take (off-diagonal tiles, unaligned rows, per-head statistics in a fused launch, fp16, ReLU on load),
rows and columns leaving together, a NaN in a row that left, the whole-statistic fallback, and run-to-run determinism.
"""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import modegpt_oracle as O
from tests import i8_model as M
from tests import i8_rows_model as RM
from tests.i8_limits import check_i8_error
from tests.test_gpu_i8_f16 import entry_err, families

pytestmark = pytest.mark.gpu
F64, F16, BF16 = torch.float64, torch.float16, torch.bfloat16
ROWS8 = [0, 31, 32, 2047, 2048, 4000, 4094, 4095]


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def exact_sigma(X):
    """X^T X of a bf16 matrix in exact integer arithmetic (tests/i8_model.digits: x = N 2^(E - 172)) -> (integers V [n][n], exponents
    e [n][n]) with sigma_ij = V_ij 2^e_ij."""
    _, E, N, rounded, _ = M.digits(X)
    assert int(rounded.sum()) == 0 and X.shape[0] <= 4096     # nothing more than 38 binades under its column maximum; int64 suffices
    hi, lo = N >> 24, N & 0xFFFFFF
    hh, hl, ll = hi.T @ hi, hi.T @ lo, lo.T @ lo
    n = X.shape[1]
    V = [[(int(hh[i, j]) << 48) + ((int(hl[i, j]) + int(hl[j, i])) << 24) + int(ll[i, j]) for j in range(i + 1)] for i in range(n)]
    return V, E


def worst_errors(S, X, special=()):
    """max over the lower triangle of |S_ij - exact_ij| / sqrt(exact_ii exact_jj), separately for the entries whose row or column is in
    `special` (columns the fp64 column kernel computed)."""
    V, E = exact_sigma(X)
    n = X.shape[1]
    val = lambda i, j: Fraction(V[i][j]) * Fraction(2) ** int(E[i] + E[j] - 344)      # noqa: E731
    diag = [math.sqrt(float(val(i, i))) for i in range(n)]
    got = S.cpu()
    worst, worst_special = 0.0, 0.0
    for i in range(n):
        for j in range(i + 1):
            e = abs(float(Fraction(got[i, j].item()) - val(i, j))) / (diag[i] * diag[j])
            if i in special or j in special:
                worst_special = max(worst_special, e)
            else:
                worst = max(worst, e)
    return worst, worst_special


def scaled(x, rows, factor, dtype=BF16):
    x = x.clone()
    x[rows] *= factor
    return x.to(dtype)


def case_gaussian():
    gen = torch.Generator().manual_seed(101)
    return scaled(torch.randn(4096, 256, generator=gen), ROWS8, 2.0 ** 10), ROWS8


def case_silu():
    """T = 3000 is no multiple of 32 and spans two list segments.  (Products below 2^-24 are flushed to zero so that no element lies
    more than 38 binades under its column maximum: the exact reference then needs no rounded-element term.)  At 128 columns the
    route without the flag is on the edge -- the fp64 column kernel takes up to 32 of them, a quarter of the statistic, and on most
    seeds that just rescues it (20 .. 32 columns out, six planes); this seed is one where it does not, as for every seed at 256
    columns (tests/test_i8_rows_host.py)."""
    gen = torch.Generator().manual_seed(114)
    T, n = 3000, 128
    x = torch.nn.functional.silu(torch.randn(T, n, generator=gen)) * torch.randn(T, n, generator=gen)
    x = torch.where(x.abs() < 2.0 ** -24, torch.zeros_like(x), x)
    rows = [0, 1, 31, 1500, 2047, 2048, 2998, 2999]
    return scaled(x, rows, 2.0 ** 6), rows


def run(ops, dev, X, rows, **kw):
    S = torch.zeros(X.shape[1], X.shape[1], dtype=F64, device=dev)
    info = {}
    planes = ops.cov_accum_i8(S, X.to(dev), route_info=info, rows=rows, **kw)
    return S, planes, info


@pytest.fixture(scope="module")
def gaussian_run(ops, dev):
    """Case 1 with the flag on, once for the tests that share it."""
    saved = ops.I8_EXACT
    ops.I8_EXACT = True
    try:
        X, rows = case_gaussian()
        ops.i8_rows_left(dev, reset=True)
        S, planes, info = run(ops, dev, X, True)
        left = ops.i8_rows_left(dev)
    finally:
        ops.I8_EXACT = saved
    return X, rows, S, planes, info, left


def check_recovery(ops, dev, X, rows, S, planes, info, left, tag):
    print(f"[rows {tag}] planes {planes} info {info} rows counted {left}")
    assert RM.choose_rows(X) == rows                       # the host model agrees on which rows leave
    assert planes in (5, 6) and info["exact"] and info["rows"] == rows and left == len(rows), info
    assert info["columns"] == []
    worst, _ = worst_errors(S, X)
    print(f"[rows {tag}] worst entry-wise error against exact arithmetic {worst:.3e}, the call's bound {info['bound']:.3e}")
    assert info["bound"] <= 5e-15 + (len(rows) + 1) * 2.0 ** -53 + 1e-30      # exact route: fp64 rounding + the row update's
    assert worst <= info["bound"], (worst, info)


def test_recovery_and_exactness_gaussian(ops, dev, monkeypatch, gaussian_run):
    monkeypatch.setattr(ops, "I8_EXACT", True)
    X, rows, S, planes, info, left = gaussian_run
    _, planes_off, info_off = run(ops, dev, X, False)
    print(f"[rows gaussian] flag off: planes {planes_off} exact {info_off['exact']}")
    assert planes_off == 0 and "rows" not in info_off      # today's behaviour: eight tokens send the whole statistic to the fp64 kernel
    check_recovery(ops, dev, X, rows, S, planes, info, left, "gaussian")


def test_recovery_and_exactness_silu_gated(ops, dev, monkeypatch):
    monkeypatch.setattr(ops, "I8_EXACT", True)
    X, rows = case_silu()
    assert M.route_of(X)["planes"] == 0                    # the host model: without the flag the whole statistic goes to the fp64 kernel
    _, planes_off, _ = run(ops, dev, X, False)
    assert planes_off == 0
    ops.i8_rows_left(dev, reset=True)
    S, planes, info = run(ops, dev, X, True)
    check_recovery(ops, dev, X, rows, S, planes, info, ops.i8_rows_left(dev), "silu_gated")


@pytest.mark.parametrize("family", ["gaussian", "relu", "cubed", "student_t", "silu_gated"])
def test_no_change_on_ordinary_data(ops, dev, family):
    gen = torch.Generator().manual_seed(23)
    X = families(gen, 900, 128)[family].to(BF16)
    ops.i8_route_counts(dev, reset=True)
    S_off, planes_off, info_off = run(ops, dev, X, False)
    counts_off = ops.i8_route_counts(dev, reset=True)
    S_on, planes_on, info_on = run(ops, dev, X, True)
    counts_on = ops.i8_route_counts(dev, reset=True)
    assert info_on.pop("rows") == [] and ops.i8_rows_left(dev) == 0
    assert torch.equal(S_on, S_off) and planes_on == planes_off and info_on == info_off and counts_on == counts_off


def test_65_scaled_rows_nothing_leaves(ops, dev):
    gen = torch.Generator().manual_seed(103)
    rows = list(range(5, 4096, 64)) + [4001]
    X = scaled(torch.randn(4096, 256, generator=gen), rows, 2.0 ** 10)
    assert len(rows) == 65 and RM.choose_rows(X) == []
    S_off, planes_off, info_off = run(ops, dev, X, False)
    S_on, planes_on, info_on = run(ops, dev, X, True)
    assert info_on.pop("rows") == []
    assert torch.equal(S_on, S_off) and planes_on == planes_off and info_on == info_off


def against_oracle(S, X, info, relu=False, ctx=None):
    R = torch.zeros(X.shape[1], X.shape[1], dtype=F64)
    (O.cov_accum_tokens_relu if relu else O.cov_accum_tokens)(R, X)
    err = entry_err(torch.tril(S).cpu(), torch.tril(R))
    print(f"[rows {ctx}] planes {info['planes']} rows {info['rows']} columns {info['columns']} bound {info['bound']:.3e} err {err:.3e}")
    check_i8_error(err, bound=info["bound"], ctx=ctx)


def test_layout_off_diagonal_tiles(ops, dev):
    gen = torch.Generator().manual_seed(104)
    rows = [7, 64, 65, 999]
    X = scaled(torch.randn(1000, 384, generator=gen), rows, 2.0 ** 10)
    S, planes, info = run(ops, dev, X, True)
    assert planes in (5, 6) and info["rows"] == rows
    assert torch.triu(S, 1).abs().max().item() == 0.0         # nothing above the diagonal, as the int8 fold
    against_oracle(S, X, info, ctx="n = 384")


def test_layout_unaligned_rows(ops, dev):
    """x a column slice with ld % 8 != 0: the scalar maximum / split kernels and the vote pass's scalar loads."""
    gen = torch.Generator().manual_seed(105)
    rows = [0, 33, 700, 1029]
    base = scaled(torch.randn(1030, 261, generator=gen), rows, 2.0 ** 10).to(dev)
    x = base[:, 2:258]
    assert x.stride(0) % 8 != 0
    S = torch.zeros(256, 256, dtype=F64, device=dev)
    info = {}
    planes = ops.cov_accum_i8(S, x, route_info=info, rows=True)
    assert planes in (5, 6) and info["rows"] == rows
    against_oracle(S, x.cpu().contiguous(), info, ctx="ld 261")


def test_layout_per_head_statistic_in_a_fused_launch(ops, dev):
    if torch.cuda.get_device_properties(dev).multi_processor_count != 256:
        pytest.skip("the fused launch's tile schedule is cut for 256 CUs")
    gen = torch.Generator().manual_seed(106)
    T, rows = 256, [3, 128, 129, 255]
    x = scaled(torch.randn(T, 2048, generator=gen), rows, 2.0 ** 10)
    q = scaled(torch.randn(T, 2 * 128, generator=gen) * 2, rows, 2.0 ** 10)
    Sx, Sq = torch.zeros(2048, 2048, dtype=F64, device=dev), torch.zeros(2, 128, 128, dtype=F64, device=dev)
    infos = []
    ops.i8_rows_left(dev, reset=True)
    planes = ops.cov_accum_i8_multi([(Sx, x.to(dev), 1), (Sq, q.to(dev), 2)], route_info=infos, rows=True)
    assert planes in (5, 6) and [i["rows"] for i in infos] == [rows, rows] and ops.i8_rows_left(dev) == 2 * len(rows), infos
    against_oracle(Sx, x, infos[0], ctx="fused, n = 2048")
    for h in range(2):
        against_oracle(Sq[h], q[:, h * 128:(h + 1) * 128].contiguous(), infos[1], ctx=f"fused, head {h}")


@pytest.mark.parametrize("relu", [False, True])
def test_layout_fp16_and_relu(ops, dev, relu):
    gen = torch.Generator().manual_seed(107)
    rows = [5, 6, 512, 998]
    X = scaled(torch.randn(1000, 128, generator=gen), rows, 2.0 ** 8, dtype=F16)
    S, planes, info = run(ops, dev, X, True, relu=relu)
    assert planes in (5, 6) and info["rows"] == rows
    against_oracle(S, X, info, relu=relu, ctx=f"fp16 relu={relu}")


def rows_and_a_column():
    gen = torch.Generator().manual_seed(108)
    rows = [3, 500, 501, 1023]
    x = torch.randn(1024, 128, generator=gen)
    x[100, 7] = 2.0 ** 18                  # a massive activation in an ordinary row: column 7's bulk sits 18 binades under it
    return scaled(x, rows, 2.0 ** 10), rows


def test_rows_and_columns_together(ops, dev, monkeypatch):
    monkeypatch.setattr(ops, "I8_EXACT", True)
    X, rows = rows_and_a_column()
    T = X.shape[0]
    model_rows, model_route = RM.route_after(X)
    # (column 7 leaves first; a call this short hands two more columns to the column kernel, as the model says)
    assert model_rows == rows and model_route["columns"][0] == 7 and len(model_route["columns"]) <= 4, model_route
    S, planes, info = run(ops, dev, X, True)
    assert planes in (5, 6) and info["rows"] == rows and info["columns"] == model_route["columns"] and info["exact"], info
    worst, worst_col = worst_errors(S, X, special=set(info["columns"]))
    print(f"[rows + column] worst {worst:.3e} (bound {info['bound']:.3e}); rows / columns of the column kernel {worst_col:.3e}")
    assert worst <= info["bound"]
    # a column that left: a plain fp64 sum of T exact products (2 T roundings) plus the row update's |R| + 1
    assert worst_col <= (2 * T + len(rows) + 1) * 2.0 ** -53


def test_nan_in_a_row_that_left(ops, dev):
    """The int8 path never sees the NaN (its row reads as +0 there, column 9 stays); the row kernel's fp64 products poison exactly
    row 9 and column 9 of sigma, as X.double().T @ X.double() does."""
    X, rows = rows_and_a_column()
    X[501, 9] = float("nan")
    S, planes, info = run(ops, dev, X, True)
    assert planes in (5, 6) and info["rows"] == rows and 9 not in info["columns"], info
    R = torch.tril(X.double().T @ X.double())
    S = torch.tril(S).cpu()
    assert torch.equal(torch.isnan(S), torch.isnan(R)) and int(torch.isnan(S).sum()) == 128
    keep = torch.ones(128, dtype=torch.bool)
    keep[9] = False
    check_i8_error(entry_err(S[keep][:, keep], R[keep][:, keep]), bound=info["bound"])


def test_fallback_runs_the_fp64_kernel_once(ops, dev):
    """Rows leave, but the rest still cannot be certified: 40 columns with a massive activation each, more than the fp64 column
    kernel takes.  The whole statistic goes through the fp64 kernel, which reads every row -- the row kernel must not add the
    rows a second time."""
    gen = torch.Generator().manual_seed(109)
    T, n = 2048, 256
    rows = [0, 31, 32, 1000, 1001, 2000, 2046, 2047]
    x = torch.randn(T, n, generator=gen)
    for k in range(40):
        x[100 + 7 * k, 3 + 6 * k] = 2.0 ** 20
    X = scaled(x, rows, 2.0 ** 10)
    model_rows, model_route = RM.route_after(X)
    assert model_rows == rows and model_route["planes"] == 0, model_route
    ops.i8_route_counts(dev, reset=True)
    S, planes, info = run(ops, dev, X, True)
    counts = ops.i8_route_counts(dev)
    print(f"[rows fallback] planes {planes} info {info} counts {counts}")
    assert planes == 0 and counts["fallback_f64"] == 1 and counts["i8_5"] + counts["i8_6"] == 0
    assert info["rows"] == [] and ops.i8_rows_left(dev) == 0          # no row was computed by the row kernel
    R = torch.zeros(n, n, dtype=F64)
    O.cov_accum_tokens(R, X)
    err = entry_err(torch.tril(S).cpu(), torch.tril(R))
    print(f"[rows fallback] err against the oracle {err:.3e}")
    assert err <= 1e-13


def test_determinism(ops, dev, monkeypatch, gaussian_run):
    monkeypatch.setattr(ops, "I8_EXACT", True)
    X, rows, S, planes, info, _ = gaussian_run
    S2, planes2, info2 = run(ops, dev, X, True)
    assert torch.equal(S, S2) and planes2 == planes and info2 == info
