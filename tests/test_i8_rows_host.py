"""CPU: the host model of the row selection of the int8 covariance (MDG_I8_ROWS; tests/i8_rows_model.py mirrors
csrc/cov_i8_rows.hip) -- no row leaves on ordinary data, exactly the scaled rows leave when a few tokens are far larger than
the rest, nothing leaves when there are too many of them -- and the cliff the feature removes: the route (tests/i8_model.route_of)
of the raw input is "the whole statistic to the fp64 kernel", the route of the input without the chosen rows is that of ordinary data.
"""
import pytest
import torch

from modegpt_amd import _lib
from tests import i8_model as M
from tests import i8_rows_model as R
from tests.test_gpu_i8_f16 import families

BF16 = torch.bfloat16
T, N = 4096, 256
ROWS8 = [0, 31, 32, 2047, 2048, 4000, 4094, 4095]
ROWS64 = list(range(5, T, 64))


@pytest.fixture(scope="module")
def base():
    torch.manual_seed(0)
    g, a, b = torch.randn(T, N), torch.randn(T, N), torch.randn(T, N)
    return {"gaussian": g, "silu_gated": torch.nn.functional.silu(a) * b}


def scaled(x, rows, factor):
    x = x.clone()
    x[rows] *= factor
    return x.to(BF16)


# (kind, rows, factor, planes of the input without those rows, planes of the raw input; None: not pinned)
SCENARIOS = [("gaussian", ROWS8, 2.0 ** 10, 5, 0), ("gaussian", ROWS64, 2.0 ** 10, 5, None), ("silu_gated", ROWS8, 2.0 ** 6, 6, 0)]


def test_constants():
    assert _lib.MDG_I8_ROWS == 16 and _lib.MDG_I8_MAX_ROWS == 64
    assert R.MAX_ROWS == _lib.MDG_I8_MAX_ROWS
    assert "mdg_cov_accum_i8_rows" in _lib.SIGNATURES


@pytest.mark.parametrize("family", ["gaussian", "relu", "cubed", "student_t", "silu_gated"])
def test_no_row_leaves_on_plain_data(family):
    gen = torch.Generator().manual_seed(23)
    X = families(gen, T, N)[family].to(BF16)
    dom = R.dominant_rows(X)
    print(f"[rows model {family}] dominant rows {len(dom)} of {T}")
    assert len(dom) > 8 * R.MAX_ROWS            # far from the limit, not just above it
    assert R.choose_rows(X) == []
    assert R.choose_rows(X, relu=True) == []


@pytest.mark.parametrize("kind,rows,factor,planes_rest,planes_raw", SCENARIOS)
def test_exactly_the_scaled_rows_leave_and_the_route_recovers(base, kind, rows, factor, planes_rest, planes_raw):
    X = scaled(base[kind], rows, factor)
    assert R.choose_rows(X) == rows
    raw = M.route_of(X)
    rest = M.route_of(R.without_rows(X, rows))
    plain = M.route_of(base[kind].to(BF16))
    longest = lambda Y, cols: int(M.list_counts(_lo(Y, cols)).max())      # noqa: E731
    print(f"[rows model {kind} {len(rows)} rows] raw: planes {raw['planes']} columns {len(raw['columns'])} exact {raw['exact']} longest list "
          f"{longest(X, raw['columns'])}; without the rows: planes {rest['planes']} exact {rest['exact']} longest list {longest(R.without_rows(X, rows), [])}")
    # the cliff: the raw input is not certified on the exact route -- with 8 rows the whole statistic goes to the fp64 kernel
    assert not raw["exact"]
    if planes_raw is not None:
        assert raw["planes"] == planes_raw
    # without the rows: the route of ordinary data of this kind
    assert rest["planes"] == planes_rest and rest["exact"] and rest["columns"] == []
    assert (plain["planes"], plain["exact"], plain["columns"]) == (rest["planes"], rest["exact"], rest["columns"])


def _lo(X, cols):
    d = M.digits(X)[0]
    lo = (d[3] != 0) | (d[4] != 0) | (d[5] != 0)
    lo[:, cols] = False
    return lo


def test_overfull_nothing_leaves(base):
    rows = ROWS64 + [4001]
    X = scaled(base["gaussian"], rows, 2.0 ** 10)
    assert R.dominant_rows(X) == sorted(rows) and len(rows) == R.MAX_ROWS + 1
    assert R.choose_rows(X) == []


def test_a_short_call_does_not_leave_as_a_whole():
    """64 tokens or fewer: every row is dominant and there are at most MAX_ROWS of them -- the minority condition keeps them."""
    gen = torch.Generator().manual_seed(3)
    X = torch.randn(48, 128, generator=gen).to(BF16)
    assert len(R.dominant_rows(X)) == 48 and R.choose_rows(X) == []


def test_relu_on_load_is_honoured(base):
    """Rows that are large only on the negative side are no outliers of max(x, 0)."""
    x = base["gaussian"].clone()
    x[ROWS8] = -x[ROWS8].abs() * 2.0 ** 10
    X = x.to(BF16)
    assert R.choose_rows(X) == ROWS8
    assert R.choose_rows(X, relu=True) == []
