"""mdg_nystrom_down / _overlapped after the split of the cross term (only the unselected columns of sigma_mlp are multiplied,
DESIGN.md section 3), at n = 384 (three tiles), d in {1, 130}, bf16 and fp64 weights.

Accuracy.  e_gpu <= 4 e_oracle + n 2^-53, both errors against the long-double solve of tests/chol_ref.py in the metric of
tests/nystrom_split_ref.column_error (per entry, relative to the largest entry of its column); e_oracle is the error of the fp64
CPU evaluation of the REFERENCE formula (oracle.modegpt_oracle.nystrom_down; with eps = 0.5, which the oracle does not take, the
same lines with that ridge).  The 4 is the margin over the reference, for a blocked summation order that differs from LAPACK's; the
floor is one rounding per term of a sum of n.  Every case prints its two errors before it asserts (pytest -s).
The eps = 0.5 cases run on a unit-diagonal statistic, where a ridge term that is missing or has the wrong sign is an error of
order one (tests/test_nystrom_split_host.py shows that on the host).

Exactness.  eps = 0, r = n, idx = arange(n): the right-hand side is exactly zero and down_f64 == W_d^T entry for entry.
A workspace full of NaN bytes, inputs inside NaN-filled wider buffers, the overlapped entry point and repeated calls all give the
same bits."""
import functools

import pytest
import torch

from tests import chol_ref as R
from tests import nystrom_split_ref as S

pytestmark = pytest.mark.gpu
F64, BF16 = torch.float64, torch.bfloat16
N = 384
RANKS = [1, 127, 128, 129, 269, N - 33, N - 32, N - 31, N - 17, N - 16, N - 15, N - 1, N]   # (n - r around one and two GEMM stages of 16)
WDT = [pytest.param(BF16, id="bf16"), pytest.param(F64, id="f64")]


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def weights(d, wdt):
    return (torch.randn(d, N, generator=torch.Generator().manual_seed(900 + d), dtype=F64) * 0.05).to(wdt)


@functools.lru_cache(maxsize=None)
def case(r, d, wdt, shuffled, eps):
    """(C, idx, W, long-double reference, error of the fp64 reference formula): computed once, never modified."""
    C = S.statistic("well", N)
    idx = S.selection(N, r, seed=1000 + r, shuffled=shuffled)
    W = weights(d, wdt)
    ref = R.nystrom(C, idx.numpy(), W.double(), eps)
    if eps == 1e-6:
        from oracle import modegpt_oracle as O
        e_oracle = S.column_error(O.nystrom_down(C, W, idx), ref)
    else:
        e_oracle = S.column_error(S.full_form(C, idx, W, eps), ref)
    return C, idx, W, ref, e_oracle


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int64)


def same(a, b):
    return all(x.shape == y.shape and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def run(ops, dev, C, idx, W, eps):
    out = ops.nystrom_down(C.to(dev), idx.to(dev), W.to(dev), eps=eps, want_f64=True)
    torch.cuda.synchronize()
    return out


def check(ops, dev, r, d, wdt, shuffled, eps):
    C, idx, W, ref, e_oracle = case(r, d, wdt, shuffled, eps)
    out, f64 = run(ops, dev, C, idx, W, eps)
    assert out.shape == (d, r) and f64.shape == (r, d)
    assert bool(torch.isfinite(f64).all())
    assert torch.equal(bits(out), bits(f64.T.to(BF16)))
    e_gpu = S.column_error(f64, ref)
    print("SPLIT r=%d d=%d %s %s eps=%g: e_gpu %.3e e_oracle %.3e ratio %.3f of the bound" % (
        r, d, str(wdt)[6:], "shuffled" if shuffled else "sorted", eps, e_gpu, e_oracle, e_gpu / (4 * e_oracle + N * S.U)))
    assert e_gpu <= 4 * e_oracle + N * S.U


@pytest.mark.parametrize("wdt", WDT)
@pytest.mark.parametrize("d", [1, 130])
@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("r", RANKS)
def test_against_long_double(ops, dev, r, shuffled, d, wdt):
    check(ops, dev, r, d, wdt, shuffled, 1e-6)


@pytest.mark.parametrize("wdt", WDT)
@pytest.mark.parametrize("d", [1, 130])
@pytest.mark.parametrize("r", [1, 269, N - 31, N])
def test_large_ridge_on_a_unit_diagonal(ops, dev, r, d, wdt):
    assert float(S.statistic("well", N).diagonal().min()) == 1.0 == float(S.statistic("well", N).diagonal().max())
    check(ops, dev, r, d, wdt, False, 0.5)


@pytest.mark.parametrize("wdt", WDT)
@pytest.mark.parametrize("d", [1, 130])
def test_zero_ridge_full_rank_returns_the_weights(ops, dev, d, wdt):
    C, W = S.statistic("well", N), weights(d, wdt)
    out, f64 = run(ops, dev, C, torch.arange(N), W, 0.0)
    assert bool((f64.cpu() == W.double().T).all())                 # (==: the zero right-hand side's sign is free)
    assert torch.equal(bits(out), bits(W.to(BF16).to(dev)))


def direct(ops, dev, C, idx, W, eps, fill=0xFF):
    """The library call itself with a workspace of the test's own, every byte `fill` (0xFF: NaN in every type it holds)."""
    from modegpt_amd import _lib
    lib = _lib.load()
    n, r, d = C.shape[0], idx.numel(), W.shape[0]
    out = torch.empty(d, r, dtype=BF16, device=dev)
    f64 = torch.empty(r, d, dtype=F64, device=dev)
    nbytes = lib.mdg_nystrom_down_ws_bytes(n, r, d)
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    rc = lib.mdg_nystrom_down(C.data_ptr(), n, C.stride(0), idx.data_ptr(), r, W.data_ptr(), d, W.stride(0), ops._DT[W.dtype],
                              float(eps), out.data_ptr(), out.stride(0), f64.data_ptr(), ws.data_ptr(), nbytes,
                              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    return out, f64


@pytest.mark.parametrize("wdt", WDT)
@pytest.mark.parametrize("r", [N - 33, N - 31, 269, N - 1])         # n - r = 33, 31, 115, 1: every one is padded to a multiple of 16
def test_poisoned_workspace(ops, dev, r, wdt):
    C, idx, W, _, _ = case(r, 130, wdt, False, 1e-6)
    C, idx, W = C.to(dev), idx.to(dev), W.to(dev)
    want = ops.nystrom_down(C, idx, W, eps=1e-6, want_f64=True)
    got = direct(ops, dev, C, idx, W, 1e-6)
    assert bool(torch.isfinite(got[1]).all())
    assert same(got, want)


@pytest.mark.parametrize("wdt", WDT)
@pytest.mark.parametrize("d", [1, 130])
@pytest.mark.parametrize("r", [269, N - 31, N])
def test_leading_dimensions_inside_nan_buffers(ops, dev, r, d, wdt):
    """C with ldc > n and W_d with ld_wd > n as column slices of NaN-filled buffers (their data pointers off the 16-byte boundary)."""
    C, idx, W, _, _ = case(r, d, wdt, False, 1e-6)
    want = run(ops, dev, C, idx, W, 1e-6)
    cbuf = torch.full((N + 3, N + 37), float("nan"), dtype=F64, device=dev)
    wbuf = torch.full((d + 2, N + 11), float("nan"), dtype=wdt, device=dev)
    cview, wview = cbuf[:N, 5:5 + N], wbuf[:d, 3:3 + N]
    cview.copy_(C)
    wview.copy_(W)
    c_before, w_before = cbuf.clone(), wbuf.clone()
    got = ops.nystrom_down(cview, idx.to(dev), wview, eps=1e-6, want_f64=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got[1]).all())
    assert same(got, want)
    assert same((cbuf, wbuf), (c_before, w_before))


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("r", [1, 269, N - 31, N])
def test_overlapped_and_repeated_calls_are_bit_identical(ops, dev, monkeypatch, r, shuffled):
    C, idx, W, _, _ = case(r, 130, BF16, shuffled, 1e-6)
    res = {}
    for overlap in (False, True, False, True):
        monkeypatch.setattr(ops, "NYSTROM_OVERLAP", overlap)
        got = run(ops, dev, C, idx, W, 1e-6)
        if overlap in res:
            assert same(got, res[overlap])
        res[overlap] = got
    assert same(res[True], res[False])

