"""No entry writes behind the workspace its size query asks for.

ops._ws, the one place the wrappers allocate workspaces, is replaced by a version that allocates the requested bytes plus a tail
guard -- as long as the workspace and at least 64 KiB, filled with one byte -- and hands on the same base pointer and byte count.
After the call and a synchronisation every guard must still hold the fill byte everywhere, and the call's outputs must be bit-equal
to the same call made without the guard.  One case per workspace layout, at the smallest shapes that reach every block of it (a
ragged 128-block, an odd rank, n - r no multiple of 16, more than one round, both routes of sqrt_psd_large, rank 0 and hd, both
statistics of the sequence kernels).  A property of the library, not of how its layouts are written down.
"""
import pytest
import torch

from tests import qk_pair_model as QK
from tests import vo_error_model as VO
from tests.test_gpu_chol import matrix
from tests.test_gpu_rank_curve import weight

pytestmark = pytest.mark.gpu
F64 = torch.float64
BF16 = torch.bfloat16
FILL = 0xA5
MIN_GUARD = 64 * 1024


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def same(a, b):
    """Bit equality of two results: tensors, None, or tuples of them."""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def selection(n, r, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:r].sort().values


def mlp_case(dev, n, d):
    return matrix("p3", n)[0].to(dev), weight(n, d, BF16).to(dev)


# ---------------------------------------------------------------- the cases: operands first, then the call to repeat
def ridge_scores(ops, dev):
    C = matrix("p3", 130)[0].to(dev)
    return lambda: ops.ridge_scores(C, 1e-4, want_sens=True)


def potrs_lower(ops, dev):
    L = matrix("p3", 130)[2].to(dev).clone()
    inv = ops.potrf_lower(L)
    B = torch.randn(130, 3, generator=torch.Generator().manual_seed(3), dtype=F64).to(dev)

    def call():
        X = B.clone()
        ops.potrs_lower(L, inv, X)
        return X
    return call


def nystrom_down(n, r, d):
    def case(ops, dev):
        C, W = mlp_case(dev, n, d)
        idx = selection(n, r, 11).to(dev)
        return lambda: ops.nystrom_down(C, idx, W, want_f64=True)
    return case


def nystrom_rank_curve(ops, dev):
    C, W = mlp_case(dev, 150, 40)
    order = torch.arange(149, -1, -1, device=dev)
    return lambda: ops.nystrom_rank_curve(C, order, W)


def nystrom_greedy_select(r, rounds):
    def case(ops, dev):
        C, W = mlp_case(dev, 150, 40)
        return lambda: ops.nystrom_greedy_select(C, W, r, rounds)
    return case


def sqrt_psd_large(want_evals):
    def case(ops, dev):
        M = matrix("p3", 130)[0].to(dev)
        return lambda: ops.sqrt_psd_large(M, 1e-6, False, True, want_evals=want_evals)     # (eigenvalues: block Jacobi; none: Newton-Schulz)
    return case


def sqrt_psd_small(ops, dev):
    M = torch.stack([matrix(kind, 6)[0] for kind in ("p3", "p8", "p6g3")]).to(dev)
    return lambda: ops.sqrt_psd_small(M, 1e-6, False, True)


def mlp_output_error(r):
    def case(ops, dev):
        C, W = mlp_case(dev, 150, 40)
        idx = selection(150, r, 12).to(dev) if r else None
        down = ops.nystrom_down(C, idx, W) if r else None
        return lambda: ops.mlp_output_error(C, W, idx, down, want_unorm2=True)
    return case


def col_sum_accum(ops, dev):
    x = torch.randn(129, 150, generator=torch.Generator().manual_seed(5)).to(BF16).to(dev)

    def call():
        s = torch.zeros(150, dtype=F64, device=dev)
        ops.col_sum_accum(s, x)
        return s
    return call


def nystrom_intercept(ops, dev):
    C, W = mlp_case(dev, 150, 40)
    idx = selection(150, 37, 13).to(dev)
    down = ops.nystrom_down(C, idx, W)
    mu = torch.randn(150, generator=torch.Generator().manual_seed(6), dtype=F64).to(dev)
    return lambda: ops.nystrom_intercept(W, down, idx, mu)


def vo_problem(dev, n_heads, n_kv):
    Wv, Wo = VO.weights(48, n_heads, n_kv, 8, BF16, seed=2)
    return matrix("p3", 48)[0].to(dev), Wv.to(dev), Wo.to(dev)


def vo_intercept(rank):
    def case(ops, dev):
        C, Wv, Wo = vo_problem(dev, 4, 2)
        v, o = ops.vo_compress(C, Wv, Wo, 4, 2, 8, rank, 1e-5) if rank else (None, None)
        mu = torch.randn(48, generator=torch.Generator().manual_seed(7), dtype=F64).to(dev)
        return lambda: ops.vo_intercept(Wv, Wo, v, o, mu, 4, 2, 8, rank)
    return case


def vo_family(n_heads, n_kv, with_b_o):
    """vo_compress with the spectrum, the V/O rank curve and vo_bias behind it on the same workspace, then vo_output_error."""
    def case(ops, dev):
        C, Wv, Wo = vo_problem(dev, n_heads, n_kv)
        gen = torch.Generator().manual_seed(8)
        b_v = torch.randn(n_kv * 8, generator=gen).to(BF16).to(dev)
        b_o = torch.randn(48, generator=gen).to(BF16).to(dev) if with_b_o else None

        def call():
            out = ops.vo_compress(C, Wv, Wo, n_heads, n_kv, 8, 3, 1e-5, want_f64=True, want_spectrum=True, want_curve=True, bias=(b_v, b_o))
            return out, ops.vo_output_error(C, Wv, Wo, n_heads, n_kv, 8, 3, out[0], out[1], want_dnorm2=True)
        return call
    return case


def qk_seq(which, raw):
    def case(ops, dev):
        B, T, H, KV, hd = 2, 17, 4, 2, 8
        q = QK.generic_rows(B, T, H, hd, 21, BF16).to(dev)
        k = QK.generic_rows(B, T, KV, hd, 22, BF16, mean_sigmas=20.0).to(dev)

        def call():
            pair = torch.zeros(H, hd, hd, dtype=F64, device=dev)
            pair_raw = torch.zeros(H, hd, hd, dtype=F64, device=dev) if raw else None
            getattr(ops, which)(pair, pair_raw, q, k, B, T, H, KV, hd)
            return pair, pair_raw
        return call
    return case


CASES = {
    "ridge_scores": ridge_scores,
    "potrs_lower": potrs_lower,
    "nystrom_down-150-37-40": nystrom_down(150, 37, 40),
    "nystrom_down-48-48-40": nystrom_down(48, 48, 40),
    "nystrom_rank_curve": nystrom_rank_curve,
    "nystrom_greedy_select-37-1": nystrom_greedy_select(37, 1),
    "nystrom_greedy_select-37-3": nystrom_greedy_select(37, 3),
    "nystrom_greedy_select-2-5": nystrom_greedy_select(2, 5),
    "nystrom_greedy_select-0-1": nystrom_greedy_select(0, 1),
    "sqrt_psd_large-jacobi": sqrt_psd_large(True),
    "sqrt_psd_large-newton": sqrt_psd_large(False),
    "sqrt_psd_small": sqrt_psd_small,
    "mlp_output_error-37": mlp_output_error(37),
    "mlp_output_error-0": mlp_output_error(0),
    "col_sum_accum": col_sum_accum,
    "nystrom_intercept": nystrom_intercept,
    "vo_intercept-3": vo_intercept(3),
    "vo_intercept-0": vo_intercept(0),
    "vo_family-4-2": vo_family(4, 2, True),
    "vo_family-2-2": vo_family(2, 2, False),
    "qk_pair_accum-raw": qk_seq("qk_pair_accum", True),
    "qk_pair_accum": qk_seq("qk_pair_accum", False),
    "qk_causal_accum-raw": qk_seq("qk_causal_accum", True),
    "qk_causal_accum": qk_seq("qk_causal_accum", False),
}
OVERLAPS = {name: (True, False) if name.startswith("nystrom_down") else (None,) for name in CASES}


@pytest.mark.parametrize("name,overlap", [(name, o) for name in CASES for o in OVERLAPS[name]])
def test_nothing_is_written_behind_the_workspace(ops, dev, monkeypatch, name, overlap):
    if overlap is not None:
        monkeypatch.setattr(ops, "NYSTROM_OVERLAP", overlap)
    call = CASES[name](ops, dev)
    plain = call()
    torch.cuda.synchronize()

    allocated = []

    def guarded_ws(nbytes, device):
        if nbytes == 0:
            return None, 0
        whole = torch.empty(nbytes + max(nbytes, MIN_GUARD), dtype=torch.uint8, device=device)
        whole[nbytes:].fill_(FILL)
        allocated.append((whole, nbytes))
        ws = whole[:nbytes]                      # the same base pointer, the same byte count
        return ws, ws.data_ptr()

    monkeypatch.setattr(ops, "_ws", guarded_ws)
    got = call()
    torch.cuda.synchronize()
    assert allocated, "the call allocated no workspace through ops._ws"
    for whole, nbytes in allocated:
        tail = whole[nbytes:]
        wrong = int((tail != FILL).sum())
        first = int((tail != FILL).nonzero()[0]) if wrong else -1
        assert not wrong, f"{name}: {wrong} guard bytes behind a workspace of {nbytes} bytes were overwritten, the first at +{first}"
    assert same(plain, got), f"{name}: the outputs differ from the call without the guard"
