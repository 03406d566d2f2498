"""The sparse-list remainder kernel of the int8 covariance's exact route (cov_i8_exact.hip: i8_lo_product_kernel, lo_events, lo_first)
against EXACT integer arithmetic, bit for bit, on inputs built so that every list length at which the walk takes another path
occurs: 0, 1, 8, 9, 15, 16, 17, 32, 33 and 64 events in a list of their own (a batch is 16 slots, the last one 8 when no more are
left; a list's head is 64 entries), and two columns of one (group, residue) list with 40 + 41 events (entries fetched again beyond
the head).  Events sit on the first and the last token, in both 2048-token segments (2048 + 33 tokens: the second ragged), in the
first and last column of a tile and of a 32-column group and in all four residues mod 4; several columns have their event on the
SAME token, so the second pass meets partner elements with digits below plane 2 and recomputes x_d; one column leaves for the
fp64 column kernel.  256 and 384 features (3 and 6 lower tiles) and one per-head statistic of 2 x 128.

Why bit for bit: the values lie on a lattice on which no fp64 sum can round (as tests/cov_ref.py's do) -- bulk m 2^k with |m| <= 3,
k in {-1, 0}, one 32 per column that fixes its exponent, events m 2^-17 / m 2^-18 with m odd, |m| <= 7: every addend of
sigma_ij, of whatever part of the decomposition, is a multiple of u_i u_j (u_i: the lowest set bit of column i) and every partial
sum is below 2^53 u_i u_j (test_lattice_keeps_every_partial_sum_exact checks that on the CPU, from the digits of
tests/i8_model.py).  The reference is the integer sum of products of tests/i8_model.digits' N -- not the code under test, and not
an fp64 product either (which agrees, on this lattice, and is asserted to)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import i8_model as M

F64 = torch.float64
T = 2048 + 33
TOP_TOKEN = 1000
OUT_COL = 77                      # bulk 11 binades under three massive elements: the route hands it to the fp64 column kernel
# The route's tolerance factor of these calls.  At 1 the greedy also takes the columns with the longest lists out (for the bound of
# the truncated product, which the exact route then does not run) and the lists this file is about would be cleared; between 8 and
# 64 only OUT_COL leaves.  The factor is an argument of the call and moves thresholds of the route alone, no arithmetic.
TOLERANCE = 16.0
# column -> events.  (group, residue) = (col // 32, col % 4); no two of these share a list except 161 / 165
EVENTS = {0: 1, 31: 15, 32: 16, 33: 17, 66: 32, 127: 33, 128: 64, 130: 9, 161: 40, 165: 41, 255: 8, 256: 17, 300: 33, 383: 16}
FIRST_TOKEN = (0, 127, 128, 256)            # columns with an event on token 0 ...
LAST_TOKEN = (31, 127, 165, 383)            # ... and on the last one


@functools.lru_cache(maxsize=None)
def inputs(n):
    """-> (X bf16 [T, n], exact sigma fp64 [n, n] both triangles, lattice margin = max_ij B_ij / (2^53 u_i u_j))"""
    rng = np.random.default_rng([n, T])
    x = rng.integers(-3, 4, size=(T, n)).astype(np.float64) * np.exp2(rng.integers(-1, 1, size=(T, n)).astype(np.float64))
    x[TOP_TOKEN, :] = 32.0
    shared = rng.choice(np.arange(1, 2048), size=6, replace=False)        # tokens several columns have an event on
    for col, count in EVENTS.items():
        if col >= n:
            continue
        fixed = ([0] if col in FIRST_TOKEN else []) + ([T - 1] if col in LAST_TOKEN else [])
        fixed += [int(t) for t in shared[:max(0, min(3, count - len(fixed) - 1))]]
        free = np.setdiff1d(np.arange(1, T - 1), np.concatenate([shared, [TOP_TOKEN]]))
        second = free[free >= 2048]
        rest = count - len(fixed)
        late = [int(t) for t in rng.choice(second, size=min(rest, 3 if count > 8 else 0), replace=False)]
        early = [int(t) for t in rng.choice(free[free < 2048], size=rest - len(late), replace=False)]
        tokens = fixed + late + early
        assert len(set(tokens)) == count
        m = rng.choice([-7, -5, -3, -1, 1, 3, 5, 7], size=count).astype(np.float64)
        x[tokens, col] = m * np.exp2(rng.choice([-17.0, -18.0], size=count))
    x[:, OUT_COL] *= 2.0 ** -11
    x[[TOP_TOKEN, 5, 1500], OUT_COL] = [32.0, -28.0, 24.0]
    X = torch.from_numpy(x).to(torch.bfloat16)
    assert torch.equal(X.double(), torch.from_numpy(x))
    d, E, N, rounded, _ = M.digits(X)
    assert int(rounded.sum()) == 0
    deep = (d[3] != 0) | (d[4] != 0) | (d[5] != 0)
    counts = deep.sum(0)
    for col in range(n):      # the lists are what the plan says (the leaving column's are cleared by the route)
        assert counts[col] == EVENTS.get(col, 0) or col == OUT_COL, (col, counts[col])
    # exact sigma: N = hi 2^24 + lo, three int64 products that cannot overflow, recombined as Python integers
    hi, lo = N >> 24, N & 0xFFFFFF
    assert np.abs(hi).max() < 2 ** 24 and T < 4096
    hh, hl, ll = hi.T @ hi, hi.T @ lo, lo.T @ lo
    V = (hh.astype(object) << 48) + ((hl + hl.T).astype(object) << 24) + ll.astype(object)
    ex = (E[:, None] + E[None, :] - 344).astype(object)
    ref = np.empty((n, n))
    for i in range(n):
        for j in range(n):
            f = float(V[i, j])
            assert int(f) == V[i, j], (i, j)                     # the sum itself is an fp64 value
            ref[i, j] = math.ldexp(f, int(ex[i, j]))
    # every partial sum of every part: |addend| <= A_ti A_tj with A = sum_s |d_s| 2^(8 (5 - s)), all multiples of u_i u_j
    A = sum(np.abs(d[s]).astype(np.float64) * 2.0 ** (8 * (5 - s)) for s in range(6))
    low = np.where(N != 0, N & -N, 1 << 62).min(axis=0).astype(np.float64)
    margin = float(((A.T @ A) / (low[:, None] * low[None, :])).max() / 2.0 ** 53)
    return X, torch.from_numpy(ref), margin


@pytest.mark.parametrize("n", [256, 384])
def test_lattice_keeps_every_partial_sum_exact(n):
    """CPU: on these inputs no fp64 addition of any part of the exact route can round (all partial sums are multiples of u_i u_j
    below 2^53 u_i u_j), the exact integer sigma is an fp64 matrix, a plain fp64 product gives the same bits, and the host model
    sends the statistic where the GPU tests need it: the exact route, one column to the fp64 column kernel."""
    X, ref, margin = inputs(n)
    assert margin < 0.5, margin
    assert torch.equal(X.double().T @ X.double(), ref)
    want = M.route_of(X, tolerance=TOLERANCE, offer_exact=True)
    assert want["planes"] in (5, 6) and want["columns"] == [OUT_COL] and want["exact"], {k: want[k] for k in ("planes", "columns", "exact")}


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


@pytest.fixture
def exact_route(ops, monkeypatch):
    """The exact route forced (MDG_I8_EXACT_ALWAYS), as the i8_route fixtures of the other int8 tests do."""
    monkeypatch.setattr(ops, "I8_EXACT", True)


def lower(S):
    return torch.tril(S.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [256, 384])
def test_sparse_lists_against_exact_integer_arithmetic(ops, dev, n, exact_route, monkeypatch):
    """sigma's lower triangle equals the exact integer result bit for bit; a second call on a fresh buffer gives the same bits,
    and so does one whose workspace was handed over filled with NaN patterns."""
    X, ref, _ = inputs(n)
    Xd = X.to(dev)
    S = torch.zeros(n, n, dtype=F64, device=dev)
    info = {}
    assert ops.cov_accum_i8(S, Xd, route_info=info, tolerance=TOLERANCE) in (5, 6)
    assert info["exact"] and info["remainder"] == "tiles" and info["columns"] == [OUT_COL], info
    got = lower(S)
    assert torch.equal(got, torch.tril(ref)), (got - torch.tril(ref)).abs().max().item()
    S2 = torch.zeros_like(S)
    ops.cov_accum_i8(S2, Xd, tolerance=TOLERANCE)
    assert torch.equal(S2, S), "events added in list order by one wave each: bit-identical from run to run"
    real_ws = ops._ws

    def poisoned(nbytes, device):
        t, p = real_ws(nbytes, device)
        if t is not None:
            t.fill_(0xFF)
        return t, p
    monkeypatch.setattr(ops, "_ws", poisoned)
    S3 = torch.zeros_like(S)
    ops.cov_accum_i8(S3, Xd, tolerance=TOLERANCE)
    assert torch.equal(S3, S)
    ops.cov_accum_i8(S3, Xd, tolerance=TOLERANCE)                                   # accumulates: sigma is read, added to and written once
    assert torch.equal(lower(S3), 2.0 * torch.tril(ref))


@pytest.mark.gpu
def test_sparse_lists_of_a_per_head_statistic(ops, dev, exact_route):
    """Two heads of 128: only the heads' own diagonal tiles exist, each with its lists of the 256-column plan."""
    X, ref, _ = inputs(256)
    S = torch.zeros(2, 128, 128, dtype=F64, device=dev)
    infos = []
    assert ops.cov_accum_i8_multi([(S, X.to(dev), 2)], report=True, route_info=infos, tolerance=TOLERANCE) in (5, 6)
    assert infos[0]["exact"] and infos[0]["remainder"] == "tiles" and infos[0]["columns"] == [OUT_COL], infos
    for h in range(2):
        want = torch.tril(ref[128 * h:128 * h + 128, 128 * h:128 * h + 128])
        assert torch.equal(lower(S[h]), want), h


@pytest.mark.gpu
def test_sparse_lists_leave_the_rest_of_a_padded_buffer_alone(ops, dev):
    """sigma inside a larger buffer (row pitch n + 8, four rows more): what lies above the diagonal, beside the matrix and
    in the rows beyond it is not written -- the fold's loads are not conditional, its stores are."""
    from modegpt_amd import _lib
    n, pitch, rows = 256, 256 + 8, 256 + 4
    X, ref, _ = inputs(n)
    Xd = X.to(dev)
    SENTINEL = -7.25
    buf = torch.full((rows, pitch), SENTINEL, dtype=F64, device=dev)
    keep = torch.ones(rows, pitch, dtype=torch.bool)
    keep[:n, :n] = ~torch.tril(torch.ones(n, n, dtype=torch.bool))
    buf[~keep.to(dev)] = 0.0
    lib = _lib.load()
    ws = torch.empty(lib.mdg_cov_accum_i8_ws_bytes(T, n), dtype=torch.uint8, device=dev)
    used = C.c_int(0)
    with torch.cuda.device(dev):
        _lib.check(lib.mdg_cov_accum_i8(Xd.data_ptr(), T, n, Xd.stride(0), buf.data_ptr(), pitch, ws.data_ptr(), ws.numel(), TOLERANCE,
                                        _lib.MDG_I8_EXACT_ALWAYS, C.byref(used), None, None, None,
                                        torch.cuda.current_stream(dev).cuda_stream), "mdg_cov_accum_i8")
    torch.cuda.synchronize(dev)
    assert used.value in (5, 6)
    got = buf.cpu()
    assert torch.equal(torch.tril(got[:n, :n]), torch.tril(ref))
    assert bool((got[keep] == SENTINEL).all())
