"""Entry points that address a large caller buffer, driven across the 4 GiB byte-offset edge.

The vector staging path of mdg_gemm_f64 loads at (uniform stage base + 32-bit per-lane byte offset).  Every case here puts the
data that matter on both sides of byte 2^32 of a buffer a little larger than that, with operands whose result is exact (small
integers) or a reference that does not share the kernel's addressing: a row read from the wrong place fails the equality.
Each case frees its buffers before the next (peak device memory about 28 GB, in the covariance case).
"""
import gc
import math

import pytest
import torch

from tests.i8_limits import check_i8_error
from tests.test_gpu_i8_fullwidth import spot_and_trace

pytestmark = pytest.mark.gpu
F64, BF16 = torch.float64, torch.bfloat16
K = 512


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def free_after(dev):
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def edge_rows(gen, edge, n_rows, M):
    """M gathered rows: most within 2000 rows of the 4 GiB row `edge` on both sides, a few from the start and the end of A."""
    near = edge - 1000 + torch.randperm(2000, generator=gen)[:M - 8]
    far = torch.cat([torch.randint(0, 64, (4,), generator=gen), n_rows - 1 - torch.randint(0, 64, (4,), generator=gen)])
    return torch.cat([near, far])


def ints_(t, gen_seed):
    """Fill a device tensor in place with integers in [-8, 8] (exact in bf16), in row slabs (no full-size temporaries)."""
    g = torch.Generator(device=t.device).manual_seed(gen_seed)
    flat = t.view(t.shape[0], -1)
    for r0 in range(0, flat.shape[0], 1 << 18):
        sl = flat[r0:r0 + (1 << 18)]
        sl.copy_(torch.randint(-8, 9, sl.shape, device=t.device, generator=g, dtype=torch.int8))


@pytest.mark.parametrize("adt", [F64, BF16], ids=["a_f64", "a_bf16"])
def test_gathered_rows_beyond_4gib(ops, dev, adt):
    """C = A[rows] B^T with A of ~4.5 GB: rows on both sides of the 4 GiB row (1 048 576 for fp64, 4 194 304 for bf16), sorted
    (the Nystrom cross term's case, vector staging path) and unsorted (spans beyond 4 GiB inside one tile), ragged M = 300."""
    es = 8 if adt == F64 else 2
    edge = (1 << 32) // (K * es)
    n_rows = edge + edge // 16                                          # ~4.5 GB either way
    A = torch.empty(n_rows, K, dtype=adt, device=dev)
    ints_(A, 1)
    gen = torch.Generator().manual_seed(2)
    M, N = 300, 200
    Bt = torch.randint(-8, 9, (N, K), generator=gen).to(BF16)
    Bd = Bt.to(dev)
    rows = edge_rows(gen, edge, n_rows, M)
    for name, r in [("sorted", rows.sort().values), ("unsorted", rows[torch.randperm(M, generator=gen)])]:
        assert int((r >= edge).sum()) > 100 and int((r < edge).sum()) > 100
        rd = r.to(dev)
        want = A[rd].double().cpu() @ Bt.double().T                     # (torch's own gather: 64-bit indexing)
        out = torch.full((M, N), float("nan"), dtype=F64, device=dev)
        ops.gemm(A, Bd, out, trans_b=True, a_rows=rd)
        got = out.cpu()
        bad = (got != want).any(1).nonzero().flatten()
        assert bad.numel() == 0, (f"{name}: {bad.numel()} of {M} gathered rows wrong; their A rows: "
                                  f"{r[bad[:8]].tolist()} (4 GiB row: {edge})")


def test_huge_leading_dimension_falls_back_to_elementwise(ops, dev):
    """No gather: an A view whose 128 tile rows span TILE * ld * 8 >= 2^32 bytes (ld = 4 194 304 + 16 doubles, M = 130, ~4.4 GB)
    must leave the vector path (host-side span check) and stay exact -- tile row 1 starts 4 GiB in."""
    ld = (1 << 22) + 16
    M, N = 130, 200
    buf = torch.empty(M, ld, dtype=F64, device=dev)
    A = buf[:, :K]
    gen = torch.Generator().manual_seed(4)
    Ah = torch.randint(-8, 9, (M, K), generator=gen).to(F64)
    A.copy_(Ah.to(dev))
    B = torch.randint(-8, 9, (K, N), generator=gen).to(F64)
    out = torch.full((M, N), float("nan"), dtype=F64, device=dev)
    ops.gemm(A, B.to(dev), out, alpha=-2.0)
    assert torch.equal(out.cpu(), -2.0 * (Ah @ B))


def test_nystrom_refit_past_the_edge(ops, dev):
    """mdg_nystrom_down at n = 24 576 (rows of the fp64 statistic from 21 846 on start 4 GiB or more past its base),
    r = 0.7 n, d = 4096, with a well-conditioned SPD C = G G^T / m + I: the refit solves (C_kk + eps I) W' = C[idx,:] W_d^T."""
    n, d, m = 24576, 4096, 4096
    r = int(0.7 * n)
    g = torch.Generator(device=dev).manual_seed(6)
    G = torch.randn(n, m, device=dev, dtype=F64, generator=g)
    Cm = G @ G.T
    del G
    Cm.div_(m)
    Cm.diagonal().add_(1.0)
    idx = torch.randperm(n, device=dev, generator=g)[:r].sort().values
    assert int(idx[-1]) * n * 8 >= 1 << 32
    Wd = (torch.randn(d, n, device=dev, generator=g) * 0.02).to(BF16)
    down, down64 = ops.nystrom_down(Cm, idx, Wd, want_f64=True)
    rhs = Cm[idx] @ Wd.double().T
    Ckk = Cm[idx][:, idx]
    del Cm
    Ckk.diagonal().add_(1e-6)
    res = ((Ckk @ down64 - rhs).abs().max() / rhs.abs().max()).item()
    assert res < 1e-9, f"(C_kk + eps I) W' - C[idx,:] W_d^T: {res:.3g} of max |rhs|"
    assert torch.equal(down, down64.T.to(BF16))


def test_covariance_of_a_batch_beyond_4gib(ops, dev, monkeypatch):
    """sigma += X^T X for X bf16 [263 144, 8192] (4.31 GB, rows beyond 4 GiB from the base) through the fp64 kernel, the int8
    route (which must not offer its exact route here: its event lists address rows with 32-bit byte offsets) and the hook's
    cov_accum_multi, each against torch fp64 products of column blocks over all tokens, plus the trace."""
    n, T = 8192, 263144
    assert T * n * 2 >= 1 << 32
    g = torch.Generator(device=dev).manual_seed(8)
    c = torch.exp(torch.empty(n, device=dev).uniform_(math.log(0.05), math.log(2.0), generator=g))
    X = torch.empty(T, n, dtype=BF16, device=dev)
    for r0 in range(0, T, 1 << 15):
        sl = X[r0:r0 + (1 << 15)]
        sl.copy_(torch.randn(sl.shape, device=dev, generator=g) * c)
    S = torch.zeros(n, n, dtype=F64, device=dev)
    ops.cov_accum(S, X)
    spot, trace = spot_and_trace(S, X, 5)
    # (a token read from the wrong row moves an entry by ~1 / T = 4e-6 of the normalisation; 1e-12 leaves both fp64 sums of
    # 263 144 terms their rounding)
    assert spot < 1e-12 and trace < 1e-12, ("fp64 kernel", spot, trace)

    monkeypatch.setattr(ops, "I8_EXACT", True)                          # the exact route wherever it is offered ...
    S.zero_()
    info = {}
    assert ops.cov_accum_i8(S, X, route_info=info) in (5, 6)
    assert info["exact"] is False, info                                 # ... and here it is not
    spot, trace = spot_and_trace(S, X, 5)
    check_i8_error(spot, info["bound"], ctx="int8 route, 4.31 GB batch")
    assert trace < 1e-12, ("int8 route", trace)

    for mode in ("i8", "f64"):
        S.zero_()
        ops.cov_accum_multi([(S, X, 1)], mode=mode)
        spot, trace = spot_and_trace(S, X, 5)
        if mode == "i8":
            check_i8_error(spot, None, ctx="cov_accum_multi i8")
        else:
            assert spot < 1e-12, ("cov_accum_multi f64", spot)
        assert trace < 1e-12, (mode, trace)


def _cache_views_past_the_edge(p, v_probe, dev):
    """k, v [2, n_kv, S, r] as views of torch.empty buffers a little over 2^31 elements each: batch 1 starts beyond byte 2^32.
    Only the viewed rows are written."""
    views = []
    for t in (p.k, v_probe):
        Bt, KV, S, r = t.shape
        batch_stride = (1 << 31) + 64
        buf = torch.empty(batch_stride + KV * S * r, dtype=t.dtype, device=dev)
        view = buf.as_strided((Bt, KV, S, r), (batch_stride, S * r, r, 1))
        assert view.stride(0) * t.element_size() > 1 << 32 and buf.numel() > 1 << 31
        view.copy_(t.to(dev))
        views.append(view)
    return views


@pytest.mark.parametrize("kernel, T, S, splits", [("fwd", 33, 33, None), ("decode", 1, 130, 3)], ids=["fwd", "decode"])
def test_attention_cache_views_past_2_31_elements(ops, dev, kernel, T, S, splits):
    """mdg_attn_fwd and mdg_attn_decode on k and v whose batch stride puts batch 1 more than 4 GiB from the base, with the weight
    probe of tests/attn_ref.py (widths 90 / 77, bf16): every key's softmax weight is exact, so a row of batch 1 read through a
    32-bit offset -- batch 0's rows, or unwritten memory -- fails bit equality on w(b, g) alone."""
    from tests import attn_ref as R
    width = (90, 77, 8, 2)
    p = R.probe_case("bf16", width, T, S)
    q = p.q.to(dev)
    for ad in list(R.probe_admissions(T, S, width[2]))[:2]:              # unmasked: causal, full
        lo, hi, _ = R.probe_expected(p, "bf16", ad.adm, width)
        outs = []
        for j0 in p.windows:
            k, v = _cache_views_past_the_edge(p, R.probe_values(p, "bf16", j0), dev)
            if kernel == "fwd":
                outs.append(ops.attn_fwd(q, k, v, p.scale, causal=ad.causal))
            else:
                outs.append(ops.attn_decode(q, k, v, p.scale, causal=ad.causal, splits=splits))
            torch.cuda.synchronize()
            del k, v
        got = torch.cat(outs, dim=3).contiguous().view(torch.int16).cpu()
        ok = (got == lo) | (got == hi)
        if not bool(ok.all()):
            b, i, h, key = (~ok).nonzero()[0].tolist()
            raise AssertionError(f"{kernel} causal={ad.causal}: weight of key {key} for (b, i, h) = ({b}, {i}, {h}) has bits "
                                 f"{int(got[b, i, h, key]):#06x}, want {int(lo[b, i, h, key]):#06x}; {int((~ok).sum())} entries differ")
