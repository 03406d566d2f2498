"""GPU: mdg_vo_intercept (the intercept of the mean-aware V/O truncation) through the raw C ABI against the long double model of
tests/vo_mean_model.py.  The factors v^ / o^ are arbitrary tensors here (the kernel serves factors from anywhere); the chain through
mdg_vo_compress is tests/test_gpu_vo_intercept_chain.py.

A priori bounds (u = 2^-53):
  delta_i     within (d + n_heads (hd + rank) + 8) u A_i,  A_i = sum_h |W_o,h[i, :]| (|W_v,g| |mu| + |b_v,g|) + |o^_h[i, :]| (|v^_g| |mu|)
  bias_f64    = b_o + delta, one fp64 addition of the delta the same call without b_o returns: the same bits
  bias_out    = bias_f64 rounded once the way torch's .to() rounds: the same bits
  norms       within (d + 8) u of the long double sums of squares of the rows the device itself produced (delta; the constant is
              what the call at rank 0 returns as delta)
Every operand sits in a NaN-filled buffer (a read beyond a row's width would poison the sums), every output between NaN guards.
Shapes (n_heads, n_kv, hd, rank, d): the prescribed ones -- grouped, MHA, rank 0, rank == hd, d past one 2048-column stage, a long
concatenated row -- and three of this file's own for forks the kernel has that those do not reach: a query-side row of n_heads hd =
2560 columns (two LDS chunks of the row stage), widths that are no multiple of 8 under an aligned leading dimension (the scalar tail
behind the 16-byte loads), and row counts that do not fill the last workgroup."""
import functools

import numpy as np
import pytest
import torch

from tests import vo_mean_model as V

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
GUARD = 16
SHAPES = [(4, 2, 32, 22, 64), (4, 4, 32, 22, 64), (2, 1, 8, 0, 24), (2, 1, 8, 8, 24), (8, 2, 128, 88, 2056), (4, 1, 128, 126, 4104),
          (20, 4, 128, 2, 16), (3, 3, 6, 5, 20), (6, 2, 10, 7, 37)]
# (w_dtype, new_dtype, biases, layout, bias dtype, out dtype); layout: tight | padded (ld = width rounded up to 8, + 8: aligned rows, a
# scalar tail where the width is no multiple of 8) | offset (operands one element off a 16-byte boundary, ld = width + 3)
VARIANTS = [("bf16", "bf16", True, "tight", torch.bfloat16, torch.bfloat16),
            ("bf16", "f64", False, "tight", None, torch.float32),
            ("f64", "bf16", True, "padded", torch.float64, torch.float64),
            ("f64", "f64", False, "padded", None, torch.bfloat16),
            ("bf16", "bf16", False, "padded", None, torch.float16),
            ("bf16", "bf16", True, "offset", torch.float32, torch.bfloat16),
            ("bf16", "f64", True, "offset", torch.float16, torch.float16)]
CASES = [(s, v) for s in SHAPES for v in range(len(VARIANTS))]


def _ids(c):
    s, v = c
    w, n, b, lay, _, _ = VARIANTS[v]
    return f"h{s[0]}kv{s[1]}hd{s[2]}r{s[3]}d{s[4]}-{w}-{n}-{'b' if b else 'nob'}-{lay}"


def _place(a, tdt, layout, dev):
    """The host matrix a [rows, width] inside a NaN-filled device buffer; returns (buffer, view, ld)."""
    rows, width = a.shape
    if layout == "tight":
        ld, off = width, 0
    elif layout == "padded":
        ld, off = (width + 7) // 8 * 8 + 8, 0
    else:
        ld, off = width + 3, 1
    # (16-byte aligned storage: torch's allocator aligns to 512 bytes; the offset variant moves the first element off the boundary)
    buf = torch.full((off + rows * ld + GUARD,), float("nan"), dtype=tdt, device=dev)
    view = buf[off:off + rows * ld].view(rows, ld)[:, :width]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(tdt))
    return buf, view, ld


def _guarded(n, tdt, dev):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=tdt, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    host = buf.cpu()
    return bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[GUARD + n:]).all())


def _code(tdt):
    from modegpt_amd import _lib
    return {torch.bfloat16: _lib.MDG_BF16, torch.float16: _lib.MDG_F16, torch.float32: _lib.MDG_F32, torch.float64: _lib.MDG_F64}[tdt]


def _call(dev, ops_, shape, rank, mu, b_v, b_o, b_tdt, out_tdt, want_out=True):
    """One mdg_vo_intercept call on placed operands.  Returns host tensors (bias_out, bias_f64, norms)."""
    from modegpt_amd import _lib
    lib = _lib.load()
    n_heads, n_kv, hd, _, d = shape
    (Wv, ld_wv), (Wo, ld_wo), (Vn, ld_v), (On, ld_o), wdt, ndt = ops_
    nbytes = lib.mdg_vo_intercept_ws_bytes(d, n_kv, hd, rank)
    assert nbytes == 8 * (n_kv * (hd + rank) + 2 * d)
    ws_buf, ws = _guarded(nbytes // 8, torch.float64, dev)
    bo_buf, bo = _guarded(d, out_tdt, dev)
    bf_buf, bf = _guarded(d, torch.float64, dev)
    nm_buf, nm = _guarded(2, torch.float64, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(lib.mdg_vo_intercept(Wv.data_ptr(), ld_wv, Wo.data_ptr(), ld_wo, _code(wdt), Vn.data_ptr() if rank else None, ld_v,
                                        On.data_ptr() if rank else None, ld_o, _code(ndt), d, n_heads, n_kv, hd, rank, mu.data_ptr(),
                                        None if b_v is None else b_v.data_ptr(), None if b_o is None else b_o.data_ptr(),
                                        _code(b_tdt) if b_tdt is not None else 0, bo.data_ptr() if want_out else None, _code(out_tdt),
                                        bf.data_ptr(), nm.data_ptr(), ws.data_ptr(), nbytes, st), "mdg_vo_intercept")
    torch.cuda.synchronize(dev)
    assert _guards_intact(ws_buf, nbytes // 8) and _guards_intact(bo_buf, d) and _guards_intact(bf_buf, d) and _guards_intact(nm_buf, 2)
    return bo.cpu().clone(), bf.cpu().clone(), nm.cpu().clone()


def _values(shape, wdt, ndt, seed):
    """Host fp64 arrays: bf16-valued where the operand is bf16, full fp64 values otherwise; mu with a mean of several spreads."""
    n_heads, n_kv, hd, rank, d = shape
    rng = np.random.default_rng(seed)
    rnd = lambda a, t: V.bf16_round(a) if t == "bf16" else a                            # noqa: E731
    w = {"W_v": rnd(rng.standard_normal((n_kv * hd, d)) / np.sqrt(d), wdt),
         "W_o": rnd(rng.standard_normal((d, n_heads * hd)) / np.sqrt(n_heads * hd), wdt),
         "v_hat": rnd(rng.standard_normal((n_kv * max(rank, 1), d)) / np.sqrt(d), ndt),
         "o_hat": rnd(rng.standard_normal((d, n_heads * max(rank, 1))) / np.sqrt(n_heads * max(rank, 1)), ndt),
         "mu": rng.standard_normal(d) + rng.uniform(-8, 8, size=d),
         "b_v": rng.standard_normal(n_kv * hd) * 0.1, "b_o": rng.standard_normal(d) * 0.1}
    return w


@functools.lru_cache(maxsize=None)
def _case(shape, variant):
    n_heads, n_kv, hd, rank, d = shape
    wdt, ndt, biased, layout, b_tdt, out_tdt = VARIANTS[variant]
    dev = torch.device("cuda:0")
    w = _values(shape, wdt, ndt, seed=97 * variant + d + 13 * rank + n_heads)
    tw = torch.bfloat16 if wdt == "bf16" else torch.float64
    tn = torch.bfloat16 if ndt == "bf16" else torch.float64
    keep = []                                                   # (the buffers behind the views)
    placed = []
    for name, t in (("W_v", tw), ("W_o", tw), ("v_hat", tn), ("o_hat", tn)):
        buf, view, ld = _place(w[name], t, layout, dev)
        keep.append(buf)
        placed.append((view, ld))
    ops_ = tuple(placed) + (tw, tn)
    mu = torch.from_numpy(w["mu"]).to(dev)
    b_v = b_o = None
    if biased:
        b_v, b_o = torch.from_numpy(w["b_v"]).to(dev).to(b_tdt), torch.from_numpy(w["b_o"]).to(dev).to(b_tdt)
        w["b_v"], w["b_o"] = b_v.double().cpu().numpy(), b_o.double().cpu().numpy()       # (the values the kernel reads)
    else:
        w["b_v"] = w["b_o"] = None
    if rank == 0:
        w["v_hat"] = w["o_hat"] = None
    full = _call(dev, ops_, shape, rank, mu, b_v, b_o, b_tdt, out_tdt)
    again = _call(dev, ops_, shape, rank, mu, b_v, b_o, b_tdt, out_tdt)
    plain = _call(dev, ops_, shape, rank, mu, b_v, None, b_tdt, out_tdt)                 # no b_o: bias_f64 IS delta
    const = _call(dev, ops_, shape, 0, mu, b_v, None, b_tdt, out_tdt)                    # rank 0: delta is the whole constant
    no_out = _call(dev, ops_, shape, rank, mu, b_v, b_o, b_tdt, out_tdt, want_out=False)
    return w, dict(full=full, again=again, plain=plain, const=const, no_out=no_out), (ops_, mu, b_v, b_o, keep)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_kernel_against_the_model(dev, case):
    shape, variant = case
    n_heads, n_kv, hd, rank, d = shape
    out_tdt = VARIANTS[variant][5]
    w, got, _ = _case(shape, variant)
    args = (w["W_v"], w["W_o"], w["v_hat"], w["o_hat"], w["mu"], n_heads, n_kv, hd, rank)
    ref, ref_const = V.delta(*args, b_v=w["b_v"])
    bound = V.delta_bound(*args, b_v=w["b_v"])
    dl = got["plain"][1].numpy()
    err = np.abs(V.ld(dl) - ref)
    print(f"delta: worst error / bound = {float((err / bound).max()):.3e}; max |delta| {float(np.abs(ref).max()):.3e}")
    assert np.all(err <= bound)
    cst = got["const"][1].numpy()
    assert np.all(np.abs(V.ld(cst) - ref_const) <= V.delta_bound(w["W_v"], w["W_o"], None, None, w["mu"], n_heads, n_kv, hd, 0, b_v=w["b_v"]))
    # bias_f64 = b_o + delta: one fp64 addition of the same delta
    want64 = dl if w["b_o"] is None else w["b_o"] + dl
    assert np.array_equal(got["full"][1].numpy(), want64)
    # bias_out: the one rounding torch makes, bit for bit
    assert got["full"][0].dtype == out_tdt
    assert torch.equal(got["full"][0], got["full"][1].to(out_tdt))
    # norms: against the rows the device produced; b_o does not enter them; rank 0 gives the constant twice
    for value, rows in ((got["plain"][2][0], dl), (got["plain"][2][1], cst), (got["const"][2][0], cst)):
        s = (V.ld(rows) ** 2).sum()
        assert abs(V.LD(value.item()) - s) <= (d + 8) * V.LD(U) * s
    assert torch.equal(got["full"][2], got["plain"][2])
    assert got["const"][2][0] == got["const"][2][1] == got["plain"][2][1]
    if rank == 0:
        assert np.array_equal(dl, cst)
    # two runs: the same bits; a NULL bias_out changes nothing else
    for a, b in zip(got["full"], got["again"]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert torch.equal(got["no_out"][1], got["full"][1]) and torch.equal(got["no_out"][2], got["full"][2])
    assert bool(torch.isnan(got["no_out"][0].double()).all())                            # (its buffer was never written)


def test_nan_containment(dev):
    shape, variant = SHAPES[0], 0
    n_heads, n_kv, hd, rank, d = shape
    w, got, (ops_, mu, b_v, b_o, _) = _case(shape, variant)
    base = got["full"]
    b_tdt, out_tdt = VARIANTS[variant][4], VARIANTS[variant][5]
    (Wv, ld_wv), (Wo, ld_wo), (Vn, ld_v), (On, ld_o), tw, tn = ops_
    nan = float("nan")
    # one row of W_o / o^: that row's bias entry alone, and the norms
    for mat, row, col in ((Wo, 17, 33), (On, 41, 5)):
        old = mat[row, col].clone()
        mat[row, col] = nan
        try:
            out = _call(dev, ops_, shape, rank, mu, b_v, b_o, b_tdt, out_tdt)
        finally:
            mat[row, col] = old
        bad = torch.isnan(out[1])
        assert bool(bad[row]) and int(bad.sum()) == 1 and bool(torch.isnan(out[0][row])) and bool(torch.isnan(out[2][0]))
        assert torch.equal(out[1][~bad], base[1][~bad]) and torch.equal(out[0][~bad], base[0][~bad])
    # one kv head's W_v, v^ or b_v: every row sums over all heads, so every entry (and the norms)
    for mat, idx in ((Wv, (hd + 3, 7)), (Vn, (2, 9)), (b_v, (5,))):
        old = mat[idx].clone()
        mat[idx] = nan
        try:
            out = _call(dev, ops_, shape, rank, mu, b_v, b_o, b_tdt, out_tdt)
        finally:
            mat[idx] = old
        assert bool(torch.isnan(out[1]).all()) and bool(torch.isnan(out[2][0]))
    after = _call(dev, ops_, shape, rank, mu, b_v, b_o, b_tdt, out_tdt)
    assert torch.equal(after[1], base[1])                                                # (the operands are back as they were)


def test_rounding_goes_through_fp32_as_torch_does(dev):
    """Zero weights at rank 0 make delta = +0, so bias_f64 is b_o and bias_out the rounding alone -- at values where rounding the double
    directly differs from rounding it through fp32 (a compiler that merges the two conversions gives 1 + 2^-10 for the second)."""
    shape = (2, 1, 8, 0, 24)
    n_heads, n_kv, hd, rank, d = shape
    b_vals = np.zeros(d)
    b_vals[:5] = [1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -11 + 2.0 ** -30, 1 + 3 * 2.0 ** -8 - 2.0 ** -30, 1e39, 7e4]
    zero = lambda rows, width: _place(np.zeros((rows, width)), torch.bfloat16, "tight", dev)                       # noqa: E731
    (bwv, Wv, ld_wv), (bwo, Wo, ld_wo) = zero(n_kv * hd, d), zero(d, n_heads * hd)
    ops_ = ((Wv, ld_wv), (Wo, ld_wo), (Wv, ld_wv), (Wo, ld_wo), torch.bfloat16, torch.bfloat16)                    # (rank 0: no factors)
    mu = torch.from_numpy(np.random.default_rng(2).standard_normal(d)).to(dev)
    b_o = torch.from_numpy(b_vals).to(dev)
    got = {}
    for out_tdt in (torch.bfloat16, torch.float16, torch.float32, torch.float64):
        bias, b64, norms = _call(dev, ops_, shape, 0, mu, None, b_o, torch.float64, out_tdt)
        assert np.array_equal(b64.numpy(), b_vals)
        assert torch.equal(bias, b64.to(out_tdt))
        got[out_tdt] = bias.double().numpy()
    inf = float("inf")
    assert got[torch.bfloat16][0] == 1.0 and got[torch.float16][1] == 1.0 and got[torch.bfloat16][2] == 1.015625
    assert got[torch.float32][3] == inf and got[torch.bfloat16][3] == inf and got[torch.float16][4] == inf


def test_bad_arguments(dev):
    from modegpt_amd import _lib
    lib = _lib.load()
    n_heads, n_kv, hd, rank, d = 4, 2, 32, 22, 64
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=dev)             # noqa: E731
    Wv, Wo, Vn, On = z(n_kv * hd, d), z(d, n_heads * hd), z(n_kv * rank, d), z(d, n_heads * rank)
    mu, bf, nm = z(d, dt=torch.float64), z(d, dt=torch.float64), z(2, dt=torch.float64)
    bv, bo, out = z(n_kv * hd), z(d), z(d)
    nbytes = lib.mdg_vo_intercept_ws_bytes(d, n_kv, hd, rank)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    BF = _lib.MDG_BF16
    good = dict(Wv=Wv.data_ptr(), ld_wv=d, Wo=Wo.data_ptr(), ld_wo=n_heads * hd, w_dtype=BF, v_new=Vn.data_ptr(), ld_v=d,
                o_new=On.data_ptr(), ld_o=n_heads * rank, new_dtype=BF, d=d, n_heads=n_heads, n_kv=n_kv, hd=hd, rank=rank,
                mu=mu.data_ptr(), b_v=bv.data_ptr(), b_o=bo.data_ptr(), b_dtype=BF, bias_out=out.data_ptr(), out_dtype=BF,
                bias_f64=bf.data_ptr(), norms=nm.data_ptr(), ws=ws.data_ptr(), ws_bytes=nbytes, stream=None)
    with torch.cuda.device(dev):
        assert lib.mdg_vo_intercept(*good.values()) == _lib.MDG_OK
        assert lib.mdg_vo_intercept(*dict(good, bias_out=None, b_v=None, b_o=None).values()) == _lib.MDG_OK
        assert lib.mdg_vo_intercept(*dict(good, rank=0, v_new=None, o_new=None).values()) == _lib.MDG_OK
        bad = [dict(Wv=None), dict(Wo=None), dict(mu=None), dict(bias_f64=None), dict(norms=None), dict(ws=None),       # a null required pointer
               dict(w_dtype=_lib.MDG_F16), dict(new_dtype=_lib.MDG_F32), dict(b_dtype=99), dict(out_dtype=99),           # an unsupported dtype
               dict(n_kv=3), dict(hd=130), dict(hd=31), dict(n_kv=0),                                                     # ... head layout
               dict(rank=-1), dict(rank=hd + 1),                                                                          # a rank outside the range
               dict(ld_wv=d - 1), dict(ld_v=d - 1), dict(ld_wo=n_heads * hd - 1), dict(ld_o=n_heads * rank - 1),         # leading dimensions
               dict(ws_bytes=nbytes - 1),                                                                                 # a workspace that is too small
               dict(v_new=None), dict(o_new=None)]                                                                        # rank > 0 without the factors
        for kw in bad:
            assert lib.mdg_vo_intercept(*dict(good, **kw).values()) == _lib.MDG_ERR_BAD_ARG, kw
            assert b"mdg_vo_intercept" in lib.mdg_last_error()
    torch.cuda.synchronize(dev)
    assert lib.mdg_vo_intercept_ws_bytes(0, 2, 32, 22) == 0 and lib.mdg_vo_intercept_ws_bytes(64, 2, 32, 33) == 0
