"""GPU: mdg_nystrom_intercept (colsum.hip: intercept_rows_kernel; row_dots.hpp: row_dots, pair_norms_kernel) through the raw C ABI, run the
way production runs it: more than one 2048-column LDS chunk, ragged last chunks, operands that take the scalar path, every dtype.

Every operand sits inside a larger buffer.  Inputs have NaN pads behind column n (or r) of every row and behind the last row, and must
come back bit for bit; outputs and the workspace (exactly mdg_nystrom_intercept_ws_bytes(d) bytes) sit between guards of a NaN with a
payload that must survive, and every entry between the guards must have been written.

Shapes (d, n, r): mean_model.INTERCEPT_SHAPES.  Layouts of W_d and of D^, independently:
  tight    ld = width, 16-byte-aligned pointer                      (vector path for bf16 where width is a multiple of 8)
  pad8     ld = width rounded up to 8, plus 8                       (vector path with NaN pads in reach of a 16-byte load)
  odd      ld = width + 3 -- + 5 where width + 3 is a multiple of 8, as for n = 2053 -- so ld is no multiple of 8: scalar path
  offset   aligned buffer, pointer one element in, ld a multiple of 8: scalar path through the pointer test alone

Lattice data (mean_model.lattice_case; tests/test_mean_model_host.py proves fp64 evaluates it exactly in any order): bias_f64 and both
norms equal the long double model TO THE BIT, in every layout, for bf16 and fp64 weights, with and without b_d, with repeated idx
entries; bias_out is torch's .to() of bias_f64.  Generic data (mean_model.generic_case): bias_f64 entry-wise within mean_model.bias_bound
(a priori: n + r exact products added in any order), the norms within (d + 2) 2^-53 of the sums of squares of the rows the device
itself produced.  Nothing is fitted to the kernel.

Measured on an MI355X: the largest bias err / bound over the generic cases is 2.42e-2 (shape B; 5.6e-5 at E, 2.1e-5 at F: the bound
grows with n + r, the error does not), the same for bf16 and fp64 weights and for the vector and the scalar path; the 131 cases of the
file take 4.6 s together, the slowest 0.4 s.

What the file found: bias_out in fp16 was rounded ONCE, from the double -- the backend merged `(float)v` and the float -> half
conversion behind it into one -- where the header and torch round through fp32: 1 + 2^-11 + 2^-30 gave 1 + 2^-10, not 1
(test_rounding_goes_through_fp32_as_torch_does; common.hpp's f64_to_f16 now keeps the two conversions apart).  mdg_vo_intercept
shared the store and the fault (tests/test_gpu_vo_intercept.py has the same values)."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import mean_model as M

pytestmark = pytest.mark.gpu

SHAPES = M.INTERCEPT_SHAPES
BF16, F16, F32, F64 = 0, 1, 2, 3                       # MDG_* element codes (asserted against _lib below)
TORCH_OF = {BF16: torch.bfloat16, F16: torch.float16, F32: torch.float32, F64: torch.float64}
INT_OF = {2: torch.int16, 4: torch.int32, 8: torch.int64}
# a NaN with a payload per element size (the fp64 one is tests/test_gpu_sympack.py's); no arithmetic produces these bits
SENTINEL = {2: 0x7FDE, 4: 0x7FC0BEEF, 8: 0x7FF8DEADBEEF1234}
GUARD = 8                                              # guard elements in front of and behind every output
LAYOUTS = ("tight", "pad8", "odd", "offset")
# (layout of W_d, layout of D^): all-tight, W-only-off, D-only-off, both-off, and the padded vector path
COMBOS_CHUNKED = [("tight", "tight"), ("pad8", "pad8"), ("odd", "tight"), ("tight", "odd"), ("offset", "tight"), ("tight", "offset"),
                  ("odd", "offset"), ("offset", "odd")]
COMBOS_SMALL = [("tight", "tight"), ("pad8", "pad8"), ("odd", "offset")]
U = 2.0 ** -53


def _lib():
    from modegpt_amd import _lib as L
    assert (L.MDG_BF16, L.MDG_F16, L.MDG_F32, L.MDG_F64) == (BF16, F16, F32, F64)
    return L


def _bits(t):
    return t.contiguous().view(INT_OF[t.element_size()])


# ------------------------------------------------------------------ operands inside larger buffers
def _geometry(width, layout):
    """(ld, pointer offset in elements)."""
    up8 = (width + 7) // 8 * 8
    if layout == "tight":
        return width, 0
    if layout == "pad8":
        return up8 + 8, 0
    if layout == "odd":
        ld = width + 3 if (width + 3) % 8 else width + 5
        assert ld % 8
        return ld, 0
    assert layout == "offset"
    return up8 + 8, 1


def _place(a, dtype, layout="tight"):
    """The fp64 numpy matrix `a` [rows, width] as `dtype` inside a NaN-filled device buffer.  -> (buffer, pointer, ld, snapshot)."""
    dev = torch.device("cuda")
    rows, width = a.shape
    ld, off = _geometry(width, layout)
    buf = torch.full((off + (rows + 1) * ld + 16,), float("nan"), dtype=dtype, device=dev)      # (NaN behind the last row too)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + rows * ld].view(rows, ld)[:, :width]
    view.copy_(torch.from_numpy(a).to(dev).to(dtype))
    ptr = buf.data_ptr() + off * buf.element_size()
    if layout in ("tight", "pad8"):
        assert ptr % 16 == 0
    return types.SimpleNamespace(buf=buf, ptr=ptr, ld=ld, snap=buf.clone(), view=view)


def _place_vec(a, dtype):
    """A vector with pads in front and behind: NaN for the floating types, an index far out of range for idx."""
    dev = torch.device("cuda")
    fill = 2 ** 62 if dtype == torch.int64 else float("nan")
    buf = torch.full((a.shape[0] + 2 * GUARD,), fill, dtype=dtype, device=dev)
    buf[GUARD:GUARD + a.shape[0]] = torch.from_numpy(a).to(dev).to(dtype)
    return types.SimpleNamespace(buf=buf, ptr=buf.data_ptr() + GUARD * buf.element_size(), snap=buf.clone())


def _unchanged(op):
    return torch.equal(_bits(op.buf), _bits(op.snap))


class _Out:
    """`count` elements of `dtype` between two guards of sentinels."""

    def __init__(self, count, dtype):
        size = torch.empty(0, dtype=dtype).element_size()
        self.count, self.sent = count, SENTINEL[size]
        sent = self.sent - (1 << (8 * size)) if self.sent >= 1 << (8 * size - 1) else self.sent
        self.raw = torch.full((count + 2 * GUARD,), sent, dtype=INT_OF[size], device="cuda")
        self.sent_signed = sent
        self.dtype = dtype
        self.ptr = self.raw.data_ptr() + GUARD * size

    def read(self):
        host = self.raw.cpu()
        body = host[GUARD:GUARD + self.count]
        guards_ok = bool((host[:GUARD] == self.sent_signed).all() and (host[GUARD + self.count:] == self.sent_signed).all())
        return body.view(self.dtype), guards_ok, int((body == self.sent_signed).sum())


def _call(W, Dh, idx, mu, d, n, r, wdt, b=None, bdt=0, odt=BF16, want_out=True, mutate=None):
    """One raw call.  Asserts the buffer discipline and returns (rc, bias_out or None, bias_f64, norms) on the host.  `mutate` edits
    the argument dictionary (the refusal tests)."""
    L = _lib()
    lib = L.load()
    outs = {"bias_f64": _Out(d, torch.float64), "norms": _Out(2, torch.float64), "ws": _Out(2 * d, torch.float64)}
    assert lib.mdg_nystrom_intercept_ws_bytes(d) == 16 * d
    if want_out:
        outs["bias_out"] = _Out(d, TORCH_OF.get(odt, torch.float64))
    a = dict(Wd=W.ptr, d=d, n=n, ld_wd=W.ld, w_dtype=wdt, down_hat=Dh.ptr, r=r, ld_down=Dh.ld, idx=idx.ptr, mu=mu.ptr,
             b_d=None if b is None else b.ptr, b_dtype=bdt, bias_out=outs["bias_out"].ptr if want_out else None, out_dtype=odt,
             bias_f64=outs["bias_f64"].ptr, norms=outs["norms"].ptr, ws=outs["ws"].ptr, ws_bytes=16 * d)
    if mutate:
        mutate(a)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.mdg_nystrom_intercept(a["Wd"], a["d"], a["n"], a["ld_wd"], a["w_dtype"], a["down_hat"], a["r"], a["ld_down"], a["idx"],
                                   a["mu"], a["b_d"], a["b_dtype"], a["bias_out"], a["out_dtype"], a["bias_f64"], a["norms"], a["ws"],
                                   a["ws_bytes"], st)
    torch.cuda.synchronize()
    for name, op in (("W_d", W), ("D^", Dh), ("idx", idx), ("mu", mu), ("b_d", b)):
        assert op is None or _unchanged(op), f"{name} was modified"
    got = {}
    for name, o in outs.items():
        body, guards_ok, untouched = o.read()
        assert guards_ok, f"a guard of {name} was overwritten"
        if rc == L.MDG_OK:
            assert untouched == 0, f"{untouched} entries of {name} were not written"
        else:
            assert untouched == o.count, f"{name} was written by a refused call"
        got[name] = body
    return rc, got.get("bias_out"), got["bias_f64"], got["norms"]


def _ok(res):
    assert res[0] == 0, _lib().last_error()
    return res[1:]


# ------------------------------------------------------------------ cases, models and placed operands, made once and shared
@functools.lru_cache(maxsize=None)
def _case(kind, name, repeat=False):
    d, n, r = SHAPES[name]
    return M.lattice_case(d, n, r, seed=1, repeat=repeat) if kind == "lattice" else M.generic_case(d, n, r, seed=1)


@functools.lru_cache(maxsize=None)
def _model(kind, name, repeat, with_b):
    c = _case(kind, name, repeat)
    b, n0, n1 = M.intercept(c["W"], c["D"], c["idx"], c["mu"], c["b_d"] if with_b else None)
    return b, M.LD(n0), M.LD(n1)


@functools.lru_cache(maxsize=8)
def _mat(kind, name, repeat, which, code, layout):
    return _place(_case(kind, name, repeat)[which], TORCH_OF[code], layout)


@functools.lru_cache(maxsize=None)
def _vec(kind, name, repeat, which, code=F64):
    return _place_vec(_case(kind, name, repeat)[which], torch.int64 if which == "idx" else TORCH_OF[code])


def _run_case(kind, name, wdt, lw="tight", ldn="tight", with_b=True, repeat=False, bdt=BF16, odt=BF16, want_out=True):
    d, n, r = SHAPES[name]
    key = (kind, name, repeat)
    b = _vec(*key, "b_d", bdt) if with_b else None
    return _ok(_call(_mat(*key, "W", wdt, lw), _mat(*key, "D", BF16, ldn), _vec(*key, "idx"), _vec(*key, "mu"), d, n, r, wdt, b=b,
                     bdt=bdt, odt=odt, want_out=want_out))


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _rounded_like_torch(bias_out, bias_f64, dtype):
    """bias_out is torch's CPU .to(dtype) of bias_f64: the same bits, NaN for NaN."""
    want = bias_f64.to(dtype)
    nan = torch.isnan(want)
    return bias_out.dtype == dtype and torch.equal(torch.isnan(bias_out), nan) and torch.equal(_bits(bias_out)[~nan], _bits(want)[~nan])


# ------------------------------------------------------------------ 1. lattice data: equality to the bit
def _lattice_params():
    out = []
    for name in SHAPES:
        for wdt in (BF16, F64):
            for lw, ldn in (COMBOS_CHUNKED if name in "DEF" else COMBOS_SMALL):
                out.append(pytest.param(name, wdt, lw, ldn, id=f"{name}-{'bf16' if wdt == BF16 else 'f64'}-{lw}-{ldn}"))
    return out


_lattice_seen = {}


def _lattice_variants(name):
    return [(True, False), (False, False)] + ([(True, True)] if name in "EF" else [])


def _check_lattice(name, wdt, lw, ldn):
    for with_b, repeat in _lattice_variants(name):
        bias, b64, norms = _run_case("lattice", name, wdt, lw, ldn, with_b=with_b, repeat=repeat)
        ref, n0, n1 = _model("lattice", name, repeat, with_b)
        assert np.array_equal(b64.numpy(), ref.astype(np.float64)), (with_b, repeat)
        assert norms[0].item() == float(n0) and norms[1].item() == float(n1), (with_b, repeat)
        assert _rounded_like_torch(bias, b64, torch.bfloat16)
        _lattice_seen.setdefault((name, with_b, repeat), {})[(wdt, lw, ldn)] = (b64, norms, bias)


@pytest.mark.parametrize("name,wdt,lw,ldn", _lattice_params())
def test_lattice_every_output_equals_the_model_to_the_bit(name, wdt, lw, ldn):
    assert M.lattice_is_exact(_case("lattice", name))
    _check_lattice(name, wdt, lw, ldn)


@pytest.mark.parametrize("name", list(SHAPES))
def test_lattice_layouts_and_weight_dtypes_agree_bit_for_bit(name):
    """Exact data: whichever path an operand takes -- 16-byte vectors or scalars, bf16 or fp64 weights -- the bits are the same."""
    combos = COMBOS_CHUNKED if name in "DEF" else COMBOS_SMALL
    for wdt in (BF16, F64):
        for lw, ldn in combos:
            if (wdt, lw, ldn) not in _lattice_seen.get((name, True, False), {}):
                _check_lattice(name, wdt, lw, ldn)
    for variant in _lattice_variants(name):
        seen = _lattice_seen[(name,) + variant]
        assert len(seen) == 2 * len(combos)
        first = seen[(BF16, "tight", "tight")]
        for key, got in seen.items():
            assert all(_same_bits(g, f) for g, f in zip(got, first)), (variant, key)


# ------------------------------------------------------------------ 2. generic data within the a priori bounds
@pytest.mark.parametrize("layout", ["tight", "odd"])
@pytest.mark.parametrize("wdt", [BF16, F64], ids=["bf16", "f64"])
@pytest.mark.parametrize("name", ["B", "E", "F"])
def test_generic_data_within_the_derived_bound(name, wdt, layout):
    d, n, r = SHAPES[name]
    c = _case("generic", name)
    worst = 0.0
    rows = {}
    for with_b in (True, False):
        bias, b64, norms = _run_case("generic", name, wdt, layout, layout, with_b=with_b)
        ref, _, _ = _model("generic", name, False, with_b)
        bound = M.bias_bound(c["W"], c["D"], c["idx"], c["mu"], c["b_d"] if with_b else None)
        err = np.abs(M.ld(b64.numpy()) - ref)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound)
        assert _rounded_like_torch(bias, b64, torch.bfloat16)
        rows[with_b] = (b64, norms)
    print(f"{name} {'bf16' if wdt == BF16 else 'f64'} {layout}: bias err / bound max {worst:.3e}")
    assert _same_bits(rows[True][1], rows[False][1])                       # b_d does not enter the norms
    # the norms against the rows the device itself produced: bias_f64 without b_d IS delta, with a zero D^ it is W_d mu
    zero = _place(np.zeros((d, r)), torch.bfloat16, layout)
    _, wmu, norms_z = _ok(_call(_mat("generic", name, False, "W", wdt, layout), zero, _vec("generic", name, False, "idx"),
                                _vec("generic", name, False, "mu"), d, n, r, wdt))
    dl, norms = M.ld(rows[False][0].numpy()), rows[False][1]
    wmu = M.ld(wmu.numpy())
    for got, v in ((norms[0], dl), (norms[1], wmu), (norms_z[0], wmu), (norms_z[1], wmu)):
        s = (v * v).sum()
        assert abs(M.LD(got.item()) - s) <= (d + 2) * M.LD(U) * s
    assert norms_z[0].item() == norms_z[1].item()


# ------------------------------------------------------------------ 3. bias dtypes and the rounding
@pytest.mark.parametrize("bdt", [BF16, F16, F32, F64, None], ids=["b_bf16", "b_f16", "b_f32", "b_f64", "b_null"])
def test_every_bias_dtype_in_and_out(bdt):
    ref, _, _ = _model("lattice", "E", False, bdt is not None)
    want = torch.from_numpy(ref.astype(np.float64))
    for odt in (BF16, F16, F32, F64, None):
        bias, b64, norms = _run_case("lattice", "E", BF16, "pad8", "odd", with_b=bdt is not None, bdt=bdt or 0,
                                     odt=0 if odt is None else odt, want_out=odt is not None)
        assert _same_bits(b64, want), (bdt, odt)                           # identical whatever the dtypes, up to the b_d term
        if odt is None:
            assert bias is None
        else:
            assert _rounded_like_torch(bias, b64, TORCH_OF[odt]), (bdt, odt)


def test_rounding_goes_through_fp32_as_torch_does():
    """W_d = 0 and D^ = 0 make delta = +0, so bias_f64 is b_d and bias_out is the rounding alone, at values where rounding the double
    directly differs from rounding it through fp32."""
    b_vals = np.array([1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -11 + 2.0 ** -30, 1 + 3 * 2.0 ** -8 - 2.0 ** -30, 1e39, 7e4, np.nan, -0.0])
    d, n, r = len(b_vals), 9, 7
    rng = np.random.default_rng(3)
    W, Dh = _place(np.zeros((d, n)), torch.bfloat16), _place(np.zeros((d, r)), torch.bfloat16, "odd")
    idx = _place_vec(rng.permutation(n)[:r].astype(np.int64), torch.int64)
    mu = _place_vec(rng.integers(-16, 17, size=n).astype(np.float64), torch.float64)
    b = _place_vec(b_vals, torch.float64)
    got = {}
    for odt in (BF16, F16, F32, F64):
        bias, b64, norms = _ok(_call(W, Dh, idx, mu, d, n, r, BF16, b=b, bdt=F64, odt=odt))
        fin = ~np.isnan(b_vals)
        assert np.array_equal(b64.numpy()[fin], b_vals[fin]) and np.isnan(b64.numpy()[~fin]).all()
        assert not np.signbit(b64.numpy()[6]) and not bool(torch.signbit(bias[6]))          # -0 + (+0) = +0
        assert _rounded_like_torch(bias, b64, TORCH_OF[odt])
        assert _same_bits(norms, torch.zeros(2, dtype=torch.float64))
        got[odt] = bias.to(torch.float64).numpy()
    inf = float("inf")
    assert got[BF16][0] == 1.0                       # directly: 1.0078125 (fp32 drops the 2^-30 and leaves a tie, which goes to even)
    assert got[F16][1] == 1.0                        # directly: 1 + 2^-10
    assert got[BF16][2] == 1.015625                  # fp32 rounds up to the tie 1 + 3 2^-8, which goes to even: 1 + 2^-6
    assert got[F32][3] == inf and got[BF16][3] == inf and got[F16][3] == inf and got[F64][3] == 1e39
    assert got[F16][4] == inf and got[F32][4] == 7e4 and got[BF16][4] == 70144.0
    assert all(np.isnan(got[o][5]) for o in got)
    assert all(got[o][6] == 0 for o in got)


# ------------------------------------------------------------------ 4. idx out of range: no memory read, NaN
@pytest.mark.parametrize("pos", [1000, 3000], ids=["first_chunk", "later_chunk"])
@pytest.mark.parametrize("bad", [-1, None, 2 ** 40], ids=["minus_one", "n", "two_to_40"])
def test_idx_out_of_range_contributes_nan_and_reads_nothing(bad, pos):
    d, n, r = SHAPES["F"]
    key = ("lattice", "F", False)
    idx = _case(*key)["idx"].copy()
    idx[pos] = n if bad is None else bad
    _, b64, norms = _ok(_call(_mat(*key, "W", BF16, "tight"), _mat(*key, "D", BF16, "tight"), _place_vec(idx, torch.int64),
                              _vec(*key, "mu"), d, n, r, BF16, b=_vec(*key, "b_d", BF16), bdt=BF16))
    assert bool(torch.isnan(b64).all()) and bool(torch.isnan(norms[0]))
    assert norms[1].item() == float(_model(*key, True)[2])                 # W_d mu does not read idx: the exact lattice bits


# ------------------------------------------------------------------ 5. a NaN stays in its row, past the first chunk too
@pytest.mark.parametrize("which,col", [("W", 4100), ("D", 2500)], ids=["W_third_chunk", "D_second_chunk"])
def test_nan_beyond_the_first_chunk_stays_in_its_row(which, col):
    d, n, r = SHAPES["F"]
    key = ("lattice", "F", False)
    row = 222
    a = _case(*key)[which].copy()
    a[row, col] = np.nan
    ops_ = {w: _mat(*key, w, BF16, "tight") for w in "WD"}
    ops_[which] = _place(a, torch.bfloat16, "tight")
    bias, b64, norms = _ok(_call(ops_["W"], ops_["D"], _vec(*key, "idx"), _vec(*key, "mu"), d, n, r, BF16, b=_vec(*key, "b_d", BF16),
                                 bdt=BF16))
    ref = torch.from_numpy(_model(*key, True)[0].astype(np.float64))
    bad = torch.isnan(b64)
    assert bool(bad[row]) and int(bad.sum()) == 1 and bool(torch.isnan(bias[row])) and int(torch.isnan(bias).sum()) == 1
    assert torch.equal(_bits(b64)[~bad], _bits(ref)[~bad])
    assert bool(torch.isnan(norms[0]))
    # (a NaN in D^ leaves W_d mu, and with it the second norm, alone)
    assert bool(torch.isnan(norms[1])) if which == "W" else norms[1].item() == float(_model(*key, True)[2])


# ------------------------------------------------------------------ 6. the same bits from run to run
@pytest.mark.parametrize("wdt", [BF16, F64], ids=["bf16", "f64"])
def test_two_calls_give_the_same_bits(wdt):
    first = _run_case("generic", "F", wdt, "tight", "odd")
    second = _run_case("generic", "F", wdt, "tight", "odd")
    assert all(_same_bits(a, b) for a, b in zip(first, second))


# ------------------------------------------------------------------ 7. the ops front end
def _dev_case(name):
    c = _case("lattice", name)
    dev = torch.device("cuda")
    return c, {k: torch.from_numpy(v).to(dev) for k, v in c.items()}


def test_ops_widens_fp16_weights_and_defaults_to_their_dtype():
    from modegpt_amd import ops
    c, t = _dev_case("D")
    W16 = t["W"].to(torch.float16)
    bias, b64, norms = ops.nystrom_intercept(W16, t["D"].to(torch.bfloat16), t["idx"], t["mu"])
    torch.cuda.synchronize()
    ref, n0, n1 = _model("lattice", "D", False, False)
    assert bias.dtype == torch.float16 and W16.dtype == torch.float16
    assert np.array_equal(b64.cpu().numpy(), ref.astype(np.float64)) and norms.cpu().tolist() == [float(n0), float(n1)]
    assert _rounded_like_torch(bias.cpu(), b64.cpu(), torch.float16)
    raw = _run_case("lattice", "D", F64, with_b=False, odt=F16)                      # the raw call on the widened weight
    assert all(_same_bits(a.cpu(), b) for a, b in zip((bias, b64, norms), raw))


def test_ops_accepts_row_strided_operands():
    from modegpt_amd import ops
    d, n, r = SHAPES["D"]
    c, t = _dev_case("D")
    Wbig = torch.full((d, n + 11), float("nan"), dtype=torch.bfloat16, device="cuda")
    Dbig = torch.full((d, r + 5), float("nan"), dtype=torch.bfloat16, device="cuda")
    Wbig[:, :n] = t["W"].to(torch.bfloat16)
    Dbig[:, 2:2 + r] = t["D"].to(torch.bfloat16)
    Wv, Dv = Wbig[:, :n], Dbig[:, 2:2 + r]
    assert Wv.stride(0) > n and Dv.stride(0) > r and not Wv.is_contiguous() and not Dv.is_contiguous()
    bd = t["b_d"].to(torch.bfloat16)
    got = ops.nystrom_intercept(Wv, Dv, t["idx"], t["mu"], b_d=bd)
    torch.cuda.synchronize()
    raw = _run_case("lattice", "D", BF16, with_b=True)
    assert all(_same_bits(a.cpu(), b) for a, b in zip(got, raw))
    assert got[0].dtype == torch.bfloat16


def test_ops_refuses_what_the_kernel_cannot_take():
    from modegpt_amd import ops
    d, n, r = SHAPES["B"]
    c, t = _dev_case("B")
    W, Dh, bd = t["W"].to(torch.bfloat16), t["D"].to(torch.bfloat16), t["b_d"].to(torch.bfloat16)
    ops.nystrom_intercept(W, Dh, t["idx"], t["mu"], b_d=bd)                           # (the arguments below differ in one thing each)
    wide = torch.zeros(d, 2 * r, dtype=torch.bfloat16, device="cuda")
    for args, kw in (((W, Dh.to(torch.float16), t["idx"], t["mu"]), {}),
                     ((W, Dh.to(torch.float64), t["idx"], t["mu"]), {}),
                     ((W, wide[:, ::2], t["idx"], t["mu"]), {}),
                     ((W, Dh, t["idx"], t["mu"][:-1]), {}),
                     ((W, Dh, t["idx"], torch.cat([t["mu"], t["mu"][:1]])), {}),
                     ((W, Dh, t["idx"], t["mu"].to(torch.float32)), {}),
                     ((W, Dh, t["idx"], t["mu"]), {"b_d": bd[:-1]}),
                     ((W, Dh, t["idx"], t["mu"]), {"b_d": torch.cat([bd, bd[:1]])})):
        with pytest.raises(ValueError):
            ops.nystrom_intercept(*args, **kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. refusals leave every output alone
def _set(**kw):
    return lambda a: a.update(kw)


REFUSALS = {
    "Wd_null": _set(Wd=None), "down_hat_null": _set(down_hat=None), "idx_null": _set(idx=None), "mu_null": _set(mu=None),
    "bias_f64_null": _set(bias_f64=None), "norms_null": _set(norms=None), "ws_null": _set(ws=None),
    "w_f16": _set(w_dtype=F16), "w_f32": _set(w_dtype=F32), "w_7": _set(w_dtype=7),
    "b_dtype_unknown": _set(b_dtype=7), "out_dtype_unknown": _set(out_dtype=7),
    "d_0": _set(d=0), "n_0": _set(n=0), "r_0": _set(r=0),
    "r_above_n": lambda a: a.update(r=a["n"] + 1, ld_down=a["n"] + 8),
    "ld_wd_short": lambda a: a.update(ld_wd=a["n"] - 1), "ld_down_short": lambda a: a.update(ld_down=a["r"] - 1),
    "ws_one_byte_short": lambda a: a.update(ws_bytes=a["ws_bytes"] - 1), "ws_misaligned": lambda a: a.update(ws=a["ws"] + 4),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_name_the_call_and_write_nothing(what):
    L = _lib()
    d, n, r = SHAPES["B"]
    key = ("lattice", "B", False)
    res = _call(_mat(*key, "W", BF16, "pad8"), _mat(*key, "D", BF16, "pad8"), _vec(*key, "idx"), _vec(*key, "mu"), d, n, r, BF16,
                b=_vec(*key, "b_d", BF16), bdt=BF16, mutate=REFUSALS[what])          # (_call asserts that nothing was written)
    assert res[0] == L.MDG_ERR_BAD_ARG and "mdg_nystrom_intercept" in L.last_error()


def test_unknown_b_dtype_without_b_d_is_accepted():
    d, n, r = SHAPES["B"]
    key = ("lattice", "B", False)
    _, b64, norms = _ok(_call(_mat(*key, "W", BF16, "pad8"), _mat(*key, "D", BF16, "pad8"), _vec(*key, "idx"), _vec(*key, "mu"), d, n, r,
                              BF16, b=None, bdt=7))
    ref, n0, n1 = _model(*key, False)
    assert np.array_equal(b64.numpy(), ref.astype(np.float64)) and norms.tolist() == [float(n0), float(n1)]
