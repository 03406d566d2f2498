"""mdg_vo_compress's own kernels (vo_factors_grouped_kernel, vo_sv_kernel, vo_factors_mha_kernel, scale_to_f64_kernel and the GEMMs
that carry P [h][r][hd] and Q [h][hd][r] into v_proj / o_proj) and mdg_vo_spectrum, against the long-double model
tests/vo_error_model.py: at every syevj instantiation (hd 2 / 6 / 16, 64, 128), at r = 1, an odd r inside and r = hd, grouped and MHA,
bf16 and widened fp32 weights, with padded leading dimensions, at degenerate spectra, and at every argument check.

Metrics, all evaluated on the host in long double on the device's FP64 outputs (M = C + rho I; tv, to: the long-double factors):
  W  max_g max |v_g M v_g^T - I_r|                                                      (needs no gap)
  P  max_h max |o_h v_g - to_h tv_g| / max |to_h tv_g|                                   (relative gap at r >= 1e-3 asserted on the model)
  F  component a signed by <v_g[a], tv_g[a]>: max_a max |s_a v_g[a] - tv_g[a]| / max |tv_g[a]|, likewise the columns of o_h
                                                                                        (every relative gap of lam[:r + 1] >= 1e-3 asserted)
  L  MHA: max |o_h^T o_h - diag(lam2[:r])| / lam2[0]
Criterion (that of tests/test_gpu_vo_error.py): err_kernel / max(err_cpu, 64 (d + hd + r) 2^-53) <= R, err_cpu the same metric on
VO.factors of the fp64 model against the same long-double truth; one R per metric, 4 x the largest ratio observed on an MI355X rounded
up to a power of two, never above 32.  Every test prints `FACTORS <case> <metric> err_kernel err_cpu ratio` before it asserts.  Nothing
is measured against the kernel itself: the bit-for-bit tests (nesting, leading dimensions) compare two calls that must agree exactly.

MEASURED on an MI355X: the block at the constants R_W .. R_B below (largest ratio per metric, and the R chosen).
"""
import functools

import numpy as np
import pytest
import torch

from tests import vo_error_model as VO
from tests.output_error_model import LD, wide
from tests.test_gpu_chol import matrix

pytestmark = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -53
RIDGE = 1e-5
GAP = 1e-3
H11, H22, H42, H31, H41 = (1, 1), (2, 2), (4, 2), (3, 1), (4, 1)

# MEASURED on an MI355X: the largest ratio err_kernel / max(err_cpu, 64 (d + hd + r) u) per metric over every FACTORS line of this
# file (23 W, 23 P, 22 F, 8 L, 13 S, 11 B), and R = 4 x that, rounded up to a power of two:
#   W  3.49e-1  acts d=70 4/1 hd=128 r=70 (hd > d): err_kernel 6.6e-13, err_cpu 1.3e-12; every other case 3e-4 .. 2e-2    -> 2
#   P  3.85e-2  the same case: err_kernel 7.3e-14, err_cpu 1.2e-13; elsewhere 5e-4 .. 2.2e-2                               -> 2^-2
#   F  5.94e-1  the same case: err_kernel 2.0e-12, err_cpu 3.4e-12 (above the floor); hd = 128 elsewhere 1.6e-2 .. 2.2e-1  -> 4
#   L  3.52e-2  p3 d=70 2/2 hd=64 r=1: err_kernel 3.4e-14, err_cpu 3.7e-14                                                 -> 2^-2
#   S  2.61e-2  p3 d=70 2/2 hd=64 r=64 (MHA, lam2): err_kernel 3.7e-14, err_cpu 3.8e-14                                    -> 2^-3
#   B  4.44e-4  acts d=70 4/2 hd=16 r=11 fp32 weights: 2.2e-16 of the bound (one or two ulp everywhere)                    -> 2^-9
# err_kernel and err_cpu agree within a factor of two or so in every line: both carry the same eigenvector sensitivity, and outside
# the hd > d case and F at hd >= 64 the floor decides.  The nesting test holds bit for bit (no GEMM path depends on the rank).
R_W = 2.0
R_P = 2.0 ** -2
R_F = 4.0
R_L = 2.0 ** -2
R_S = 2.0 ** -3       # mdg_vo_spectrum: out[0], [1], [3], [6], [7]
R_B = 2.0 ** -9       # mdg_vo_spectrum: the Weyl bound, relative, in units of 64 d u


# ---------------------------------------------------------------- problems and their references (computed once, never modified)
@functools.lru_cache(maxsize=None)
def problem(kind, d, n_heads, n_kv, hd, wdt, grade, dead=None):
    """(C, W_v, W_o) on the host.  dead = (kv head, row): that row of W_v is exactly zero."""
    Wv, Wo = VO.weights(d, n_heads, n_kv, hd, wdt, seed=len(kind), grade=grade)
    if dead is not None:
        Wv = Wv.clone()
        Wv[dead[0] * hd + dead[1]] = 0
    return matrix(kind, d)[0], Wv, Wo


@functools.lru_cache(maxsize=None)
def spectra(key, ridge, dtype):
    kind, d, n_heads, n_kv, hd = key[:5]
    C, Wv, Wo = problem(*key)
    return VO.spectra(C, ridge, Wv, Wo, n_heads, n_kv, hd, dtype)


@functools.lru_cache(maxsize=None)
def model_factors(key, r, ridge, dtype):
    kind, d, n_heads, n_kv, hd = key[:5]
    C, Wv, Wo = problem(*key)
    return VO.factors(spectra(key, ridge, dtype), Wv, Wo, n_heads, n_kv, hd, r, dtype)


def gaps_hold(key, r, ridge, metric):
    """The gap the metric needs, on the long-double model (P: the relative gap at r; F: every gap of lam[:r + 1]; lam2 too for MHA)."""
    for lam, _, lam2, _ in spectra(key, ridge, LD):
        if metric == "P":
            if VO.relative_gap_at(lam if lam2 is None else lam2, r) < GAP:
                return False
        elif metric == "F":
            if VO.min_relative_gap(lam[:r + 1]) < GAP or (lam2 is not None and VO.min_relative_gap(lam2[:r + 1]) < GAP):
                return False
    return True


def metric_values(key, r, ridge, v, o, metric, keep=None):
    kind, d, n_heads, n_kv, hd = key[:5]
    C = problem(*key)[0]
    if metric == "W":
        return VO.whitening_error(C, ridge, v, n_kv, r, keep)
    if metric == "L":
        return VO.mha_gram_error(o, spectra(key, ridge, LD), n_heads, r)
    tv, to = model_factors(key, r, ridge, LD)
    fn = VO.head_map_error if metric == "P" else VO.signed_factor_error
    return fn(v, o, tv, to, n_heads, n_kv, r)


RATIOS = {"W": R_W, "P": R_P, "F": R_F, "L": R_L}


def report(case, metric, err, err_cpu, size):
    ratio = err / max(err_cpu, 64 * size * U)
    print("FACTORS %-58s %s err_kernel %.3e err_cpu %.3e ratio %.2e" % (case, metric, err, err_cpu, ratio))
    return ratio


def check_metrics(case, key, r, ridge, v64, o64, metrics, need_gaps=True, keep=None):
    """Every metric of `metrics` on the device's fp64 factors against the fp64 model's; prints, then asserts.  need_gaps False: P and
    F are checked only where their gap holds on the model (the degenerate cases)."""
    kind, d, n_heads, n_kv, hd = key[:5]
    done, failed = [], []
    for m in metrics:
        if m in "PF":
            if need_gaps:
                assert gaps_hold(key, r, ridge, m), "%s: the model lost the gap %s needs" % (case, m)
            elif not gaps_hold(key, r, ridge, m):
                continue
        cv, co = model_factors(key, r, ridge, np.float64)
        err = metric_values(key, r, ridge, v64, o64, m, keep)
        err_cpu = metric_values(key, r, ridge, cv, co, m, keep)
        ratio = report(case, m, err, err_cpu, d + hd + r)
        done.append(m)
        if not ratio <= RATIOS[m]:
            failed.append("%s ratio %.3g > %g" % (m, ratio, RATIOS[m]))
    assert not failed, "%s: %s" % (case, "; ".join(failed))
    return done


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def device_factors(key, r, ridge):
    """(v bf16, o bf16, v_f64, o_f64) of ops.vo_compress, computed once per case, never modified."""
    from modegpt_amd import ops
    kind, d, n_heads, n_kv, hd = key[:5]
    C, Wv, Wo = problem(*key)
    return ops.vo_compress(C.to("cuda:0"), Wv.to("cuda:0"), Wo.to("cuda:0"), n_heads, n_kv, hd, r, ridge, want_f64=True)


def name_of(key, r):
    kind, d, (n_heads, n_kv), hd, wdt = key[0], key[1], key[2:4], key[4], key[5]
    return "%s d=%d %d/%d hd=%d r=%d %s" % (kind, d, n_heads, n_kv, hd, r, str(wdt)[6:])


# ---------------------------------------------------------------- 1. accuracy
# (hd, r, d, heads, kind, weight dtype, grade): the three syevj instantiations (run-time n: 2, 6, 16; 64; 128), r = 1 / odd inside / hd
# for each of hd 16, 64, 128, grouped 4/2, 3/1, 4/1 and MHA 1/1, 2/2, bf16 and fp32 (widened to fp64) weights, d in {1, 70, 257, 384}.
# hd = 128 only with n_heads <= 4 and d <= 384, d = 384 with at most two kv heads: the long-double model stays within seconds per problem,
# and the cases of one problem share its decomposition.
CASES = [
    (2, 1, 1, H11, "p3", BF16, 0.5), (2, 2, 70, H42, "acts", F32, 0.5),
    (6, 5, 257, H31, "p6g3", F32, 0.7),
    (16, 1, 70, H42, "acts", BF16, 0.8), (16, 11, 70, H42, "acts", BF16, 0.8), (16, 16, 70, H42, "acts", BF16, 0.8),
    (16, 11, 70, H22, "p6g3", F32, 0.8), (16, 16, 70, H41, "p3", F32, 0.8),
    (64, 1, 70, H22, "p3", BF16, 0.93), (64, 41, 70, H22, "p3", BF16, 0.93), (64, 64, 384, H42, "acts", BF16, 0.93),
    (128, 1, 257, H31, "acts", BF16, 0.96), (128, 87, 257, H31, "acts", BF16, 0.96), (128, 128, 257, H31, "acts", BF16, 0.96),
    (128, 87, 257, H22, "p3", BF16, 0.96),
]


def case_key(hd, r, d, heads, kind, wdt, grade, dead=None):
    return (kind, d, heads[0], heads[1], hd, wdt, grade, dead)


def case_id(c):
    hd, r, d, h, kind, wdt, grade = c
    return "hd%d-r%d-d%d-h%dkv%d-%s-%s" % (hd, r, d, h[0], h[1], kind, str(wdt)[6:])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_factors_against_long_double(dev, case):
    hd, r, d, (n_heads, n_kv), kind, wdt, grade = case
    key = case_key(*case)
    v, o, v64, o64 = device_factors(key, r, RIDGE)
    assert v.shape == v64.shape == (n_kv * r, d) and o.shape == o64.shape == (d, n_heads * r)
    assert v.dtype == o.dtype == BF16 and v64.dtype == o64.dtype == F64
    assert all(bool(torch.isfinite(t).all()) for t in (v, o, v64, o64))
    assert torch.equal(v, v64.to(BF16)) and torch.equal(o, o64.to(BF16))         # the stored tensors: the casts of exactly these values
    check_metrics(name_of(key, r), key, r, RIDGE, v64.cpu(), o64.cpu(), "WPFL" if n_heads == n_kv else "WPF")


# ---------------------------------------------------------------- 2. degenerate spectra
def test_head_dim_above_d(dev):
    """hd = 128 > d = 70: G has rank 70 and 58 eigenvalues that are rounding noise of either sign; r = 70 keeps all of the range."""
    hd, r, d, heads = 128, 70, 70, H41
    key = case_key(hd, r, d, heads, "acts", BF16, 0.96)
    v, o, v64, o64 = device_factors(key, r, RIDGE)
    assert all(bool(torch.isfinite(t).all()) for t in (v, o, v64, o64))
    assert torch.equal(v, v64.to(BF16)) and torch.equal(o, o64.to(BF16))
    done = check_metrics(name_of(key, r) + " hd>d", key, r, RIDGE, v64.cpu(), o64.cpu(), "WPF", need_gaps=False)
    assert "W" in done
    # and a rank beyond the range of G: nothing may be NaN or Inf (the clamp and the s > 0 branch)
    for t in device_factors(key, hd, RIDGE):
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("heads", [H42, H22], ids=["grouped", "mha"])
def test_dead_value_channel(dev, heads):
    """Row 5 of kv head 1's W_v is exactly zero, r = hd: G has a zero row and column, the eigensolver never rotates it, its eigenvalue
    is exactly 0 and sorts last.  Grouped: 1 / s is not formed, the component is exactly zero in v and in every o_h of the group."""
    hd, d = 16, 70
    n_heads, n_kv = heads
    r, group = hd, n_heads // n_kv
    key = case_key(hd, r, d, heads, "acts", BF16, 0.8, dead=(1, 5))
    assert spectra(key, RIDGE, LD)[1][0][-1] == 0 and spectra(key, RIDGE, LD)[1][0][-2] > 0
    v, o, v64, o64 = device_factors(key, r, RIDGE)
    assert all(bool(torch.isfinite(t).all()) for t in (v, o, v64, o64))
    assert torch.equal(v, v64.to(BF16)) and torch.equal(o, o64.to(BF16))
    if n_heads != n_kv:
        assert bool((v64[1 * r + r - 1] == 0).all()) and bool((v[1 * r + r - 1] == 0).all())
        for h in range(group, 2 * group):
            assert bool((o64[:, h * r + r - 1] == 0).all()) and bool((o[:, h * r + r - 1] == 0).all())
        assert bool((v64[r - 1] != 0).any()) and bool((o64[:, r - 1] != 0).any())                  # kv head 0 is alive
        check_metrics(name_of(key, r) + " dead r-1", key, r - 1, RIDGE, v64.cpu().view(n_kv, r, d)[:, :r - 1].reshape(-1, d),
                      o64.cpu().view(d, n_heads, r)[:, :, :r - 1].reshape(d, -1), "W")
        # (the rank r - 1 model of the same problem: its fp64 factors are the yardstick of the remaining components)
    else:
        check_metrics(name_of(key, r) + " dead", key, r, RIDGE, v64.cpu(), o64.cpu(), "P")


@pytest.mark.parametrize("heads,kind", [(H42, "acts"), (H22, "acts")], ids=["grouped", "mha"])
def test_zero_ridge(dev, heads, kind):
    hd, r, d = 16, 11, 70
    key = case_key(hd, r, d, heads, kind, BF16, 0.8)
    v, o, v64, o64 = device_factors(key, r, 0.0)
    assert torch.equal(v, v64.to(BF16)) and torch.equal(o, o64.to(BF16))
    check_metrics(name_of(key, r) + " ridge=0", key, r, 0.0, v64.cpu(), o64.cpu(), "WPFL" if heads[0] == heads[1] else "WPF")
    _, _, v64r, o64r = device_factors(key, r, RIDGE)
    assert not same(v64, v64r)                                                   # (the ridge is in the factors)


# ---------------------------------------------------------------- 3. nesting
@pytest.mark.parametrize("hd,r,d,heads,kind,wdt,grade", [(16, 11, 70, H42, "acts", BF16, 0.8), (16, 11, 70, H22, "p6g3", F32, 0.8),
                                                         (128, 87, 257, H31, "acts", BF16, 0.96), (128, 87, 257, H22, "p3", BF16, 0.96)],
                         ids=["grouped-hd16", "mha-hd16", "grouped-hd128", "mha-hd128"])
def test_rank_r_is_a_prefix_of_rank_hd(dev, hd, r, d, heads, kind, wdt, grade):
    """P and Q do not depend on r beyond their stride and the GEMM sums k in a fixed order per entry: the factors of rank r are the
    first r components of the factors of rank hd, bit for bit."""
    n_heads, n_kv = heads
    key = case_key(hd, r, d, heads, kind, wdt, grade)
    _, _, v_r, o_r = device_factors(key, r, RIDGE)
    _, _, v_f, o_f = device_factors(key, hd, RIDGE)
    for g in range(n_kv):
        assert same(v_r[g * r:(g + 1) * r], v_f[g * hd:g * hd + r]), "v, kv head %d" % g
    for h in range(n_heads):
        assert same(o_r[:, h * r:(h + 1) * r], o_f[:, h * hd:h * hd + r]), "o, head %d" % h


# ---------------------------------------------------------------- the C ABI directly
GUARD_ROWS = 2
FILL = -7.0


def padded(A, fill, dev, pad):
    """A in the top-left corner of a buffer GUARD_ROWS taller and `pad` columns wider, filled with `fill`: (buffer, view)."""
    buf = torch.full((A.shape[0] + GUARD_ROWS, A.shape[1] + pad), fill, dtype=A.dtype, device=dev)
    buf[:A.shape[0], :A.shape[1]] = A.to(dev)
    return buf, buf[:A.shape[0], :A.shape[1]]


def padding_intact(buf, view, before):
    """Everything of buf outside view holds the bits of `before`."""
    now = buf.clone()
    now[:view.shape[0], :view.shape[1]] = before[:view.shape[0], :view.shape[1]]
    return torch.equal(bits(now), bits(before))


class RawCall:
    """One problem's buffers for mdg_vo_compress / mdg_vo_spectrum through the C ABI.  Inputs sit in NaN-filled buffers, outputs in
    buffers filled with FILL, every one `pad` columns wider than its matrix (v_f64 / o_f64 have no leading dimension: rows only) and
    GUARD_ROWS taller; the workspace is filled with 0xAB bytes."""

    def __init__(self, dev, key, r, pad, f64_weights=False):
        from modegpt_amd import _lib
        self.lib, self._lib, self.dev = _lib.load(), _lib, dev
        kind, d, n_heads, n_kv, hd = key[:5]
        C, Wv, Wo = problem(*key)
        if f64_weights or Wv.dtype != BF16:
            Wv, Wo = Wv.double(), Wo.double()
        self.code = _lib.MDG_BF16 if Wv.dtype == BF16 else _lib.MDG_F64
        nan = float("nan")
        self.shape = (d, n_heads, n_kv, hd, r)
        self.inputs = [padded(t, nan, dev, pad) for t in (C, Wv, Wo)]
        empty = lambda rows, cols, dt: torch.zeros(rows, cols, dtype=dt)                     # noqa: E731
        self.outputs = [padded(empty(n_kv * r, d, BF16), FILL, dev, pad), padded(empty(d, n_heads * r, BF16), FILL, dev, pad),
                        padded(empty(n_kv * r, d, F64), FILL, dev, 0), padded(empty(d, n_heads * r, F64), FILL, dev, 0)]
        for buf, view in self.outputs:
            buf.fill_(FILL)
        self.spec = torch.full((n_kv + GUARD_ROWS, 8), FILL, dtype=F64, device=dev)
        self.nbytes = self.lib.mdg_vo_compress_ws_bytes(d, n_heads, n_kv, hd)
        self.ws = torch.full((self.nbytes,), 0xAB, dtype=torch.uint8, device=dev)
        self.before = [b.clone() for b, _ in self.inputs + self.outputs]

    def args(self, ridge):
        d, n_heads, n_kv, hd, r = self.shape
        (C, _), (Wv, _), (Wo, _) = self.inputs
        (v, _), (o, _), (v64, _), (o64, _) = self.outputs
        return dict(cov_x=C.data_ptr(), d=d, ldc=C.stride(0), Wv=Wv.data_ptr(), ld_wv=Wv.stride(0), Wo=Wo.data_ptr(), ld_wo=Wo.stride(0),
                    w_dtype=self.code, n_heads=n_heads, n_kv=n_kv, hd=hd, rank=r, ridge=ridge, v_out=v.data_ptr(), ld_v=v.stride(0),
                    o_out=o.data_ptr(), ld_o=o.stride(0), v_f64=v64.data_ptr(), o_f64=o64.data_ptr(), ws=self.ws.data_ptr(),
                    ws_bytes=self.nbytes, stream=None)

    def compress(self, ridge=RIDGE, **override):
        a = self.args(ridge)
        a.update(override)
        with torch.cuda.device(self.dev):
            a["stream"] = torch.cuda.current_stream(self.dev).cuda_stream
            rc = self.lib.mdg_vo_compress(*a.values())
        torch.cuda.synchronize(self.dev)
        return rc

    def spectrum(self, ridge=RIDGE, eps=0.0, **override):
        a = self.args(ridge)
        a = dict(ws=a["ws"], ws_bytes=a["ws_bytes"], cov_x=a["cov_x"], d=a["d"], ldc=a["ldc"], Wv=a["Wv"], ld_wv=a["ld_wv"],
                 w_dtype=a["w_dtype"], n_heads=a["n_heads"], n_kv=a["n_kv"], hd=a["hd"], rank=a["rank"], ridge=ridge, eps=eps,
                 out=self.spec.data_ptr(), stream=None)
        a.update(override)
        with torch.cuda.device(self.dev):
            a["stream"] = torch.cuda.current_stream(self.dev).cuda_stream
            rc = self.lib.mdg_vo_spectrum(*a.values())
        torch.cuda.synchronize(self.dev)
        return rc

    def views(self):
        return [view for _, view in self.outputs]

    def intact(self):
        """The inputs and the padding of every output are what they were."""
        ok = all(torch.equal(bits(b), bits(b0)) for (b, _), b0 in zip(self.inputs, self.before[:3]))
        return ok and all(padding_intact(b, view, b0) for (b, view), b0 in zip(self.outputs, self.before[3:]))

    def untouched(self):
        """Nothing was launched: every output and the workspace still hold their fill."""
        torch.cuda.synchronize(self.dev)
        return (all(bool((b == FILL).all()) for b, _ in self.outputs) and bool((self.spec == FILL).all())
                and bool((self.ws == 0xAB).all()))


LD_CASES = [(16, 11, 70, H42, "acts", 0.8, False), (16, 11, 70, H42, "acts", 0.8, True), (16, 11, 70, H22, "p6g3", 0.8, False),
            (16, 11, 70, H22, "p6g3", 0.8, True)]
LD_IDS = ["grouped-bf16", "grouped-f64", "mha-bf16", "mha-f64"]


# ---------------------------------------------------------------- 4. leading dimensions and containment
@pytest.mark.parametrize("hd,r,d,heads,kind,grade,f64w", LD_CASES, ids=LD_IDS)
def test_leading_dimensions_plus_8(dev, hd, r, d, heads, kind, grade, f64w):
    """Every leading dimension + 8 (NaN beside the inputs, FILL beside the outputs): no alignment predicate of the GEMM changes, so
    the results are the bits of the contiguous call; the padding is intact bit for bit."""
    from modegpt_amd import _lib
    key = case_key(hd, r, d, heads, kind, BF16, grade)
    plain, wide_ = RawCall(dev, key, r, 0, f64w), RawCall(dev, key, r, 8, f64w)
    assert plain.compress() == _lib.MDG_OK and wide_.compress() == _lib.MDG_OK
    assert wide_.args(RIDGE)["ld_o"] == heads[0] * r + 8 and wide_.args(RIDGE)["ldc"] == d + 8
    for a, b in zip(plain.views(), wide_.views()):
        assert bool(torch.isfinite(a).all()) and same(a, b)
    assert plain.intact() and wide_.intact()
    if not f64w:                                                                  # and the front end gives the raw call
        for a, b in zip(plain.views(), device_factors(key, r, RIDGE)):
            assert same(a, b)


@pytest.mark.parametrize("hd,r,d,heads,kind,grade,f64w", LD_CASES, ids=LD_IDS)
def test_leading_dimensions_plus_3(dev, hd, r, d, heads, kind, grade, f64w):
    """Every leading dimension + 3: every GEMM on its general path.  The metrics of the accuracy test, the bf16 outputs the casts of
    the fp64 ones, the padding intact."""
    from modegpt_amd import _lib
    key = case_key(hd, r, d, heads, kind, BF16, grade)
    call = RawCall(dev, key, r, 3, f64w)
    assert call.compress() == _lib.MDG_OK
    v, o, v64, o64 = call.views()
    assert all(bool(torch.isfinite(t).all()) for t in (v, o, v64, o64))
    assert torch.equal(v, v64.to(BF16)) and torch.equal(o, o64.to(BF16))
    assert call.intact()
    check_metrics(name_of(key, r) + " ld+3" + (" f64w" if f64w else ""), key, r, RIDGE, v64.cpu(), o64.cpu(),
                  "WPFL" if heads[0] == heads[1] else "WPF")


def test_poisoned_statistic_is_reported_and_contained(dev):
    """sigma_x with one NaN row and column (tests/test_gpu_eigh.poisoned's nan_row_col): MDG_ERR_NO_CONVERGE naming the non-finite
    input, every access in bounds.  Nothing is asserted about the outputs."""
    from modegpt_amd import _lib
    hd, r, d, heads = 16, 11, 70, H42
    key = case_key(hd, r, d, heads, "acts", BF16, 0.8)
    call = RawCall(dev, key, r, 3)
    C = call.inputs[0][1]
    i = d // 2 + 1
    C[i, :] = float("nan")
    C[:, i] = float("nan")
    call.before[0] = call.inputs[0][0].clone()
    assert call.compress() == _lib.MDG_ERR_NO_CONVERGE
    assert b"non-finite" in call.lib.mdg_last_error()
    assert call.intact()
    good = RawCall(dev, key, r, 3)                                                # and a good call passes afterwards
    assert good.compress() == _lib.MDG_OK and bool(torch.isfinite(good.views()[2]).all())


# ---------------------------------------------------------------- 5. mdg_vo_spectrum
EPS = 2.0 ** -20


def check_spectrum(case, key, r, rows, eps=EPS, diag_of=None):
    """rows: the device's [n_kv, 8] (host).  out[0], [1], [3], [6], [7] against the long-double spectrum by the criterion (relative to
    lam_1; [3] to 1), the Weyl bound to R_B 64 d u relative, [2] and [5] evaluated on the device's own out[0], out[1], out[4]."""
    kind, d, n_heads, n_kv, hd = key[:5]
    C, Wv, Wo = problem(*key)
    grouped = n_heads != n_kv
    rows = rows.numpy()
    assert rows.shape == (n_kv, 8)
    err = err_cpu = 0.0
    for g, (spec, spec64) in enumerate(zip(spectra(key, RIDGE, LD), spectra(key, RIDGE, np.float64))):
        lam, lam64 = (spec[0], spec64[0]) if grouped else (spec[2], spec64[2])
        nxt = lambda l: l[r] if r < hd else l.dtype.type(0)                       # noqa: E731
        share = lambda l: l[:r].sum() / l.sum()                                    # noqa: E731
        want = [lam[r - 1], nxt(lam), lam[0], lam[hd - 1]]
        got = wide(rows[g, [0, 1, 6, 7]])
        cpu = wide(np.array([lam64[r - 1], nxt(lam64), lam64[0], lam64[hd - 1]]))
        err = max(err, float(np.abs(got - want).max() / lam[0]), float(abs(LD(rows[g, 3]) - share(lam))))
        err_cpu = max(err_cpu, float(np.abs(cpu - want).max() / lam[0]), float(abs(LD(share(lam64)) - share(lam))))
        l_r, l_next = rows[g, 0], rows[g, 1]
        s_r, s_next = np.sqrt(max(l_r, 0.0)), np.sqrt(max(l_next, 0.0))
        assert abs(rows[g, 2] - ((s_r - s_next) / s_r if s_r > 0 else 0.0)) <= 4 * U
        if r == hd:
            assert rows[g, 1].tobytes() == np.float64(0.0).tobytes()              # +0.0 bit for bit
            assert rows[g, 2] == 1.0 or not l_r > 0
        if grouped:
            assert rows[g, 5] == (1.0 if l_r - l_next > 2.0 * rows[g, 4] else 0.0)
        else:
            assert np.isnan(rows[g, 4]) and np.isnan(rows[g, 5])
    ratio = report(case, "S", err, err_cpu, d + hd + r)
    failed = [] if ratio <= R_S else ["S ratio %.3g > %g" % (ratio, R_S)]
    if grouped:
        want_b = VO.weyl_bound(problem(*key)[0] if diag_of is None else diag_of, Wv, n_kv, hd, eps)
        rel = float((np.abs(wide(rows[:, 4]) - want_b) / want_b).max())
        ratio_b = rel / (64 * d * U)
        print("FACTORS %-58s B rel_err %.3e of the bound, in units of 64 d u: ratio %.2e" % (case, rel, ratio_b))
        assert bool((rows[:, 4] > 0).all())
        if not ratio_b <= R_B:
            failed.append("B ratio %.3g > %g" % (ratio_b, R_B))
    assert not failed, "%s: %s" % (case, "; ".join(failed))


def run_spectrum(dev, key, r, eps=EPS, wv_view=None, c_view=None, spectrum_cov=None):
    from modegpt_amd import ops
    kind, d, n_heads, n_kv, hd = key[:5]
    C, Wv, Wo = problem(*key)
    Cd = C.to(dev) if c_view is None else c_view
    Wvd = Wv.to(dev) if wv_view is None else wv_view
    out = ops.vo_compress(Cd, Wvd, Wo.to(dev), n_heads, n_kv, hd, r, RIDGE, want_spectrum=True, spectrum_eps=eps, spectrum_cov=spectrum_cov)
    torch.cuda.synchronize(dev)
    return out[-1].cpu()


# (hd, r, d, heads, kind, dtype, grade): the scalar path (fp64 and bf16 weights, d = 70), hd = 128 (scalar: d = 257) and hd = 2 on the
# vector path, rank == hd, MHA
SPECTRUM_CASES = [(16, 11, 70, H42, "acts", F32, 0.8), (16, 11, 70, H42, "acts", BF16, 0.8), (128, 87, 257, H31, "acts", BF16, 0.96),
                  (2, 1, 72, H42, "p3", BF16, 0.5), (16, 16, 70, H42, "acts", BF16, 0.8), (128, 128, 257, H31, "acts", BF16, 0.96),
                  (16, 11, 70, H22, "p6g3", F32, 0.8), (64, 64, 70, H22, "p3", BF16, 0.93)]


@pytest.mark.parametrize("case", SPECTRUM_CASES, ids=case_id)
def test_spectrum_against_long_double(dev, case):
    hd, r, d, heads, kind, wdt, grade = case
    key = case_key(*case)
    check_spectrum(name_of(key, r) + " spectrum", key, r, run_spectrum(dev, key, r))


@pytest.mark.parametrize("how", ["vector", "scalar-f64", "scalar-misaligned"])
def test_spectrum_across_the_chunk_boundary(dev, how):
    """d = 2120 > 2048: two chunks of the staged diagonal, the second 72 columns long.  bf16 on the 16-byte path, fp32 weights (the
    fp64 kernel) and a bf16 W_v one element off the 16-byte boundary on the scalar path."""
    hd, r, d, heads = 16, 11, 2120, (2, 1)
    key = case_key(hd, r, d, heads, "acts", F32 if how == "scalar-f64" else BF16, 0.8)
    view = None
    if how == "scalar-misaligned":
        Wv = problem(*key)[1]
        buf = torch.full((Wv.shape[0], d + 8), float("nan"), dtype=BF16, device=dev)
        view = buf[:, 1:1 + d]
        view.copy_(Wv)
        assert view.data_ptr() % 16 == 2
    check_spectrum(name_of(key, r) + " " + how, key, r, run_spectrum(dev, key, r, wv_view=view))


def test_spectrum_padded_and_with_its_own_diagonal(dev):
    """ldc and ld_wv padded with NaN (through the C ABI: the guards of `out` too), and spectrum_cov with a diagonal of its own."""
    from modegpt_amd import _lib
    hd, r, d, heads = 16, 11, 70, H42
    key = case_key(hd, r, d, heads, "acts", BF16, 0.8)
    call = RawCall(dev, key, r, 3)
    assert call.compress() == _lib.MDG_OK and call.spectrum(eps=EPS) == _lib.MDG_OK
    assert bool((call.spec[heads[1]:] == FILL).all()) and call.intact()
    check_spectrum(name_of(key, r) + " padded", key, r, call.spec[:heads[1]].cpu())
    wide_ = RawCall(dev, key, r, 8)                                               # (+ 8: the vector path is out at d = 70 either way)
    assert wide_.compress() == _lib.MDG_OK and wide_.spectrum(eps=EPS) == _lib.MDG_OK
    assert same(wide_.spec, call.spec)
    other = matrix("p3", d)[0]
    rows = run_spectrum(dev, key, r, spectrum_cov=other.to(dev))
    assert not np.array_equal(rows[:, 4].numpy(), call.spec[:heads[1], 4].cpu().numpy())
    check_spectrum(name_of(key, r) + " spectrum_cov", key, r, rows, diag_of=other)
    zero = run_spectrum(dev, key, r, eps=0.0)
    assert bool((bits(zero[:, 4]) == 0).all()) and bool((zero[:, 5] == 1.0).all())  # eps = 0: the gap alone


# ---------------------------------------------------------------- 6. argument checks
def test_bad_arguments_of_vo_compress(dev):
    from modegpt_amd import _lib
    hd, r, d, (n_heads, n_kv) = 16, 11, 70, H42
    key = case_key(hd, r, d, H42, "p3", BF16, 0.8)
    call = RawCall(dev, key, r, 0)
    bad = [(dict(hd=15), b"head layout"), (dict(hd=130), b"head layout"), (dict(hd=0), b"head layout"), (dict(rank=0), b"rank"),
           (dict(rank=hd + 1), b"rank"), (dict(n_kv=3), b"head layout"), (dict(n_kv=0), b"head layout"),
           (dict(w_dtype=_lib.MDG_F16), b"bf16 or f64"), (dict(w_dtype=_lib.MDG_F32), b"bf16 or f64"),
           (dict(ldc=d - 1), b"leading"), (dict(ld_wv=d - 1), b"leading"), (dict(ld_wo=n_heads * hd - 1), b"leading"),
           (dict(ld_v=d - 1), b"leading"), (dict(ld_o=n_heads * r - 1), b"leading"), (dict(d=0), b"leading"),
           (dict(ws_bytes=call.nbytes - 1), b"workspace"), (dict(ws=None), b"workspace"),
           (dict(cov_x=None), b"null"), (dict(Wv=None), b"null"), (dict(Wo=None), b"null"), (dict(v_out=None), b"null"),
           (dict(o_out=None), b"null")]
    for kw, msg in bad:
        assert call.compress(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        assert msg in call.lib.mdg_last_error(), (kw, call.lib.mdg_last_error())
        with pytest.raises(RuntimeError):
            _lib.check(call.compress(**kw), "mdg_vo_compress")
    assert call.untouched()                                                       # nothing was enqueued
    assert call.compress(v_f64=None, o_f64=None) == _lib.MDG_OK                   # the fp64 outputs are optional
    v, o, v64, o64 = call.views()
    assert bool(torch.isfinite(v).all()) and bool((v64 == FILL).all()) and bool((o64 == FILL).all())
    assert same(v, device_factors(key, r, RIDGE)[0]) and same(o, device_factors(key, r, RIDGE)[1])


def test_bad_arguments_of_vo_spectrum(dev):
    from modegpt_amd import _lib
    hd, r, d, (n_heads, n_kv) = 16, 11, 70, H42
    key = case_key(hd, r, d, H42, "p3", BF16, 0.8)
    call = RawCall(dev, key, r, 0)
    bad = [(dict(hd=15), b"head layout"), (dict(hd=130), b"head layout"), (dict(hd=0), b"head layout"), (dict(rank=0), b"rank"),
           (dict(rank=hd + 1), b"rank"), (dict(n_kv=3), b"head layout"), (dict(n_kv=0), b"head layout"),
           (dict(w_dtype=_lib.MDG_F16), b"bf16 or f64"), (dict(w_dtype=_lib.MDG_F32), b"bf16 or f64"),
           (dict(ldc=d - 1), b"leading"), (dict(ld_wv=d - 1), b"leading"), (dict(d=0), b"leading"),
           (dict(ws_bytes=call.nbytes - 1), b"workspace"), (dict(ws=None), b"workspace"),
           (dict(cov_x=None), b"null"), (dict(Wv=None), b"null"), (dict(out=None), b"null"),
           (dict(eps=-1e-30), b"error bound"), (dict(eps=float("nan")), b"error bound"), (dict(ridge=float("nan")), b"ridge")]
    for kw, msg in bad:
        assert call.spectrum(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        assert msg in call.lib.mdg_last_error(), (kw, call.lib.mdg_last_error())
        with pytest.raises(RuntimeError):
            _lib.check(call.spectrum(**kw), "mdg_vo_spectrum")
    assert call.untouched()
    assert call.compress() == _lib.MDG_OK and call.spectrum(eps=EPS) == _lib.MDG_OK
    assert bool(torch.isfinite(call.spec[:n_kv]).all()) and bool((call.spec[n_kv:] == FILL).all())
