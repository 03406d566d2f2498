"""fp16 activations and ReLU-on-load on the int8 digit-plane covariance (MDG_I8_F16 / MDG_I8_RELU; csrc/cov_i8.hpp F16Elem): the
exact route against exact integer arithmetic, the truncated product against its own bound, the int32 fold interval on the worst
element the enumeration found (scripts/probes/i8_int32_bound_f16.py), Inf / NaN columns, the ReLU flag for both element types,
the fused launch, the dispatch of ops.cov_accum_multi, and OPT's fc1 hook.  Every GPU step runs once.
"""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import modegpt_oracle as O
from tests.i8_limits import REFERENCE_ROUNDING, check_i8_error

pytestmark = pytest.mark.gpu
F64, F16, BF16 = torch.float64, torch.float16, torch.bfloat16
EXACT_ROUNDING = 5e-15          # include/modegpt_hip.h MDG_I8_EXACT_ROUNDING


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def families(gen, T, n):
    c = torch.exp(torch.empty(n).uniform_(math.log(0.05), math.log(2.0), generator=gen))
    z = lambda: torch.randn(T, n, generator=gen)       # noqa: E731
    t3 = z() / torch.sqrt((z() ** 2 + z() ** 2 + z() ** 2) / 3)
    return {"gaussian": z() * c, "relu": torch.relu(z()) * c, "cubed": z() ** 3 * c, "student_t": (t3 * c).clamp(-6e4, 6e4),
            "silu_gated": torch.nn.functional.silu(z()) * z() * c}


def entry_err(S, R):
    """max over the lower triangle of |S - R|_ij / sqrt(R_ii R_jj)."""
    d = torch.sqrt(torch.diagonal(R))
    d = torch.where(d > 0, d, torch.ones_like(d))
    return (torch.tril(S - R).abs() / (d[:, None] * d[None, :])).max().item()


def exact_sigma_units(X):
    """fp16 [T, n] (finite) -> [n][n] Python ints: X^T X in units of 2^-48, exactly (every fp16 value is a multiple of 2^-24)."""
    xi = np.round(np.ldexp(X.double().numpy(), 24)).astype(np.int64)
    assert (np.ldexp(xi.astype(np.float64), -24) == X.double().numpy()).all()
    A, B = xi >> 20, xi & ((1 << 20) - 1)                # xi = A 2^20 + B, |A| < 2^20, 0 <= B < 2^20: int64 products cannot overflow
    AA, AB, BB = A.T @ A, A.T @ B, B.T @ B
    n = X.shape[1]
    return [[(int(AA[i, j]) << 40) + ((int(AB[i, j]) + int(AB[j, i])) << 20) + int(BB[i, j]) for j in range(n)] for i in range(n)]


@pytest.mark.parametrize("family,T", [("gaussian", 900), ("silu_gated", 3000), ("extremes", 2500)])
def test_fp16_exact_route_against_exact_integer_arithmetic(ops, dev, monkeypatch, family, T):
    """MDG_I8_EXACT_ALWAYS on fp16 data against the exact integer sum: entry-wise error <= MDG_I8_EXACT_ROUNDING, the call says it
    was exact, and the bound it reports IS MDG_I8_EXACT_ROUNDING -- the rho term of an fp16 call is identically 0."""
    monkeypatch.setattr(ops, "I8_EXACT", True)
    gen = torch.Generator().manual_seed(11)
    n = 128
    if family == "extremes":        # columns mixing the largest fp16 value with 2^-24 subnormals (29 binades apart) on Gaussian columns
        X = (torch.randn(T, n, generator=gen) * 100).to(F16)
        X[::7, 0:8] = 65504.0
        X[1::7, 0:8] = 2.0 ** -24
        X[2::7, 0:8] = -3 * 2.0 ** -24
        X[5, 0:8] = -65504.0
    else:
        X = families(gen, T, n)[family].to(F16)
        X[3, 5], X[4, 5], X[6, 9] = 2.0 ** -24, -2.0 ** -14, 1023 * 2.0 ** -24       # subnormals among ordinary columns
    S = torch.zeros(n, n, dtype=F64, device=dev)
    info = {}
    planes = ops.cov_accum_i8(S, X.to(dev), route_info=info)
    print(f"[fp16 exact {family}] planes {planes} info {dict((k, v) for k, v in info.items() if k != 'stats')}")
    # (the route may hand heavy-tailed columns of the "extremes" set to the fp64 column kernel, as it does for bf16; the others stay)
    assert planes in (5, 6) and info["exact"] and (info["columns"] == [] or family == "extremes"), info
    assert info["bound"] == EXACT_ROUNDING and info["x"] == 0.0, info
    ex = exact_sigma_units(X)
    got = S.cpu()
    unit = Fraction(1, 1 << 48)
    diag = [math.sqrt(float(ex[i][i] * unit)) for i in range(n)]
    worst, worst_left, left = 0.0, 0.0, set(info["columns"])
    for i in range(n):
        for j in range(i + 1):
            e = abs(float(Fraction(got[i, j].item()) - ex[i][j] * unit)) / (diag[i] * diag[j])
            if i in left or j in left:
                worst_left = max(worst_left, e)
            else:
                worst = max(worst, e)
    print(f"[fp16 exact {family}] worst entry-wise error {worst:.3e}; rows / columns of the fp64 column kernel {worst_left:.3e}")
    assert worst <= EXACT_ROUNDING, worst
    # a column that left is a plain fp64 sum of T exact products: at most 2 T roundings of 2^-53 relative to sum |terms| <= sqrt(sigma_ii sigma_jj)
    assert worst_left <= 2 * T * 2.0 ** -53, worst_left


@pytest.mark.parametrize("family", ["gaussian", "relu", "cubed", "student_t", "silu_gated"])
def test_fp16_truncated_product_within_its_own_bound(ops, dev, monkeypatch, family):
    monkeypatch.setattr(ops, "I8_EXACT", False)
    gen = torch.Generator().manual_seed(23)
    T, n = 4096, 256
    X = families(gen, T, n)[family].to(F16)
    S = torch.zeros(n, n, dtype=F64, device=dev)
    info = {}
    planes = ops.cov_accum_i8(S, X.to(dev), route_info=info)
    R = torch.zeros(n, n, dtype=F64)
    O.cov_accum_tokens(R, X)
    if planes == 0:                  # the whole statistic went through the fp64 kernel: nothing of the int8 product to bound
        err = entry_err(S.cpu(), R)
        print(f"[fp16 truncated {family}] fp64 fallback, err {err:.3e}")
        assert err <= REFERENCE_ROUNDING
        return
    cols = info["columns"]
    err = entry_err(S.cpu(), R)
    print(f"[fp16 truncated {family}] planes {planes} columns {cols} bound {info['bound']:.3e} err {err:.3e}")
    assert not info["exact"]
    check_i8_error(err, bound=info["bound"], ctx=(family, info["planes"]))


def test_fp16_fold_interval_on_the_worst_element(ops, dev):
    """More tokens than one fold interval (2047 k-steps = 65504 tokens) and than 65535, every element the one whose digits the
    enumeration found worst -- (-3, -128, -128, 0, 0, 0): -1793 2^-10 four binades under its column's maximum, 32768 per token in
    class 3 -- below one row that sets that maximum (16).  sigma = 16^2 + (T - 1) v^2 exactly; a longer fold interval overflows int32."""
    T, n = 65504 + 2048 + 96, 128
    v, u = -1793 * 2.0 ** -10, 16.0
    X = torch.full((T, n), v, dtype=F16)
    X[0] = u
    assert X[1, 0].item() == v
    S = torch.zeros(n, n, dtype=F64, device=dev)
    info = {}
    planes = ops.cov_accum_i8(S, X.to(dev), route_info=info)
    want = u * u + (T - 1) * v * v
    got = torch.tril(S.cpu())
    print(f"[fp16 fold] planes {planes} exact {info['exact']} want {want!r} got min {got[got != 0].min().item()!r} max {got.max().item()!r}")
    assert planes in (5, 6)
    assert torch.equal(got, torch.tril(torch.full((n, n), want, dtype=F64)))


def _same_nonfinite(A, B):
    return torch.equal(torch.isnan(A), torch.isnan(B)) and torch.equal(torch.isinf(A) * torch.sign(A), torch.isinf(B) * torch.sign(B))


def test_fp16_inf_and_nan_columns_leave_for_the_column_kernel(ops, dev):
    gen = torch.Generator().manual_seed(5)
    T, n = 1024, 256
    X = torch.randn(T, n, generator=gen).to(F16)
    X[17, 3], X[100, 70], X[900, 130] = float("inf"), float("nan"), float("-inf")
    Xd = X.to(dev)
    S, R = torch.zeros(n, n, dtype=F64, device=dev), torch.zeros(n, n, dtype=F64, device=dev)
    info = {}
    planes = ops.cov_accum_i8(S, Xd, route_info=info)
    ops.cov_accum(R, Xd)
    print(f"[fp16 inf/nan] planes {planes} columns {info['columns']}")
    assert planes in (5, 6) and sorted(info["columns"]) == [3, 70, 130], info
    S, R = torch.tril(S).cpu(), torch.tril(R).cpu()
    assert _same_nonfinite(S, R)
    fin = torch.isfinite(R)
    out = torch.zeros(n, dtype=torch.bool)
    out[[3, 70, 130]] = True
    touched = out[:, None] | out[None, :]
    assert not torch.isfinite(R[touched & torch.tril(torch.ones(n, n, dtype=torch.bool))]).all()
    # the rows / columns of the columns that left: the column kernel's plain fp64 sums against the fp64 kernel's
    d = torch.sqrt(torch.diagonal(R).clamp_min(0))
    d = torch.where(torch.isfinite(d) & (d > 0), d, torch.ones_like(d))
    rel = ((S - R).abs() / (d[:, None] * d[None, :]))
    assert rel[fin & touched].max().item() <= REFERENCE_ROUNDING
    check_i8_error(rel[fin & ~touched].max().item(), bound=info["bound"])


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_relu_flag_matches_the_fp64_kernel(ops, dev, dtype):
    """MDG_I8_RELU for both element types, with a -0 and a sign-bit-set NaN in the input: the finite part equals
    ops.cov_accum(relu=True) within the call's bound; the NaN stays a NaN (torch.relu's semantics) and its column leaves."""
    gen = torch.Generator().manual_seed(31)
    T, n = 2048, 256
    X = (torch.randn(T, n, generator=gen) * 3).to(dtype)
    X[0, 0] = -0.0
    neg_nan = torch.tensor([0xFE00 - 65536 if dtype == F16 else 0xFFC0 - 65536], dtype=torch.int16).view(dtype)
    assert torch.isnan(neg_nan).all()
    X[1, 1] = neg_nan[0]
    Xd = X.to(dev)
    S, R = torch.zeros(n, n, dtype=F64, device=dev), torch.zeros(n, n, dtype=F64, device=dev)
    info = {}
    planes = ops.cov_accum_i8(S, Xd, route_info=info, relu=True)
    ops.cov_accum(R, Xd, relu=True)
    W = torch.zeros(n, n, dtype=F64)
    O.cov_accum_tokens_relu(W, X)
    S, R, W = torch.tril(S).cpu(), torch.tril(R).cpu(), torch.tril(W)
    print(f"[relu {dtype}] planes {planes} columns {info['columns']} fp64 kernel NaN entries {int(torch.isnan(R).sum())} "
          f"oracle NaN entries {int(torch.isnan(W).sum())} int8 NaN entries {int(torch.isnan(S).sum())}")
    assert planes in (5, 6) and 1 in info["columns"], info             # (the route may take further columns out of a short call)
    assert torch.equal(torch.isnan(S), torch.isnan(W))                     # the NaN's row and column, as torch.relu + fp64 product
    keep = torch.ones(n, dtype=torch.bool)
    keep[1] = False        # (mdg_cov_accum's own ReLU turns a NaN into 0; the int8 route keeps it, as torch.relu and the oracle do)
    Sk, Rk = S[keep][:, keep], R[keep][:, keep]
    err = entry_err(Sk, Rk)
    print(f"[relu {dtype}] err against the fp64 kernel {err:.3e} bound {info['bound']:.3e}")
    check_i8_error(err, bound=info["bound"])
    assert S[0, 0].item() > 0 and not torch.isnan(Sk).any()


def test_fp16_fused_launch_with_per_head_statistics(ops, dev):
    if torch.cuda.get_device_properties(dev).multi_processor_count != 256:
        pytest.skip("the fused launch's tile schedule is cut for 256 CUs")
    gen = torch.Generator(device=dev).manual_seed(41)
    T, d, hq, hk = 2048, 2048, 16, 4
    x = torch.randn(T, d, device=dev, generator=gen).to(F16)
    q = (torch.randn(T, hq * 128, device=dev, generator=gen) * 2).to(F16)
    k = (torch.randn(T, hk * 128, device=dev, generator=gen) * 0.5).to(F16)
    Sx, Sq, Sk = (torch.zeros(d, d, dtype=F64, device=dev), torch.zeros(hq, 128, 128, dtype=F64, device=dev),
                  torch.zeros(hk, 128, 128, dtype=F64, device=dev))
    infos = []
    planes = ops.cov_accum_i8_multi([(Sx, x, 1), (Sq, q, hq), (Sk, k, hk)], route_info=infos)
    Rx, Rq, Rk = torch.zeros_like(Sx), torch.zeros_like(Sq), torch.zeros_like(Sk)
    ops.cov_accum(Rx, x)
    ops.cov_accum(Rq, q, n_heads=hq)
    ops.cov_accum(Rk, k, n_heads=hk)
    assert planes in (5, 6) and len(infos) == 3
    errs = [entry_err(Sx, Rx)] + [max(entry_err(S[h], R[h]) for h in range(S.shape[0])) for S, R in ((Sq, Rq), (Sk, Rk))]
    print(f"[fp16 fused] planes {planes} errs {errs} bounds {[i['bound'] for i in infos]}")
    for e, i in zip(errs, infos):
        check_i8_error(e, bound=i["bound"])


def test_fp16_dispatch_takes_the_int8_route(ops, dev):
    """fp16 statistics through ops.cov_accum_multi(mode="i8") are counted on the int8 path, and ops.cov_accum_i8 takes an fp16
    tensor.  (Before fp16 support the counts stayed 0 -- the statistic went to the fp64 kernel unannounced -- and the direct call
    raised ValueError.)"""
    gen = torch.Generator(device=dev).manual_seed(43)
    T, n = 2048, 2048
    x = torch.randn(T, n, device=dev, generator=gen).to(F16)
    before = ops.i8_route_counts(dev)
    S = torch.zeros(n, n, dtype=F64, device=dev)
    ops.cov_accum_multi([(S, x, 1)], mode="i8")
    after = ops.i8_route_counts(dev)
    assert after["i8_5"] + after["i8_6"] == before["i8_5"] + before["i8_6"] + 1, (before, after)
    assert after["fallback_f64"] == before["fallback_f64"]
    S2 = torch.zeros(n, n, dtype=F64, device=dev)
    info = {}
    assert ops.cov_accum_i8(S2, x, route_info=info) in (5, 6)
    assert torch.equal(S, S2)                       # the same kernels, run-to-run bit-identical
    R = torch.zeros(n, n, dtype=F64, device=dev)
    ops.cov_accum(R, x)
    check_i8_error(entry_err(S, R), bound=info["bound"])


def test_opt_fc1_hook_takes_the_int8_route_when_wide(ops, dev):
    """The OPT fc1 statistic (ReLU on load) of an fp16 activation 4096 wide through the real hook: counted on the int8 path, on
    the exact route, and within the exact route's bound of the oracle's ReLU covariance; 3072 wide stays on the fp64 kernel."""
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    gen = torch.Generator(device=dev).manual_seed(47)
    out = (torch.randn(2, 1024, 4096, device=dev, generator=gen) * 1.5).to(F16)
    S = [torch.zeros(4096, 4096, dtype=F64, device=dev)]
    before = ops.i8_route_counts(dev)
    ModelAdapter._make_fc_hook(0, S)(None, None, out)
    after = ops.i8_route_counts(dev)
    assert after["i8_5"] + after["i8_6"] == before["i8_5"] + before["i8_6"] + 1 and after["exact"] == before["exact"] + 1, (before, after)
    R = torch.zeros(4096, 4096, dtype=F64)
    O.cov_accum_tokens_relu(R, out.cpu())
    err = entry_err(torch.tril(S[0]).cpu(), torch.tril(R))
    print(f"[opt fc1 hook] err {err:.3e}")
    assert err <= EXACT_ROUNDING + REFERENCE_ROUNDING
    narrow = (torch.randn(2, 512, 3072, device=dev, generator=gen)).to(F16)
    Sn = [torch.zeros(3072, 3072, dtype=F64, device=dev)]
    ModelAdapter._make_fc_hook(0, Sn)(None, None, narrow)
    assert ops.i8_route_counts(dev) == after
    Rn = torch.zeros_like(Sn[0])
    ops.cov_accum(Rn, narrow, relu=True)
    assert torch.equal(Sn[0], Rn)
