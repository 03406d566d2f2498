"""Host side of the fp16 element type of the int8 digit-plane covariance (csrc/cov_i8.hpp F16Elem, MDG_I8_F16 / MDG_I8_RELU):
a Python model of the fp16 split over ALL 65536 bit patterns, the int32 headroom of the plane-pair classes against the fold
interval the source states, the claim that the x_d of every listed element is an fp16 value again, and which error bound the
selection certificate is taken against for a given set of route counts.  No GPU.
"""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP_F16, NP_ = 35, 6


def f16_parts(bits):
    """bit patterns (int64 array) -> (signed significand |sig| < 2^11, effective exponent on the fp32 scale: field + 112, subnormals
    113, Inf / NaN 255) -- F16Elem::parts.  value = sig 2^(ee - 137)."""
    e, m = (bits >> 10) & 0x1F, bits & 0x3FF
    sig = np.where(e > 0, m + 1024, m) * np.where(bits >> 15, -1, 1)
    ee = np.where(e == 31, 255, np.maximum(e, 1) + 112)
    return sig, ee


def balanced(N):
    """int64 array N -> [6, ...] balanced base-256 digits, most significant first."""
    ds, R = [], N.copy()
    for _ in range(NP_ - 1):
        b = ((R + 128) & 0xFF) - 128
        ds.append(b)
        R = (R - b) >> 8
    ds.append(R)
    return np.stack(ds[::-1])


ALL = np.arange(65536, dtype=np.int64)
FINITE = ALL[((ALL >> 10) & 0x1F) != 31]


def test_source_constants_match_the_model():
    hpp = open(os.path.join(ROOT, "modegpt_amd", "csrc", "cov_i8.hpp")).read()
    assert "TOP_SHIFT_F16 = 8 * NP - 13" in hpp and "constexpr int NP = 6" in hpp
    hdr = open(os.path.join(ROOT, "include", "modegpt_hip.h")).read()
    from modegpt_amd import _lib
    assert re.search(r"#define MDG_I8_F16 (\d+)", hdr).group(1) == str(_lib.MDG_I8_F16) == "4"
    assert re.search(r"#define MDG_I8_RELU (\d+)", hdr).group(1) == str(_lib.MDG_I8_RELU) == "8"


@pytest.mark.parametrize("e_max", [1, 2, 11, 12, 13, 15, 24, 29, 30])
def test_every_finite_fp16_pattern_splits_exactly(e_max):
    """Against a column maximum of exponent field e_max (effective 1 .. 30): every finite pattern that can sit in such a column is
    an exact 48-bit integer of the column's unit 2^(E - 172) -- nothing is rounded -- and its six balanced digits rebuild it."""
    sig, ee = f16_parts(FINITE)
    E = e_max + 112
    inside = (ee <= E) | (sig == 0)
    sig, ee, bits = sig[inside], ee[inside], FINITE[inside]
    sh = E - ee
    assert sh.max() <= 29 < TOP_F16                      # the "rounded elements" counter stays 0: no shift ever exceeds the top shift
    N = sig << (TOP_F16 - sh)
    assert np.abs(N).max() < 1 << 46
    d = balanced(N)
    assert d[1:].min() >= -128 and d[1:].max() <= 127 and np.abs(d[0]).max() <= 64
    rebuilt = sum(d[s].astype(object) * 256 ** (NP_ - 1 - s) for s in range(NP_))
    assert (rebuilt == N.astype(object)).all()
    # and the integer IS the value: N 2^(E - 172) == float(pattern), exactly (both sides exact in fp64)
    val = torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(torch.float16).double().numpy()
    assert (np.ldexp(N.astype(np.float64), E - 172) == val).all()


def _fold_steps():
    hpp = open(os.path.join(ROOT, "modegpt_amd", "csrc", "cov_i8.hpp")).read()
    f16 = int(re.search(r"constexpr int FLUSH_STEPS_F16 = (\d+);", hpp).group(1))
    bf16 = int(re.search(r"constexpr int FLUSH_STEPS = (\d+);", hpp).group(1))
    assert "static_assert(FLUSH_STEPS <= FLUSH_STEPS_F16" in hpp      # the product kernels fold every FLUSH_STEPS k-steps for both types
    return bf16, f16


def _probe():
    spec = importlib.util.spec_from_file_location("i8_int32_bound_f16", os.path.join(ROOT, "scripts", "probes", "i8_int32_bound_f16.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fp16_int32_growth_allows_the_fold_interval():
    """(largest class sum one token can add) x (tokens between two folds) < 2^31 for fp16 digit vectors, the interval read from
    cov_i8.hpp.  The per-token figure is an upper bound over every pair of producible digit vectors and every subset of plane
    pairs a class can keep, and it is attained (so the interval cannot be lengthened either)."""
    probe = _probe()
    bf16_steps, f16_steps = _fold_steps()
    bound, attained = probe.per_token_bound(), probe.attained_per_token()
    assert attained[0] == bound == 32768, (bound, attained)
    assert bf16_steps == 2047
    for steps in (bf16_steps, f16_steps):
        assert bound * steps * 32 < 2 ** 31
    assert bound * (f16_steps + 1) * 32 >= 2 ** 31


def test_x_d_of_every_listed_fp16_element_is_an_fp16_value():
    """The dense-list remainder kernels read an fp16 copy of x in which every listed element (one with a nonzero digit below
    plane 2) is replaced by x_d = its top three digit planes.  For every finite bit pattern and every column maximum: x_d is a
    finite fp16 value (round trip through torch.float16 is the identity), has at most 11 significant bits, and x - x_d is the
    listed remainder L 2^(E - 172) with |L| <= 2^23 + 2^15 + 2^7."""
    sig, ee = f16_parts(FINITE)
    listed_total = 0
    for e_max in range(1, 31):
        E = e_max + 112
        inside = (ee <= E) & (sig != 0)
        N = sig[inside] << (TOP_F16 - (E - ee[inside]))
        d = balanced(N)
        L = d[3] * 65536 + d[4] * 256 + d[5]
        listed = L != 0
        if e_max <= 12:                          # nothing lies 12 binades under such a maximum: every element is a multiple of 2^24
            assert not listed.any()              # units (below e_max 12 that grid would be finer than fp16's own 2^-24)
            continue
        Nd = (N - L)[listed]
        assert (Nd % (1 << 24) == 0).all() and np.abs(L).max() <= (1 << 23) + (1 << 15) + (1 << 7)
        M = np.abs(Nd >> 24)
        width = np.where(M > 0, np.floor(np.log2(np.maximum(M, 1))).astype(np.int64) + 1 - _trailing_zeros(M), 0)
        assert width.max() <= 11
        xd = np.ldexp(Nd.astype(np.float64), E - 172)
        back = torch.from_numpy(xd).to(torch.float16)
        assert torch.isfinite(back).all() and (back.double().numpy() == xd).all()
        listed_total += int(listed.sum())
    assert listed_total > 100000                 # (the claim was exercised: elements 12 .. 29 binades under the maximum)


def _trailing_zeros(M):
    M = np.where(M == 0, 1, M)
    return np.log2(M & -M).astype(np.int64)


def test_relu_bit_semantics_model():
    """MDG_I8_RELU on the bits (relu_bits, cov_i8.hpp): sign bit set -> +0, except a NaN, which stays -- the same values as
    torch.relu for every fp16 and bf16 pattern."""
    for dtype, nan_above in ((torch.float16, 0x7C00), (torch.bfloat16, 0x7F80)):
        bits = ALL.copy()
        out = np.where(((bits & 0x8000) != 0) & ((bits & 0x7FFF) <= nan_above), 0, bits)
        x = torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(dtype)
        got = torch.from_numpy(out.astype(np.uint16).view(np.int16).copy()).view(dtype).double()
        want = torch.relu(x.double())
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        ok = ~torch.isnan(want)
        assert torch.equal(got[ok], want[ok])


def _adapter(arch, routes, tokens=1 << 20):
    from modegpt_amd import engine
    ad = type("Adapter", (engine.TensorAdapter,), {"arch": arch})(dict(engine.SHAPES["tiny"]), {})
    ad.calib_tokens = tokens
    ad.cov_routes = routes
    return ad


def test_covariance_error_eps_follows_the_routes_taken():
    """The certificate's eps comes from what ran (adapter.cov_routes), not from arch and shape."""
    from modegpt_amd.compression.compress_mlp import covariance_error_eps
    f64 = ((1 << 20) / 4 + 4) * 2.0 ** -53
    i8 = 1.1e-11 + 64 * 2.0 ** -53
    zero = {"i8_5": 0, "i8_6": 0, "fallback_f64": 0, "fp64_columns": 0, "exact": 0}
    # an fp16 Llama whose statistics ran on the int8 planes
    assert abs(covariance_error_eps(_adapter("llama", dict(zero, i8_5=64, i8_6=32, exact=96)), 8192) - i8) < 1e-25
    # a wide OPT: fc1 (ffn 16384) took the int8 route with ReLU on load -- no longer excluded by its architecture
    assert abs(covariance_error_eps(_adapter("opt", dict(zero, i8_5=48, exact=24)), 16384) - i8) < 1e-25
    # OPT-125m's shape: ffn 3072 stays on the fp64 kernel, nothing was counted
    assert covariance_error_eps(_adapter("opt", dict(zero)), 3072) == f64
    # a model none of whose statistics took the int8 route (fp32 activations, say), at a width the int8 route would take
    assert covariance_error_eps(_adapter("llama", dict(zero)), 8192) == f64
    # a mix: a statistic or single columns fell back
    assert covariance_error_eps(_adapter("llama", dict(zero, i8_6=10, fallback_f64=2)), 8192) == max(i8, f64)
    assert covariance_error_eps(_adapter("llama", dict(zero, i8_6=10, fp64_columns=3)), 8192) == max(i8, f64)
