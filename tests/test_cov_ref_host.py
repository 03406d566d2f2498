"""The covariance references of tests/cov_ref.py checked on the host, and the path every shape of tests/test_gpu_cov.py is chosen
for checked against the library's own size queries (which need no device).  No GPU.

The token counts of the GPU file are picked so that a call is unsplit, split in two, or split with a last part of exactly one
token.  What decides that is the library's cost model; if the model changes, the assertions here fail, and whoever changes it picks
new token counts with the same properties instead of letting the coverage lapse."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from modegpt_amd import _lib
from tests import cov_ref as R

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float64]


def test_long_double_is_extended():
    assert np.finfo(R.LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_inputs_are_on_the_lattice(dtype):
    x = R.exact_inputs(400, 24, dtype, seed=1)
    assert x.dtype == dtype and x.shape == (400, 24)
    v = x.double()
    assert torch.equal(v, R.exact_inputs(400, 24, torch.float64, seed=1)), "the same values in every element type"
    zeros = v == 0
    assert 0.15 < zeros.double().mean().item() < 0.35
    assert bool((zeros & torch.signbit(v)).any()) and bool((zeros & ~torch.signbit(v)).any()), "both zeros"
    assert bool((v > 0).any()) and bool((v < 0).any())
    for j in range(24):                                  # one power of two per column, integers of at most 15 on it
        col = v[:, j].abs()
        assert any(torch.equal(col / 2.0 ** e, (col / 2.0 ** e).round()) and (col / 2.0 ** e).max().item() <= R.MANT
                   for e in range(-R.EXP, R.EXP + 1)), j


@pytest.mark.parametrize("heads,relu", [(1, False), (3, False), (1, True), (3, True)])
def test_exact_cov_equals_integer_arithmetic(heads, relu):
    tokens, feat = 37, 5
    x = R.exact_inputs(tokens, heads * feat, torch.bfloat16, seed=2)
    got = R.exact_cov(x, heads, relu)
    rows = [[Fraction(float(v)) for v in row] for row in x.double().tolist()]
    for h in range(heads):
        for i in range(feat):
            for j in range(feat):
                s = Fraction(0)
                for r in rows:
                    a, b = r[h * feat + i], r[h * feat + j]
                    if relu:
                        a, b = max(a, Fraction(0)), max(b, Fraction(0))
                    s += a * b
                assert Fraction(got[h, i, j].item()) == s, (h, i, j)
    assert torch.equal(got, got.transpose(-1, -2))
    # accumulation onto an earlier exact result of the same columns == the concatenated tokens
    both = R.exact_cov(torch.cat([x, x[:9]]), heads, relu)
    assert torch.equal(R.exact_cov(x[:9], heads, relu, sigma0=got), both)


def test_exact_cov_does_not_depend_on_the_order():
    x = R.exact_inputs(5000, 16, torch.float32, seed=4)
    want = R.exact_cov(x)
    perm = torch.randperm(5000, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.exact_cov(x[perm]), want)
    parts = sum(R.exact_cov(x[a:a + 613]) for a in range(0, 5000, 613))
    assert torch.equal(parts, want)
    v = x.double()
    s = torch.zeros(16, 16, dtype=torch.float64)
    for t in range(4999, -1, -1):                        # one token at a time, backwards
        s += torch.outer(v[t], v[t])
    assert torch.equal(s, want[0])


@pytest.mark.parametrize("heads,relu", [(1, False), (2, True)])
def test_longdouble_cov_equals_exact_cov_on_integer_data(heads, relu):
    x = R.exact_inputs(300, heads * 20, torch.float16, seed=5)
    s, scale = R.longdouble_cov(x, heads, relu)
    want = R.exact_cov(x, heads, relu)
    assert s.dtype == R.LD and scale.dtype == R.LD
    assert np.array_equal(s.astype(np.float64).view(np.int64), (want.numpy() + 0.0).view(np.int64))
    dg = np.sqrt(np.einsum("hii->hi", want.numpy()).astype(R.LD))
    assert np.array_equal(scale, dg[:, :, None] * dg[:, None, :])
    assert np.all(np.abs(s) <= scale * (1 + R.LD(2.0) ** -60))             # Cauchy-Schwarz
    assert np.all(R.longdouble_abs_cov(x, heads) >= np.abs(R.longdouble_cov(x, heads, False)[0]))


def test_split_plan_arithmetic():
    per = 128 * 128 * 8
    assert R.split_plan(0, 255, 128, 1) == (1, 256, 255)
    assert R.split_plan(2 * per, 256, 128, 1) == (2, 128, 128)
    assert R.split_plan(9 * 3 * per, 1153, 256, 1) == (9, 144, 1)
    assert R.split_plan(9 * 3 * 3 * per, 1160, 200, 3) == (9, 144, 8)
    with pytest.raises(AssertionError):
        R.split_plan(12 * per, 1153, 128, 1)             # twelve splits of 112 tokens would leave the last one empty
    with pytest.raises(AssertionError):
        R.split_plan(per + 8, 300, 128, 1)


def plan(tokens, n_feat, batch):
    return R.split_plan(_lib.load().mdg_cov_accum_ws_bytes(tokens, n_feat, batch), tokens, n_feat, batch)


def test_gpu_shapes_take_the_path_they_are_named_for():
    assert plan(255, 128, 1)[0] == 1
    assert plan(256, 128, 1) == (2, 128, 128)
    for n_feat in (128, 256):
        assert plan(1153, n_feat, 1)[2] == 1, "a last split of exactly one token"
        assert plan(1160, n_feat, 1)[2] == 8, "a last split shorter than one 16-token stage"
        for tokens in list(range(1, 51)) + [63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128, 129, 254, 255]:
            assert plan(tokens, n_feat, 1)[0] == 1, tokens
        for tokens in (256, 257, 300, 1153, 1160, 4099):
            assert plan(tokens, n_feat, 1)[0] > 1, tokens
    assert _lib.load().mdg_cov_accum_ws_bytes(40, 128, 768) == 0
    for n_feat, batch in [(1, 1), (2, 1), (7, 1), (16, 1), (127, 1), (129, 1), (131, 1), (200, 1), (300, 1), (20, 3), (200, 3), (64, 2)]:
        assert plan(200, n_feat, batch)[0] == 1, (n_feat, batch)
        assert plan(333, n_feat, batch)[0] > 1, (n_feat, batch)
    assert plan(515, 128, 3)[0] > 1 and plan(2048, 64, 4)[0] > 1
    for tokens in (40, 300):
        assert (plan(tokens, 256, 1)[0] > 1) == (tokens == 300)
    assert plan(3000, 256, 1)[0] > 1 and plan(3000, 200, 1)[0] > 1


def multi_ws(shapes, dtype=_lib.MDG_BF16):
    """mdg_cov_accum_multi_ws_bytes of (tokens, n_feat, batch) problems; the query reads sizes only, the pointers just have to be
    non-null and 16-byte aligned."""
    arr = (_lib.CovProblem * len(shapes))(*[_lib.CovProblem(4096, t, f, b, f * b, 4096, f, f * f) for t, f, b in shapes])
    return _lib.load().mdg_cov_accum_multi_ws_bytes(len(shapes), arr, dtype)


def test_multi_shapes_split_their_problems():
    per = 128 * 128 * 8
    widths = [(512, 1), (256, 1), (128, 4), (128, 2)]
    tiles = [R.n_tri(f) * b for f, b in widths]
    same = multi_ws([(8200, f, b) for f, b in widths])
    assert same == 2 * sum(tiles) * per > 0, "every problem of case (a) in two splits"
    mixed = multi_ws([(t, f, b) for t, (f, b) in zip((8200, 300, 8193, 17), widths)])
    assert mixed == 2 * (tiles[0] + tiles[2]) * per > 0, "case (b): the 8200- and 8193-token problems split, the short ones do not"
    assert multi_ws([(40, 128, 768), (40, 256, 1)]) == 0, "case (c): first problem of 768 tiles unsplit, 40 tokens never split"
    assert multi_ws([(8200, 128, 768), (8200, 256, 1)]) == 2 * 3 * per, "768 tiles in front: only the second problem splits"
    assert multi_ws([(8200, 128, 767), (8200, 256, 1)]) == 2 * (767 + 3) * per
