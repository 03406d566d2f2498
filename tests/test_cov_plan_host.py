"""Which launches ops.cov_accum_multi makes for a layer's statistics, in which order and on which stream -- characterised on the CPU:
the entries it dispatches to (ops.cov_accum_i8, ops.cov_accum_i8_multi, ops._cov_accum_fused) and the stream calls are replaced
by recorders, the real ops.cov_accum_multi runs on CPU tensors of the right shapes and dtypes, and the recorded trace is compared
with the one written down here per case.  Then the pure planner (ops.plan_cov_launches) against the same traces, and the one
predicate for "takes the int8 planes" (ops.takes_i8_planes) against the route covariance_error_eps predicts and the one the
dispatch takes.  No GPU.
"""
import contextlib
import itertools
import types

import pytest
import torch

from modegpt_amd import ops
from modegpt_amd.compression.compress_mlp import I8_GUARANTEED_EPS, covariance_error_eps

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
FORK, JOIN = "side.wait_stream(main)", "main.wait_stream(side)"


def stat(width, n_heads=1, dtype=BF16, tokens=8):
    """(sigma, x, n_heads) of one statistic: n_heads == 1 a [width, width] matrix, else n_heads Grams of `width` each.  sigma is a
    stride-0 view of one element (only its shape, dim and dtype are read here)."""
    shape = (width, width) if n_heads == 1 else (n_heads, width, width)
    return torch.zeros(1, dtype=torch.float64).expand(shape), torch.zeros(tokens, n_heads * width, dtype=dtype), n_heads


class _Stream:
    def __init__(self, name, trace):
        self.name, self.trace = name, trace

    def wait_stream(self, other):
        self.trace.append(f"{self.name}.wait_stream({other.name})")


def run_recorded(monkeypatch, items, mode, fuse, overlap, fusable=True):
    """The trace of ops.cov_accum_multi(items, mode): ("i8" | "i8_multi" | "f64", [(width, n_heads) ...], on the side stream) per
    launch, FORK / JOIN per stream wait, in the order they happen."""
    trace, on_side = [], [False]
    main, side = _Stream("main", trace), _Stream("side", trace)

    def shapes(its):
        return [(s.shape[-1], h) for s, _, h in its]

    def single(sigma, x, **kw):
        assert kw == {"report": False}
        trace.append(("i8", [(sigma.shape[-1], 1)], on_side[0]))

    def multi(its, **kw):
        assert kw == {"report": False}
        trace.append(("i8_multi", shapes(its), on_side[0]))

    def fused(its):
        trace.append(("f64", shapes(its), on_side[0]))

    @contextlib.contextmanager
    def stream(s):
        assert s is side
        on_side[0] = True
        try:
            yield
        finally:
            on_side[0] = False

    monkeypatch.setattr(ops, "cov_accum_i8", single)
    monkeypatch.setattr(ops, "cov_accum_i8_multi", multi)
    monkeypatch.setattr(ops, "_cov_accum_fused", fused)
    monkeypatch.setattr(ops, "_fusable_device", lambda device: fusable)
    monkeypatch.setattr(ops, "_side_stream", lambda device, *a, **kw: side)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: main)
    monkeypatch.setattr(torch.cuda, "stream", stream)
    monkeypatch.setattr(ops, "I8_FUSE", fuse)
    monkeypatch.setattr(ops, "COV_OVERLAP_SMALL", overlap)
    ops.cov_accum_multi(items, mode=mode)
    return trace


def i8(*s):
    return ("i8", list(s), False)


def i8m(*s):
    return ("i8_multi", list(s), False)


def f64(*s, side=False):
    return ("f64", list(s), side)


def gqa_layer(d_ff, d, n_heads, n_kv):
    """sigma_mlp, sigma_x, per-head sigma_q / sigma_k of head_dim 128: fused, sigma_mlp keeps a launch of its own and the three
    others share one; unfused, the planes run largest first and the heads go to the fp64 kernel -- beside the last plane on the
    side stream with the overlap on, after the planes without."""
    m, x, q, k = (d_ff, 1), (d, 1), (128, n_heads), (128, n_kv)

    def expect(fuse, overlap):
        if fuse:
            return [i8(m), i8m(x, q, k)]
        return [i8(m), FORK, f64(q, k, side=True), i8(x), JOIN] if overlap else [i8(m), i8(x), f64(q, k)]
    return [stat(d_ff), stat(d), stat(128, n_heads), stat(128, n_kv)], expect


def _same(trace):
    return lambda fuse, overlap: trace


def _unfused(with_overlap, without):
    return lambda fuse, overlap: with_overlap if overlap else without


M, X, Q, K = (14336, 1), (4096, 1), (128, 32), (128, 8)
LLAMA = [stat(14336), stat(4096), stat(128, 32), stat(128, 8)]
LLAMA_UNFUSED = _unfused([i8(M), FORK, f64(Q, K, side=True), i8(X), JOIN], [i8(M), i8(X), f64(Q, K)])

# name -> (items, expected trace as a function of (I8_FUSE, COV_OVERLAP_SMALL), keyword arguments of run_recorded)
CASES = {
    "llama-3-8b": (*gqa_layer(14336, 4096, 32, 8), {}),
    "qwen3-14b": (*gqa_layer(17408, 5120, 40, 8), {}),
    "llama-2-7b (MHA)": (*gqa_layer(11008, 4096, 32, 32), {}),
    # OPT-125m: sigma_x 768 wide and heads of 64 -- nothing for the int8 planes, one fp64 call on the caller's stream
    "opt-125m": ([stat(768), stat(64, 12), stat(64, 12)], _same([f64((768, 1), (64, 12), (64, 12))]), {}),
    # heads of 64 beside wide planes: a `rest` -- on the side stream BEFORE the int8 launches when fused, beside the last plane when not
    "heads of 64 beside wide planes": (
        [stat(8192), stat(2048), stat(64, 4), stat(64, 2)],
        lambda fuse, overlap: ([FORK, f64((64, 4), (64, 2), side=True), i8((8192, 1)), i8((2048, 1)), JOIN] if fuse and overlap else
                               [i8((8192, 1)), FORK, f64((64, 4), (64, 2), side=True), i8((2048, 1)), JOIN] if overlap else
                               [i8((8192, 1)), i8((2048, 1)), f64((64, 4), (64, 2))]), {}),
    "one wide plane alone": ([stat(4096)], _same([i8(X)]), {}),
    "two planes, no heads": ([stat(14336), stat(4096)], _same([i8(M), i8(X)]), {}),
    # the largest plane is not a member of the shared group: three planes and two head statistics make a group of FOUR, which fuses
    "three planes, two head statistics": (
        [stat(14336), stat(4096), stat(2048), stat(128, 32), stat(128, 8)],
        lambda fuse, overlap: ([i8(M), i8m(X, (2048, 1), Q, K)] if fuse else
                               [i8(M), i8(X), FORK, f64(Q, K, side=True), i8((2048, 1)), JOIN] if overlap else
                               [i8(M), i8(X), i8((2048, 1)), f64(Q, K)]), {}),
    # ... four planes and two head statistics a group of five: more than one int8 launch takes, never fused
    "four planes, two head statistics": (
        [stat(14336), stat(8192), stat(4096), stat(2048), stat(128, 32), stat(128, 8)],
        _unfused([i8(M), i8((8192, 1)), i8(X), FORK, f64(Q, K, side=True), i8((2048, 1)), JOIN],
                 [i8(M), i8((8192, 1)), i8(X), i8((2048, 1)), f64(Q, K)]), {}),
    "shared group of two dtypes": (
        [stat(14336), stat(4096), stat(128, 32, F16)],
        _unfused([i8(M), FORK, f64(Q, side=True), i8(X), JOIN], [i8(M), i8(X), f64(Q)]), {}),
    # the largest statistic's dtype is not compared with the group's (it has a launch of its own)
    "largest statistic of another dtype": (
        [stat(14336, dtype=F16), stat(4096), stat(128, 32), stat(128, 8)],
        lambda fuse, overlap: [i8(M), i8m(X, Q, K)] if fuse else LLAMA_UNFUSED(fuse, overlap), {}),
    "token counts differ between planes and heads": (
        [stat(14336), stat(4096), stat(128, 32, tokens=16), stat(128, 8, tokens=16)], LLAMA_UNFUSED, {}),
    # ... a `rest` item's token count is not looked at
    "token counts differ only in a rest item": (
        [stat(14336), stat(4096), stat(128, 32), stat(64, 2, tokens=16)],
        lambda fuse, overlap: ([FORK, f64((64, 2), side=True), i8(M), i8m(X, Q), JOIN] if fuse and overlap else
                               [i8(M), i8m(X, Q), f64((64, 2))] if fuse else
                               [i8(M), FORK, f64(Q, (64, 2), side=True), i8(X), JOIN] if overlap else
                               [i8(M), i8(X), f64(Q, (64, 2))]), {}),
    "fp32 layer": ([stat(14336, dtype=F32), stat(4096, dtype=F32), stat(128, 32, F32), stat(128, 8, F32)],
                   _same([f64(M, X, Q, K)]), {}),
    # sigma_mlp 14400 wide stays on fp64; sigma_x is the only plane, so it is the shared group's first member.  Unfused, the heads
    # come BEFORE the rest in the fp64 call
    "width not a multiple of 128": (
        [stat(14400), stat(4096), stat(128, 32), stat(128, 8)],
        lambda fuse, overlap: ([FORK, f64((14400, 1), side=True), i8m(X, Q, K), JOIN] if fuse and overlap else
                               [i8m(X, Q, K), f64((14400, 1))] if fuse else
                               [FORK, f64(Q, K, (14400, 1), side=True), i8(X), JOIN] if overlap else
                               [i8(X), f64(Q, K, (14400, 1))]), {}),
    # no plane: the heads of 128 have nothing to share a launch with, and go first in the one fp64 call
    "widths below I8_MIN_FEATURES": ([stat(1024), stat(512), stat(128, 4), stat(128, 2)],
                                     _same([f64((128, 4), (128, 2), (1024, 1), (512, 1))]), {}),
    "device that is not fusable": (LLAMA, LLAMA_UNFUSED, {"fusable": False}),
    "mode f64": (LLAMA, _same([f64(M, X, Q, K)]), {"mode": "f64"}),
    "all items empty": ([stat(14336, tokens=0), stat(4096, tokens=0), stat(128, 32, tokens=0)], _same([]), {}),
}
SWITCHES = list(itertools.product((True, False), (True, False)))


@pytest.mark.parametrize("fuse,overlap", SWITCHES)
@pytest.mark.parametrize("name", list(CASES))
def test_cov_accum_multi_launches(monkeypatch, name, fuse, overlap):
    items, expect, kw = CASES[name]
    assert run_recorded(monkeypatch, items, kw.get("mode", "i8"), fuse, overlap, kw.get("fusable", True)) == expect(fuse, overlap)


@pytest.mark.parametrize("fuse,overlap", SWITCHES)
def test_cov_accum_multi_default_mode_and_bad_mode(monkeypatch, fuse, overlap):
    monkeypatch.setattr(ops, "COV_MODE", "f64")        # (mode=None reads ops.COV_MODE at call time)
    assert run_recorded(monkeypatch, LLAMA, None, fuse, overlap) == [f64(M, X, Q, K)]
    with pytest.raises(ValueError, match="covariance mode"):
        run_recorded(monkeypatch, LLAMA, "int8", fuse, overlap)
    assert run_recorded(monkeypatch, [stat(4096, tokens=0)], "int8", fuse, overlap) == []     # (nothing to do: the mode is not looked at)


# ---------------------------------------------------------------- the pure planner against the same traces
needs_planner = pytest.mark.skipif(not hasattr(ops, "plan_cov_launches"), reason="the planner is not part of this checkout")


def trace_of_plan(steps, descs):
    """What walking `steps` records: a side-stream fp64 step is the fork and the launch, the join is the wait back."""
    out = []
    for step in steps:
        if step == ops.COV_JOIN:
            out.append(JOIN)
            continue
        kind, idx = step[0], step[1]
        assert kind in ("i8", "i8_multi", "f64") and (kind != "i8" or len(idx) == 1) and (kind != "i8_multi" or 2 <= len(idx) <= 4)
        side = kind == "f64" and step[2]
        if side:
            out.append(FORK)
        out.append((kind, [(descs[i].width, descs[i].n_heads) for i in idx], side))
    return out


def describe(items):
    return [ops.CovStat(s.shape[-1], h, x.dtype, s.dim(), x.numel() // x.shape[-1]) for s, x, h in items if x.numel() > 0]


@needs_planner
@pytest.mark.parametrize("fuse,overlap", SWITCHES)
@pytest.mark.parametrize("name", list(CASES))
def test_planner_returns_the_recorded_trace(monkeypatch, name, fuse, overlap):
    items, expect, kw = CASES[name]
    descs = describe(items)
    steps = ops.plan_cov_launches(descs, kw.get("mode", "i8"), fuse=fuse, overlap=overlap, fusable_device=kw.get("fusable", True),
                                  min_features=2048)
    assert trace_of_plan(steps, descs) == expect(fuse, overlap)
    assert trace_of_plan(steps, descs) == run_recorded(monkeypatch, items, kw.get("mode", "i8"), fuse, overlap, kw.get("fusable", True))
    assert sorted(i for s in steps if s != ops.COV_JOIN for i in s[1]) == list(range(len(descs)))      # every statistic exactly once
    assert steps.count(ops.COV_JOIN) == sum(1 for s in steps if s[0] == "f64" and s[2]) <= 1


@needs_planner
def test_planner_is_pure_and_rejects_a_bad_mode(monkeypatch):
    """The switches are arguments: the module's own values are not read, and nothing of CUDA or the library is touched."""
    descs = describe(LLAMA)
    for name in ("I8_FUSE", "COV_OVERLAP_SMALL"):
        monkeypatch.setattr(ops, name, False)
    monkeypatch.setattr(ops, "I8_MIN_FEATURES", 1 << 20)
    monkeypatch.setattr(ops, "COV_MODE", "f64")
    monkeypatch.setattr(ops._lib, "load", lambda: pytest.fail("the planner loaded the library"))
    monkeypatch.setattr(ops, "_fusable_device", lambda d: pytest.fail("the planner asked for the device"))
    steps = ops.plan_cov_launches(descs, "i8", fuse=True, overlap=True, fusable_device=True, min_features=2048)
    assert steps == [("i8", [0]), ("i8_multi", [1, 2, 3])]
    assert ops.plan_cov_launches(descs, "i8", fuse=True, overlap=True, fusable_device=True, min_features=8192) == \
        [("f64", [1], True), ("i8_multi", [0, 2, 3]), ops.COV_JOIN]      # (sigma_x is no plane now: fp64, beside the int8 launch)
    with pytest.raises(ValueError, match="covariance mode"):
        ops.plan_cov_launches(descs, "int8", fuse=True, overlap=True, fusable_device=True, min_features=2048)
    assert ops.plan_cov_launches([], "i8", fuse=True, overlap=True, fusable_device=True, min_features=2048) == []


# ---------------------------------------------------------------- one predicate for "takes the int8 planes"
WIDTHS = (640, 2048, 3072, 4096, 14336, 14400)
# Does the MLP statistic (bf16) of this width run on the int8 planes?  Recorded from the parent of the commit that added the
# predicate: what covariance_error_eps predicts without route counts == what the hook's entry dispatches to.
TAKES_I8 = {
    ("llama", "i8"): {640: False, 2048: True, 3072: True, 4096: True, 14336: True, 14400: False},
    ("opt", "i8"): {640: False, 2048: False, 3072: False, 4096: True, 14336: True, 14400: False},
    ("llama", "f64"): dict.fromkeys(WIDTHS, False),
    ("opt", "f64"): dict.fromkeys(WIDTHS, False),
}


def dispatched_to_i8(monkeypatch, arch, width):
    """Which entry the hook of sigma_mlp reaches: ops.cov_accum_fc_relu (OPT: ReLU on load) or ops.cov_accum_multi."""
    calls = []
    monkeypatch.setattr(ops, "cov_accum_i8", lambda sigma, x, **kw: calls.append(("i8", kw.get("relu", False))))
    monkeypatch.setattr(ops, "cov_accum", lambda sigma, x, **kw: calls.append(("f64", kw.get("relu", False))))
    monkeypatch.setattr(ops, "_cov_accum_fused", lambda its: calls.append(("f64", False)))
    monkeypatch.setattr(ops, "_fusable_device", lambda device: True)
    sigma, x, _ = stat(width)
    if arch == "opt":
        ops.cov_accum_fc_relu(sigma, x)
    else:
        ops.cov_accum_multi([(sigma, x, 1)])
    assert len(calls) == 1 and calls[0][1] == (arch == "opt")
    return calls[0][0] == "i8"


@pytest.mark.parametrize("mode", ["i8", "f64"])
@pytest.mark.parametrize("arch", ["llama", "opt"])
@pytest.mark.parametrize("width", WIDTHS)
def test_predicted_route_is_the_dispatched_one(monkeypatch, width, arch, mode):
    monkeypatch.setattr(ops, "COV_MODE", mode)
    adapter = types.SimpleNamespace(arch=arch, calib_tokens=1 << 20, config=types.SimpleNamespace(calib_size=32))
    eps_f64, eps_i8 = ((1 << 20) / 4 + 4) * 2.0 ** -53, I8_GUARANTEED_EPS * 1.0 + 64 * 2.0 ** -53
    want = TAKES_I8[arch, mode][width]
    assert covariance_error_eps(adapter, width) == (eps_i8 if want else eps_f64)
    assert dispatched_to_i8(monkeypatch, arch, width) == want
    if hasattr(ops, "takes_i8_planes"):
        assert (mode == "i8" and ops.takes_i8_planes(width, BF16, relu=arch == "opt")) == want


@needs_planner
def test_predicate_element_types_heads_and_thresholds(monkeypatch):
    assert ops.takes_i8_planes(4096, F16) and not ops.takes_i8_planes(4096, F32) and not ops.takes_i8_planes(4096, torch.float64)
    assert ops.takes_i8_planes(128, BF16, n_heads=8) and not ops.takes_i8_planes(64, BF16, n_heads=8)       # per-head: head_dim 128
    assert not ops.takes_i8_planes(128, F32, n_heads=8) and not ops.takes_i8_planes(128, BF16)
    assert ops.takes_i8_planes(256, BF16, min_features=256) and not ops.takes_i8_planes(256, BF16, relu=True, min_features=256)
    monkeypatch.setattr(ops, "I8_MIN_FEATURES", 256)          # (read at call time, like the tests and the benchmark set it)
    assert ops.takes_i8_planes(256, BF16) and not ops.takes_i8_planes(128, BF16)
    monkeypatch.setattr(ops, "FC_I8_MIN_FEATURES", 2048)
    assert ops.takes_i8_planes(2048, BF16, relu=True)
