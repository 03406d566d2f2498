"""CPU: the reference of the rotary-kernel tests (tests/rope_ref.py) checked against the oracle, against mutated chains and
against the dispatch plan -- everything test_gpu_rope.py relies on, without a GPU.

  * the oracle chain (O.masked_rms_norm then O.apply_rotary_compressed) lies inside the interval at every element;
  * the interval is not vacuous: it is a single number on all but a capped share of the elements (bf16 / f16), and a chain
    with a wrong eps, divisor, weight gather or row falls outside on >= 1 % of the elements (all dtypes; for fp32, whose
    intervals are all wider than one number, this is the guard);
  * the portable torch path of the patched attention equals the oracle chain bit for bit;
  * every case reaches the kernel variant it declares (mdg_rope_gather_plan, no device), and the declared variants cover
    every template instantiation and run-time fork of csrc/rope.hip.
"""
import itertools

import pytest
import torch

from oracle import modegpt_oracle as O
from tests import rope_ref as R
from tests.golden_util import ROPE_CASES, RopeCase

CASES = [(n, dt) for n in R.SHAPES for dt in R.DTYPES]


def _chain(i):
    return R.oracle_chain(i.x, i.w, R.EPS, i.mask, i.n_kv, i.cos, i.sin, rope_mask=i.rope_mask)


@pytest.mark.parametrize("name,dt", CASES)
def test_oracle_chain_inside_interval_and_interval_tight(name, dt):
    i = R.make_inputs(name, dt)
    plain, (lo, hi) = R.reference(name, dt)
    got = _chain(i)
    ok = R.inside(got, lo, hi)
    share = R.nondegenerate_share(lo, hi)
    print(f"{name} {dt}: inside {ok.double().mean().item():.6f}, non-degenerate {share:.4%}")
    assert torch.isfinite(got.float()).all() and torch.isfinite(lo.float()).all() and torch.isfinite(hi.float()).all()
    assert ok.all(), f"{(~ok).sum().item()} of {ok.numel()} oracle elements outside the interval"
    assert share <= R.NONDEGENERATE_CAP[dt], f"non-degenerate share {share:.4f}"
    # the special rows are what they claim to be
    x = i.x.double()
    assert (x[R.SPECIAL["zero"]] == 0).all()
    assert abs(x[R.SPECIAL["rms1e-3"]].pow(2).mean().sqrt().item() / 1e-3 - 1) < 0.05
    assert x[R.SPECIAL["big"]][0].item() >= 59904
    assert (i.w == 0).any() and (i.w > 0).any() and (i.w < 0).any()


@pytest.mark.parametrize("name", [n for n in ROPE_CASES if n != "bf16_full"])
def test_golden_normed_fixtures_inside_interval(name):
    """The three normed fixtures of rope.npz: the oracle chain on the fixture's inputs, and the rotation of the REFERENCE's
    own normed tensors (nq / nk), lie inside the interval."""
    c = RopeCase(name)
    for x_bhtr, n_ref, heads_kv in ((c.q, c.nq, c.n_kv), (c.k, c.nk, c.n_kv)):
        x = x_bhtr.transpose(1, 2).contiguous()              # [B, T, H, r]
        kv = heads_kv if x.shape[2] != c.n_kv else c.n_kv
        lo, hi = R.norm_rope_interval(x, c.norm_w, R.EPS, c.mask, kv, c.cos, c.sin)
        for got in (R.oracle_chain(x, c.norm_w, R.EPS, c.mask, kv, c.cos, c.sin), R.rotate(n_ref.transpose(1, 2), c.cos, c.sin, c.mask, kv)):
            assert R.inside(got, lo, hi).all()


# ---------------------------------------------------------------- mutated chains fall outside
def _mutated(i, kind):
    """The oracle chain with one mistake.  Written out (not through O.masked_rms_norm) so that each mistake is one edit."""
    B, T, H, r = i.dims
    xf = i.x.to(torch.float32)
    eps, div = R.EPS, r
    if kind == "eps_dropped":
        eps = 0.0
    elif kind == "eps_1e-5":
        eps = 1e-5
    elif kind == "divisor_hd":
        div = i.hd
    inv = torch.rsqrt(xf.pow(2).sum(-1, keepdim=True) / div + eps)
    if kind == "inv_neighbour_head":
        inv = inv.roll(1, dims=2)
    elif kind == "inv_2^-12":
        inv = inv * (1 + 2.0 ** -12)
    m = torch.repeat_interleave(i.mask, H // i.n_kv, dim=0)
    w = i.w[:r].expand(H, r) if kind == "weight_not_gathered" else i.w[m]
    n = (w[None, None] * (xf * inv)).to(i.x.dtype)
    return R.rotate(n.transpose(1, 2), i.cos, i.sin, i.rope_mask, i.n_kv)


MUTATIONS = ["none", "eps_dropped", "eps_1e-5", "divisor_hd", "weight_not_gathered", "inv_neighbour_head", "inv_2^-12"]


def _applies(name, dt, kind):
    B, T, n_h, n_kv, hd, r, layout = R.SHAPES[name]
    if kind == "divisor_hd" and r == hd:
        return False                     # the same number: nothing is mutated
    if kind == "weight_not_gathered" and layout == "nomask":
        return False                     # the identity mask gathers nothing
    if kind == "inv_2^-12" and dt != "f32":
        return False                     # below the half types' own rounding (2^-9, 2^-12 relative)
    return True


@pytest.mark.parametrize("name,dt", CASES)
def test_mutated_chains_fall_outside(name, dt):
    i = R.make_inputs(name, dt)
    _, (lo, hi) = R.reference(name, dt)
    assert R.inside(_mutated(i, "none"), lo, hi).all()       # the written-out chain itself is the oracle's
    for kind in MUTATIONS[1:]:
        if not _applies(name, dt, kind):
            continue
        out = 1.0 - R.inside(_mutated(i, kind), lo, hi).double().mean().item()
        print(f"{name} {dt} {kind}: {out:.2%} outside")
        assert out >= 0.01, f"{kind}: only {out:.4f} of the elements leave the interval"


# ---------------------------------------------------------------- the portable torch path
@pytest.mark.parametrize("name,dt", CASES)
@pytest.mark.parametrize("norm", [False, True])
def test_torch_fallback_matches_oracle(name, dt, norm):
    from modegpt_amd.patchers import compressed_attention as ca
    i = R.make_inputs(name, dt)
    B, T, H, r = i.dims
    got = ca._rope_gather_torch(i.x.reshape(B, T, H * r), i.cos, i.sin, i.rope_mask, H, i.n_kv, i.w if norm else None, R.EPS)
    want = _chain(i) if norm else R.reference(name, dt)[0]
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got.view(torch.int32 if dt == "f32" else torch.int16), want.view(torch.int32 if dt == "f32" else torch.int16))


# ---------------------------------------------------------------- which kernel variant each case reaches
@pytest.fixture(scope="module")
def ops():
    from modegpt_amd import ops as _ops       # the library loads without a GPU; the plan needs no device
    return _ops


@pytest.mark.parametrize("name,dt", CASES)
@pytest.mark.parametrize("norm", [False, True])
def test_case_reaches_declared_variant(ops, name, dt, norm):
    plan = R.synthetic_plan(ops, name, dt, norm)
    assert R.variant_of(plan) == R.declared(name, dt, norm)
    B, T, n_h, n_kv, hd, r, _ = R.SHAPES[name]
    assert plan["norm"] == int(norm)
    assert plan["grid"] == (8 * n_kv, -(-B * plan["t_tiles"] // 8), (n_h // n_kv) // plan["hpt"])
    assert plan["t_tiles"] == -(-T // plan["tt"]) and plan["n_tiles"] == B * plan["t_tiles"]
    assert plan["lds_attr"] == int(plan["lds"] > 64 * 1024) and plan["lds"] <= 160 * 1024


def test_declared_variants_cover_every_instantiation_and_fork(ops):
    plans = {(n, dt, norm): R.synthetic_plan(ops, n, dt, norm) for n, dt in CASES for norm in (False, True)}
    direct = {k: p for k, p in plans.items() if p["route"] == "direct"}
    tile = {k: p for k, p in plans.items() if p["route"] == "tile"}
    # rope_gather_kernel<DT, VEC, NORM, HPT>: 3 x 2 x 2 x 3 = 36
    have = {(k[1], p["vec"], k[2], p["hpt"]) for k, p in direct.items()}
    assert have == set(itertools.product(R.DTYPES, (2, 4), (False, True), (1, 2, 4)))
    # rope_tile_kernel<DT, NORM, HALF_EVEN>: 3 x 2 x 2 = 12, each CH with each parity of the half
    have = {(k[1], k[2], p["half_even"]) for k, p in tile.items()}
    assert have == set(itertools.product(R.DTYPES, (False, True), (0, 1)))
    assert {(p["hpt"], p["half_even"]) for p in tile.values()} == set(itertools.product((1, 2, 4), (0, 1)))
    # run-time forks, with the norm (where they change what the norm does) and both ways
    normed = [p for k, p in direct.items() if k[2]]
    assert {p["iters"] > 1 for p in normed} == {False, True}
    for f in ("one_shot", "nw_vec16", "cs_vec16"):
        assert {p[f] for p in normed} == {0, 1}, f
    assert {(p["one_shot"], p["nw_vec16"]) for p in normed} >= {(1, 1), (1, 0), (0, 1), (0, 0)}
    for dt in R.DTYPES:                                                    # per dtype: PER16 differs
        assert {p["one_shot"] for k, p in direct.items() if k[1] == dt and k[2]} == {0, 1}, dt
    normed_tile = [p for k, p in tile.items() if k[2]]
    for f in ("nw_vec16", "cs_vec16", "hp1"):
        assert {p[f] for p in normed_tile} == {0, 1}, f
    # the shrinking tt, more than one token tile with B > 1, dead tokens in a direct tile
    assert any(p["tt"] < 64 // p["hpt"] for p in tile.values())
    assert any(p["t_tiles"] > 1 and R.SHAPES[k[0]][0] > 1 and R.SHAPES[k[0]][1] % p["tt"] for k, p in tile.items())
    assert any(p["t_tiles"] > 1 and R.SHAPES[k[0]][0] > 1 and R.SHAPES[k[0]][1] % p["tt"] for k, p in direct.items())
    # above 64 KB of LDS: the direct kernel with and without the norm.  The tile route cannot get there: its tt halves
    # until the tile fits 64 KB, and at tt = 1 the widest problem the entry point takes (CH 4, r = hd = 256, fp32) needs
    # 2 * 4096 + 2048 + 1024 + 16 + 512 bytes.
    assert {k[2] for k, p in direct.items() if p["lds_attr"]} == {False, True}
    assert not any(p["lds_attr"] for p in tile.values())
    worst = ops.rope_plan_at(torch.float32, 1, 1, 4, 1, 256, 256, 1025, 4, 1 << 20, 2 << 20, 0, None, 3 << 20, 4 << 20)
    assert worst["route"] == "tile" and worst["lds"] <= 64 * 1024
    # copy widths: everything between one element and 16 bytes
    for dt, widths in (("bf16", {2, 4, 8, 16}), ("f16", {2, 4, 8, 16}), ("f32", {4, 8, 16})):
        assert {p["wi"] for k, p in tile.items() if k[1] == dt} == widths, dt
        assert {p["wo"] for k, p in tile.items() if k[1] == dt} == widths, dt


def test_plan_refuses_what_the_kernel_refuses_and_empty_is_zero(ops):
    with pytest.raises(RuntimeError, match="even"):
        ops.rope_plan_at(torch.bfloat16, 1, 1, 4, 2, 3, 16, 12, 512, 1024, 2048, 0, 4096, None, 8192)
    with pytest.raises(RuntimeError, match="no mask"):
        ops.rope_plan_at(torch.bfloat16, 1, 1, 4, 2, 4, 16, 16, 512, 1024, 2048, 0, None, None, 8192)
    p = ops.rope_plan_at(torch.bfloat16, 0, 5, 4, 2, 4, 16, 16, 512, 1024, 2048, 0, 4096, None, 8192)
    assert p["n_tiles"] == 0 and p["grid"] == (0, 0, 0)


def test_bench_shape_plan_is_the_pre_refactor_dispatch(ops):
    """bench.py's rope row: [16, 2048, 32 x 88] bf16, 8 kv heads, head_dim 128, masked, no norm.  The values below are read
    off the dispatch code as it stood before it became rope_plan: group 4 -> hpt 4; half 44 -> vec 4; direct kernel;
    16 tokens per tile -> 128 tiles per batch, 2048 tiles; grid (8 * 8, 2048 / 8, 1); LDS (16 * 2 + 1) * 128 * 2 bytes."""
    p = ops.rope_plan_at(torch.bfloat16, 16, 2048, 32, 8, 88, 128, 32 * 88, 1 << 30, 2 << 30, 3 << 30, 0, 4 << 30, None, 5 << 30)
    assert R.variant_of(p) == "direct hpt4 vec4 it1 os1 cs1 nw0 big0 tiles128"
    assert p["grid"] == (64, 256, 1) and p["n_tiles"] == 2048 and p["lds"] == 8448 and p["tt"] == 16
