"""The attention kernels' template matrix stays closed (no GPU, no library call).

attn_fwd_kernel and attn_decode_kernel are instantiated per (NQ, NV) in {4, 8, 16} x {2, 4, 8} (tests/attn_ref.template_of), and the
instantiations differ in more than a constant: launch bounds, prefetch, staging trip counts, LDS size.  Each of the four families of
GPU tests -- prefill and decode, unmasked and masked -- must run all nine; a shape list that loses one fails here, on any machine.
Also: the trip-count sweep reaches every nq and every nv, the first width of every bucket and the last of the one below occur, and
the weight probe's CPU assertions (tests/attn_ref.py) hold for every probe case."""
import pytest
import torch

from tests import attn_ref as R
from tests import test_gpu_attn_decode, test_gpu_attn_mask

ALL = set(R.TEMPLATES)


def templates(shapes):
    return {R.template_of(s[0], s[1]) for s in shapes}


def test_template_of_states_the_buckets():
    assert len(ALL) == 9
    assert [R.template_of(r, 1)[0] for r in (2, 64, 66, 128, 130, 256)] == [4, 4, 8, 8, 16, 16]
    assert [R.template_of(2, r)[1] for r in (1, 64, 65, 128, 129, 256)] == [2, 2, 4, 4, 8, 8]


@pytest.mark.parametrize("family, shapes", [
    ("prefill, unmasked: attn_ref.SHAPES", R.SHAPES),
    ("prefill, masked: test_gpu_attn_mask.WIDTHS + EDGE_WIDTHS", test_gpu_attn_mask.WIDTHS + test_gpu_attn_mask.EDGE_WIDTHS),
    ("decode, unmasked: test_gpu_attn_decode.SHAPES", test_gpu_attn_decode.SHAPES),
    ("decode, masked: test_gpu_attn_mask.WIDTHS + EDGE_WIDTHS", test_gpu_attn_mask.WIDTHS + test_gpu_attn_mask.EDGE_WIDTHS),
    ("the weight probe, all four: attn_ref.PROBE_WIDTHS", R.PROBE_WIDTHS),
], ids=["prefill", "prefill-masked", "decode", "decode-masked", "probe"])
def test_every_family_runs_all_nine_templates(family, shapes):
    missing = ALL - templates(shapes)
    assert not missing, f"{family} runs no shape of template(s) (NQ, NV) = {sorted(missing)}"


def test_decode_shapes_fit_the_decode_kernel():
    for r_qk, r_vo, T, S, H, KV in test_gpu_attn_decode.SHAPES + R.sweep_shapes(R.SWEEP_DECODE_TS):
        assert T * (H // KV) <= 32
    for w in test_gpu_attn_mask.WIDTHS + test_gpu_attn_mask.EDGE_WIDTHS:
        assert any(T * (w[2] // w[3]) <= 32 for T, S in test_gpu_attn_mask.decode_ts(w)), w
    for w in R.PROBE_WIDTHS:
        assert all(T * (w[2] // w[3]) <= 32 for T, S in R.PROBE_DECODE_TS), w


def test_the_sweep_reaches_every_trip_count():
    assert len(R.SWEEP) == 32
    assert {-(-r_qk // 16) for r_qk, _ in R.SWEEP} == set(range(1, 17))
    assert {-(-r_vo // 32) for _, r_vo in R.SWEEP} == set(range(1, 9))
    assert all(r_qk % 2 == 0 and r_qk % 16 == 14 for r_qk, _ in R.SWEEP)
    assert {r_vo % 32 for _, r_vo in R.SWEEP} == {1, 31}                    # both ends of the last column tile


def test_the_bucket_edges_occur():
    shapes = (R.SHAPES + test_gpu_attn_decode.SHAPES + test_gpu_attn_mask.WIDTHS + test_gpu_attn_mask.EDGE_WIDTHS + R.PROBE_WIDTHS)
    r_qks, r_vos = {s[0] for s in shapes}, {s[1] for s in shapes}
    assert {64, 66, 128, 130} <= r_qks, sorted({64, 66, 128, 130} - r_qks)
    assert {64, 65, 128, 129} <= r_vos, sorted({64, 65, 128, 129} - r_vos)


@pytest.mark.parametrize("width", R.PROBE_WIDTHS, ids=R.width_id)
def test_the_probe_is_exact_on_paper(width):
    """probe_case asserts bit-identical fp32 logits per query, exact integers and the window partition; probe_admissions asserts
    n <= 2^24 and rows with n = 0, n = 1 and n = S; probe_expected that the two accepted roundings are equal or neighbours."""
    r_qk, r_vo, H, KV = width
    for dt in sorted(R.DTYPES):
        for T, S in R.PROBE_FWD_TS + R.PROBE_DECODE_TS:
            p = R.probe_case(dt, width, T, S)
            assert p.windows[0] == 0 and len(p.windows) == -(-S // r_vo)
            v = torch.stack([R.probe_values(p, dt, j0) for j0 in p.windows])
            assert torch.equal((v != 0).sum(dim=(0, 4)), torch.ones(R.B, KV, S, dtype=torch.int64))   # every key probed exactly once
            kinds = set()
            for ad in R.probe_admissions(T, S, H):
                kinds.add((ad.name, ad.layout))
                if dt == "bf16" or ad.layout in (None, "contiguous"):
                    lo, hi, differ = R.probe_expected(p, dt, ad.adm, width)
                    assert lo.shape == (R.B, T, H, len(p.windows) * r_vo) and differ <= int(ad.adm.sum())
            assert len(kinds) == 1 + len(R.PROBE_KINDS) * len(R.PROBE_LAYOUTS)


def test_the_tile_mask_holds_every_state():
    """The whole-tile mask at the prefill shape: tiles of all three summary states, and a key tile no unit admits."""
    from tests.test_gpu_attn_mask import summary_ref
    T, S = R.PROBE_FWD_TS[0]
    for ad in R.probe_admissions(T, S, 4):
        if ad.name == "tiles" and ad.layout in ("contiguous", "per-head") and not ad.causal:
            s = summary_ref(ad.base.expand(R.B, ad.base.shape[1], T, S))
            assert set(s.flatten().tolist()) == {0, 1, 2}
            assert bool((s[..., -1] == 0).all())
