"""ops.attn_fwd_paged8 (mdg_attn_fwd_paged8: any T straight from the paged fp8 KV cache), per sequence (i) within the project's bound
4 u max_j |v_deq| of the float64 softmax over the sequence's own dequantised keys and (ii) bit-identical to ops.attn_fwd_kv8 on that
sequence alone.  The batches are tests/test_gpu_kv8_paged.py's: shuffled pages; poison pages, unused pages and rows beyond S_b hold
NaN, so a wrong read shows as NaN, never as a fault."""
import pytest
import torch

from tests import attn_ref as R
from tests.test_gpu_kv8 import graded, reference  # noqa: F401  (graded: what paged_batch lays out)
from tests.test_gpu_kv8_paged import KV, ops, paged_batch  # noqa: F401  (ops: a fixture)

pytestmark = pytest.mark.gpu
WINDOW = 256                                                              # csrc/attn_fwd_paged8.hip: table entries staged in LDS


def check_batch(ops, dev, dt, page, width, G, T, lens, causal, mask=None, alone=True):
    (r_qk, r_vo), dtype, B, H = width, R.DTYPES[dt], len(lens), KV * G
    pools, table, seqs = paged_batch(dt, page, width, lens, dev, ops, 1000 * r_qk + 10 * page + G)
    q = torch.randn(B, H, T, r_qk, generator=torch.Generator().manual_seed(r_qk + G)).to(dtype)
    raw = max(float((q[b:b + 1].double() @ s[4].double().repeat_interleave(G, dim=1).transpose(2, 3)).abs().max()) for b, s in enumerate(seqs) if lens[b])
    scale = min(r_qk ** -0.5, 20.0 / raw)
    padded = torch.full((B, T, H * r_vo + 5), 7.0, dtype=dtype, device=dev)           # out: a caller-owned view with sentinel padding
    out = padded[..., :H * r_vo].view(B, T, H, r_vo)
    got = ops.attn_fwd_paged8(q.to(dev), pools[0], pools[1], table, torch.tensor(lens, dtype=torch.int32).to(dev), r_vo, scale,
                              causal=causal, max_S=max(lens), mask=None if mask is None else mask.to(dev), out=out)
    assert got is out and bool((padded[..., H * r_vo:] == 7.0).all()), "the padding of out was written"
    got = got.cpu()
    for b, S in enumerate(lens):
        if S == 0:
            assert bool((got[b] == 0).all()), "an empty slot must give zeros"
            continue
        kd, ks, vd, vs, k, v = seqs[b]
        adm = R.admitted(T, S, causal)[None, None].expand(1, H, T, S)
        if mask is not None:
            adm = adm & mask[b:b + 1, :, :, :S]
        want, vmax, _ = reference(q[b:b + 1], k, v, scale, adm)
        err = (got[b:b + 1].double() - want).abs()
        bound = 4.0 * R.UNIT_ROUNDOFF[dt] * vmax
        print(f"{dt} page{page} qk{r_qk} vo{r_vo} G{G} T{T} S{S} causal={causal} masked={mask is not None}: max err / bound = "
              f"{float((err / bound.clamp(min=1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), f"sequence {b} (S={S})"                    # a query without a key: bound 0, so zeros
        if alone and not (causal and S < T):                              # attn_fwd_kv8 refuses causal with S < T
            one = ops.attn_fwd_kv8(q[b:b + 1].to(dev), kd, ks, vd, vs, S, r_vo, scale, causal=causal,
                                   mask=None if mask is None else mask[b:b + 1, :, :, :S].contiguous().to(dev)).cpu()
            assert torch.equal(R.bits(got[b:b + 1]), R.bits(one)), f"sequence {b} (S={S}): not the bits of attn_fwd_kv8"


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("group", [(4, 1), (1, 33), (4, 40)], ids=lambda g: "G%d-T%d" % g)
@pytest.mark.parametrize("width", [(6, 3), (90, 77), (128, 128), (130, 200)], ids=lambda w: "qk%d-vo%d" % w)
@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_every_sequence_attends_over_its_own_pages_with_the_bits_of_the_contiguous_kernel(ops, dev, dt, page, width, group, causal):
    G, T = group      # one unit; two query tiles with a ragged last one; more than four units: two workgroups of one kv head
    # one key past a tile and page edge, exactly full pages, the shortest causal length, an empty slot
    check_batch(ops, dev, dt, page, width, G, T, (257, 128, max(T, 1), 0), causal)


@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_causal_with_fewer_keys_than_queries_gives_the_first_queries_zeros(ops, dev, dt):
    check_batch(ops, dev, dt, 64, (90, 77), 4, 40, (20, 5, 70), True, alone=False)


@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_a_left_padded_mask_and_a_fully_masked_query(ops, dev, dt, page):
    T, lens = 40, (257, 128, 40, 0)
    mask = torch.zeros(len(lens), 1, T, max(lens), dtype=torch.bool)
    for b, S in enumerate(lens):                                          # the causal rule of each sequence lives in the mask
        mask[b, 0, :, :S] = R.admitted(T, S, True) if S else False
    mask[0, :, :, :70] = False                                            # sequence 0 is left-padded past the first tile
    mask[1, :, 1, :] = False                                              # a query that sees nothing
    check_batch(ops, dev, dt, page, (90, 77), 4, T, lens, False, mask)


@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_a_sequence_longer_than_the_table_window(ops, dev, dt):
    check_batch(ops, dev, dt, 64, (6, 3), 1, 33, (64 * WINDOW + 65,), True)
