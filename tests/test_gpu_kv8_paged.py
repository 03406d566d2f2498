"""The paged fp8 KV cache on the GPU: ops.kv8_paged_append / ops.kv8_paged_dequant bit for bit against the CPU reference of
tests/test_gpu_kv8.py laid into pages by a shuffled block table, and ops.attn_decode_paged8 per sequence (a) within mdg_attn_decode's
bound 4 u max_j |v_deq| of the float64 softmax over the sequence's own dequantised keys and (b) bit-identical to ops.attn_decode_kv8
on that sequence alone.  Pages no sequence may read hold e4m3 NaN bytes and NaN scales: a wrong read shows as NaN, never as a fault."""
import pytest
import torch

from tests import attn_ref as R
from tests.test_gpu_kv8 import NAN8, graded, quantise, reference

pytestmark = pytest.mark.gpu
KV = 2


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def pool_of(n_pages, page, pitch, byte, scale, dev):
    return (torch.full((n_pages, KV, page, pitch), byte, dtype=torch.uint8, device=dev),
            torch.full((n_pages, KV, page), scale, device=dev))


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("width", [(6, 3), (90, 77), (256, 256)], ids=lambda w: "qk%d-vo%d" % w)
@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_append_lands_every_row_in_its_page_bit_for_bit_and_the_gather_inverts_it(ops, dev, dt, page, width, T):
    dtype, B, n_pages = R.DTYPES[dt], 3, 9
    pos = (0, page - 2, page)                                     # a fresh sequence, rows across a page boundary, a new page's start
    table = torch.tensor([[7, 2], [0, 8], [5, 1]], dtype=torch.int32)     # shuffled, non-monotone; pages 3, 4, 6 belong to nobody
    k_src = graded((B, KV, T, width[0]), dtype, 31 * width[0] + T)
    v_rows = graded((B, T, KV, width[1]), dtype, 37 * width[1] + T)       # token-major, as a projection writes V
    k_src[0, 0, 0] = 0                                                    # an all-zero row
    pools = [pool_of(n_pages, page, ops.kv8_pitch(r), 0xAB, -7.0, dev) for r in width]
    ops.kv8_paged_append(k_src.to(dev), v_rows.to(dev).transpose(1, 2), pools[0], pools[1], table.to(dev), torch.tensor(pos, dtype=torch.int32).to(dev))
    for (data, scale), src, r in zip(pools, (k_src, v_rows.transpose(1, 2)), width):
        want_d, want_s = (t.cpu().clone() for t in pool_of(n_pages, page, ops.kv8_pitch(r), 0xAB, -7.0, "cpu"))
        q8, s = quantise(src)
        for b in range(B):
            for t in range(T):
                pid, off = int(table[b, (pos[b] + t) // page]), (pos[b] + t) % page
                want_d[pid, :, off] = 0                                   # the padding bytes
                want_d[pid, :, off, :r] = q8[b, :, t]
                want_s[pid, :, off] = s[b, :, t]
        assert torch.equal(data.cpu(), want_d) and torch.equal(scale.cpu(), want_s), f"r={r}: the pool differs from the reference"
        back = ops.kv8_paged_dequant((data, scale), table.to(dev), 2 * page, r, dtype).cpu()
        exact = (want_d.view(torch.float8_e4m3fn).float() * want_s[..., None])[table.long()]     # [B, 2, KV, page, pitch]
        exact = exact.transpose(1, 2).reshape(B, KV, 2 * page, -1)[..., :r]
        normal = torch.ones_like(exact, dtype=torch.bool) if dt == "bf16" else (exact == 0) | (exact.abs() >= 2.0 ** -14)
        for b in range(B):                                                # the rows the append wrote (the others hold the fill)
            rows = slice(pos[b], pos[b] + T)
            assert torch.equal(back[b, :, rows].float()[normal[b, :, rows]], exact[b, :, rows][normal[b, :, rows]]), f"r={r}: gather"


def lay(x, page, pids, pool, S_cap, dev, ops):
    """Sequence rows x [1, KV, S, r] quantised into pages `pids` of the CPU pool (data, scale) and, NaN-encoded beyond S, into a
    contiguous cache of S_cap rows on the GPU: returns (data, scale) of that cache and the dequantised values in x's dtype."""
    S, r = x.shape[2], x.shape[3]
    q8, s = quantise(x)
    data = torch.full((1, KV, S_cap, pool[0].shape[3]), NAN8, dtype=torch.uint8)
    scale = torch.full((1, KV, S_cap), float("nan"))
    data[:, :, :S] = 0
    data[:, :, :S, :r] = q8
    scale[:, :, :S] = s
    for p, pid in enumerate(pids):
        n = min(S - p * page, page)
        pool[0][pid, :, :n] = data[0, :, p * page:p * page + n]
        pool[1][pid, :, :n] = scale[0, :, p * page:p * page + n]
    return data.to(dev), scale.to(dev), (q8.view(torch.float8_e4m3fn).float() * s[..., None]).to(x.dtype)


def paged_batch(dt, page, width, lens, dev, ops, seed):
    """B = len(lens) sequences in shuffled pages; table entries beyond a sequence's pages point at a poison page; poison pages,
    unused pages and rows beyond S_b hold NaN.  Returns (pools on the GPU, table, per-sequence (k cache, v cache, k_deq, v_deq))."""
    dtype, B = R.DTYPES[dt], len(lens)
    table_len = -(-max(lens) // page) + 1
    n_pages = sum(-(-S // page) for S in lens) + 3
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    poison, free = perm[0], perm[1:]
    table = torch.full((B, table_len), poison, dtype=torch.int32)
    pools = [(torch.full((n_pages, KV, page, ops.kv8_pitch(r)), NAN8, dtype=torch.uint8), torch.full((n_pages, KV, page), float("nan")))
             for r in width]
    seqs = []
    for b, S in enumerate(lens):
        if S == 0:                                                        # an empty slot: its table row is all poison
            seqs.append(None)
            continue
        pids = [free.pop() for _ in range(-(-S // page))]
        table[b, :len(pids)] = torch.tensor(pids, dtype=torch.int32)
        kd, ks, k = lay(graded((1, KV, S, width[0]), dtype, seed + 10 * b + 1), page, pids, pools[0], S + 3, dev, ops)
        vd, vs, v = lay(graded((1, KV, S, width[1]), dtype, seed + 10 * b + 2), page, pids, pools[1], S + 3, dev, ops)
        seqs.append((kd, ks, vd, vs, k, v))
    return [(d.to(dev), s.to(dev)) for d, s in pools], table.to(dev), seqs


def check_batch(ops, dev, dt, page, width, G, T, lens, splits_list, causal, mask=None):
    (r_qk, r_vo), dtype, B, H = width, R.DTYPES[dt], len(lens), KV * G
    pools, table, seqs = paged_batch(dt, page, width, lens, dev, ops, 1000 * r_qk + 10 * page + G)
    q = torch.randn(B, H, T, r_qk, generator=torch.Generator().manual_seed(r_qk + G)).to(dtype)
    raw = max(float((q[b:b + 1].double() @ s[4].double().repeat_interleave(G, dim=1).transpose(2, 3)).abs().max()) for b, s in enumerate(seqs) if lens[b])
    scale = min(r_qk ** -0.5, 20.0 / raw)
    seq_lens = torch.tensor(lens, dtype=torch.int32).to(dev)
    for splits in splits_list:
        torch.full((1 << 20,), float("nan"), device=dev)                  # what the call's workspace lands on
        padded = torch.full((B, T, H * r_vo + 5), 7.0, dtype=dtype, device=dev)       # out: a caller-owned view with sentinel padding
        out = padded[..., :H * r_vo].view(B, T, H, r_vo)
        got = ops.attn_decode_paged8(q.to(dev), pools[0], pools[1], table, seq_lens, r_vo, scale, causal=causal, max_S=max(lens),
                                     splits=splits, out=out, mask=None if mask is None else mask.to(dev))
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
            print(f"{dt} page{page} qk{r_qk} vo{r_vo} G{G} T{T} S{S} causal={causal} splits={splits}: max err / bound = "
                  f"{float((err / bound.clamp(min=1e-300)).max()):.3f}")
            assert bool((err <= bound).all()), f"sequence {b} (S={S}), {splits} splits"
            alone = ops.attn_decode_kv8(q[b:b + 1].to(dev), kd, ks, vd, vs, S, r_vo, scale, causal=causal, splits=splits,
                                        mask=None if mask is None else mask[b:b + 1, :, :, :S].contiguous().to(dev)).cpu()
            assert torch.equal(R.bits(got[b:b + 1]), R.bits(alone)), f"sequence {b} (S={S}), {splits} splits: not the bits of attn_decode_kv8"


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("group", [(4, 1), (1, 3), (8, 4)], ids=lambda g: "G%d-T%d" % g)
@pytest.mark.parametrize("width", [(6, 3), (90, 77), (128, 128), (130, 200)], ids=lambda w: "qk%d-vo%d" % w)
@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_decode_gives_every_sequence_its_own_keys_and_the_bits_of_the_contiguous_kernel(ops, dev, dt, page, width, group, causal):
    G, T = group
    # one key past a tile and page edge, exactly full pages, the shortest causal length, an empty slot
    check_batch(ops, dev, dt, page, width, G, T, (257, 128, T, 0), (1, 3, 256), causal)


@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_decode_under_a_left_padded_mask_and_a_fully_masked_query(ops, dev, dt, page):
    T, lens = 3, (257, 128, 3, 0)
    mask = torch.zeros(len(lens), 1, T, max(lens), dtype=torch.bool)
    for b, S in enumerate(lens):                                          # the causal rule of each sequence lives in the mask
        mask[b, 0, :, :S] = R.admitted(T, S, True) if S else False
    mask[0, :, :, :70] = False                                            # sequence 0 is left-padded past the first tile
    mask[1, :, 1, :] = False                                              # a query that sees nothing
    check_batch(ops, dev, dt, page, (90, 77), 4, T, lens, (1, 3, 256), False, mask)
