"""CPU models of the post-RoPE row tests (test_rope_rows_host.py on the CPU, test_gpu_rope_rows.py and test_gpu_qk_rope_stat.py on
the GPU): torch on the CPU, no engine.

rope_rows(x, cos, sin, n_heads, hd) is torch's eager expression x * cos + rotate_half(x) * sin on x viewed as [B, T, n_heads, hd]:
every product and the sum is rounded to the tensor dtype by the op that forms it.  test_rope_rows_host.py pins it, bit for bit, to
transformers.models.llama.modeling_llama.apply_rotary_pos_emb on every case below, so the GPU tests compare the kernel with the
library's expression and not with the engine.
"""
import functools

import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
HEAD_DIMS = (2, 6, 16, 64, 128, 256)          # 2: one pair; 6: an odd half; 16: the smallest with a 16-byte pack per half (bf16, f32)
N_HEADS = (1, 3, 5, 8, 6)                     # 1, 3, 5: one head per lane item; 6: two; 8: four
BT = ((1, 1), (1, 5), (2, 70))
TABLES = ("shared", "per_batch_halves_differ")


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def rope_rows(x, cos, sin, n_heads, hd):
    """x [B, T, n_heads*hd], cos / sin [B or 1, T, hd] of x's dtype -> x's shape."""
    B, T, W = x.shape
    xv = x.reshape(B, T, n_heads, hd)
    c, s = cos[:, :, None, :], sin[:, :, None, :]
    return ((xv * c) + (rotate_half(xv) * s)).reshape(B, T, W)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(got, want):
    """Bit equality, signs of zeros included.  NaNs must sit at the same places; their payload and sign are not compared (IEEE 754
    leaves the NaN an operation returns to the implementation, and x86 and the GPU differ there)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(bits(got)[~gn], bits(want)[~wn]))


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(dt, hd, n_heads, B, T, tables):
    """x [B, T, n_heads*hd] with rows at every scale from ~1e-5 to ~10 (tests/rope_ref.make_inputs), a -0.0, a 60000 (representable
    in f16), an all-zero row and an all-(-0.0) row where there are rows to spare; cos / sin per `tables`; the expected rows.
    Computed once per case, never modified."""
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(((hd * 16 + n_heads) * 4 + B) * 128 + T + 7 * TABLES.index(tables))
    scale = 10.0 ** (-2.5 + 1.0 * torch.randn(B, T, n_heads, 1, generator=gen)).clamp(-5.0, 1.0)
    x = torch.randn(B, T, n_heads, hd, generator=gen) * scale
    x[0, 0, 0, 0] = -0.0
    x[0, 0, 0, hd - 1] = 60000.0
    if B * T * n_heads > 1:
        x[B - 1, T - 1, n_heads - 1] = 0.0
    if B * T * n_heads > 2:
        x[B - 1, T - 1, 0] = -0.0
    x = x.to(dtype).reshape(B, T, n_heads * hd)
    Bc = 1 if tables == "shared" else B
    if tables == "shared":
        ang = torch.rand(Bc, T, hd // 2, generator=gen) * 6.28
        emb = torch.cat((ang, ang), -1)
    else:
        emb = torch.rand(Bc, T, hd, generator=gen) * 6.28          # the two halves are independent: nothing may assume them equal
    c = Case()
    c.x, c.cos, c.sin = x, emb.cos().to(dtype), emb.sin().to(dtype)
    c.n_heads, c.hd, c.dims = n_heads, hd, (B, T)
    c.want = rope_rows(c.x, c.cos, c.sin, n_heads, hd)
    return c


def all_cases(dt, hd):
    for n_heads in N_HEADS:
        for B, T in BT:
            for tables in TABLES:
                yield make_case(dt, hd, n_heads, B, T, tables)


# ---------------------------------------------------------------- the exact lattice of test_gpu_qk_rope_stat.py
def lattice_case(hd, n_heads, tokens, seed):
    """x[t, c] = m 2^e_c with integer |m| <= 15 and e_c = e_{c + hd/2} (bf16 holds it exactly), tables of quarter turns only --
    (cos, sin) in {(1, 0), (0, 1), (-1, 0), (0, -1)} per token and pair, both halves alike -- so every rotated value is +- a lattice
    value and every product of two of them, and every sum of such products over the tokens, is exact in fp64.
    Returns (x [1, tokens, n_heads*hd] bf16, cos, sin [1, tokens, hd] bf16)."""
    gen = torch.Generator().manual_seed(seed)
    half = hd // 2
    e = torch.randint(-6, 7, (half,), generator=gen)
    e = torch.cat((e, e)).double()
    m = torch.randint(-15, 16, (1, tokens, n_heads, hd), generator=gen).double()
    x = (m * 2.0 ** e).to(torch.bfloat16).reshape(1, tokens, n_heads * hd)
    turn = torch.randint(0, 4, (1, tokens, half), generator=gen)
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[turn]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[turn]
    return x, torch.cat((cos, cos), -1).to(torch.bfloat16), torch.cat((sin, sin), -1).to(torch.bfloat16)
