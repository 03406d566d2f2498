"""mdg_qk_pair_accum -- the within-sequence, shift-invariant Q/K statistic  pair[h] += sum_s G^q_s (.) (G^k_s - m m^T / T)  and its
uncentred twin pair_raw, against the host models of tests/qk_pair_model.py.

Criteria (a priori, from the summation structure the header describes; nothing is fitted to what the kernel gives):
  LATTICE   integer rows |x| <= 8 (keys + 3), T a power of two: every product, sum and m m^T / T is exact in fp64 -> bit equality
            with the rational model
  GENERIC   |pair - long double| <= (4T + B + 8) 2^-53 sum_s sqrt(G^q_aa G^q_bb) sqrt(G^k_aa G^k_bb), entry-wise, same for pair_raw;
            at T = 1 pair is exactly zero
  ORDER     one call over B sequences = B single-sequence calls, in bits; two runs identical; accumulation; bit symmetry
  CROSS     B = 1: pair_raw against the Hadamard product of ops.cov_accum's per-head Grams, within the sum of both bounds
            ((4T + 9) + (2T + 2)) 2^-53 of the same scale: each Gram of cov_accum carries T roundings, their product one more
  CONTAIN   a NaN / Inf of q in head h reaches pair[h], pair_raw[h] only; of k in kv head v the heads of group v only
  REFUSE    every refusal returns MDG_ERR_BAD_ARG with its message and leaves the outputs untouched; B = 0, T = 0 launch nothing
  CURVE     ops.qk_rank_curve(P, ones, ridges 0) on an integer-valued P equals the plain sum over the dropped block, bit for bit

MEASURED on an MI355X: LATTICE bit-equal at every shape; GENERIC largest error / bound, bf16 0.038 / 0.048 / 0.052 (hd 6 / 40 / 128), f16
0.046 / 0.071 / 0.099, f32 0.095 / 0.135 / 0.177; CROSS 0.0000 at hd 128 and 40 (the two kernels round alike)."""
import numpy as np
import pytest
import torch

from tests import qk_pair_model as M

pytestmark = pytest.mark.gpu
F64 = torch.float64
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int64)


def place(x, dev, layout):
    """The rows on the device: "plain" contiguous; "padded" pitch = width + 8 elements; "offset" a view one element into a
    buffer (a pointer that is not 16-byte aligned: the element-wise path)."""
    n, w = x.shape
    if layout == "plain":
        return x.to(dev).contiguous()
    if layout == "padded":
        buf = torch.full((n, w + 8), 7.0, dtype=x.dtype, device=dev)       # the padding holds a value that must not be read
        buf[:, :w] = x.to(dev)
        return buf[:, :w]
    buf = torch.full((n * w + 1,), 7.0, dtype=x.dtype, device=dev)
    v = buf[1:].view(n, w)
    v.copy_(x.to(dev))
    return v


def run(ops, dev, q, k, B, T, H, KV, hd, layout="plain", raw=True, into=None):
    pair = torch.zeros(H, hd, hd, dtype=F64, device=dev) if into is None else into[0]
    pr = (torch.zeros(H, hd, hd, dtype=F64, device=dev) if into is None else into[1]) if raw else None
    ops.qk_pair_accum(pair, pr, place(q, dev, layout), place(k, dev, layout), B, T, H, KV, hd)
    return pair, pr


# ---------------------------------------------------------------- exact lattice
@pytest.mark.parametrize("hd", [8, 64, 128])
@pytest.mark.parametrize("g", [1, 4])
def test_lattice_equals_the_rational_model_bit_for_bit(ops, dev, hd, g):
    KV = 1 if hd == 128 else 2
    H = KV * g
    for T in (16, 64):
        for B in (1, 3):
            q = M.lattice_rows(B, T, H, hd, 100 + hd + T + B)
            k = M.lattice_rows(B, T, KV, hd, 200 + hd + T + B, offset=3)
            want, want_raw = M.exact_pair(q, k, B, T, H, KV, hd)
            pair, raw = run(ops, dev, q, k, B, T, H, KV, hd)
            assert torch.equal(bits(pair), bits(want)), "LATTICE pair hd %d g %d T %d B %d" % (hd, g, T, B)
            assert torch.equal(bits(raw), bits(want_raw)), "LATTICE pair_raw hd %d g %d T %d B %d" % (hd, g, T, B)
    print("LATTICE hd %d g %d: pair and pair_raw equal the rational model bit for bit, T 16 / 64, B 1 / 3" % (hd, g))


# ---------------------------------------------------------------- generic data
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("hd", [6, 40, 128])
def test_generic_within_the_derived_bound(ops, dev, dt, hd):
    KV = 1 if hd == 128 else 2
    H = 2 * KV
    layouts = ("plain", "padded", "offset")
    worst, n = 0.0, 0
    for T in (1, 5, 17, 100):
        for B in (1, 2, 5):
            layout = layouts[n % 3]
            n += 1
            q = M.generic_rows(B, T, H, hd, 1000 + n, DT[dt])
            k = M.generic_rows(B, T, KV, hd, 2000 + n, DT[dt], mean_sigmas=20.0)
            P, R, scale = M.longdouble_pair(q, k, B, T, H, KV, hd)
            lim = M.bound(scale, B, T)
            pair, raw = run(ops, dev, q, k, B, T, H, KV, hd, layout=layout)
            for name, got, ref in (("pair", pair, P), ("pair_raw", raw, R)):
                err = np.abs(got.cpu().numpy().astype(M.LD) - ref)
                assert bool((err[lim == 0] == 0).all())
                frac = float((err[lim > 0] / lim[lim > 0]).max())
                worst = max(worst, frac)
                assert frac <= 1.0, "GENERIC %s %s hd %d T %d B %d %s: error / bound = %.3g" % (name, dt, hd, T, B, layout, frac)
            if T == 1:
                assert bool((pair == 0).all()), "T = 1: the centred statistic must be exactly zero"
            assert torch.equal(bits(pair), bits(pair.transpose(1, 2))) and torch.equal(bits(raw), bits(raw.transpose(1, 2)))
    print("GENERIC %s hd %d: largest error / bound = %.4f over T 1/5/17/100 x B 1/2/5, three layouts" % (dt, hd, worst))


# ---------------------------------------------------------------- order and determinism
@pytest.mark.parametrize("hd,layout", [(128, "plain"), (40, "offset")])
def test_order_determinism_accumulation_symmetry(ops, dev, hd, layout):
    B, T, H, KV = 4, 37, 4, 2
    q = M.generic_rows(B, T, H, hd, 31, torch.bfloat16)
    k = M.generic_rows(B, T, KV, hd, 32, torch.bfloat16, mean_sigmas=20.0)
    one = run(ops, dev, q, k, B, T, H, KV, hd, layout=layout)
    again = run(ops, dev, q, k, B, T, H, KV, hd, layout=layout)
    acc = (torch.zeros(H, hd, hd, dtype=F64, device=dev), torch.zeros(H, hd, hd, dtype=F64, device=dev))
    for b in range(B):
        run(ops, dev, q[b * T:(b + 1) * T], k[b * T:(b + 1) * T], 1, T, H, KV, hd, layout=layout, into=acc)
    for x, y, z in zip(one, again, acc):
        assert torch.equal(bits(x), bits(y)), "two runs differ"
        assert torch.equal(bits(x), bits(z)), "one call over B = 4 differs from four single-sequence calls"
        assert torch.equal(bits(x), bits(x.transpose(1, 2))), "triangles differ"
    # a non-zero accumulator is added to: pair0 + (one call's sum), the sum folded onto pair0 one sequence at a time
    start = torch.full((H, hd, hd), 3.0, dtype=F64, device=dev)
    got = run(ops, dev, q, k, B, T, H, KV, hd, layout=layout, into=(start.clone(), start.clone()))
    scale = torch.from_numpy(M.longdouble_pair(q, k, B, T, H, KV, hd)[2].astype(np.float64)).to(dev)     # >= sum_s |p_s| entry-wise
    for gt, x in zip(got, one):
        assert not torch.equal(bits(gt), bits(x))
        tol = 2 * (B + 1) * M.U * (3.0 + scale)                      # B roundings of a running sum on either side
        assert bool(((gt - (x + 3.0)).abs() <= tol).all())
    # without pair_raw: the same pair
    only, none = run(ops, dev, q, k, B, T, H, KV, hd, layout=layout, raw=False)
    assert none is None and torch.equal(bits(only), bits(one[0]))


# ---------------------------------------------------------------- cross-check against the covariance kernel
@pytest.mark.parametrize("hd", [128, 40])
def test_raw_equals_the_product_of_cov_accum_grams(ops, dev, hd):
    T, H, KV = 100, 4, 2
    q = M.generic_rows(1, T, H, hd, 41, torch.bfloat16)
    k = M.generic_rows(1, T, KV, hd, 42, torch.bfloat16, mean_sigmas=20.0)
    _, raw = run(ops, dev, q, k, 1, T, H, KV, hd)
    sq = torch.zeros(H, hd, hd, dtype=F64, device=dev)
    sk = torch.zeros(KV, hd, hd, dtype=F64, device=dev)
    ops.cov_accum(sq, q.to(dev), n_heads=H)
    ops.cov_accum(sk, k.to(dev), n_heads=KV)
    ops.cov_finalize(sq, 1.0)
    ops.cov_finalize(sk, 1.0)
    want = sq * sk.repeat_interleave(H // KV, 0)
    _, _, scale = M.longdouble_pair(q, k, 1, T, H, KV, hd)
    lim = ((4 * T + 9) + (2 * T + 2)) * M.U * scale
    err = np.abs(raw.cpu().numpy().astype(M.LD) - want.cpu().numpy().astype(M.LD))
    frac = float((err / lim).max())
    print("CROSS hd %d: |pair_raw - sigma_q (.) sigma_k| / bound = %.4f" % (hd, frac))
    assert frac <= 1.0


# ---------------------------------------------------------------- non-finite containment
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_stays_in_its_heads(ops, dev, bad):
    B, T, H, KV, hd = 2, 19, 4, 2, 40
    q = M.generic_rows(B, T, H, hd, 51, torch.bfloat16)
    k = M.generic_rows(B, T, KV, hd, 52, torch.bfloat16, mean_sigmas=20.0)
    clean = run(ops, dev, q, k, B, T, H, KV, hd)
    qb = q.clone()
    qb[T + 3, 1 * hd + 5] = bad                                   # head 1, second sequence
    for got, ref in zip(run(ops, dev, qb, k, B, T, H, KV, hd), clean):
        assert not bool(torch.isfinite(got[1]).all())
        for h in (0, 2, 3):
            assert torch.equal(bits(got[h]), bits(ref[h])), "q non-finite in head 1 reached head %d" % h
    kb = k.clone()
    kb[2, 1 * hd + 7] = bad                                       # kv head 1 serves heads 2, 3
    for got, ref in zip(run(ops, dev, q, kb, B, T, H, KV, hd), clean):
        assert not bool(torch.isfinite(got[2]).all()) and not bool(torch.isfinite(got[3]).all())
        for h in (0, 1):
            assert torch.equal(bits(got[h]), bits(ref[h])), "k non-finite in kv head 1 reached head %d" % h


# ---------------------------------------------------------------- refusals and empty calls
def test_refusals_and_empty_calls_touch_nothing(ops, dev):
    from modegpt_amd import _lib
    lib = _lib.load()
    B, T, H, KV, hd = 2, 8, 4, 2, 16
    q = torch.ones(B * T, H * hd, dtype=torch.bfloat16, device=dev)
    k = torch.ones(B * T, KV * hd, dtype=torch.bfloat16, device=dev)
    pair = torch.full((H, hd, hd), 5.0, dtype=F64, device=dev)
    raw = torch.full((H, hd, hd), 6.0, dtype=F64, device=dev)
    need = lib.mdg_qk_pair_ws_bytes(B, H, hd, 1)
    assert need == 2 * 8 * B * H * hd * hd and lib.mdg_qk_pair_ws_bytes(B, H, hd, 0) == need // 2
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    good = dict(q=q.data_ptr(), ld_q=H * hd, k=k.data_ptr(), ld_k=KV * hd, dtype=_lib.MDG_BF16, B=B, T=T, n_heads=H, n_kv=KV, hd=hd,
                pair=pair.data_ptr(), pair_raw=raw.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)

    def call(**over):
        a = {**good, **over}
        return lib.mdg_qk_pair_accum(a["q"], a["ld_q"], a["k"], a["ld_k"], a["dtype"], a["B"], a["T"], a["n_heads"], a["n_kv"], a["hd"],
                                     a["pair"], a["pair_raw"], a["ws"], a["ws_bytes"], torch.cuda.current_stream(dev).cuda_stream)

    refused = [(dict(dtype=_lib.MDG_F64), "dtype"), (dict(dtype=9), "dtype"), (dict(hd=0), "head_dim"), (dict(hd=129), "head_dim"),
               (dict(n_heads=0), "n_heads"), (dict(n_kv=0), "n_kv"), (dict(n_kv=3), "n_kv"), (dict(ld_q=H * hd - 1), "ld_q"),
               (dict(ld_k=KV * hd - 1), "ld_k"), (dict(B=-1), "negative"), (dict(T=-1), "negative"), (dict(q=None), "null"),
               (dict(k=None), "null"), (dict(pair=None), "null"), (dict(ws=None), "null"), (dict(ws_bytes=need - 1), "workspace")]
    for over, word in refused:
        assert call(**over) == _lib.MDG_ERR_BAD_ARG, over
        msg = _lib.last_error()
        assert msg.startswith("mdg_qk_pair_accum:") and word in msg, (over, msg)
    for over in (dict(B=0), dict(T=0), dict(B=0, q=None, k=None, ws=None, ws_bytes=0)):
        assert call(**over) == _lib.MDG_OK, over
    torch.cuda.synchronize()
    assert bool((pair == 5.0).all()) and bool((raw == 6.0).all()), "a refused or empty call wrote to the outputs"
    # the Python surface refuses with its own messages, and takes empty calls
    with pytest.raises(ValueError, match="multiple of n_kv"):
        ops.qk_pair_accum(pair, raw, q, k, B, T, H, 3, hd)
    with pytest.raises(ValueError, match="head_dim"):
        ops.qk_pair_accum(pair, raw, q, k, B, T, H, KV, 200)
    with pytest.raises(ValueError, match="q_rows must be"):
        ops.qk_pair_accum(pair, raw, q[:-1], k, B, T, H, KV, hd)
    with pytest.raises(ValueError, match="pair must be"):
        ops.qk_pair_accum(pair.float(), raw, q, k, B, T, H, KV, hd)
    ops.qk_pair_accum(pair, raw, q[:0], k[:0], 0, T, H, KV, hd)
    torch.cuda.synchronize()
    assert bool((pair == 5.0).all()) and bool((raw == 6.0).all())
    assert call() == _lib.MDG_OK                                  # and the good call does run
    torch.cuda.synchronize()
    assert bool((raw == 6.0 + B * T * T).all()) and bool((pair == 5.0).all())      # all-ones rows: G = T, centred part 0


# ---------------------------------------------------------------- the report's kernel on (P, ones)
@pytest.mark.parametrize("g", [1, 2])
def test_rank_curve_on_p_and_ones_is_the_plain_sum_over_the_dropped_block(ops, dev, g):
    """metrics["qk_logit_error_seq"] comes from the existing ops.qk_rank_curve with cov_q = P, cov_k = ones, ridges 0: a product with
    1.0 is exact, so on an integer-valued P the curve equals sum_{a,b in D} P_h[a,b] bit for bit at every rank."""
    from modegpt_amd import _lib
    KV, hd = 2, 16
    H, ns = KV * g, hd // 2
    gen = torch.Generator().manual_seed(7 + g)
    A = torch.randint(-9, 10, (H, hd, hd), generator=gen).to(F64)
    P = (A + A.transpose(1, 2)).to(dev)
    order = torch.stack([torch.randperm(ns, generator=gen) for _ in range(KV)]).to(dev)
    mode = _lib.MDG_QK_ROPE_GROUPED if g > 1 else _lib.MDG_QK_ROPE_MHA
    ones = torch.ones(KV, hd, hd, dtype=F64, device=dev)
    curve_h, curve = (t.cpu() for t in ops.qk_rank_curve(P, ones, mode, 0.0, 0.0, order, want_greedy=False)[:2])
    Pc, oc = P.cpu(), order.cpu()
    for m in range(ns + 1):
        for kv in range(KV):
            D = torch.cat((oc[kv][m:], oc[kv][m:] + ns))
            per_head = [float(Pc[h][D][:, D].sum()) for h in range(kv * g, (kv + 1) * g)]
            assert [float(curve_h[h][m]) for h in range(kv * g, (kv + 1) * g)] == per_head
            assert float(curve[kv][m]) == sum(per_head)
