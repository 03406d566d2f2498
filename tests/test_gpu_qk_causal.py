"""mdg_qk_causal_accum -- the causal Q/K statistic  pair[h] += sum_s sum_i (q_i q_i^T) (.) (K_i / n_i - m_i m_i^T / n_i^2)  over the keys
j <= i each query can see, and its uncentred twin pair_raw, against the host models of tests/qk_causal_model.py.

Criteria (a priori, from the expression the header states; nothing is fitted to what the kernel gives):
  LATTICE   integer rows |x| <= 8 (keys + 3): every entry within the header's bound (4T + B + 8) 2^-53 A of the correctly rounded
            exact rational value (plus that value's own half ulp).  The kernel's expression is exact -- and the outputs then equal
            the rational model BIT FOR BIT -- exactly where every n_i is a power of two whose reciprocal multiplies exactly, i.e.
            T <= 2 (n = 1, 2): those cases are asserted to the bit, at every hd, g and B.  From T = 3 on 1 / 3 rounds and only the
            bound is promised (T 16 / 64).
  GENERIC   |pair - long double| <= (4T + B + 8) 2^-53 A, A = sum_s sum_i |q_ia q_ib| sqrt(K_i[a,a] K_i[b,b]) / n_i, entry-wise, same
            for pair_raw; at T = 1 pair is exactly zero
  ORDER     one call over B sequences = B single-sequence calls, in bits; two runs identical; accumulation; bit symmetry
  CONTAIN   a NaN / Inf of q in head h reaches pair[h], pair_raw[h] only; of k in kv head v the heads of group v only
  REFUSE    every refusal returns MDG_ERR_BAD_ARG with its message and leaves outputs AND workspace untouched; B = 0, T = 0 launch nothing
  DISAGREE  the case of tests/test_qk_causal_model_host.py on the device: ops.qk_select on (P^c, ones) and on (P, ones) give the
            masks the long-double model predicts, and the causal objective of the causal mask is <= that of the full mask
"""
import numpy as np
import pytest
import torch

from tests import qk_causal_model as C
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
    ops.qk_causal_accum(pair, pr, place(q, dev, layout), place(k, dev, layout), B, T, H, KV, hd)
    return pair, pr


# ---------------------------------------------------------------- exact lattice
@pytest.mark.parametrize("hd", [8, 64, 128])
@pytest.mark.parametrize("g", [1, 4])
def test_lattice_within_the_bound_of_the_rational_value_and_exact_where_the_expression_is(ops, dev, hd, g):
    KV = 1 if hd == 128 else 2
    H = KV * g
    worst = 0.0
    for T in (1, 2, 16, 64):
        for B in (1, 3):
            q = M.lattice_rows(B, T, H, hd, 100 + hd + T + B)
            k = M.lattice_rows(B, T, KV, hd, 200 + hd + T + B, offset=3)
            want, want_raw = C.exact_causal(q, k, B, T, H, KV, hd)
            pair, raw = run(ops, dev, q, k, B, T, H, KV, hd)
            if T <= 2:
                assert torch.equal(bits(pair), bits(want)), "LATTICE exact pair hd %d g %d T %d B %d" % (hd, g, T, B)
                assert torch.equal(bits(raw), bits(want_raw)), "LATTICE exact pair_raw hd %d g %d T %d B %d" % (hd, g, T, B)
                continue
            # A from integer data in fp64: sums of at most B T terms, each a product and a square root -- (B T + 4) roundings
            Q = M.split_heads(q.double().numpy(), B, T, H, hd)
            Kr = M.split_heads(k.double().numpy(), B, T, KV, hd)
            diag = np.sqrt(np.cumsum(Kr ** 2, axis=2))                              # [B, KV, T, hd]: sqrt(K_i[a,a])
            n = np.arange(1, T + 1, dtype=np.float64)[None, None, :, None]
            A = np.einsum("shia,shic->hac", np.abs(Q) * np.repeat(diag, g, axis=1) / n, np.abs(Q) * np.repeat(diag, g, axis=1))
            lim = torch.from_numpy((4 * T + B + 8) * M.U * A * (1 - (B * T + 4) * 2.0 ** -52))
            for name, got, ref in (("pair", pair, want), ("pair_raw", raw, want_raw)):
                err = (got.cpu() - ref).abs()                                       # (Sterbenz or not: one more rounding of the difference)
                tol = lim + 2 * M.U * ref.abs()                                     # the reference's own half ulp, and the difference's
                assert bool((err <= tol).all()), "LATTICE %s hd %d g %d T %d B %d: %.3g" % (name, hd, g, T, B, float((err / tol).max()))
                worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
            assert torch.equal(bits(pair), bits(pair.transpose(1, 2))) and torch.equal(bits(raw), bits(raw.transpose(1, 2)))
    print("LATTICE hd %d g %d: bit-equal at T 1 / 2; largest error / bound %.4f at T 16 / 64, B 1 / 3" % (hd, g, worst))


# ---------------------------------------------------------------- generic data
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("hd", [6, 40, 128])
def test_generic_within_the_derived_bound(ops, dev, dt, hd):
    KV = 1 if hd == 128 else 2
    H = 2 * KV
    layouts = ("plain", "padded", "offset")
    worst, n = 0.0, 0
    for T in (1, 2, 5, 16, 17, 33, 100):
        for B in (1, 2, 5):
            layout = layouts[(n + n // 3) % 3]                          # every B meets every layout: the shift moves by one per T
            n += 1
            q = M.generic_rows(B, T, H, hd, 1000 + n, DT[dt])
            k = M.generic_rows(B, T, KV, hd, 2000 + n, DT[dt], mean_sigmas=20.0)
            P, R, A = C.longdouble_causal(q, k, B, T, H, KV, hd)
            lim = C.bound(A, B, T)
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
    print("GENERIC %s hd %d: largest error / bound = %.4f over T 1/2/5/16/17/33/100 x B 1/2/5, three layouts" % (dt, hd, worst))


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
    A = torch.from_numpy(C.longdouble_causal(q, k, B, T, H, KV, hd)[2].astype(np.float64)).to(dev)     # >= sum_s |p_s| entry-wise
    for gt, x in zip(got, one):
        assert not torch.equal(bits(gt), bits(x))
        tol = 2 * (B + 1) * M.U * (3.0 + A)                          # B roundings of a running sum on either side
        assert bool(((gt - (x + 3.0)).abs() <= tol).all())
    # without pair_raw: the same pair
    only, none = run(ops, dev, q, k, B, T, H, KV, hd, layout=layout, raw=False)
    assert none is None and torch.equal(bits(only), bits(one[0]))


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
    need = lib.mdg_qk_causal_ws_bytes(B, H, hd, 1)
    assert need == 2 * 8 * B * H * hd * hd and lib.mdg_qk_causal_ws_bytes(B, H, hd, 0) == need // 2
    assert lib.mdg_qk_causal_ws_bytes(0, H, hd, 1) == 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    ws0, pair0, raw0 = ws.clone(), bits(pair), bits(raw)
    good = dict(q=q.data_ptr(), ld_q=H * hd, k=k.data_ptr(), ld_k=KV * hd, dtype=_lib.MDG_BF16, B=B, T=T, n_heads=H, n_kv=KV, hd=hd,
                pair=pair.data_ptr(), pair_raw=raw.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)

    def call(**over):
        a = {**good, **over}
        return lib.mdg_qk_causal_accum(a["q"], a["ld_q"], a["k"], a["ld_k"], a["dtype"], a["B"], a["T"], a["n_heads"], a["n_kv"], a["hd"],
                                       a["pair"], a["pair_raw"], a["ws"], a["ws_bytes"], torch.cuda.current_stream(dev).cuda_stream)

    refused = [(dict(dtype=_lib.MDG_F64), "dtype"), (dict(dtype=9), "dtype"), (dict(hd=0), "head_dim"), (dict(hd=129), "head_dim"),
               (dict(n_heads=0), "n_heads"), (dict(n_kv=0), "n_kv"), (dict(n_kv=3), "n_kv"), (dict(ld_q=H * hd - 1), "ld_q"),
               (dict(ld_k=KV * hd - 1), "ld_k"), (dict(B=-1), "negative"), (dict(T=-1), "negative"), (dict(q=None), "null"),
               (dict(k=None), "null"), (dict(pair=None), "null"), (dict(ws=None), "null"), (dict(ws_bytes=need - 1), "workspace")]
    for over, word in refused:
        assert call(**over) == _lib.MDG_ERR_BAD_ARG, over
        msg = _lib.last_error()
        assert msg.startswith("mdg_qk_causal_accum:") and word in msg, (over, msg)
    for over in (dict(B=0), dict(T=0), dict(B=0, q=None, k=None, ws=None, ws_bytes=0)):
        assert call(**over) == _lib.MDG_OK, over
    torch.cuda.synchronize()
    assert torch.equal(bits(pair), pair0) and torch.equal(bits(raw), raw0), "a refused or empty call wrote to the outputs"
    assert torch.equal(ws, ws0), "a refused or empty call wrote to the workspace"
    # the Python surface refuses with its own messages, and takes empty calls
    with pytest.raises(ValueError, match="multiple of n_kv"):
        ops.qk_causal_accum(pair, raw, q, k, B, T, H, 3, hd)
    with pytest.raises(ValueError, match="head_dim"):
        ops.qk_causal_accum(pair, raw, q, k, B, T, H, KV, 200)
    with pytest.raises(ValueError, match="q_rows must be"):
        ops.qk_causal_accum(pair, raw, q[:-1], k, B, T, H, KV, hd)
    with pytest.raises(ValueError, match="pair must be"):
        ops.qk_causal_accum(pair.float(), raw, q, k, B, T, H, KV, hd)
    ops.qk_causal_accum(pair, raw, q[:0], k[:0], 0, T, H, KV, hd)
    torch.cuda.synchronize()
    assert torch.equal(bits(pair), pair0) and torch.equal(bits(raw), raw0)
    assert call() == _lib.MDG_OK                                  # and the good call does run
    torch.cuda.synchronize()
    # all-ones rows: K_i = n_i, m_i = n_i, so the centred part is 0 and every query adds K_i / n_i = 1: B T in all, up to the
    # rounding of 1 / n_i (|n_i fl(1 / n_i) - 1| <= 2^-53 per token)
    assert bool(((raw - (6.0 + B * T)).abs() <= 2 * B * T * M.U * (6.0 + B * T)).all()) and bool(((pair - 5.0).abs() <= 2 * B * T * M.U * 5.0).all())
    assert not torch.equal(ws, ws0)


# ---------------------------------------------------------------- the two rules disagree where they should, on the device
@pytest.mark.parametrize("where,amplitude,T", [("late", 24.0, 24), ("first", 60.0, 512)])
def test_the_disagreement_case_on_the_device(ops, dev, where, amplitude, T):
    from modegpt_amd import _lib
    d = C.DIS
    B, H, KV, hd, sp = (d[n] for n in ("B", "H", "KV", "hd", "special"))
    ns, rank = hd // 2, hd // 2
    q, k = C.disagreement_rows(where, amplitude, T=T)
    Pc = run(ops, dev, q, k, B, T, H, KV, hd)[0]
    Pf = torch.zeros(H, hd, hd, dtype=F64, device=dev)
    ops.qk_pair_accum(Pf, None, q.to(dev), k.to(dev), B, T, H, KV, hd)
    ones = torch.ones(KV, hd, hd, dtype=F64, device=dev)
    mode = _lib.MDG_QK_ROPE_GROUPED
    mask_c = ops.qk_select(Pc, ones, rank, mode, 0.0, 0.0)[0].cpu()
    mask_f = ops.qk_select(Pf, ones, rank, mode, 0.0, 0.0)[0].cpu()
    # the model's prediction: the rank/2 best units by the long-double scores, in descending order, then the same + ns
    want = []
    for Pm in (C.longdouble_causal(q, k, B, T, H, KV, hd)[0], M.longdouble_pair(q, k, B, T, H, KV, hd)[0]):
        sc = C.unit_scores(Pm, KV)[0]
        top = sorted(range(ns), key=lambda u: (-float(sc[u]), u))[:rank // 2]
        want.append(top)
    for mask, top in ((mask_c, want[0]), (mask_f, want[1])):
        assert sorted(mask[0].tolist()) == sorted(top + [u + ns for u in top]), (where, mask.tolist(), top)
    in_c, in_f = sp in mask_c[0].tolist(), sp in mask_f[0].tolist()
    assert (in_c, in_f) == ((False, True) if where == "late" else (True, False))

    def objective(P, mask):
        D = sorted(set(range(hd)) - set(mask[0].tolist()))
        Ph = P.cpu().numpy()
        return sum(float(Ph[h][np.ix_(D, D)].sum()) for h in range(H))
    oc, of = objective(Pc, mask_c), objective(Pc, mask_f)
    print("DISAGREE %s: causal objective of the causal mask %.6g, of the full mask %.6g" % (where, oc, of))
    assert oc <= of
