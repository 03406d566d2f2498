"""GPU: the three entry points built on csrc/row_dots.hpp (mdg_nystrom_intercept, mdg_vo_intercept, mdg_vo_bias) give, bit for bit,
what the library gave before they shared one row routine.

tests/golden/row_dots_bits.json holds every output of every case below as recorded from the build of the commit BEFORE the routine
was shared (`python -m tests.test_gpu_row_dots_bits record` on the GPU at that commit).  It is what a later change of the routine is
measured against: a change that moves a bit changes the summation order (or a rounding) of three features at once.  Never regenerate
it to make a failing build pass.

Inputs come from a closed-form integer formula, ((a i + b j + c i j) mod p - p / 2) / q with one correctly rounded fp64 division (then
one round-to-nearest to bf16 / fp16 where the operand is 16-bit), so they are the same on every machine and library version.  The
vectors are full fp64 values, so no product is exact and the sums depend on their order: test_the_inputs_see_the_order checks that on
the host.  Every case crosses an LDS chunk (2048 columns) with a ragged tail at every call site of the routine, has a row count that
is no multiple of 16, and comes with the rows aligned for the 16-byte loads (ld a multiple of 8) and not (ld odd), for every element
type the entry point dispatches to.

An output of up to 64 entries is stored whole, as float.hex() strings (a NaN as "nan:" and its 16 hex digits); a longer one as its
first 37 entries and the SHA-256 of all its fp64 bytes (mdg_vo_intercept's head stage needs d > 2048 columns, and d is also the length
of its outputs).  The 16-bit `bias` outputs are widened exactly to fp64 first."""
import hashlib
import json
import os
import struct
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_dots_bits.json")
WHOLE, HEAD = 64, 37
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}


# ------------------------------------------------------------------ inputs
def grid(rows, cols, a, b, c, p, q):
    """[rows, cols] fp64, entry (i, j) = ((a i + b j + c i j) mod p - p // 2) / q: one correctly rounded division of two integers."""
    i = torch.arange(rows, dtype=torch.int64)[:, None]
    j = torch.arange(cols, dtype=torch.int64)[None, :]
    return (((a * i + b * j + c * i * j) % p) - p // 2).to(torch.float64) / q


def placed(values, dtype, ld, dev):
    """`values` [rows, cols] rounded to dtype, as a view of a [rows, ld] device buffer whose pad columns hold NaN (never read: a NaN
    would reach a sum).  The base is the allocator's (16-byte aligned), so ld alone decides between the 16-byte and the scalar loads."""
    rows, cols = values.shape
    buf = torch.full((rows, ld), float("nan"), dtype=dtype)
    buf[:, :cols] = values.to(dtype)
    return buf.to(dev)[:, :cols]


def up8(n):
    return (n + 7) // 8 * 8


def odd(n):
    return n | 1


# (name, dtype of W_d, aligned rows, dtype of b_d or None, an index out of range)
MLP_D, MLP_N = 37, 2048 + 29
MLP_CASES = [("bf16-vec", "bf16", True, "bf16", False), ("bf16-scalar", "bf16", False, "f16", False), ("f64-vec", "f64", True, None, False),
             ("f64-scalar", "f64", False, None, False), ("bf16-vec-badidx", "bf16", True, "bf16", True)]
# (name, dtype of W_v / W_o, dtype of v^ / o^, aligned rows, rank): 18 query / 6 kv heads of 118 -> 2124 columns of W_o, 2070 of o^
VI_D, VI_HEADS, VI_KV, VI_HD, VI_RANK = 2048 + 13, 18, 6, 118, 115
VI_CASES = [("bf16-bf16-vec", "bf16", "bf16", True, VI_RANK), ("bf16-bf16-scalar", "bf16", "bf16", False, VI_RANK),
            ("bf16-f64-vec", "bf16", "f64", True, VI_RANK), ("f64-bf16-vec", "f64", "bf16", True, VI_RANK),
            ("f64-f64", "f64", "f64", False, VI_RANK), ("bf16-rank0-vec", "bf16", "bf16", True, 0)]
# (name, dtype of W_o, aligned rows): 62 query / 2 kv heads of 34 -> 2108 columns; d = 37 >= hd keeps every Gram matrix regular
VB_D, VB_HEADS, VB_KV, VB_HD, VB_RANK = 37, 62, 2, 34, 20
VB_CASES = [("bf16-vec", "bf16", True), ("bf16-scalar", "bf16", False), ("f16-vec", "f16", True), ("f16-scalar", "f16", False),
            ("f64", "f64", False)]


def mlp_inputs():
    W = grid(MLP_D, MLP_N, 7, 13, 3, 1009, 1013)
    idx = torch.tensor([j for j in range(MLP_N) if j % 257 != 3], dtype=torch.int64)           # r = 2068: 2048 + 20
    D = grid(MLP_D, idx.numel(), 11, 5, 1, 997, 1019)
    mu = grid(1, MLP_N, 0, 17, 0, 991, 3001)[0] + 0.125
    b = grid(1, MLP_D, 0, 29, 0, 61, 67)[0]
    return W, D, idx, mu, b


def vi_inputs():
    Wv = grid(VI_KV * VI_HD, VI_D, 7, 13, 3, 1009, 1013 * 16)
    Wo = grid(VI_D, VI_HEADS * VI_HD, 5, 19, 1, 1013, 1019 * 16)
    Vn = grid(VI_KV * VI_RANK, VI_D, 3, 11, 7, 997, 1009 * 16)
    On = grid(VI_D, VI_HEADS * VI_RANK, 13, 7, 5, 1019, 1021 * 16)
    mu = grid(1, VI_D, 0, 17, 0, 991, 3001)[0] + 0.125
    b_v = grid(1, VI_KV * VI_HD, 0, 29, 0, 61, 67)[0]
    b_o = grid(1, VI_D, 0, 31, 0, 73, 79)[0]
    return Wv, Wo, Vn, On, mu, b_v, b_o


def vb_inputs():
    Wv = grid(VB_KV * VB_HD, VB_D, 7, 13, 3, 1009, 1013)
    Wo = grid(VB_D, VB_HEADS * VB_HD, 5, 19, 1, 1013, 1019)
    i = torch.arange(VB_D, dtype=torch.int64)
    C = (((3 * (i[:, None] + i[None, :]) + 5 * i[:, None] * i[None, :]) % 97) - 48).to(torch.float64) / (97 * 40)   # symmetric, |.| < 1/80
    C[i, i] = 2.0 + i.to(torch.float64) / 37                                                                       # diagonally dominant
    b_v = grid(1, VB_KV * VB_HD, 0, 29, 0, 61, 67)[0]
    b_o = grid(1, VB_D, 0, 31, 0, 73, 79)[0]
    return Wv, Wo, C, b_v, b_o


# ------------------------------------------------------------------ the calls
def run_mlp(dev):
    from modegpt_amd import ops
    W, D, idx, mu, b = mlp_inputs()
    r = idx.numel()
    out = {}
    for name, wdt, aligned, bdt, bad in MLP_CASES:
        Wd = placed(W, DT[wdt], up8(MLP_N) if aligned else odd(MLP_N), dev)
        Dh = placed(D, torch.bfloat16, up8(r) if aligned else odd(r), dev)
        ix = idx.clone()
        if bad:
            ix[2055] = MLP_N                                   # (behind the first chunk; the staged NaN reaches every row of D^ mu[idx])
        bd = None if bdt is None else b.to(DT[bdt]).to(dev)
        bias, b64, norms = ops.nystrom_intercept(Wd, Dh, ix.to(dev), mu.to(dev), bd)
        out["mlp/" + name] = {"bias": bias, "bias_f64": b64, "norms": norms}
    return out


def run_vi(dev):
    from modegpt_amd import ops
    Wv, Wo, Vn, On, mu, b_v, b_o = vi_inputs()
    out = {}
    for name, wdt, ndt, aligned, rank in VI_CASES:
        ld = up8 if aligned else odd
        wv, wo = placed(Wv, DT[wdt], ld(VI_D), dev), placed(Wo, DT[wdt], ld(VI_HEADS * VI_HD), dev)
        vn = on = None
        if rank:
            vn, on = placed(Vn, DT[ndt], ld(VI_D), dev), placed(On, DT[ndt], ld(VI_HEADS * VI_RANK), dev)
        bias, b64, norms = ops.vo_intercept(wv, wo, vn, on, mu.to(dev), VI_HEADS, VI_KV, VI_HD, rank, b_v=b_v.to(dev), b_o=b_o.to(dev),
                                            out_dtype=torch.bfloat16 if wdt == "bf16" else torch.float64)
        out["vo_intercept/" + name] = {"bias": bias, "bias_f64": b64, "norms": norms}
    return out


def run_vb(dev):
    from modegpt_amd import ops
    Wv, Wo, C, b_v, b_o = vb_inputs()
    out = {}
    for name, wdt, aligned in VB_CASES:
        wv = Wv.to(DT[wdt]).to(dev)
        wo = placed(Wo, DT[wdt], up8(VB_HEADS * VB_HD) if aligned else odd(VB_HEADS * VB_HD), dev)
        for form, bo in (("fold", b_o.to(dev)), ("project", None)):
            o_bias, v_bias, resid = ops.vo_compress(C.to(dev), wv, wo, VB_HEADS, VB_KV, VB_HD, VB_RANK, 0.0, bias=(b_v.to(dev), bo))[-1]
            got = {"resid": resid}
            got.update({"o_bias": o_bias} if bo is not None else {"v_bias": v_bias})
            out[f"vo_bias/{name}/{form}"] = got
    return out


FAMILIES = {"mlp": run_mlp, "vo_intercept": run_vi, "vo_bias": run_vb}


# ------------------------------------------------------------------ the fixture
def bits_of(t):
    """The fp64 bit patterns of a device tensor (16-bit and fp32 outputs widened exactly), as a CPU int64 vector."""
    return t.detach().cpu().to(torch.float64).reshape(-1).contiguous().view(torch.int64)


def to_text(bit):
    v = struct.unpack("<d", struct.pack("<q", bit))[0]
    return "nan:%016x" % (bit & 0xFFFFFFFFFFFFFFFF) if v != v else v.hex()


def to_bits(text):
    if text.startswith("nan:"):
        return struct.unpack("<q", struct.pack("<Q", int(text[4:], 16)))[0]
    return struct.unpack("<q", struct.pack("<d", float.fromhex(text)))[0]


def encode(t):
    b = bits_of(t)
    keep = b.numel() if b.numel() <= WHOLE else HEAD
    return {"n": b.numel(), "head": [to_text(v) for v in b[:keep].tolist()],
            "sha256": hashlib.sha256(struct.pack("<%dq" % b.numel(), *b.tolist())).hexdigest()}


def record(path):
    dev = torch.device("cuda:0")
    doc = {}
    for family, run in FAMILIES.items():
        for case, outs in run(dev).items():
            torch.cuda.synchronize(dev)
            doc[case] = {k: encode(v) for k, v in outs.items()}
            finite = all(bool(torch.isfinite(v).all()) for v in outs.values())
            assert finite or "badidx" in case, f"{case}: a non-finite output in a case that should have none"
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(doc)} cases -> {path}")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_outputs_are_the_recorded_bits(dev, golden, family):
    got = FAMILIES[family](dev)
    torch.cuda.synchronize(dev)
    assert sorted(got) == sorted(k for k in golden if k.startswith(family + "/"))
    wrong = []
    for case, outs in got.items():
        assert sorted(outs) == sorted(golden[case]), case
        for name, t in outs.items():
            want, have = golden[case][name], bits_of(t)
            head = torch.tensor([to_bits(s) for s in want["head"]], dtype=torch.int64)
            same = have.numel() == want["n"] and torch.equal(have[:head.numel()], head) and encode(t)["sha256"] == want["sha256"]
            print(f"{case} {name}: {'same bits' if same else 'DIFFERS'}")
            if not same:
                first = next((i for i, (a, b) in enumerate(zip(have.tolist(), head.tolist())) if a != b), None)
                wrong.append((case, name, first, None if first is None else (to_text(have[first].item()), want["head"][first])))
    assert not wrong, wrong


def test_a_bad_index_is_nan_everywhere_and_nowhere_else(golden):
    """(what the recorded bits say, spelled out: the case with an index out of range is NaN in every row, the others in none)"""
    for case, outs in golden.items():
        for name, rec in outs.items():
            nans = sum(s.startswith("nan:") for s in rec["head"])
            if "badidx" in case:
                assert nans == (1 if name == "norms" else len(rec["head"])), (case, name)       # ||W_d mu||^2 never sees idx
            else:
                assert nans == 0, (case, name)


# ------------------------------------------------------------------ host: the inputs can see a change of order
def test_the_inputs_see_the_order():
    """A row's products summed in fp64 in ascending and in descending column order differ, at every call site's operands: were the
    sums exact (as sums of products of two bf16 values are), no change of the routine's order could show in the bits."""
    W, D, idx, mu, _ = mlp_inputs()
    Wv, Wo, Vn, On, vmu, _, _ = vi_inputs()
    a = (Wv.to(torch.bfloat16).to(torch.float64) @ vmu)
    a_cols = a.reshape(VI_KV, VI_HD).repeat_interleave(VI_HEADS // VI_KV, 0).reshape(-1)
    _, bWo, _, b_v, _ = vb_inputs()
    b_cols = b_v.reshape(VB_KV, VB_HD).repeat_interleave(VB_HEADS // VB_KV, 0).reshape(-1)
    sites = {"W_d mu": (W[0].to(torch.bfloat16), mu), "D^ mu[idx]": (D[0].to(torch.bfloat16), mu[idx]),
             "W_v mu": (Wv[0].to(torch.bfloat16), vmu), "v^ mu": (Vn[0].to(torch.bfloat16), vmu),
             "W_o a": (Wo[0].to(torch.bfloat16), a_cols), "W_o b_v (bf16)": (bWo[0].to(torch.bfloat16), b_cols),
             "W_o b_v (f16)": (bWo[0].to(torch.float16), b_cols), "W_o b_v (f64)": (bWo[0], b_cols)}
    for site, (row, vec) in sites.items():
        prods = (row.to(torch.float64) * vec).tolist()
        up = down = 0.0
        for p in prods:
            up += p
        for p in reversed(prods):
            down += p
        assert up != down, site


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "record":
        sys.exit("usage: python -m tests.test_gpu_row_dots_bits record [path]   (at the commit the fixture is taken from, on the GPU)")
    record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
