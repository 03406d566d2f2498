"""CPU: mdg_attn_decode checks its arguments without a device, its two pure host functions (workspace size, default split count)
say what the header says, and MODEGPT_FUSED_ATTN_DECODE -- alone, or on CPU tensors -- leaves the compressed forward on HF's
attention interface, bit for bit."""
import itertools

import pytest
import torch

from modegpt_amd import _lib
from tests.test_attn_fwd_host import FAR, K, O, Q, V, _tiny, refused


def _ws_bytes(B, T, n_heads, r_vo, splits):
    """The partials the header documents: per (batch, head, query, split) O_s [r_vo rounded up to 4], m_s, l_s and two pad floats."""
    return B * T * n_heads * splits * ((r_vo + 3) // 4 * 4 + 4) * 4


W = 0x500000                                              # the workspace: like Q, K, V, O never dereferenced
NEED = _ws_bytes(2, 5, 4, 3, 3)                           # 3840 bytes for call_decode's defaults


def call_decode(lib, q=Q, k=K, v=V, dtype=_lib.MDG_BF16, B=2, T=5, S=9, n_heads=4, n_kv=2, r_qk=6, r_vo=3, kbs=2 * 9 * 6, khs=9 * 6,
                kts=6, vbs=2 * 9 * 3, vhs=9 * 3, vts=3, scale=0.5, causal=1, splits=3, ws=W, ws_bytes=NEED, out=O, ld_out=12):
    return lib.mdg_attn_decode(q, k, v, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, kbs, khs, kts, vbs, vhs, vts, scale, causal,
                               splits, ws, ws_bytes, out, ld_out, None)


def test_bad_arguments_return_a_status_and_a_message_without_a_device():
    lib = _lib.load()
    inf, nan = float("inf"), float("nan")
    need = NEED

    def call(**kw):
        return call_decode(lib, **kw)

    assert lib.mdg_attn_decode_ws_bytes(2, 5, 4, 3, 3) == need == 3840
    tile = " exceed the tile of 32 columns (use mdg_attn_fwd)"
    short = " bytes is short of mdg_attn_decode_ws_bytes = "
    bad = [  # dtype
           (dict(dtype=99), "mdg_attn_decode: dtype 99 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(dtype=_lib.MDG_F32), "mdg_attn_decode: dtype 2 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(dtype=_lib.MDG_F64), "mdg_attn_decode: dtype 3 (bf16 or f16; fp32 inputs are out of scope)"),
           # negative
           (dict(B=-1), "mdg_attn_decode: negative extent"), (dict(T=-1), "mdg_attn_decode: negative extent"),
           (dict(S=-1, causal=0), "mdg_attn_decode: negative extent"),
           # n_kv
           (dict(n_heads=5), "mdg_attn_decode: n_heads=5 is not a positive multiple of n_kv=2"),
           (dict(n_kv=0), "mdg_attn_decode: n_heads=4 is not a positive multiple of n_kv=0"),
           (dict(n_kv=3), "mdg_attn_decode: n_heads=4 is not a positive multiple of n_kv=3"),
           # even, 256
           (dict(r_qk=5), "mdg_attn_decode: r_qk=5 must be even, >= 2 and <= 256"),
           (dict(r_qk=0), "mdg_attn_decode: r_qk=0 must be even, >= 2 and <= 256"),
           (dict(r_qk=258, kts=258), "mdg_attn_decode: r_qk=258 must be even, >= 2 and <= 256"),
           # r_vo
           (dict(r_vo=0), "mdg_attn_decode: r_vo=0 must be in 1..256"),
           (dict(r_vo=257, vts=257, ld_out=4 * 257), "mdg_attn_decode: r_vo=257 must be in 1..256"),
           # the tile: T * G = 33 (MHA, 33 queries), 17 * 2 = 34, 1 * 33
           (dict(T=33, S=40, n_heads=2, n_kv=2, ld_out=6), "mdg_attn_decode: T=33 queries x group of 1 heads" + tile),
           (dict(T=17, S=20), "mdg_attn_decode: T=17 queries x group of 2 heads" + tile),
           (dict(T=1, n_heads=33, n_kv=1, ld_out=99), "mdg_attn_decode: T=1 queries x group of 33 heads" + tile),
           # splits
           (dict(splits=0), "mdg_attn_decode: splits=0 must be in 1..256"),
           (dict(splits=257), "mdg_attn_decode: splits=257 must be in 1..256"),
           (dict(splits=-1), "mdg_attn_decode: splits=-1 must be in 1..256"),
           # causal
           (dict(S=4), "mdg_attn_decode: causal with S=4 < T=5 keys"),
           # stride
           (dict(kts=5), "mdg_attn_decode: k token stride 5 < r_qk=6"), (dict(vts=2), "mdg_attn_decode: v token stride 2 < r_vo=3"),
           # ld_out
           (dict(ld_out=11), "mdg_attn_decode: ld_out=11 < n_heads*r_vo=12"),
           # scale
           (dict(scale=0.0), "mdg_attn_decode: scale 0 must be finite and positive"),
           (dict(scale=-1.0), "mdg_attn_decode: scale -1 must be finite and positive"),
           (dict(scale=inf), "mdg_attn_decode: scale inf must be finite and positive"),
           (dict(scale=nan), "mdg_attn_decode: scale nan must be finite and positive"),
           # null
           (dict(q=None), "mdg_attn_decode: null pointer"), (dict(k=None), "mdg_attn_decode: null pointer"),
           (dict(v=None), "mdg_attn_decode: null pointer"), (dict(out=None), "mdg_attn_decode: null pointer"),
           # null workspace, short, aligned
           (dict(ws=None), "mdg_attn_decode: null workspace"),
           (dict(ws_bytes=need - 1), "mdg_attn_decode: workspace of 3839" + short + "3840"),
           (dict(ws_bytes=0), "mdg_attn_decode: workspace of 0" + short + "3840"),
           (dict(splits=4), "mdg_attn_decode: workspace of 3840" + short + "5120"),   # one more split than the workspace was sized for
           (dict(ws=W + 4), "mdg_attn_decode: workspace must be 16-byte aligned"),
           # overlap
           (dict(out=Q), "mdg_attn_decode: out overlaps q"), (dict(out=Q + 2 * (2 * 4 * 5 * 6 - 1)), "mdg_attn_decode: out overlaps q"),
           (dict(q=O + 2), "mdg_attn_decode: out overlaps q"),
           (dict(out=K + 2 * 50), "mdg_attn_decode: out overlaps k"), (dict(out=V + 2 * 100), "mdg_attn_decode: out overlaps v"),
           (dict(k=O + 2 * 119), "mdg_attn_decode: out overlaps k"), (dict(v=O - 2 * 107), "mdg_attn_decode: out overlaps v"),
           # the workspace against each operand: its first and its last byte inside the operand's span, and the operand inside it
           (dict(ws=Q), "mdg_attn_decode: workspace overlaps q"),
           (dict(ws=Q + 2 * 2 * 4 * 5 * 6 - 16), "mdg_attn_decode: workspace overlaps q"),
           (dict(q=W + need - 2), "mdg_attn_decode: workspace overlaps q"),
           (dict(ws=K + 16), "mdg_attn_decode: workspace overlaps k"), (dict(k=W + need - 2), "mdg_attn_decode: workspace overlaps k"),
           (dict(ws=V + 16), "mdg_attn_decode: workspace overlaps v"), (dict(v=W + need - 2), "mdg_attn_decode: workspace overlaps v"),
           (dict(ws=O), "mdg_attn_decode: workspace overlaps out"),
           (dict(ws=O + 2 * 10 * 12 - 16), "mdg_attn_decode: workspace overlaps out"),
           (dict(out=W + need - 2), "mdg_attn_decode: workspace overlaps out"),
           # the entry's own bounds: the index overflow before the empty call and the pointers, the launch bound after the spans
           (dict(B=2 ** 50), "mdg_attn_decode: B*T overflows"),
           (dict(B=2 ** 31, out=FAR, ws=FAR // 2, ws_bytes=2 ** 31 * 1920), "mdg_attn_decode: B=2147483648 exceeds one launch"),
           # two faults at once: the first check in the order above decides
           (dict(dtype=99, B=-1), "mdg_attn_decode: dtype 99 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(r_qk=5, T=17, S=20), "mdg_attn_decode: r_qk=5 must be even, >= 2 and <= 256"),
           (dict(r_vo=0, T=17, S=20), "mdg_attn_decode: r_vo=0 must be in 1..256"),
           (dict(T=17, S=20, splits=0), "mdg_attn_decode: T=17 queries x group of 2 heads" + tile),
           (dict(splits=0, S=4), "mdg_attn_decode: splits=0 must be in 1..256"),
           (dict(S=4, kts=5), "mdg_attn_decode: causal with S=4 < T=5 keys"),
           (dict(scale=0.0, B=2 ** 50), "mdg_attn_decode: scale 0 must be finite and positive"),
           (dict(B=2 ** 50, q=None), "mdg_attn_decode: B*T overflows"),
           (dict(q=None, ws=None), "mdg_attn_decode: null pointer"),
           (dict(ws=None, ws_bytes=0), "mdg_attn_decode: null workspace"),
           (dict(ws=W + 4, ws_bytes=need - 1), "mdg_attn_decode: workspace of 3839" + short + "3840"),
           (dict(ws=W + 4, out=W), "mdg_attn_decode: workspace must be 16-byte aligned"),
           (dict(ws=O, q=O), "mdg_attn_decode: workspace overlaps out"),
           (dict(out=Q, k=Q), "mdg_attn_decode: out overlaps q"), (dict(out=Q, ws=Q + 256), "mdg_attn_decode: out overlaps q"),
           (dict(ws=Q, out=K), "mdg_attn_decode: workspace overlaps q"),
           (dict(ws=K, out=V), "mdg_attn_decode: workspace overlaps k"),
           (dict(out=K, v=K), "mdg_attn_decode: out overlaps k")]
    refused(lib, call, bad, "mdg_attn_decode")
    # the neighbours of the refused extents are not refused for THAT reason: T * G = 32 passes the tile check (and then fails on the
    # workspace this call did not size for it)
    assert call(T=16, S=20, ws_bytes=0) == _lib.MDG_ERR_BAD_ARG
    assert lib.mdg_last_error().decode() == "mdg_attn_decode: workspace of 0" + short + "12288"
    # an empty call is not an error and launches nothing, whatever the pointers
    assert call(B=0, q=None, out=None, ws=None, ws_bytes=0) == _lib.MDG_OK
    assert call(T=0, k=None, v=None, ws=None, ws_bytes=0) == _lib.MDG_OK


def test_workspace_size_is_monotone_and_holds_the_partials():
    lib = _lib.load()

    def f(B, T, n_heads, r_vo, splits):
        return lib.mdg_attn_decode_ws_bytes(B, T, n_heads, r_vo, splits)

    base = dict(B=2, T=3, n_heads=8, r_vo=77, splits=5)
    grid = dict(B=[1, 2, 3, 16], T=[1, 2, 3, 32], n_heads=[1, 8, 9, 32], r_vo=[1, 3, 4, 5, 77, 128, 255, 256],
                splits=[1, 2, 5, 255, 256])
    for name, values in grid.items():
        got = [f(**{**base, name: x}) for x in values]
        assert got == sorted(got), (name, got)
        for x, g in zip(values, got):
            a = {**base, name: x}
            partials = a["B"] * a["T"] * a["n_heads"] * a["splits"] * (a["r_vo"] + 2) * 4          # O_s, m_s, l_s in fp32
            assert g >= partials and g == _ws_bytes(**a), (a, g)
    assert f(1, 1, 32, 256, 256) == 32 * 256 * 260 * 4
    assert f(2 ** 20, 32, 1, 256, 256) == 2 ** 20 * 32 * 256 * 260 * 4                            # 64-bit
    assert f(0, 1, 8, 77, 4) == 0 and f(1, 0, 8, 77, 4) == 0


def _rule(B, n_kv, S, n_cu):
    """The rule of DESIGN.md section 8, restated: one workgroup per CU, no chunk under 4 key tiles of 64 (one for each wave of the
    workgroup: the constant the sweep of scripts/probes/attn_decode_timing.py set), at most 256 splits."""
    tiles = -(-S // 64)
    cap = min(-(-tiles // 4), 256)
    return max(1, min(n_cu // (B * n_kv), cap))


def test_default_split_count_follows_the_rule():
    f = _lib.load().mdg_attn_decode_splits
    for B, n_kv, S, n_cu in itertools.product([1, 2, 3, 16, 64, 300], [1, 2, 8, 32], [1, 63, 64, 65, 2048, 8191, 8192, 32768, 10 ** 6],
                                              [1, 64, 104, 256, 304, 100000]):
        got = f(B, n_kv, S, n_cu)
        assert 1 <= got <= min(-(-S // 64), 256), (B, n_kv, S, n_cu, got)
        assert got == _rule(B, n_kv, S, n_cu), (B, n_kv, S, n_cu, got)
        if B * n_kv >= n_cu:
            assert got == 1
        assert got == f(B, n_kv, S, n_cu)                                  # a pure function: the same answer again
    assert f(1, 8, 8192, 256) == 32 and f(1, 8, 2048, 256) == 8 and f(1, 8, 1024, 256) == 4 and f(16, 8, 8192, 256) == 2
    assert f(1, 8, 32768, 256) == 32 and f(1, 1, 10 ** 6, 100000) == 256 and f(1, 8, 65, 256) == 1 and f(1, 8, 257, 256) == 2
    assert f(1, 8, 0, 256) == 1 and f(0, 8, 64, 256) == 1 and f(1, 8, 64, 0) == 1


def test_ops_attn_decode_refuses_cpu_tensors():
    from modegpt_amd import ops
    q = torch.zeros(1, 2, 1, 4, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attn_decode(q, q, q, 1.0)


@pytest.mark.parametrize("kind", ["llama", "opt"])
def test_decode_switch_alone_or_on_cpu_takes_the_interface_bit_for_bit(kind, monkeypatch):
    model, ca = _tiny(kind)
    assert set(ca.ATTN_KERNELS) == {"fwd", "decode"} and set(ca.ATTN_CALLS) == {"hip", "interface"}
    assert ca._DECODE_SPLITS is None
    ids = torch.arange(12).reshape(2, 6) % 64                       # T * G = 12 (llama), 6 (opt): inside the decode kernel's domain
    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE", "MODEGPT_REQUIRE_HIP"):
        monkeypatch.delenv(name, raising=False)
    calls, kernels = dict(ca.ATTN_CALLS), dict(ca.ATTN_KERNELS)
    with torch.no_grad():
        off = model(ids).logits
    assert ca.ATTN_CALLS == {"hip": calls["hip"], "interface": calls["interface"] + 2}
    monkeypatch.setenv("MODEGPT_FUSED_ATTN_DECODE", "1")            # alone: no effect
    with torch.no_grad():
        alone = model(ids).logits
    assert ca.ATTN_CALLS == {"hip": calls["hip"], "interface": calls["interface"] + 4}
    monkeypatch.setenv("MODEGPT_FUSED_ATTN", "1")                   # both, on CPU tensors: still the interface
    with torch.no_grad():
        both = model(ids).logits
    assert ca.ATTN_CALLS == {"hip": calls["hip"], "interface": calls["interface"] + 6}
    assert ca.ATTN_KERNELS == kernels and not any(kernels.values())  # nothing in a process without a device ever counts a kernel
    assert torch.equal(alone.view(torch.int16), off.view(torch.int16)) and torch.equal(both.view(torch.int16), off.view(torch.int16))
