"""CPU: mdg_attn_decode checks its arguments without a device, its two pure host functions (workspace size, default split count)
say what the header says, and MODEGPT_FUSED_ATTN_DECODE -- alone, or on CPU tensors -- leaves the compressed forward on HF's
attention interface, bit for bit."""
import itertools

import pytest
import torch

from modegpt_amd import _lib
from tests.test_attn_fwd_host import _tiny


def _ws_bytes(B, T, n_heads, r_vo, splits):
    """The partials the header documents: per (batch, head, query, split) O_s [r_vo rounded up to 4], m_s, l_s and two pad floats."""
    return B * T * n_heads * splits * ((r_vo + 3) // 4 * 4 + 4) * 4


def test_bad_arguments_return_a_status_and_a_message_without_a_device():
    lib = _lib.load()
    Q, K, V, O, W = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000  # never dereferenced: every call below is refused before any device work
    inf, nan = float("inf"), float("nan")
    need = _ws_bytes(2, 5, 4, 3, 3)

    def call(q=Q, k=K, v=V, dtype=_lib.MDG_BF16, B=2, T=5, S=9, n_heads=4, n_kv=2, r_qk=6, r_vo=3, kbs=2 * 9 * 6, khs=9 * 6, kts=6,
             vbs=2 * 9 * 3, vhs=9 * 3, vts=3, scale=0.5, causal=1, splits=3, ws=W, ws_bytes=need, out=O, ld_out=12):
        return lib.mdg_attn_decode(q, k, v, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, kbs, khs, kts, vbs, vhs, vts, scale, causal,
                                   splits, ws, ws_bytes, out, ld_out, None)

    assert lib.mdg_attn_decode_ws_bytes(2, 5, 4, 3, 3) == need
    bad = [(dict(dtype=99), "dtype"), (dict(dtype=_lib.MDG_F32), "dtype"), (dict(dtype=_lib.MDG_F64), "dtype"),
           (dict(B=-1), "negative"), (dict(T=-1), "negative"), (dict(S=-1, causal=0), "negative"),
           (dict(n_heads=5), "n_kv"), (dict(n_kv=0), "n_kv"), (dict(n_kv=3), "n_kv"),
           (dict(r_qk=5), "even"), (dict(r_qk=0), "even"), (dict(r_qk=258, kts=258), "256"),
           (dict(r_vo=0), "r_vo"), (dict(r_vo=257, vts=257, ld_out=4 * 257), "r_vo"),
           # the tile: T * G = 33 (MHA, 33 queries), 17 * 2 = 34, 1 * 33
           (dict(T=33, S=40, n_heads=2, n_kv=2, ld_out=6), "tile"), (dict(T=17, S=20), "tile"),
           (dict(T=1, n_heads=33, n_kv=1, ld_out=99), "tile"),
           (dict(splits=0), "splits"), (dict(splits=257), "splits"), (dict(splits=-1), "splits"),
           (dict(S=4), "causal"),
           (dict(kts=5), "stride"), (dict(vts=2), "stride"),
           (dict(ld_out=11), "ld_out"),
           (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=inf), "scale"), (dict(scale=nan), "scale"),
           (dict(q=None), "null"), (dict(k=None), "null"), (dict(v=None), "null"), (dict(out=None), "null"),
           (dict(ws=None), "null workspace"), (dict(ws_bytes=need - 1), "short"), (dict(ws_bytes=0), "short"),
           (dict(splits=4), "short"),                                    # one more split than the workspace was sized for
           (dict(ws=W + 4), "aligned"),
           (dict(out=Q), "overlap"), (dict(out=Q + 2 * (2 * 4 * 5 * 6 - 1)), "overlap"), (dict(q=O + 2), "overlap"),
           (dict(out=K + 2 * 50), "overlap"), (dict(out=V + 2 * 100), "overlap"),
           (dict(k=O + 2 * 119), "overlap"), (dict(v=O - 2 * 107), "overlap"),
           # the workspace against each operand: its first and its last byte inside the operand's span, and the operand inside it
           (dict(ws=Q), "workspace overlaps q"), (dict(ws=Q + 2 * 2 * 4 * 5 * 6 - 16), "workspace overlaps q"),
           (dict(q=W + need - 2), "workspace overlaps q"),
           (dict(ws=K + 16), "workspace overlaps k"), (dict(k=W + need - 2), "workspace overlaps k"),
           (dict(ws=V + 16), "workspace overlaps v"), (dict(v=W + need - 2), "workspace overlaps v"),
           (dict(ws=O), "workspace overlaps out"), (dict(ws=O + 2 * 10 * 12 - 16), "workspace overlaps out"),
           (dict(out=W + need - 2), "workspace overlaps out")]
    for kw, word in bad:
        assert call(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        assert word in lib.mdg_last_error().decode(), (kw, lib.mdg_last_error())
        with pytest.raises(RuntimeError):
            _lib.check(call(**kw), "mdg_attn_decode")
    # the neighbours of the refused extents are not refused for THAT reason: T * G = 32 passes the tile check (and then fails on the
    # workspace this call did not size for it)
    assert call(T=16, S=20, ws_bytes=0) == _lib.MDG_ERR_BAD_ARG and "short" in lib.mdg_last_error().decode()
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
