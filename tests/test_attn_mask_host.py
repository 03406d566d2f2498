"""CPU: the masked attention entries (mdg_attn_mask_summary, mdg_attn_fwd_masked, mdg_attn_decode_masked) check their arguments
without a device, mdg_attn_mask_summary_bytes says what the header says, and MODEGPT_FUSED_ATTN_MASK -- alone, or on CPU tensors --
leaves the compressed forward of a padded batch on HF's attention interface, bit for bit."""
import pytest
import torch

from modegpt_amd import _lib
from tests.test_attn_fwd_host import _tiny

# never dereferenced: every call below is refused before any device work
Q, K, V, O, W, M, SM = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000


def test_summary_size_is_one_byte_per_tile():
    f = _lib.load().mdg_attn_mask_summary_bytes
    for B, Hm, T, S in [(1, 1, 1, 1), (2, 1, 5, 9), (2, 4, 32, 64), (2, 4, 33, 65), (3, 8, 70, 200), (16, 1, 8192, 8192), (1, 32, 1, 10 ** 6)]:
        assert f(B, Hm, T, S) == B * Hm * -(-T // 32) * -(-S // 64), (B, Hm, T, S)
    assert f(2 ** 20, 32, 2 ** 20, 2 ** 20) == 2 ** 20 * 32 * 2 ** 15 * 2 ** 14                        # 64-bit
    assert f(0, 1, 5, 9) == 0 and f(2, 0, 5, 9) == 0 and f(2, 1, 0, 9) == 0 and f(2, 1, 5, 0) == 0 and f(-1, 1, 5, 9) == 0


def _refused(lib, call, bad, name):
    for kw, word in bad:
        assert call(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        msg = lib.mdg_last_error().decode()
        assert word in msg and msg.startswith(name + ":"), (kw, msg)
        with pytest.raises(RuntimeError):
            _lib.check(call(**kw), name)


def test_summary_bad_arguments_return_a_status_and_a_message_without_a_device():
    lib = _lib.load()
    need = 2 * 1 * 1 * 1

    def call(mask=M, B=2, Hm=1, T=5, S=9, mbs=45, mhs=0, mqs=9, summary=SM, summary_bytes=need):
        return lib.mdg_attn_mask_summary(mask, B, Hm, T, S, mbs, mhs, mqs, summary, summary_bytes, None)

    bad = [(dict(B=-1), "negative"), (dict(T=-1), "negative"), (dict(S=-1), "negative"), (dict(Hm=0), "Hm"), (dict(Hm=-2), "Hm"),
           (dict(mbs=-45), "stride"), (dict(mhs=-1), "stride"), (dict(mqs=-9), "stride"),
           (dict(mask=None), "null mask"), (dict(summary=None), "null summary"),
           (dict(summary_bytes=need - 1), "short"), (dict(summary_bytes=0), "short"), (dict(Hm=4), "short"),
           (dict(summary=M), "overlaps"), (dict(summary=M + 45 + 4 * 9 + 8), "overlaps"), (dict(mask=SM + 1), "overlaps")]
    _refused(lib, call, bad, "mdg_attn_mask_summary")
    # an empty call is not an error and launches nothing, whatever the pointers
    for kw in (dict(B=0), dict(T=0), dict(S=0)):
        assert call(mask=None, summary=None, summary_bytes=0, **kw) == _lib.MDG_OK, kw


def test_fwd_masked_bad_arguments_return_a_status_and_a_message_without_a_device():
    lib = _lib.load()
    inf, nan = float("inf"), float("nan")
    need = 2                                                          # B * Hm * ceil(5 / 32) * ceil(9 / 64)

    def call(q=Q, k=K, v=V, dtype=_lib.MDG_BF16, B=2, T=5, S=9, n_heads=4, n_kv=2, r_qk=6, r_vo=3, kbs=2 * 9 * 6, khs=9 * 6, kts=6,
             vbs=2 * 9 * 3, vhs=9 * 3, vts=3, scale=0.5, causal=1, out=O, ld_out=12, mask=M, Hm=1, mbs=45, mhs=0, mqs=9,
             summary=SM, summary_bytes=need):
        return lib.mdg_attn_fwd_masked(q, k, v, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, kbs, khs, kts, vbs, vhs, vts, scale, causal,
                                       out, ld_out, None, mask, Hm, mbs, mhs, mqs, summary, summary_bytes)

    out_bytes = 2 * (9 * 12 + 12)                                     # B * T rows of pitch 12, the last one 12 wide
    bad = [  # everything mdg_attn_fwd refuses
           (dict(dtype=99), "dtype"), (dict(dtype=_lib.MDG_F32), "dtype"), (dict(B=-1), "negative"), (dict(T=-1), "negative"),
           (dict(S=-1, causal=0), "negative"), (dict(n_heads=5), "n_kv"), (dict(n_kv=0), "n_kv"), (dict(n_kv=3), "n_kv"),
           (dict(r_qk=5), "even"), (dict(r_qk=0), "even"), (dict(r_qk=258, kts=258), "256"), (dict(r_vo=0), "r_vo"),
           (dict(r_vo=257, vts=257, ld_out=4 * 257), "r_vo"), (dict(S=4), "causal"), (dict(kts=5), "stride"), (dict(vts=2), "stride"),
           (dict(ld_out=11), "ld_out"), (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=inf), "scale"),
           (dict(scale=nan), "scale"), (dict(q=None), "null"), (dict(k=None), "null"), (dict(v=None), "null"), (dict(out=None), "null"),
           (dict(out=Q), "overlaps q"), (dict(out=K + 2 * 50), "overlaps k"), (dict(out=V + 2 * 100), "overlaps v"),
           # and the mask's own
           (dict(Hm=2), "Hm"), (dict(Hm=0), "Hm"), (dict(Hm=3), "Hm"), (dict(Hm=-1), "Hm"),
           (dict(mbs=-45), "negative mask stride"), (dict(mhs=-1), "negative mask stride"), (dict(mqs=-9), "negative mask stride"),
           (dict(mask=None), "null mask"), (dict(summary=None), "null summary"),
           (dict(summary_bytes=need - 1), "short"), (dict(summary_bytes=0), "short"),
           (dict(Hm=4, mhs=90, mbs=360), "short"),                    # a per-head mask needs four times the summary
           # spans against out, computed with the strides: first byte, last byte, out inside the mask; a 0 stride counts extent 1
           (dict(mask=O), "out overlaps mask"), (dict(mask=O - (45 + 4 * 9 + 9) + 1), "out overlaps mask"),
           (dict(mask=O + out_bytes - 1), "out overlaps mask"), (dict(out=M + 2), "out overlaps mask"),
           (dict(mask=O - 8, mbs=0, mqs=0), "out overlaps mask"),      # one row of 9 bytes for every query: its last byte is out's first
           (dict(summary=O), "out overlaps summary"), (dict(summary=O - 1), "out overlaps summary"),
           (dict(summary=O + out_bytes - 1), "out overlaps summary")]
    _refused(lib, call, bad, "mdg_attn_fwd_masked")
    # the neighbours of the refused spans pass the mask checks: the call is then refused for its summary, which is checked next
    for kw in (dict(mask=O - (45 + 4 * 9 + 9)), dict(mask=O + out_bytes), dict(mask=O - 9, mbs=0, mqs=0),
               dict(Hm=4, mhs=90, mbs=360)):
        assert call(summary_bytes=0, **kw) == _lib.MDG_ERR_BAD_ARG and "short" in lib.mdg_last_error().decode(), kw
    # an empty call is not an error and launches nothing, whatever the pointers
    assert call(B=0, q=None, out=None, mask=None, summary=None, summary_bytes=0) == _lib.MDG_OK
    assert call(T=0, k=None, v=None, mask=None, summary=None, summary_bytes=0) == _lib.MDG_OK


def test_decode_masked_bad_arguments_return_a_status_and_a_message_without_a_device():
    lib = _lib.load()
    need = lib.mdg_attn_decode_ws_bytes(2, 5, 4, 3, 3)

    def call(q=Q, k=K, v=V, dtype=_lib.MDG_BF16, B=2, T=5, S=9, n_heads=4, n_kv=2, r_qk=6, r_vo=3, kbs=2 * 9 * 6, khs=9 * 6, kts=6,
             vbs=2 * 9 * 3, vhs=9 * 3, vts=3, scale=0.5, causal=1, splits=3, ws=W, ws_bytes=need, out=O, ld_out=12, mask=M, Hm=1,
             mbs=45, mhs=0, mqs=9):
        return lib.mdg_attn_decode_masked(q, k, v, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, kbs, khs, kts, vbs, vhs, vts, scale,
                                          causal, splits, ws, ws_bytes, out, ld_out, None, mask, Hm, mbs, mhs, mqs)

    out_bytes = 2 * (9 * 12 + 12)
    bad = [  # everything mdg_attn_decode refuses
           (dict(dtype=99), "dtype"), (dict(B=-1), "negative"), (dict(n_heads=5), "n_kv"), (dict(r_qk=5), "even"), (dict(r_vo=0), "r_vo"),
           (dict(T=17, S=20), "tile"), (dict(splits=0), "splits"), (dict(splits=257), "splits"), (dict(S=4), "causal"),
           (dict(kts=5), "stride"), (dict(vts=2), "stride"), (dict(ld_out=11), "ld_out"), (dict(scale=0.0), "scale"),
           (dict(q=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null workspace"), (dict(ws_bytes=need - 1), "short"),
           (dict(ws=W + 4), "aligned"), (dict(out=Q), "overlap"), (dict(ws=Q), "workspace overlaps q"),
           (dict(ws=O), "workspace overlaps out"), (dict(out=W + need - 2), "workspace overlaps out"),
           # and the mask's own
           (dict(Hm=2), "Hm"), (dict(Hm=0), "Hm"), (dict(mbs=-45), "negative mask stride"), (dict(mhs=-1), "negative mask stride"),
           (dict(mqs=-9), "negative mask stride"), (dict(mask=None), "null mask"),
           (dict(mask=O), "out overlaps mask"), (dict(mask=O - (45 + 4 * 9 + 9) + 1), "out overlaps mask"),
           (dict(mask=O + out_bytes - 1), "out overlaps mask"), (dict(mask=O - 8, mbs=0, mqs=0), "out overlaps mask"),
           (dict(mask=W + need - 1), "workspace overlaps mask"), (dict(mask=W - (45 + 4 * 9 + 9) + 1), "workspace overlaps mask")]
    _refused(lib, call, bad, "mdg_attn_decode_masked")
    # the neighbours of the refused spans pass the mask checks: the call is then refused for its q, which is checked next
    for kw in (dict(mask=O - (45 + 4 * 9 + 9)), dict(mask=O + out_bytes), dict(mask=O - 9, mbs=0, mqs=0), dict(mask=W + need)):
        assert call(q=O + 2, **kw) == _lib.MDG_ERR_BAD_ARG and "out overlaps q" in lib.mdg_last_error().decode(), kw
    assert call(B=0, q=None, out=None, ws=None, ws_bytes=0, mask=None) == _lib.MDG_OK
    assert call(T=0, k=None, v=None, ws=None, ws_bytes=0, mask=None) == _lib.MDG_OK


def test_the_unmasked_entries_keep_their_names_in_their_messages():
    lib = _lib.load()
    assert lib.mdg_attn_fwd(Q, K, V, 99, 2, 5, 9, 4, 2, 6, 3, 108, 54, 6, 54, 27, 3, 0.5, 1, O, 12, None) == _lib.MDG_ERR_BAD_ARG
    assert lib.mdg_last_error().decode().startswith("mdg_attn_fwd: dtype")
    assert lib.mdg_attn_decode(Q, K, V, 99, 2, 5, 9, 4, 2, 6, 3, 108, 54, 6, 54, 27, 3, 0.5, 1, 3, W, 1 << 20, O, 12,
                               None) == _lib.MDG_ERR_BAD_ARG
    assert lib.mdg_last_error().decode().startswith("mdg_attn_decode: dtype")


def test_ops_refuse_cpu_tensors_with_a_mask():
    from modegpt_amd import ops
    q = torch.zeros(1, 2, 1, 4, dtype=torch.bfloat16)
    mask = torch.ones(1, 1, 1, 1, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attn_fwd(q, q, q, 1.0, mask=mask)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attn_decode(q, q, q, 1.0, mask=mask)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attn_mask_summary(mask)


@pytest.mark.parametrize("kind", ["llama", "opt"])
def test_mask_switch_alone_or_on_cpu_takes_the_interface_bit_for_bit(kind, monkeypatch):
    model, ca = _tiny(kind)
    assert set(ca.ATTN_MASKED) == {"fwd", "decode"} and set(ca.ATTN_KERNELS) == {"fwd", "decode"}
    assert set(ca.ATTN_CALLS) == {"hip", "interface"}                # the existing tables keep their keys
    ids = torch.arange(12).reshape(2, 6) % 64
    pad = torch.tensor([[1, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1]])     # row 1 left-padded by two: HF hands every layer a bool 4-D mask
    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE", "MODEGPT_FUSED_ATTN_MASK", "MODEGPT_REQUIRE_HIP"):
        monkeypatch.delenv(name, raising=False)
    calls, kernels, masked = dict(ca.ATTN_CALLS), dict(ca.ATTN_KERNELS), dict(ca.ATTN_MASKED)
    with torch.no_grad():
        off = model(ids, attention_mask=pad).logits
    assert ca.ATTN_CALLS == {"hip": calls["hip"], "interface": calls["interface"] + 2}
    monkeypatch.setenv("MODEGPT_FUSED_ATTN_MASK", "1")               # alone: no effect
    with torch.no_grad():
        alone = model(ids, attention_mask=pad).logits
    assert ca.ATTN_CALLS == {"hip": calls["hip"], "interface": calls["interface"] + 4}
    monkeypatch.setenv("MODEGPT_FUSED_ATTN", "1")                    # both (and the decode switch), on CPU tensors: still the interface
    monkeypatch.setenv("MODEGPT_FUSED_ATTN_DECODE", "1")
    with torch.no_grad():
        both = model(ids, attention_mask=pad).logits
    assert ca.ATTN_CALLS == {"hip": calls["hip"], "interface": calls["interface"] + 6}
    assert ca.ATTN_KERNELS == kernels and ca.ATTN_MASKED == masked and not any(masked.values())
    assert torch.equal(alone.view(torch.int16), off.view(torch.int16)) and torch.equal(both.view(torch.int16), off.view(torch.int16))
