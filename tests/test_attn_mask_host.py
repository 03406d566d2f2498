"""CPU: the masked attention entries (mdg_attn_mask_summary, mdg_attn_fwd_masked, mdg_attn_decode_masked) check their arguments
without a device, mdg_attn_mask_summary_bytes says what the header says, and MODEGPT_FUSED_ATTN_MASK -- alone, or on CPU tensors --
leaves the compressed forward of a padded batch on HF's attention interface, bit for bit."""
import pytest
import torch

from modegpt_amd import _lib
from tests.test_attn_decode_host import W, call_decode
from tests.test_attn_fwd_host import K, O, Q, V, _tiny, call_fwd, refused

M, SM = 0x600000, 0x700000                                # the mask and the summary: like Q, K, V, O, W never dereferenced


def same_apart_from_the_name(lib, shared, masked, name, unmasked):
    """The masked entry `name` refuses each of `shared` with the words of the entry it is named after, under its own name."""
    for kw, text in shared:
        assert unmasked(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        plain = lib.mdg_last_error().decode()
        assert masked(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        assert plain.startswith(name[:-len("_masked")] + ": "), (kw, plain)
        assert lib.mdg_last_error().decode() == text == name + plain[len(name) - len("_masked"):], (kw, plain)


def test_summary_size_is_one_byte_per_tile():
    f = _lib.load().mdg_attn_mask_summary_bytes
    for B, Hm, T, S in [(1, 1, 1, 1), (2, 1, 5, 9), (2, 4, 32, 64), (2, 4, 33, 65), (3, 8, 70, 200), (16, 1, 8192, 8192), (1, 32, 1, 10 ** 6)]:
        assert f(B, Hm, T, S) == B * Hm * -(-T // 32) * -(-S // 64), (B, Hm, T, S)
    assert f(2 ** 20, 32, 2 ** 20, 2 ** 20) == 2 ** 20 * 32 * 2 ** 15 * 2 ** 14                        # 64-bit
    assert f(0, 1, 5, 9) == 0 and f(2, 0, 5, 9) == 0 and f(2, 1, 0, 9) == 0 and f(2, 1, 5, 0) == 0 and f(-1, 1, 5, 9) == 0


def test_summary_bad_arguments_return_a_status_and_a_message_without_a_device():
    lib = _lib.load()
    need = 2 * 1 * 1 * 1

    def call(mask=M, B=2, Hm=1, T=5, S=9, mbs=45, mhs=0, mqs=9, summary=SM, summary_bytes=need):
        return lib.mdg_attn_mask_summary(mask, B, Hm, T, S, mbs, mhs, mqs, summary, summary_bytes, None)

    short = " bytes is short of mdg_attn_mask_summary_bytes = "
    bad = [  # negative
           (dict(B=-1), "mdg_attn_mask_summary: negative extent"), (dict(T=-1), "mdg_attn_mask_summary: negative extent"),
           (dict(S=-1), "mdg_attn_mask_summary: negative extent"),
           # Hm
           (dict(Hm=0), "mdg_attn_mask_summary: mask heads Hm=0 must be positive"),
           (dict(Hm=-2), "mdg_attn_mask_summary: mask heads Hm=-2 must be positive"),
           # stride
           (dict(mbs=-45), "mdg_attn_mask_summary: negative mask stride (-45, 0, 9)"),
           (dict(mhs=-1), "mdg_attn_mask_summary: negative mask stride (45, -1, 9)"),
           (dict(mqs=-9), "mdg_attn_mask_summary: negative mask stride (45, 0, -9)"),
           # null mask, null summary, short
           (dict(mask=None), "mdg_attn_mask_summary: null mask"), (dict(summary=None), "mdg_attn_mask_summary: null summary"),
           (dict(summary_bytes=need - 1), "mdg_attn_mask_summary: summary of 1" + short + "2"),
           (dict(summary_bytes=0), "mdg_attn_mask_summary: summary of 0" + short + "2"),
           (dict(Hm=4), "mdg_attn_mask_summary: summary of 2" + short + "8"),
           # overlaps
           (dict(summary=M), "mdg_attn_mask_summary: summary overlaps mask"),
           (dict(summary=M + 45 + 4 * 9 + 8), "mdg_attn_mask_summary: summary overlaps mask"),
           (dict(mask=SM + 1), "mdg_attn_mask_summary: summary overlaps mask")]
    refused(lib, call, bad, "mdg_attn_mask_summary")
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
    short = " bytes is short of mdg_attn_mask_summary_bytes = "
    shared = [  # everything mdg_attn_fwd refuses: dtype, negative, n_kv
           (dict(dtype=99), "mdg_attn_fwd_masked: dtype 99 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(dtype=_lib.MDG_F32), "mdg_attn_fwd_masked: dtype 2 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(B=-1), "mdg_attn_fwd_masked: negative extent"), (dict(T=-1), "mdg_attn_fwd_masked: negative extent"),
           (dict(S=-1, causal=0), "mdg_attn_fwd_masked: negative extent"),
           (dict(n_heads=5), "mdg_attn_fwd_masked: n_heads=5 is not a positive multiple of n_kv=2"),
           (dict(n_kv=0), "mdg_attn_fwd_masked: n_heads=4 is not a positive multiple of n_kv=0"),
           (dict(n_kv=3), "mdg_attn_fwd_masked: n_heads=4 is not a positive multiple of n_kv=3"),
           # even, 256, r_vo, causal, stride, ld_out
           (dict(r_qk=5), "mdg_attn_fwd_masked: r_qk=5 must be even, >= 2 and <= 256"),
           (dict(r_qk=0), "mdg_attn_fwd_masked: r_qk=0 must be even, >= 2 and <= 256"),
           (dict(r_qk=258, kts=258), "mdg_attn_fwd_masked: r_qk=258 must be even, >= 2 and <= 256"),
           (dict(r_vo=0), "mdg_attn_fwd_masked: r_vo=0 must be in 1..256"),
           (dict(r_vo=257, vts=257, ld_out=4 * 257), "mdg_attn_fwd_masked: r_vo=257 must be in 1..256"),
           (dict(S=4), "mdg_attn_fwd_masked: causal with S=4 < T=5 keys"),
           (dict(kts=5), "mdg_attn_fwd_masked: k token stride 5 < r_qk=6"),
           (dict(vts=2), "mdg_attn_fwd_masked: v token stride 2 < r_vo=3"),
           (dict(ld_out=11), "mdg_attn_fwd_masked: ld_out=11 < n_heads*r_vo=12"),
           # scale, null, overlaps
           (dict(scale=0.0), "mdg_attn_fwd_masked: scale 0 must be finite and positive"),
           (dict(scale=-1.0), "mdg_attn_fwd_masked: scale -1 must be finite and positive"),
           (dict(scale=inf), "mdg_attn_fwd_masked: scale inf must be finite and positive"),
           (dict(scale=nan), "mdg_attn_fwd_masked: scale nan must be finite and positive"),
           (dict(q=None), "mdg_attn_fwd_masked: null pointer"), (dict(k=None), "mdg_attn_fwd_masked: null pointer"),
           (dict(v=None), "mdg_attn_fwd_masked: null pointer"), (dict(out=None), "mdg_attn_fwd_masked: null pointer"),
           (dict(out=Q), "mdg_attn_fwd_masked: out overlaps q"), (dict(out=K + 2 * 50), "mdg_attn_fwd_masked: out overlaps k"),
           (dict(out=V + 2 * 100), "mdg_attn_fwd_masked: out overlaps v"),
           # its own bounds, and two faults at once
           (dict(B=2 ** 60), "mdg_attn_fwd_masked: B*T overflows"),
           (dict(dtype=99, B=-1), "mdg_attn_fwd_masked: dtype 99 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(out=Q, k=Q), "mdg_attn_fwd_masked: out overlaps q")]
    bad = [  # the mask's own: Hm
           (dict(Hm=2), "mdg_attn_fwd_masked: mask heads Hm=2 must be 1 or n_heads=4"),
           (dict(Hm=0), "mdg_attn_fwd_masked: mask heads Hm=0 must be 1 or n_heads=4"),
           (dict(Hm=3), "mdg_attn_fwd_masked: mask heads Hm=3 must be 1 or n_heads=4"),
           (dict(Hm=-1), "mdg_attn_fwd_masked: mask heads Hm=-1 must be 1 or n_heads=4"),
           # negative mask stride
           (dict(mbs=-45), "mdg_attn_fwd_masked: negative mask stride (-45, 0, 9)"),
           (dict(mhs=-1), "mdg_attn_fwd_masked: negative mask stride (45, -1, 9)"),
           (dict(mqs=-9), "mdg_attn_fwd_masked: negative mask stride (45, 0, -9)"),
           # null mask, null summary, short
           (dict(mask=None), "mdg_attn_fwd_masked: null mask"), (dict(summary=None), "mdg_attn_fwd_masked: null summary"),
           (dict(summary_bytes=need - 1), "mdg_attn_fwd_masked: summary of 1" + short + "2"),
           (dict(summary_bytes=0), "mdg_attn_fwd_masked: summary of 0" + short + "2"),
           (dict(Hm=4, mhs=90, mbs=360), "mdg_attn_fwd_masked: summary of 2" + short + "8"),   # a per-head mask needs four times the summary
           # spans against out, computed with the strides: first byte, last byte, out inside the mask; a 0 stride counts extent 1
           (dict(mask=O), "mdg_attn_fwd_masked: out overlaps mask"),
           (dict(mask=O - (45 + 4 * 9 + 9) + 1), "mdg_attn_fwd_masked: out overlaps mask"),
           (dict(mask=O + out_bytes - 1), "mdg_attn_fwd_masked: out overlaps mask"),
           (dict(out=M + 2), "mdg_attn_fwd_masked: out overlaps mask"),
           (dict(mask=O - 8, mbs=0, mqs=0), "mdg_attn_fwd_masked: out overlaps mask"),   # one row of 9 bytes for every query: its last byte is out's first
           (dict(summary=O), "mdg_attn_fwd_masked: out overlaps summary"),
           (dict(summary=O - 1), "mdg_attn_fwd_masked: out overlaps summary"),
           (dict(summary=O + out_bytes - 1), "mdg_attn_fwd_masked: out overlaps summary"),
           # two faults at once: the operands come before the mask, the mask before the summary
           (dict(out=V + 2 * 100, Hm=3), "mdg_attn_fwd_masked: out overlaps v"),
           (dict(mask=None, Hm=3), "mdg_attn_fwd_masked: mask heads Hm=3 must be 1 or n_heads=4"),
           (dict(mask=None, mqs=-9), "mdg_attn_fwd_masked: negative mask stride (45, 0, -9)"),
           (dict(mask=None, summary=None), "mdg_attn_fwd_masked: null mask"),
           (dict(mask=O, summary_bytes=0), "mdg_attn_fwd_masked: out overlaps mask"),
           (dict(mask=O, summary=O), "mdg_attn_fwd_masked: out overlaps mask"),
           (dict(summary=None, summary_bytes=0), "mdg_attn_fwd_masked: null summary"),
           (dict(summary=O, summary_bytes=0), "mdg_attn_fwd_masked: summary of 0" + short + "2")]
    refused(lib, call, shared + bad, "mdg_attn_fwd_masked")
    same_apart_from_the_name(lib, shared, call, "mdg_attn_fwd_masked", lambda **kw: call_fwd(lib, **kw))
    # the neighbours of the refused spans pass the mask checks: the call is then refused for its summary, which is checked next
    for kw, n in ((dict(mask=O - (45 + 4 * 9 + 9)), "2"), (dict(mask=O + out_bytes), "2"), (dict(mask=O - 9, mbs=0, mqs=0), "2"),
                  (dict(Hm=4, mhs=90, mbs=360), "8")):
        assert call(summary_bytes=0, **kw) == _lib.MDG_ERR_BAD_ARG, kw
        assert lib.mdg_last_error().decode() == "mdg_attn_fwd_masked: summary of 0" + short + n, kw
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
    assert need == 3840
    shared = [  # everything mdg_attn_decode refuses: dtype, negative, n_kv, even, r_vo
           (dict(dtype=99), "mdg_attn_decode_masked: dtype 99 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(B=-1), "mdg_attn_decode_masked: negative extent"),
           (dict(n_heads=5), "mdg_attn_decode_masked: n_heads=5 is not a positive multiple of n_kv=2"),
           (dict(r_qk=5), "mdg_attn_decode_masked: r_qk=5 must be even, >= 2 and <= 256"),
           (dict(r_vo=0), "mdg_attn_decode_masked: r_vo=0 must be in 1..256"),
           # tile, splits, causal, stride, ld_out, scale
           (dict(T=17, S=20), "mdg_attn_decode_masked: T=17 queries x group of 2 heads exceed the tile of 32 columns (use mdg_attn_fwd)"),
           (dict(splits=0), "mdg_attn_decode_masked: splits=0 must be in 1..256"),
           (dict(splits=257), "mdg_attn_decode_masked: splits=257 must be in 1..256"),
           (dict(S=4), "mdg_attn_decode_masked: causal with S=4 < T=5 keys"),
           (dict(kts=5), "mdg_attn_decode_masked: k token stride 5 < r_qk=6"),
           (dict(vts=2), "mdg_attn_decode_masked: v token stride 2 < r_vo=3"),
           (dict(ld_out=11), "mdg_attn_decode_masked: ld_out=11 < n_heads*r_vo=12"),
           (dict(scale=0.0), "mdg_attn_decode_masked: scale 0 must be finite and positive"),
           # null, null workspace, short, aligned, overlap
           (dict(q=None), "mdg_attn_decode_masked: null pointer"), (dict(out=None), "mdg_attn_decode_masked: null pointer"),
           (dict(ws=None), "mdg_attn_decode_masked: null workspace"),
           (dict(ws_bytes=need - 1), "mdg_attn_decode_masked: workspace of 3839 bytes is short of mdg_attn_decode_ws_bytes = 3840"),
           (dict(ws=W + 4), "mdg_attn_decode_masked: workspace must be 16-byte aligned"),
           (dict(out=Q), "mdg_attn_decode_masked: out overlaps q"), (dict(ws=Q), "mdg_attn_decode_masked: workspace overlaps q"),
           (dict(ws=O), "mdg_attn_decode_masked: workspace overlaps out"),
           (dict(out=W + need - 2), "mdg_attn_decode_masked: workspace overlaps out"),
           # its own bounds, and two faults at once
           (dict(B=2 ** 50), "mdg_attn_decode_masked: B*T overflows"),
           (dict(dtype=99, B=-1), "mdg_attn_decode_masked: dtype 99 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(r_qk=5, T=17, S=20), "mdg_attn_decode_masked: r_qk=5 must be even, >= 2 and <= 256"),
           (dict(T=17, S=20, splits=0),
            "mdg_attn_decode_masked: T=17 queries x group of 2 heads exceed the tile of 32 columns (use mdg_attn_fwd)"),
           (dict(splits=0, S=4), "mdg_attn_decode_masked: splits=0 must be in 1..256"),
           (dict(ws=W + 4, ws_bytes=need - 1),
            "mdg_attn_decode_masked: workspace of 3839 bytes is short of mdg_attn_decode_ws_bytes = 3840"),
           (dict(out=Q, k=Q), "mdg_attn_decode_masked: out overlaps q"),
           (dict(ws=K, out=V), "mdg_attn_decode_masked: workspace overlaps k")]
    bad = [  # the mask's own: Hm, negative mask stride, null mask
           (dict(Hm=2), "mdg_attn_decode_masked: mask heads Hm=2 must be 1 or n_heads=4"),
           (dict(Hm=0), "mdg_attn_decode_masked: mask heads Hm=0 must be 1 or n_heads=4"),
           (dict(mbs=-45), "mdg_attn_decode_masked: negative mask stride (-45, 0, 9)"),
           (dict(mhs=-1), "mdg_attn_decode_masked: negative mask stride (45, -1, 9)"),
           (dict(mqs=-9), "mdg_attn_decode_masked: negative mask stride (45, 0, -9)"),
           (dict(mask=None), "mdg_attn_decode_masked: null mask"),
           # out overlaps mask, workspace overlaps mask
           (dict(mask=O), "mdg_attn_decode_masked: out overlaps mask"),
           (dict(mask=O - (45 + 4 * 9 + 9) + 1), "mdg_attn_decode_masked: out overlaps mask"),
           (dict(mask=O + out_bytes - 1), "mdg_attn_decode_masked: out overlaps mask"),
           (dict(mask=O - 8, mbs=0, mqs=0), "mdg_attn_decode_masked: out overlaps mask"),
           (dict(mask=W + need - 1), "mdg_attn_decode_masked: workspace overlaps mask"),
           (dict(mask=W - (45 + 4 * 9 + 9) + 1), "mdg_attn_decode_masked: workspace overlaps mask"),
           # two faults at once: out against the workspace, then the mask (its own checks, out, the workspace), then q, k, v
           (dict(ws=O, mask=O + 1024), "mdg_attn_decode_masked: workspace overlaps out"),
           (dict(ws=O, Hm=3), "mdg_attn_decode_masked: workspace overlaps out"),
           (dict(mask=None, Hm=3), "mdg_attn_decode_masked: mask heads Hm=3 must be 1 or n_heads=4"),
           (dict(Hm=3, out=Q), "mdg_attn_decode_masked: mask heads Hm=3 must be 1 or n_heads=4"),
           (dict(mask=None, out=Q), "mdg_attn_decode_masked: null mask"),
           (dict(mask=O + 16, ws=O + 32, out=O), "mdg_attn_decode_masked: workspace overlaps out"),
           (dict(mask=Q, out=Q), "mdg_attn_decode_masked: out overlaps mask"),
           (dict(mask=Q, ws=Q), "mdg_attn_decode_masked: workspace overlaps mask"),
           (dict(mask=W, q=O + 2), "mdg_attn_decode_masked: workspace overlaps mask")]
    refused(lib, call, shared + bad, "mdg_attn_decode_masked")
    same_apart_from_the_name(lib, shared, call, "mdg_attn_decode_masked", lambda **kw: call_decode(lib, **kw))
    # the neighbours of the refused spans pass the mask checks: the call is then refused for its q, which is checked next
    for kw in (dict(mask=O - (45 + 4 * 9 + 9)), dict(mask=O + out_bytes), dict(mask=O - 9, mbs=0, mqs=0), dict(mask=W + need)):
        assert call(q=O + 2, **kw) == _lib.MDG_ERR_BAD_ARG and lib.mdg_last_error().decode() == "mdg_attn_decode_masked: out overlaps q", kw
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
