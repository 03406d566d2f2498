"""CPU: mdg_attn_fwd checks its arguments without a device, and the MODEGPT_FUSED_ATTN switch of the compressed forward leaves CPU
tensors (and, unset, everything) on HF's attention interface, bit for bit."""
import pytest
import torch

from modegpt_amd import _lib


Q, K, V, O = 0x100000, 0x200000, 0x300000, 0x400000        # never dereferenced: every call below is refused before any device work
FAR = 1 << 62                                             # a pointer beyond every span a huge batch makes


def refused(lib, call, bad, name):
    """Every (arguments, message) of `bad` is refused by `call` with MDG_ERR_BAD_ARG and exactly that message, under `name`."""
    for kw, text in bad:
        assert text.startswith(name + ": "), text
        assert call(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        assert lib.mdg_last_error().decode() == text, (kw, lib.mdg_last_error())
        with pytest.raises(RuntimeError):
            _lib.check(call(**kw), name)


def call_fwd(lib, q=Q, k=K, v=V, dtype=_lib.MDG_BF16, B=2, T=5, S=9, n_heads=4, n_kv=2, r_qk=6, r_vo=3, kbs=2 * 9 * 6, khs=9 * 6, kts=6,
             vbs=2 * 9 * 3, vhs=9 * 3, vts=3, scale=0.5, causal=1, out=O, ld_out=12):
    return lib.mdg_attn_fwd(q, k, v, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, kbs, khs, kts, vbs, vhs, vts, scale, causal,
                            out, ld_out, None)


def test_bad_arguments_return_a_status_and_a_message_without_a_device():
    lib = _lib.load()
    inf, nan = float("inf"), float("nan")

    def call(**kw):
        return call_fwd(lib, **kw)

    bad = [  # dtype
           (dict(dtype=99), "mdg_attn_fwd: dtype 99 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(dtype=_lib.MDG_F32), "mdg_attn_fwd: dtype 2 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(dtype=_lib.MDG_F64), "mdg_attn_fwd: dtype 3 (bf16 or f16; fp32 inputs are out of scope)"),
           # negative
           (dict(B=-1), "mdg_attn_fwd: negative extent"), (dict(T=-1), "mdg_attn_fwd: negative extent"),
           (dict(S=-1, causal=0), "mdg_attn_fwd: negative extent"),
           # n_kv
           (dict(n_heads=5), "mdg_attn_fwd: n_heads=5 is not a positive multiple of n_kv=2"),
           (dict(n_kv=0), "mdg_attn_fwd: n_heads=4 is not a positive multiple of n_kv=0"),
           (dict(n_kv=3), "mdg_attn_fwd: n_heads=4 is not a positive multiple of n_kv=3"),
           # even, 256
           (dict(r_qk=5), "mdg_attn_fwd: r_qk=5 must be even, >= 2 and <= 256"),
           (dict(r_qk=0), "mdg_attn_fwd: r_qk=0 must be even, >= 2 and <= 256"),
           (dict(r_qk=258, kts=258), "mdg_attn_fwd: r_qk=258 must be even, >= 2 and <= 256"),
           # r_vo
           (dict(r_vo=0), "mdg_attn_fwd: r_vo=0 must be in 1..256"),
           (dict(r_vo=257, vts=257, ld_out=4 * 257), "mdg_attn_fwd: r_vo=257 must be in 1..256"),
           # causal
           (dict(S=4), "mdg_attn_fwd: causal with S=4 < T=5 keys"),
           # stride
           (dict(kts=5), "mdg_attn_fwd: k token stride 5 < r_qk=6"), (dict(vts=2), "mdg_attn_fwd: v token stride 2 < r_vo=3"),
           # ld_out
           (dict(ld_out=11), "mdg_attn_fwd: ld_out=11 < n_heads*r_vo=12"),
           # scale
           (dict(scale=0.0), "mdg_attn_fwd: scale 0 must be finite and positive"),
           (dict(scale=-1.0), "mdg_attn_fwd: scale -1 must be finite and positive"),
           (dict(scale=inf), "mdg_attn_fwd: scale inf must be finite and positive"),
           (dict(scale=nan), "mdg_attn_fwd: scale nan must be finite and positive"),
           # null
           (dict(q=None), "mdg_attn_fwd: null pointer"), (dict(k=None), "mdg_attn_fwd: null pointer"),
           (dict(v=None), "mdg_attn_fwd: null pointer"), (dict(out=None), "mdg_attn_fwd: null pointer"),
           # overlap
           (dict(out=Q), "mdg_attn_fwd: out overlaps q"), (dict(out=Q + 2 * (2 * 4 * 5 * 6 - 1)), "mdg_attn_fwd: out overlaps q"),
           (dict(q=O + 2), "mdg_attn_fwd: out overlaps q"),
           (dict(out=K + 2 * 50), "mdg_attn_fwd: out overlaps k"), (dict(out=V + 2 * 100), "mdg_attn_fwd: out overlaps v"),
           (dict(k=O + 2 * 119), "mdg_attn_fwd: out overlaps k"), (dict(v=O - 2 * 107), "mdg_attn_fwd: out overlaps v"),
           # the entry's own bounds: the index overflow before the empty call and the pointers, the launch bound after the spans
           (dict(B=2 ** 60), "mdg_attn_fwd: B*T overflows"),
           (dict(B=2 ** 31, out=FAR), "mdg_attn_fwd: B=2147483648, T=5 exceed one launch"),
           # two faults at once: the first check in the order above decides
           (dict(dtype=99, B=-1), "mdg_attn_fwd: dtype 99 (bf16 or f16; fp32 inputs are out of scope)"),
           (dict(r_vo=0, S=4), "mdg_attn_fwd: r_vo=0 must be in 1..256"),
           (dict(S=4, kts=5), "mdg_attn_fwd: causal with S=4 < T=5 keys"),
           (dict(scale=0.0, B=2 ** 60), "mdg_attn_fwd: scale 0 must be finite and positive"),
           (dict(B=2 ** 60, q=None), "mdg_attn_fwd: B*T overflows"),
           (dict(q=None, out=K), "mdg_attn_fwd: null pointer"),
           (dict(out=Q, k=Q), "mdg_attn_fwd: out overlaps q"), (dict(out=K, v=K), "mdg_attn_fwd: out overlaps k"),
           (dict(B=2 ** 31, v=FAR, out=FAR), "mdg_attn_fwd: out overlaps v")]
    refused(lib, call, bad, "mdg_attn_fwd")
    # an empty call is not an error and launches nothing, whatever the pointers
    assert call(B=0, q=None, out=None) == _lib.MDG_OK and call(T=0, k=None, v=None) == _lib.MDG_OK


def test_ops_attn_fwd_refuses_cpu_tensors():
    from modegpt_amd import ops
    q = torch.zeros(1, 2, 3, 4, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attn_fwd(q, q, q, 1.0)


def _tiny(kind):
    transformers = pytest.importorskip("transformers")
    from modegpt_amd.adapters.model_adapter import ModelAdapter  # noqa: F401  (the package's patchers import through it)
    torch.manual_seed(0)
    if kind == "opt":
        cfg = transformers.OPTConfig(hidden_size=32, ffn_dim=64, num_hidden_layers=2, num_attention_heads=4, vocab_size=64,
                                     max_position_embeddings=32, word_embed_proj_dim=32)
        model = transformers.OPTForCausalLM(cfg)
    else:
        cfg = transformers.LlamaConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                       num_key_value_heads=2, vocab_size=64, max_position_embeddings=32)
        model = transformers.LlamaForCausalLM(cfg)
    model = model.to(torch.bfloat16).eval()
    model.config._attn_implementation = "sdpa"
    from modegpt_amd.patchers import compressed_attention as ca
    ca._install(model, kind, None)
    return model, ca


@pytest.mark.parametrize("kind", ["llama", "opt"])
def test_switch_on_cpu_takes_the_interface_bit_for_bit_and_unset_never_counts_hip(kind, monkeypatch):
    model, ca = _tiny(kind)
    ids = torch.arange(12).reshape(2, 6) % 64
    monkeypatch.delenv("MODEGPT_FUSED_ATTN", raising=False)
    monkeypatch.delenv("MODEGPT_REQUIRE_HIP", raising=False)
    before = dict(ca.ATTN_CALLS)
    with torch.no_grad():
        off = model(ids).logits
    assert ca.ATTN_CALLS["hip"] == before["hip"] and ca.ATTN_CALLS["interface"] == before["interface"] + 2
    monkeypatch.setenv("MODEGPT_FUSED_ATTN", "1")
    with torch.no_grad():
        on = model(ids).logits
    assert ca.ATTN_CALLS["hip"] == before["hip"] and ca.ATTN_CALLS["interface"] == before["interface"] + 4
    assert torch.equal(on.view(torch.int16), off.view(torch.int16))
    assert set(ca.PATH_CALLS) == {"hip", "torch"}                  # the rotary counters are a separate table, untouched
