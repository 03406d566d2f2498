"""MODEGPT_FUSED_ATTN=1 end to end: the shipped modeling files of the fixture checkpoints (tests/golden/ckpt_*.npz) with the attention
product on mdg_attn_fwd.

  * driven layer by layer WITHOUT a mask (attention_mask=None: the condition under which the switch engages), every layer's product
    is served by the kernel (ATTN_CALLS) and the logits agree with the fixture's `logits_reference` (the reference's own modules,
    explicit causal mask) within the 3e-2 of the largest logit the existing fixture tests grant the GPU path;
  * greedy decoding with a KV cache through the model's own forward (prefill T = S, then T = 1 with S growing; sdpa, so HF hands
    the attention no mask): the tokens with the switch on equal those with it off at every step whose top-2 logit gap in the
    switch-off run exceeds the tolerance.  Tolerance: TWICE the largest deviation of the switch-off bf16 logits from an fp32 eager
    run of the same checkpoint on the same tokens -- measured in the test, printed, recorded in DESIGN.md section 8 -- and the fused
    logits must stay within it of the fp32 run as well.  The fused and the fp32 run are fed the switch-off run's tokens, so every
    step is comparable by itself.  At most one step in ten may fall under the gap and go uncompared;
  * an explicit 4-D mask keeps the call on HF's interface, bit-identical to the switch being off."""
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PROMPT_LEN, STEPS = 8, 12
# The fixtures are random-initialised: their logits are nearly flat and most prompts give top-2 gaps inside bf16 noise.  These seeds
# were chosen, over 300 prompts of PROMPT_LEN uniform tokens each, from the SWITCH-OFF run alone (bf16 sdpa against fp32 eager): the
# prompt whose smallest top-2 gap over the 13 steps is the largest multiple of the tolerance (llama: 4 x, qwen3: 16 x).
PROMPT_SEED = {"llama": 106, "qwen3": 221}


def _load(kind, tmp_path, monkeypatch, dev, dtype=torch.bfloat16, impl="sdpa"):
    transformers = pytest.importorskip("transformers")
    from tests.golden_util import materialise_checkpoint
    monkeypatch.setenv("HF_MODULES_CACHE", str(tmp_path / "hf_modules"))
    monkeypatch.setenv("MODEGPT_REQUIRE_HIP", "1")
    out, ids, z = materialise_checkpoint(kind, str(tmp_path / "model"))
    m = transformers.AutoModelForCausalLM.from_pretrained(out, trust_remote_code=True, dtype=dtype).to(dev).eval()
    m.config._attn_implementation = impl
    mod = sys.modules[type(m).__module__.rsplit(".", 1)[0] + ".compressed_attention"]
    return m, mod, ids.to(dev), z


def drive(model, ids, kind, mask="none"):
    """The model's own modules in order, as tests/golden_util.layer_drive / opt_drive run them, with attention_mask=None
    (mask="none") or their explicit additive causal mask (mask="4d")."""
    B, T = ids.shape
    with torch.no_grad():
        if kind == "opt":
            dec = model.model.decoder
            am = torch.ones(B, T, dtype=torch.long, device=ids.device)
            pos = (torch.cumsum(am, dim=1) * am - 1).long()
            h = dec.embed_tokens(ids)
            if dec.project_in is not None:
                h = dec.project_in(h)
            h = h + dec.embed_positions(am, 0, position_ids=pos)
            layers, kw = dec.layers, {}
        else:
            core = model.model
            h = core.embed_tokens(ids)
            pos = torch.arange(T, device=ids.device)[None].expand(B, T)
            layers, kw = core.layers, dict(position_ids=pos, position_embeddings=core.rotary_emb(h, pos))
        am4 = None
        if mask == "4d":
            am4 = torch.full((T, T), torch.finfo(h.dtype).min, dtype=h.dtype, device=ids.device).triu(1)[None, None]
        for layer in layers:
            out = layer(h, attention_mask=am4, **kw)
            h = out[0] if isinstance(out, tuple) else out
        if kind == "opt":
            if dec.final_layer_norm is not None:
                h = dec.final_layer_norm(h)
            if dec.project_out is not None:
                h = dec.project_out(h)
            return model.lm_head(h).float()
        return model.lm_head(model.model.norm(h)).float()


@pytest.mark.parametrize("kind", ["llama", "qwen3", "opt"])
def test_fixture_checkpoint_with_the_fused_kernel_matches_the_reference_modeling(dev, kind, tmp_path, monkeypatch):
    m, mod, ids, z = _load(kind, tmp_path, monkeypatch, dev)
    monkeypatch.setenv("MODEGPT_FUSED_ATTN", "1")
    before = dict(mod.ATTN_CALLS)
    got = drive(m, ids, kind).cpu().numpy()
    n_layers = m.config.num_hidden_layers
    assert mod.ATTN_CALLS["hip"] == before["hip"] + n_layers and mod.ATTN_CALLS["interface"] == before["interface"], mod.ATTN_CALLS
    want = z["logits_reference"]
    err = float(np.abs(got - want).max())
    print(f"{kind}: fused logits vs the reference modeling: max |diff| = {err:.3e}, largest logit {float(np.abs(want).max()):.3e}")
    assert err <= 3e-2 * np.abs(want).max(), err


@pytest.mark.parametrize("kind", ["llama", "qwen3", "opt"])
def test_explicit_mask_stays_on_the_interface_bit_for_bit(dev, kind, tmp_path, monkeypatch):
    m, mod, ids, z = _load(kind, tmp_path, monkeypatch, dev)
    monkeypatch.delenv("MODEGPT_FUSED_ATTN", raising=False)
    off = drive(m, ids, kind, mask="4d")
    monkeypatch.setenv("MODEGPT_FUSED_ATTN", "1")
    before = dict(mod.ATTN_CALLS)
    on = drive(m, ids, kind, mask="4d")
    assert mod.ATTN_CALLS["hip"] == before["hip"], mod.ATTN_CALLS
    assert mod.ATTN_CALLS["interface"] == before["interface"] + m.config.num_hidden_layers, mod.ATTN_CALLS
    assert torch.equal(on, off)


def greedy(model, prompt, steps, forced=None):
    """Prefill on `prompt`, then `steps` single-token steps with the cache: (last-position logits [steps + 1, B, V] fp32, tokens
    [steps + 1, B]).  With `forced` ([steps + 1, B]) those tokens are fed instead of the run's own argmax."""
    logits, toks = [], []
    with torch.no_grad():
        out = model(input_ids=prompt, use_cache=True)
        for t in range(steps + 1):
            last = out.logits[:, -1].float()
            logits.append(last)
            toks.append(last.argmax(-1))
            if t == steps:
                break
            nxt = (toks[-1] if forced is None else forced[t])[:, None]
            out = model(input_ids=nxt, past_key_values=out.past_key_values, use_cache=True)
    return torch.stack(logits), torch.stack(toks)


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_greedy_decoding_with_a_kv_cache_gives_the_same_tokens(dev, kind, tmp_path, monkeypatch):
    m, mod, ids, z = _load(kind, tmp_path, monkeypatch, dev)
    prompt = torch.randint(0, 97, (1, PROMPT_LEN), generator=torch.Generator().manual_seed(PROMPT_SEED[kind])).to(dev)
    n_layers, n_calls = m.config.num_hidden_layers, STEPS + 1
    monkeypatch.delenv("MODEGPT_FUSED_ATTN", raising=False)
    before = dict(mod.ATTN_CALLS)
    off_logits, off_toks = greedy(m, prompt, STEPS)
    assert mod.ATTN_CALLS["hip"] == before["hip"] and mod.ATTN_CALLS["interface"] == before["interface"] + n_layers * n_calls
    monkeypatch.setenv("MODEGPT_FUSED_ATTN", "1")
    before = dict(mod.ATTN_CALLS)
    on_logits, on_toks = greedy(m, prompt, STEPS, forced=off_toks)
    assert mod.ATTN_CALLS["hip"] == before["hip"] + n_layers * n_calls and mod.ATTN_CALLS["interface"] == before["interface"], \
        mod.ATTN_CALLS                                                       # prefill and every decode step ran the kernel
    monkeypatch.delenv("MODEGPT_FUSED_ATTN", raising=False)
    m32 = m.float()
    m32.config._attn_implementation = "eager"
    ref_logits, _ = greedy(m32, prompt, STEPS, forced=off_toks)

    dev_off = float((off_logits - ref_logits).abs().max())
    dev_on = float((on_logits - ref_logits).abs().max())
    tol = 2.0 * dev_off
    top2 = off_logits.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]                                        # [steps + 1, B]
    compared = gap > tol
    skipped = int((~compared).sum())
    print(f"{kind}: switch-off bf16 vs fp32 eager: max |dlogit| = {dev_off:.3e}; fused vs fp32 eager: {dev_on:.3e}; tolerance "
          f"{tol:.3e}; smallest top-2 gap {float(gap.min()):.3e}; {skipped} of {gap.numel()} steps under the gap")
    assert skipped * 10 <= gap.numel(), f"{skipped} of {gap.numel()} steps have a top-2 gap under {tol:.3e}"
    assert dev_on <= tol, (dev_on, tol)
    assert torch.equal(on_toks[compared], off_toks[compared]), (on_toks, off_toks)
