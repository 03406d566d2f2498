"""Fp8KVCache end to end without the decode switch: the protocol of tests/test_gpu_kv8_e2e.py on the same fixtures and forced tokens,
fed as the prompt, then a chunk of CHUNK tokens in one call, then single steps -- every call against the non-empty cache is served by
mdg_attn_fwd_kv8 (ATTN_KERNELS["fwd_kv8"]) and nothing is dequantised.  MODEGPT_FUSED_ATTN_MASK=1 stands beside MODEGPT_FUSED_ATTN=1:
Transformers hands a chunk fed against a non-empty cache (1 < T < S) a bool causal mask, which MODEGPT_FUSED_ATTN=1 alone leaves on
HF's interface; with it the chunk runs the masked kernel and the single steps the unmasked one.

Run A keeps its cache in an Fp8KVCache.  Run B is that file's round-trip layer (quantise, dequant(), hand bf16 tensors on), so
mdg_attn_fwd serves its calls on the SAME dequantised values: A against B isolates the new kernel.  Tolerance: that file's, twice the
deviation of the switch-off bf16 run from an fp32 eager run; identical tokens where the top-2 gap exceeds it."""
import pytest
import torch

from tests.test_gpu_attn_fwd_e2e import PROMPT_LEN, PROMPT_SEED, STEPS, _load, greedy

pytestmark = pytest.mark.gpu
CHUNK = 4


def chunked_with(model, cache, prompt, forced):
    """Logits [STEPS + 1, B, V] at the positions of greedy()'s: the prompt's last, every position of the chunk, each single step."""
    feeds = [prompt, forced[:CHUNK].T] + [forced[t][:, None] for t in range(CHUNK, STEPS)]
    logits = []
    with torch.no_grad():
        for ids in feeds:
            out = model(input_ids=ids, past_key_values=cache, use_cache=True).logits.float()
            logits += list(out.transpose(0, 1)) if ids is feeds[1] else [out[:, -1]]
    return torch.stack(logits), len(feeds) - 1


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_chunked_prefill_and_steps_from_the_fp8_cache(dev, kind, tmp_path, monkeypatch):
    from transformers.cache_utils import Cache

    from modegpt_amd.patchers.kv8_cache import Fp8KVCache, Fp8KVLayer

    class RoundTripLayer(Fp8KVLayer):                 # run B: the same planes, read back whole and handed on as tensors
        def update(self, key_states, value_states, *args, **kwargs):
            k, v = super().update(key_states, value_states, *args, **kwargs)
            return (k.fresh, v.fresh) if k.S == key_states.shape[2] else (k.dequant(), v.dequant())

    m, mod, ids, z = _load(kind, tmp_path, monkeypatch, dev)
    prompt = torch.randint(0, 97, (1, PROMPT_LEN), generator=torch.Generator().manual_seed(PROMPT_SEED[kind])).to(dev)
    n_layers = m.config.num_hidden_layers
    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE"):
        monkeypatch.delenv(name, raising=False)
    off_logits, off_toks = greedy(m, prompt, STEPS)

    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_MASK"):
        monkeypatch.setenv(name, "1")
    monkeypatch.setitem(mod.ATTN_KERNELS, "fwd_kv8", 0)          # (taken out again afterwards: the key appears with the first call)
    before, masked = dict(mod.ATTN_KERNELS), mod.ATTN_MASKED["fwd"]
    cache = Fp8KVCache()
    a_logits, cached_calls = chunked_with(m, cache, prompt, off_toks)
    assert mod.ATTN_KERNELS["fwd_kv8"] == n_layers * cached_calls, mod.ATTN_KERNELS
    assert mod.ATTN_KERNELS["fwd"] == before["fwd"] + n_layers and mod.ATTN_KERNELS["decode"] == before["decode"]   # the first prefill
    assert mod.ATTN_MASKED["fwd"] == masked + n_layers                                                           # the chunk
    assert cache.get_seq_length() == PROMPT_LEN + STEPS and all(layer.copies == 0 for layer in cache.layers)
    b_logits, _ = chunked_with(m, Cache(layer_class_to_replicate=RoundTripLayer), prompt, off_toks)
    assert mod.ATTN_KERNELS["fwd"] == before["fwd"] + n_layers * (2 + cached_calls)

    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_MASK"):
        monkeypatch.delenv(name, raising=False)
    m32 = m.float()
    m32.config._attn_implementation = "eager"
    ref_logits, _ = greedy(m32, prompt, STEPS, forced=off_toks)

    tol = 2.0 * float((off_logits - ref_logits).abs().max())
    top2 = b_logits.topk(2, dim=-1).values
    compared = top2[..., 0] - top2[..., 1] > tol
    print(f"{kind}: fp8 cache vs fp32 eager: max |dlogit| = {float((a_logits - ref_logits).abs().max()):.3e} (bf16 cache, switches off: "
          f"{tol / 2:.3e}); kernel vs round trip: {float((a_logits - b_logits).abs().max()):.3e}, tolerance {tol:.3e}; "
          f"{int((~compared).sum())} of {compared.numel()} steps under the top-2 gap")
    assert int((~compared).sum()) * 10 <= compared.numel()
    assert float((a_logits - b_logits).abs().max()) <= tol
    assert torch.equal(a_logits.argmax(-1)[compared], b_logits.argmax(-1)[compared])
