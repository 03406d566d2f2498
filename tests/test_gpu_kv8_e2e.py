"""Fp8KVCache end to end: greedy decoding through the shipped modeling files of the fixture checkpoints with both fused-attention
switches set, the 8 + 12 token protocol of tests/test_gpu_attn_decode_e2e.py (tokens forced from the switch-off run).

Run A keeps its cache in an Fp8KVCache: every decode step is served by mdg_attn_decode_kv8 (ATTN_KERNELS["decode_kv8"] counts them).
Run B is the same generate with a test-local cache that quantises with ops.kv8_append, reads everything back with ops.kv8_dequant
and hands the bf16 tensors on, so mdg_attn_decode serves the steps on the SAME dequantised values: A against B isolates the new
kernel.  Tolerance for A against B: that file's, twice the deviation of the switch-off bf16 run from an fp32 eager run -- what two
bf16 runs of one model may differ by -- and identical tokens at the compared steps.  A's own deviation from the fp32 run is what
fp8 quantisation costs these fixtures; it is printed, not asserted."""
import pytest
import torch

from tests.test_gpu_attn_fwd_e2e import PROMPT_LEN, PROMPT_SEED, STEPS, _load, greedy

pytestmark = pytest.mark.gpu


def greedy_with(model, cache, prompt, forced):
    logits, ids = [], prompt
    with torch.no_grad():
        for t in range(STEPS + 1):
            out = model(input_ids=ids, past_key_values=cache, use_cache=True)
            logits.append(out.logits[:, -1].float())
            ids = forced[t][:, None]
    return torch.stack(logits)


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_greedy_decoding_from_the_fp8_cache(dev, kind, tmp_path, monkeypatch):
    from transformers.cache_utils import Cache

    from modegpt_amd import ops
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

    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE"):
        monkeypatch.setenv(name, "1")
    monkeypatch.setitem(mod.ATTN_KERNELS, "decode_kv8", 0)
    before = dict(mod.ATTN_KERNELS)
    cache = Fp8KVCache()
    a_logits = greedy_with(m, cache, prompt, off_toks)
    assert mod.ATTN_KERNELS["decode_kv8"] == n_layers * STEPS, mod.ATTN_KERNELS          # every single-token step
    assert mod.ATTN_KERNELS["decode"] + mod.ATTN_KERNELS["fwd"] == before["decode"] + before["fwd"] + n_layers   # the prefill
    assert cache.get_seq_length() == PROMPT_LEN + STEPS and all(layer.copies == 0 for layer in cache.layers)
    b_logits = greedy_with(m, Cache(layer_class_to_replicate=RoundTripLayer), prompt, off_toks)
    assert mod.ATTN_KERNELS["decode_kv8"] == n_layers * STEPS

    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE"):
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
