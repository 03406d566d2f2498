"""PagedFp8KVCache end to end: the llama and qwen3 fixture checkpoints of tests/test_gpu_kv8_e2e.py with both fused-attention switches
set, a 56-token prompt and 12 forced single-token steps, so that the steps cross the page boundary at 64 tokens (the fixtures are
rotary models: their max_position_embeddings of 32 sizes no table and limits nothing).  Every step x layer is served by
mdg_attn_decode_paged8, and the logits equal those of the same run on an Fp8KVCache EXACTLY: the appended bytes are the same and the
paged kernel gives every sequence the bits of mdg_attn_decode_kv8."""
import pytest
import torch

from tests.test_gpu_attn_fwd_e2e import STEPS, _load
from tests.test_gpu_kv8_e2e import greedy_with

pytestmark = pytest.mark.gpu
PROMPT = 56


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_paged_cache_gives_the_logits_of_the_contiguous_cache_bit_for_bit(dev, kind, tmp_path, monkeypatch):
    from modegpt_amd.patchers.kv8_cache import Fp8KVCache
    from modegpt_amd.patchers.kv8_paged_cache import PagedFp8KVCache

    m, mod, ids, z = _load(kind, tmp_path, monkeypatch, dev)
    gen = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, 97, (2, PROMPT), generator=gen).to(dev)
    forced = torch.randint(0, 97, (STEPS + 1, 2), generator=gen).to(dev)
    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE"):
        monkeypatch.setenv(name, "1")
    monkeypatch.setitem(mod.ATTN_KERNELS, "decode_paged8", 0)
    cache = PagedFp8KVCache(n_pages=5, page=64)
    paged = greedy_with(m, cache, prompt, forced)
    assert mod.ATTN_KERNELS["decode_paged8"] == m.config.num_hidden_layers * STEPS, mod.ATTN_KERNELS
    assert cache.get_seq_length() == PROMPT + STEPS and cache.pages_in_use == 4
    flat = greedy_with(m, Fp8KVCache(), prompt, forced)
    assert mod.ATTN_KERNELS["decode_paged8"] == m.config.num_hidden_layers * STEPS
    assert float((paged - flat).abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="exhausted"), torch.no_grad():                 # 2 sequences x 3 pages: one page short
        m(input_ids=torch.zeros(2, 64, dtype=torch.long, device=dev), past_key_values=cache, use_cache=True)
    cache.reset()
    assert cache.pages_in_use == 0 and cache.get_seq_length() == 0
