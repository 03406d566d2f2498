"""PagedFp8KVCache end to end without the decode switch: the chunked_with protocol of tests/test_gpu_attn_fwd_kv8_e2e.py on the llama
and qwen3 fixtures with MODEGPT_FUSED_ATTN=1 and MODEGPT_FUSED_ATTN_MASK=1 -- a 56-token prompt, then a chunk of 10 tokens in one call
(positions 56 .. 65: across the page edge at 64; Transformers hands it a bool causal mask), then single steps.  Every call against the
non-empty cache is served by mdg_attn_fwd_paged8 straight from the pages -- nothing is gathered -- and the logits equal those of the
same run on an Fp8KVCache EXACTLY: the appended bytes are the same and the paged kernel gives every sequence the bits of
mdg_attn_fwd_kv8."""
import pytest
import torch

from tests import test_gpu_attn_fwd_kv8_e2e as flat_e2e
from tests.test_gpu_attn_fwd_e2e import STEPS, _load

pytestmark = pytest.mark.gpu
PROMPT, CHUNK = 56, 10


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_chunk_across_a_page_edge_and_steps_straight_from_the_pages(dev, kind, tmp_path, monkeypatch):
    from modegpt_amd import ops
    from modegpt_amd.patchers.kv8_cache import Fp8KVCache
    from modegpt_amd.patchers.kv8_paged_cache import PagedFp8KVCache

    def gathered(*args, **kwargs):
        raise AssertionError("ops.kv8_paged_dequant was called: a cached call gathered the pages")

    m, mod, ids, z = _load(kind, tmp_path, monkeypatch, dev)
    gen = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, 97, (2, PROMPT), generator=gen).to(dev)
    forced = torch.randint(0, 97, (STEPS + 1, 2), generator=gen).to(dev)
    monkeypatch.delenv("MODEGPT_FUSED_ATTN_DECODE", raising=False)
    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_MASK"):
        monkeypatch.setenv(name, "1")
    monkeypatch.setattr(flat_e2e, "CHUNK", CHUNK)
    monkeypatch.setattr(ops, "kv8_paged_dequant", gathered)
    for key in ("fwd_paged8", "fwd_kv8"):                          # (taken out again afterwards: a key appears with the first call)
        monkeypatch.setitem(mod.ATTN_KERNELS, key, 0)
    masked, n_layers = mod.ATTN_MASKED["fwd"], m.config.num_hidden_layers
    cache = PagedFp8KVCache(n_pages=5, page=64)
    paged, cached_calls = flat_e2e.chunked_with(m, cache, prompt, forced)
    assert cached_calls == 1 + STEPS - CHUNK and mod.ATTN_KERNELS["fwd_paged8"] == n_layers * cached_calls, mod.ATTN_KERNELS
    assert mod.ATTN_MASKED["fwd"] == masked + n_layers                                    # the chunk
    assert cache.get_seq_length() == PROMPT + STEPS and cache.pages_in_use == 4
    flat, _ = flat_e2e.chunked_with(m, Fp8KVCache(), prompt, forced)
    assert mod.ATTN_KERNELS["fwd_paged8"] == n_layers * cached_calls
    assert float((paged - flat).abs().max()) == 0.0
