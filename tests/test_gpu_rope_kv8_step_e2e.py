"""MODEGPT_FUSED_KV_STEP=1 end to end: the llama and qwen3 fixture checkpoints with both fused-attention switches set, a 56-token
prompt and 12 forced single-token steps (tests/test_gpu_kv8_paged_e2e.py's protocol), on an Fp8KVCache and on a PagedFp8KVCache.  The
run with the switch is compared with the run without it: every layer call takes the fused step, the attention kernels serve the same
calls, and the logits are EQUAL for llama (no norm: the same bits reach the cache and attention); for qwen3 the norm's sum of squares
has another order, so the difference stays within tests/test_gpu_kv8_e2e.py's tolerance -- twice the switch-off bf16 run's deviation
from an fp32 eager run -- with identical tokens at the compared steps."""
import pytest
import torch

from tests.test_gpu_attn_fwd_e2e import STEPS, _load, greedy
from tests.test_gpu_kv8_e2e import greedy_with

pytestmark = pytest.mark.gpu
PROMPT = 56
SWITCHES = ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE")


@pytest.mark.parametrize("paged", [False, True], ids=["planes", "paged"])
@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_fused_step_gives_the_logits_of_the_chain(dev, kind, paged, tmp_path, monkeypatch):
    from modegpt_amd.patchers.kv8_cache import Fp8KVCache
    from modegpt_amd.patchers.kv8_paged_cache import PagedFp8KVCache

    m, mod, ids, z = _load(kind, tmp_path, monkeypatch, dev)
    n_layers = m.config.num_hidden_layers
    gen = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, 97, (2, PROMPT), generator=gen).to(dev)
    forced = torch.randint(0, 97, (STEPS + 1, 2), generator=gen).to(dev)
    new_cache = (lambda: PagedFp8KVCache(n_pages=5, page=64)) if paged else Fp8KVCache
    for name in SWITCHES:
        monkeypatch.setenv(name, "1")
    runs, kernels = {}, {}
    for on in (False, True):
        monkeypatch.setenv("MODEGPT_FUSED_KV_STEP", "1" if on else "0")
        monkeypatch.setitem(mod.KV_STEPS, "fused", 0)
        before = dict(mod.ATTN_KERNELS)
        cache = new_cache()
        runs[on] = greedy_with(m, cache, prompt, forced)
        kernels[on] = {k: n - before.get(k, 0) for k, n in mod.ATTN_KERNELS.items()}
        assert mod.KV_STEPS["fused"] == (n_layers * (STEPS + 1) if on else 0)
        assert cache.get_seq_length() == PROMPT + STEPS
    assert kernels[True] == kernels[False] and sum(kernels[True].values()) == n_layers * (STEPS + 1), kernels
    diff = float((runs[True] - runs[False]).abs().max())
    if kind == "llama":
        assert diff == 0.0
        return
    for name in SWITCHES + ("MODEGPT_FUSED_KV_STEP",):
        monkeypatch.delenv(name, raising=False)
    off_logits, _ = greedy(m, prompt, STEPS, forced=forced)
    m32 = m.float()
    m32.config._attn_implementation = "eager"
    ref_logits, _ = greedy(m32, prompt, STEPS, forced=forced)
    tol = 2.0 * float((off_logits - ref_logits).abs().max())
    top2 = runs[False].topk(2, dim=-1).values
    compared = top2[..., 0] - top2[..., 1] > tol
    print(f"{kind} {'paged' if paged else 'planes'}: fused step vs chain: max |dlogit| = {diff:.3e}, tolerance {tol:.3e}; "
          f"{int((~compared).sum())} of {compared.numel()} steps under the top-2 gap")
    assert diff <= tol
    assert torch.equal(runs[True].argmax(-1)[compared], runs[False].argmax(-1)[compared])
