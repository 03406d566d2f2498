"""MODEGPT_FUSED_ATTN=1 with MODEGPT_FUSED_ATTN_DECODE=1 end to end: greedy decoding with a KV cache through the shipped modeling
files of the fixture checkpoints, the protocol of tests/test_gpu_attn_fwd_e2e.py (same prompts and seeds, 8 prompt tokens plus 12
steps, tokens forced from the switch-off run).

Tolerance: TWICE the largest deviation of the switch-off bf16 logits from an fp32 eager run of the same checkpoint on the same
tokens, measured here and printed.  At most one step in ten may fall under the top-2 gap and go uncompared.  The run with both
switches is made twice -- with the split rule and with _DECODE_SPLITS = 3 -- and must give the switch-off tokens at every compared
step and logits within the tolerance of the fp32 run both times.  ATTN_KERNELS says which kernel served: the calls with
T * G <= 32 (G from the fixture's config) count under "decode", the rest under "fwd"; ATTN_CALLS["hip"] counts both."""
import pytest
import torch

from tests.test_gpu_attn_fwd_e2e import PROMPT_LEN, PROMPT_SEED, STEPS, _load, greedy

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_greedy_decoding_on_the_split_key_kernel_gives_the_same_tokens(dev, kind, tmp_path, monkeypatch):
    m, mod, ids, z = _load(kind, tmp_path, monkeypatch, dev)
    prompt = torch.randint(0, 97, (1, PROMPT_LEN), generator=torch.Generator().manual_seed(PROMPT_SEED[kind])).to(dev)
    cfg = m.config
    n_layers, G = cfg.num_hidden_layers, cfg.num_attention_heads // cfg.num_key_value_heads
    per_call_T = [PROMPT_LEN] + [1] * STEPS                                  # the prefill, then one token per step
    n_decode = n_layers * sum(1 for T in per_call_T if T * G <= 32)
    n_fwd = n_layers * len(per_call_T) - n_decode
    assert n_decode >= n_layers * STEPS                                      # every single-token step is in the domain

    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE"):
        monkeypatch.delenv(name, raising=False)
    off_logits, off_toks = greedy(m, prompt, STEPS)

    # only MODEGPT_FUSED_ATTN=1: the decode kernel serves nothing
    monkeypatch.setenv("MODEGPT_FUSED_ATTN", "1")
    calls, kernels = dict(mod.ATTN_CALLS), dict(mod.ATTN_KERNELS)
    greedy(m, prompt, 2, forced=off_toks)
    assert mod.ATTN_KERNELS == {"fwd": kernels["fwd"] + 3 * n_layers, "decode": kernels["decode"]}, mod.ATTN_KERNELS
    assert mod.ATTN_CALLS == {"hip": calls["hip"] + 3 * n_layers, "interface": calls["interface"]}, mod.ATTN_CALLS

    monkeypatch.setenv("MODEGPT_FUSED_ATTN_DECODE", "1")
    runs = {}
    for label, splits in (("rule", None), ("3 splits", 3)):
        monkeypatch.setattr(mod, "_DECODE_SPLITS", splits)
        calls, kernels = dict(mod.ATTN_CALLS), dict(mod.ATTN_KERNELS)
        runs[label] = greedy(m, prompt, STEPS, forced=off_toks)
        assert mod.ATTN_CALLS == {"hip": calls["hip"] + n_layers * 13, "interface": calls["interface"]}, mod.ATTN_CALLS
        assert mod.ATTN_KERNELS == {"fwd": kernels["fwd"] + n_fwd, "decode": kernels["decode"] + n_decode}, mod.ATTN_KERNELS
    monkeypatch.setattr(mod, "_DECODE_SPLITS", None)

    for name in ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE"):
        monkeypatch.delenv(name, raising=False)
    m32 = m.float()
    m32.config._attn_implementation = "eager"
    ref_logits, _ = greedy(m32, prompt, STEPS, forced=off_toks)

    dev_off = float((off_logits - ref_logits).abs().max())
    tol = 2.0 * dev_off
    top2 = off_logits.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]                                        # [steps + 1, B]
    compared = gap > tol
    skipped = int((~compared).sum())
    print(f"{kind}: G = {G}, {n_decode} products on the decode kernel, {n_fwd} on mdg_attn_fwd; switch-off bf16 vs fp32 eager: max "
          f"|dlogit| = {dev_off:.3e}; tolerance {tol:.3e}; smallest top-2 gap {float(gap.min()):.3e}; {skipped} of {gap.numel()} "
          f"steps under the gap")
    assert skipped * 10 <= gap.numel(), f"{skipped} of {gap.numel()} steps have a top-2 gap under {tol:.3e}"
    for label, (on_logits, on_toks) in runs.items():
        dev_on = float((on_logits - ref_logits).abs().max())
        print(f"{kind}: split-key decode ({label}) vs fp32 eager: max |dlogit| = {dev_on:.3e}")
        assert dev_on <= tol, (label, dev_on, tol)
        assert torch.equal(on_toks[compared], off_toks[compared]), (label, on_toks, off_toks)
