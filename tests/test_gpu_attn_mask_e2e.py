"""MODEGPT_FUSED_ATTN_MASK=1 end to end: a left-padded batch through the shipped modeling files of the fixture checkpoints, greedy
decoding with a KV cache, the protocol of tests/test_gpu_attn_fwd_e2e.py (8 prompt positions plus 12 steps, tokens forced from the
switch-off run).

The batch: row 0 holds 8 real tokens, row 1 holds 5 real tokens left-padded by 3; attention_mask goes in with the prefill and grows
by ones at every step, so Transformers hands every layer of every call a bool [2, 1, T, S] mask (the causal rule ANDed with the
padding columns).  With MODEGPT_FUSED_ATTN=1, MODEGPT_FUSED_ATTN_DECODE=1 and MODEGPT_FUSED_ATTN_MASK=1 every one of those products
runs on the engine's kernels (ATTN_CALLS, ATTN_KERNELS, ATTN_MASKED); without MODEGPT_FUSED_ATTN_MASK the same run is served by
HF's interface, as every masked call was before the switch existed.

Only last-position logits are compared, so the rows of the pad queries (which see no key at all: zeros from the kernels) are never
read.  The compressed forward uses batch row 0's rotary table for every row (the reference's behaviour); the unpadded prompt sits
in row 0, and both runs share the table either way.

Tolerance: TWICE the largest deviation of the switch-off bf16 last-position logits from an fp32 eager run of the same checkpoint
on the same padded input, measured here and printed.  The fused run must stay within it of the fp32 run and give the switch-off
tokens at every (step, row) whose top-2 gap exceeds it; at most one (step, row) pair in ten may go uncompared.

PROMPT_SEED: chosen over 300 padded prompt pairs from the SWITCH-OFF run alone (bf16 sdpa against fp32 eager on the same padded
input), before any fused run.  Two of the 26 (step, row) pairs may go uncompared, so the seed taken is the one whose THIRD-smallest
top-2 gap is the largest multiple of the tolerance.  The search ran the switch-off forward's portable torch path on the CPU (same
checkpoints, same protocol): llama seed 297 -- third-smallest gap 2.93e-2 = 2.5 x the tolerance 1.15e-2, smallest gap 1.37e-2, no
pair under the tolerance; qwen3 seed 139 -- third-smallest gap 2.54e-2 = 2.0 x the tolerance 1.27e-2, smallest gap 2.0e-3, one pair
under the tolerance.  The test measures and prints the GPU's own figures; the cap is asserted on those."""
import pytest
import torch

from tests.test_gpu_attn_fwd_e2e import PROMPT_LEN, STEPS, _load

pytestmark = pytest.mark.gpu

PAD = 3
PROMPT_SEED = {"llama": 297, "qwen3": 139}
SWITCHES = ("MODEGPT_FUSED_ATTN", "MODEGPT_FUSED_ATTN_DECODE", "MODEGPT_FUSED_ATTN_MASK")


def padded_batch(seed, dev):
    """(input ids [2, 8], attention_mask [2, 8]): row 1 left-padded by PAD positions (token 0 there; it is never attended)."""
    prompt = torch.randint(0, 97, (2, PROMPT_LEN), generator=torch.Generator().manual_seed(seed))
    attn = torch.ones(2, PROMPT_LEN, dtype=torch.long)
    prompt[1, :PAD] = 0
    attn[1, :PAD] = 0
    return prompt.to(dev), attn.to(dev)


def greedy_padded(model, prompt, attn, steps, forced=None):
    """tests/test_gpu_attn_fwd_e2e.greedy with an attention_mask that grows by a column of ones per step."""
    logits, toks = [], []
    with torch.no_grad():
        out = model(input_ids=prompt, attention_mask=attn, use_cache=True)
        for t in range(steps + 1):
            last = out.logits[:, -1].float()
            logits.append(last)
            toks.append(last.argmax(-1))
            if t == steps:
                break
            nxt = (toks[-1] if forced is None else forced[t])[:, None]
            attn = torch.cat([attn, torch.ones_like(attn[:, :1])], dim=1)
            out = model(input_ids=nxt, attention_mask=attn, past_key_values=out.past_key_values, use_cache=True)
    return torch.stack(logits), torch.stack(toks)


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_left_padded_greedy_decoding_runs_on_the_kernels_and_gives_the_same_tokens(dev, kind, tmp_path, monkeypatch):
    m, mod, ids, z = _load(kind, tmp_path, monkeypatch, dev)
    prompt, attn = padded_batch(PROMPT_SEED[kind], dev)
    cfg = m.config
    n_layers, G = cfg.num_hidden_layers, cfg.num_attention_heads // cfg.num_key_value_heads
    per_call_T = [PROMPT_LEN] + [1] * STEPS
    n_decode = n_layers * sum(1 for T in per_call_T if T * G <= 32)
    n_fwd = n_layers * len(per_call_T) - n_decode
    assert n_decode >= n_layers * STEPS

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    off_logits, off_toks = greedy_padded(m, prompt, attn, STEPS)
    assert bool(torch.isfinite(off_logits).all())

    # without the feature: the fused switches alone leave every masked call on HF's interface, bit for bit
    monkeypatch.setenv("MODEGPT_FUSED_ATTN", "1")
    monkeypatch.setenv("MODEGPT_FUSED_ATTN_DECODE", "1")
    calls, kernels, masked = dict(mod.ATTN_CALLS), dict(mod.ATTN_KERNELS), dict(mod.ATTN_MASKED)
    same_logits, _ = greedy_padded(m, prompt, attn, STEPS, forced=off_toks)
    assert mod.ATTN_CALLS == {"hip": calls["hip"], "interface": calls["interface"] + n_layers * 13}, mod.ATTN_CALLS
    assert mod.ATTN_KERNELS == kernels and mod.ATTN_MASKED == masked
    assert torch.equal(same_logits, off_logits)

    # with it: every layer of every call is served by the kernels
    monkeypatch.setenv("MODEGPT_FUSED_ATTN_MASK", "1")
    calls, kernels, masked = dict(mod.ATTN_CALLS), dict(mod.ATTN_KERNELS), dict(mod.ATTN_MASKED)
    on_logits, on_toks = greedy_padded(m, prompt, attn, STEPS, forced=off_toks)
    assert mod.ATTN_CALLS == {"hip": calls["hip"] + n_layers * 13, "interface": calls["interface"]}, mod.ATTN_CALLS
    assert mod.ATTN_KERNELS == {"fwd": kernels["fwd"] + n_fwd, "decode": kernels["decode"] + n_decode}, mod.ATTN_KERNELS
    assert mod.ATTN_MASKED == {"fwd": masked["fwd"] + n_fwd, "decode": masked["decode"] + n_decode}, mod.ATTN_MASKED
    assert bool(torch.isfinite(on_logits).all())
    runs = {"three switches": (on_logits, on_toks)}

    # ... and without the decode switch by mdg_attn_fwd_masked alone (the fixtures' T * G fits the decode tile even at the prefill)
    monkeypatch.delenv("MODEGPT_FUSED_ATTN_DECODE")
    calls, kernels, masked = dict(mod.ATTN_CALLS), dict(mod.ATTN_KERNELS), dict(mod.ATTN_MASKED)
    runs["prefill kernel only"] = greedy_padded(m, prompt, attn, STEPS, forced=off_toks)
    assert mod.ATTN_CALLS == {"hip": calls["hip"] + n_layers * 13, "interface": calls["interface"]}, mod.ATTN_CALLS
    assert mod.ATTN_KERNELS == {"fwd": kernels["fwd"] + n_layers * 13, "decode": kernels["decode"]}, mod.ATTN_KERNELS
    assert mod.ATTN_MASKED == {"fwd": masked["fwd"] + n_layers * 13, "decode": masked["decode"]}, mod.ATTN_MASKED

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    m32 = m.float()
    m32.config._attn_implementation = "eager"
    ref_logits, _ = greedy_padded(m32, prompt, attn, STEPS, forced=off_toks)

    dev_off = float((off_logits - ref_logits).abs().max())
    tol = 2.0 * dev_off
    top2 = off_logits.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]                                        # [steps + 1, 2]
    compared = gap > tol
    skipped = int((~compared).sum())
    print(f"{kind}: G = {G}, {n_decode} masked products on the decode kernel, {n_fwd} on mdg_attn_fwd_masked; switch-off bf16 vs fp32 "
          f"eager: max |dlogit| = {dev_off:.3e}; tolerance {tol:.3e}; smallest top-2 gap "
          f"{float(gap.min()):.3e}; {skipped} of {gap.numel()} (step, row) pairs under the gap")
    assert skipped * 10 <= gap.numel(), f"{skipped} of {gap.numel()} (step, row) pairs have a top-2 gap under {tol:.3e}"
    for label, (logits, toks) in runs.items():
        dev_on = float((logits - ref_logits).abs().max())
        print(f"{kind}: masked kernels ({label}) vs fp32 eager: max |dlogit| = {dev_on:.3e}")
        assert dev_on <= tol, (label, dev_on, tol)
        assert torch.equal(toks[compared], off_toks[compared]), (label, toks, off_toks)
