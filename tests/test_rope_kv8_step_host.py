"""CPU: mdg_rope_kv8_step / mdg_rope_kv8_paged_step refuse bad shapes with a message before any device work and take an empty call,
and MODEGPT_FUSED_KV_STEP=1 leaves a cache without a `step` method on the two rope_gather calls + update."""
import pytest
import torch

from modegpt_amd import _lib
from tests.test_attn_fwd_host import _tiny

P = 0x100000                                              # never dereferenced: every call below returns before any device work


def call(lib, paged, T=1, r_qk=6, k_pitch=16, page=64):
    head = (P, 12, 2 * P, 12, 3 * P, 6, 3, 6, _lib.MDG_BF16, 2, T, 2, 2, r_qk, 3, 16, 4 * P, 5 * P, 0, 6 * P, None, None, 1e-6, 7 * P, None,
            8 * P, 9 * P, 10 * P, 11 * P)
    if paged:
        return lib.mdg_rope_kv8_paged_step(*head, 4, page, k_pitch, 16, 12 * P, 2, 13 * P, None)
    return lib.mdg_rope_kv8_step(*head, 8, k_pitch, 16, 0, None)


@pytest.mark.parametrize("paged", [False, True], ids=["planes", "paged"])
def test_bad_shapes_are_refused_with_a_message_and_an_empty_call_is_ok(paged):
    lib = _lib.load()
    name = "mdg_rope_kv8_paged_step" if paged else "mdg_rope_kv8_step"
    bad = [(dict(r_qk=5), "r_qk=5 must be even"), (dict(k_pitch=0), "pitch=0 must be a multiple of 16 and >= mdg_kv8_pitch(6) = 16")]
    if paged:
        bad.append((dict(page=96), "page=96 must be a positive multiple of 64"))
    for kw, text in bad:
        assert call(lib, paged, **kw) == _lib.MDG_ERR_BAD_ARG, kw
        assert lib.mdg_last_error().decode().startswith(name + ": ") and text in lib.mdg_last_error().decode(), lib.mdg_last_error()
    assert call(lib, paged, T=0) == _lib.MDG_OK


def test_switch_with_a_cache_that_has_no_step_takes_the_old_path(monkeypatch):
    from transformers.cache_utils import DynamicCache
    model, ca = _tiny("llama")
    ids = torch.arange(12).reshape(2, 6) % 64
    monkeypatch.delenv("MODEGPT_REQUIRE_HIP", raising=False)
    monkeypatch.delenv("MODEGPT_FUSED_KV_STEP", raising=False)
    with torch.no_grad():
        off = model(ids, past_key_values=DynamicCache(config=model.config), use_cache=True).logits
    monkeypatch.setenv("MODEGPT_FUSED_KV_STEP", "1")
    before = dict(ca.PATH_CALLS)
    with torch.no_grad():
        on = model(ids, past_key_values=DynamicCache(config=model.config), use_cache=True).logits
    assert ca.KV_STEPS == {"fused": 0}
    assert ca.PATH_CALLS["torch"] == before["torch"] + 4           # q and k of both layers: the two rope_gather calls
    assert torch.equal(on.view(torch.int16), off.view(torch.int16))
