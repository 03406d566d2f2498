"""CPU: a checkpoint whose only carried bias is the MLP refit's intercept (MODEGPT_MLP_INTERCEPT=1: config.projection_biases ==
["down"]) round-trips through the modeling file shipped with it -- strict load, logits of the live model bit for bit, in a process
that cannot import the engine.  Llama and Qwen3 here (tests/test_bias_checkpoint_host.py covers the families whose own biases are
carried); the biases are random, since a zero bias could be dropped without anybody noticing."""
import json
import os
import subprocess
import sys

import pytest
import torch

REBUILD = {"llama": ("LlamaRebuild.py", "LlamaForCausalLM"), "qwen3": ("DenseQwenRebuild.py", "Qwen3ForCausalLM")}


def _model(kind, scratch):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    common = dict(hidden_size=64, intermediate_size=160, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                  head_dim=16, vocab_size=97, max_position_embeddings=32)
    if kind == "qwen3":
        model = transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**common))
    else:
        model = transformers.LlamaForCausalLM(transformers.LlamaConfig(**common))
    src = os.path.join(str(scratch), "source_" + kind)
    model.to(torch.bfloat16).save_pretrained(src)
    return transformers.AutoModelForCausalLM.from_pretrained(src, dtype=torch.bfloat16).eval()


def _stand_in(kind, scratch):
    """A live 'compressed' model without a GPU: per-layer shapes that differ between the layers, random bf16 weights, and a random
    bias on down_proj alone -- layer 1's an exact zero, what convert_model gives a layer that was not refitted."""
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.patchers import install_compressed_attention
    model = _model(kind, scratch)
    ad = ModelAdapter.from_model(model, None)
    g = torch.Generator().manual_seed(29)
    n_h, n_kv, hd, d = ad.n_heads, ad.n_kv_heads, ad.head_dim, ad.d_model

    def lin(rows, cols, bias=None):
        m = torch.nn.Linear(cols, rows, bias=bias is not None, dtype=torch.bfloat16)
        m.weight.data.copy_((torch.randn(rows, cols, generator=g) * cols ** -0.5).to(torch.bfloat16))
        if bias is not None:
            m.bias.data.copy_((torch.randn(rows, generator=g) * bias).to(torch.bfloat16))
        return m

    masks = []
    for i in range(ad.n_layers):
        r_qk, r_mlp = 8 + 2 * i, 100 + 7 * i
        ad.replace_attn_layers(i, lin(n_h * r_qk, d), lin(n_kv * r_qk, d), lin(n_kv * r_qk, d), lin(d, n_h * r_qk))
        ad.replace_mlp_layers(i, lin(r_mlp, d), lin(d, r_mlp, bias=0.3 if i == 0 else 0.0), lin(r_mlp, d))
        idx = torch.stack([torch.randperm(hd // 2, generator=g)[:r_qk // 2] for _ in range(n_kv)])
        masks.append(torch.cat((idx, idx + hd // 2), dim=1))
    install_compressed_attention(ad, masks)
    return ad, masks


@pytest.mark.parametrize("kind", sorted(REBUILD))
def test_down_bias_alone_round_trips_through_the_shipped_modeling_file(kind, tmp_path):
    from modegpt_amd.model_utils import save_compressed_model
    ad, masks = _stand_in(kind, tmp_path)
    model = ad.model
    model.config._attn_implementation = "eager"
    ids = torch.randint(0, 97, (2, 12), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = model(ids).logits.float()
    out = str(tmp_path / "model")
    ad.patch_config()
    save_compressed_model(ad, rotary_masks=masks, save_dir=out, source_model_name="none")
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert cfg["projection_biases"] == ["down"]
    fname, cls = REBUILD[kind]
    assert cfg["auto_map"]["AutoModelForCausalLM"] == f"{fname[:-3]}.{cls}"
    torch.save({"ids": ids, "state": {k: v.clone() for k, v in model.state_dict().items()}}, str(tmp_path / "live.pt"))
    script = f'''
import importlib.util, torch, transformers
assert importlib.util.find_spec("modegpt_amd") is None, "the engine must NOT be importable here"
m, info = transformers.AutoModelForCausalLM.from_pretrained({out!r}, trust_remote_code=True, dtype=torch.bfloat16, output_loading_info=True)
m = m.eval()
assert type(m).__module__.endswith({fname[:-3]!r}), type(m).__module__
bad = {{k: sorted(v) for k, v in info.items() if k in ("missing_keys", "unexpected_keys", "mismatched_keys") and len(v)}}
assert not bad, bad
live = torch.load({str(tmp_path / "live.pt")!r})
got = m.state_dict()
assert set(got) == set(live["state"]), sorted(set(got) ^ set(live["state"]))
assert sum(k.endswith("down_proj.bias") for k in got) == 2 and not any(k.endswith("up_proj.bias") or k.endswith("q_proj.bias") for k in got)
for k, v in live["state"].items():
    assert got[k].shape == v.shape and got[k].dtype == v.dtype and torch.equal(got[k], v), k
assert not bool(got["model.layers.1.mlp.down_proj.bias"].any())
m.config._attn_implementation = "eager"
with torch.no_grad():
    logits = m(live["ids"]).logits.float()
torch.save(logits, {str(tmp_path / "logits.pt")!r})
'''
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["HF_MODULES_CACHE"] = str(tmp_path / "hf_modules")
    p = subprocess.run([sys.executable, "-c", script], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    got = torch.load(str(tmp_path / "logits.pt"))
    assert torch.equal(got, want), float((got - want).abs().max())
    # the inputs can see the bias: with it zeroed the logits are others
    for mod in model.modules():
        if isinstance(mod, torch.nn.Linear) and mod.bias is not None:
            mod.bias.data.zero_()
    with torch.no_grad():
        dropped = model(ids).logits.float()
    assert float((dropped - want).abs().max()) > 1e-2 * float(want.abs().max())


def test_convert_model_gives_an_unrefitted_layer_an_exact_zero_bias(tmp_path, monkeypatch):
    """With the switch on, an MLP artefact without down_bias (a layer outside the target layers, or written without the switch)
    becomes a down_proj with an exact zero bias, so that projection_biases() is uniform; with the switch off it stays bias-free."""
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    g = torch.Generator().manual_seed(2)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(torch.bfloat16)      # noqa: E731
    for switch, expect in (("1", ["down"]), (None, [])):
        if switch is None:
            monkeypatch.delenv("MODEGPT_MLP_INTERCEPT", raising=False)
        else:
            monkeypatch.setenv("MODEGPT_MLP_INTERCEPT", switch)
        ad = ModelAdapter.from_model(_model("llama", tmp_path), None)
        layers = tmp_path / f"layers_{switch}"
        layers.mkdir()
        for i in range(ad.n_layers):
            art = {"up": rnd(100, 64), "gate": rnd(100, 64), "down": rnd(64, 100)}
            if i == 0 and switch:
                art["down_bias"] = rnd(64)
            torch.save(art, str(layers / f"layer_{i}_mlp"))
        ad.convert_model(saved_layers_dir=str(layers), suffixes=("mlp",), device="cpu")
        assert [n for n in ad.projection_biases() if n == "down"] == expect
        b1 = ad.get_mlp_components(1).down_proj.bias
        assert (b1 is None) if switch is None else (b1.dtype == torch.bfloat16 and not bool(b1.any()))
