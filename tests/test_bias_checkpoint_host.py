"""CPU: a checkpoint whose projections carry biases (MODEGPT_KEEP_BIAS=1, Qwen2) round-trips through the modeling file shipped
with it -- strict load, logits of the live model bit for bit, in a process that cannot import the engine -- and an OPT checkpoint
written that way still loads into the reference's OPTRebuild modules."""
import json
import os
import subprocess
import sys

import pytest
import torch

KINDS = ("opt", "llama", "qwen2")
REFERENCE_OPT = "/root/reference/src/patchers/OPTRebuild.py"
# which projections carry a bias after compression: OPT's v bias is folded into out_proj's, Llama's (attention_bias, mlp_bias) too,
# Qwen2 keeps q / k and the projected v bias (o_proj has none to fold into)
CARRIED = {"opt": ["up", "down", "q", "k", "o"], "llama": ["up", "gate", "down", "q", "k", "o"], "qwen2": ["q", "k", "v"]}
REBUILD = {"opt": ("OPTRebuild.py", "OPTForCausalLM"), "llama": ("LlamaRebuild.py", "LlamaForCausalLM"),
           "qwen2": ("Qwen2Rebuild.py", "Qwen2ForCausalLM")}


def _model(kind, scratch):
    """A random-init bf16 model the way a run gets it: saved and loaded from disk (a model cast with .to(bfloat16) would carry a
    bf16-rounded rotary frequency table, which no loaded checkpoint has)."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    if kind == "opt":
        cfg = transformers.OPTConfig(hidden_size=64, ffn_dim=160, num_hidden_layers=2, num_attention_heads=4, vocab_size=97,
                                     max_position_embeddings=32, word_embed_proj_dim=64)
        model = transformers.OPTForCausalLM(cfg)
    else:
        common = dict(hidden_size=64, intermediate_size=160, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      head_dim=16, vocab_size=97, max_position_embeddings=32)
        if kind == "qwen2":
            model = transformers.Qwen2ForCausalLM(transformers.Qwen2Config(**common))
        else:
            model = transformers.LlamaForCausalLM(transformers.LlamaConfig(attention_bias=True, mlp_bias=True, **common))
    src = os.path.join(str(scratch), "source_" + kind)
    model.to(torch.bfloat16).save_pretrained(src)
    return transformers.AutoModelForCausalLM.from_pretrained(src, dtype=torch.bfloat16).eval()


def _compressed_stand_in(kind, scratch):
    """A live 'compressed' model without a GPU: per-layer shapes that differ between the layers, random bf16 weights, and RANDOM biases
    (std 0.15: HF initialises biases to zero, which would make every check here vacuous) exactly on the projections a bias-carrying
    run leaves them on.  Returns (adapter, masks)."""
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.patchers import install_compressed_attention
    model = _model(kind, scratch)
    ad = ModelAdapter.from_model(model, None)
    assert ad.arch == kind
    g = torch.Generator().manual_seed(23)
    n_h, n_kv, hd, d = ad.n_heads, ad.n_kv_heads, ad.head_dim, ad.d_model
    has = set(CARRIED[kind])

    def lin(rows, cols, slot):
        m = torch.nn.Linear(cols, rows, bias=slot in has, dtype=torch.bfloat16)
        m.weight.data.copy_((torch.randn(rows, cols, generator=g) * cols ** -0.5).to(torch.bfloat16))
        if slot in has:
            m.bias.data.copy_((torch.randn(rows, generator=g) * 0.15).to(torch.bfloat16))
        return m

    masks = []
    for i in range(ad.n_layers):
        r_qk, r_mlp = 8 + 2 * i, 100 + 7 * i
        r_vo = 9 + i if kind == "opt" else r_qk
        ad.replace_attn_layers(i, lin(n_h * r_qk, d, "q"), lin(n_kv * r_qk, d, "k"), lin(n_kv * r_vo, d, "v"), lin(d, n_h * r_vo, "o"))
        ad.replace_mlp_layers(i, lin(r_mlp, d, "up"), lin(d, r_mlp, "down"), None if kind == "opt" else lin(r_mlp, d, "gate"))
        idx = torch.stack([torch.randperm(hd // 2, generator=g)[:r_qk // 2] for _ in range(n_kv)])
        masks.append(torch.cat((idx, idx + hd // 2), dim=1))
    masks = None if kind == "opt" else masks
    install_compressed_attention(ad, masks)
    return ad, masks


def _save(ad, masks, out):
    from modegpt_amd.model_utils import save_compressed_model
    ad.patch_config()
    save_compressed_model(ad, rotary_masks=masks, save_dir=out, source_model_name="none")


@pytest.mark.parametrize("kind", KINDS)
def test_biased_checkpoint_round_trips_through_the_shipped_modeling_file(kind, tmp_path):
    ad, masks = _compressed_stand_in(kind, tmp_path)
    model = ad.model
    model.config._attn_implementation = "eager"
    ids = torch.randint(0, 97, (2, 12), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = model(ids).logits.float()
    out = str(tmp_path / "model")
    _save(ad, masks, out)
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert cfg["projection_biases"] == CARRIED[kind]
    fname, cls = REBUILD[kind]
    assert cfg["auto_map"]["AutoModelForCausalLM"] == f"{fname[:-3]}.{cls}"
    assert os.path.exists(os.path.join(out, fname)) and os.path.exists(os.path.join(out, "compressed_attention.py"))
    torch.save({"ids": ids, "state": {k: v.clone() for k, v in model.state_dict().items()}}, str(tmp_path / "live.pt"))
    script = f'''
import importlib.util, json, torch, transformers
assert importlib.util.find_spec("modegpt_amd") is None, "the engine must NOT be importable here"
m, info = transformers.AutoModelForCausalLM.from_pretrained({out!r}, trust_remote_code=True, dtype=torch.bfloat16, output_loading_info=True)
m = m.eval()
assert type(m).__module__.endswith({fname[:-3]!r}), type(m).__module__
bad = {{k: sorted(v) for k, v in info.items() if k in ("missing_keys", "unexpected_keys", "mismatched_keys") and len(v)}}
assert not bad, bad                                         # strict: the modules hold exactly the parameters the state dict does
live = torch.load({str(tmp_path / "live.pt")!r})
got = m.state_dict()
assert set(got) == set(live["state"]), sorted(set(got) ^ set(live["state"]))
for k, v in live["state"].items():
    assert got[k].shape == v.shape and got[k].dtype == v.dtype and torch.equal(got[k], v), k
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
    # ... and the inputs can see a dropped bias: the same modules with their biases zeroed give other logits
    for mod in model.modules():
        if isinstance(mod, torch.nn.Linear) and mod.bias is not None:
            mod.bias.data.zero_()
    with torch.no_grad():
        dropped = model(ids).logits.float()
    assert float((dropped - want).abs().max()) > 5e-2 * float(want.abs().max())


@pytest.mark.parametrize("kind", ["opt", "llama"])
def test_checkpoint_without_the_field_loads_bias_free_as_before(kind, tmp_path):
    """No carried bias -> no config.projection_biases, and the modeling file builds bias-free projections (the behaviour before the
    switch existed: tests/test_host.py covers it in full; here only that the field is absent and the load is strict)."""
    transformers = pytest.importorskip("transformers")
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    model = _model(kind, tmp_path)
    ad = ModelAdapter.from_model(model, None)
    mk = lambda rows, cols: torch.nn.Linear(cols, rows, bias=False, dtype=torch.bfloat16)      # noqa: E731
    for i in range(ad.n_layers):
        ad.replace_attn_layers(i, mk(32, 64), mk(32 if kind == "opt" else 16, 64), mk(32 if kind == "opt" else 16, 64), mk(64, 32))
        ad.replace_mlp_layers(i, mk(100, 64), mk(64, 100), None if kind == "opt" else mk(100, 64))
    masks = None if kind == "opt" else [torch.arange(8)[None].repeat(2, 1) for _ in range(2)]
    out = str(tmp_path / "model")
    _save(ad, masks, out)
    assert "projection_biases" not in json.load(open(os.path.join(out, "config.json")))
    loaded, info = transformers.AutoModelForCausalLM.from_pretrained(out, trust_remote_code=True, dtype=torch.bfloat16,
                                                                     output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"], info
    assert set(loaded.state_dict()) == set(model.state_dict())


def test_biased_opt_checkpoint_loads_into_the_reference_modules(tmp_path):
    """Where the reference checkout is present: its OPTRebuild.OPTModel, constructed from OUR config (it creates every bias from
    config.enable_bias), takes every tensor of a bias-carrying OPT checkpoint; the one key it misses per layer is v_proj.bias, which
    it zero-fills (the v bias sits in out_proj.bias); driven module by module (its OPTForCausalLM does not construct under
    transformers 5) it gives the live model's logits."""
    if not os.path.exists(REFERENCE_OPT):
        pytest.skip("reference checkout not present")
    import importlib.util
    from safetensors.torch import load_file
    from tests.golden_util import opt_drive
    ad, masks = _compressed_stand_in("opt", tmp_path)
    model = ad.model
    model.config._attn_implementation = "eager"
    ids = torch.randint(0, 97, (2, 12), generator=torch.Generator().manual_seed(6))
    want = opt_drive(model, ids)
    out = str(tmp_path / "model")
    _save(ad, masks, out)
    spec = importlib.util.spec_from_file_location("reference_opt_rebuild", REFERENCE_OPT)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod          # (transformers inspects the file a model class comes from)
    spec.loader.exec_module(mod)
    import transformers
    rconf = transformers.OPTConfig.from_pretrained(out)
    assert rconf.enable_bias
    ref = mod.OPTModel(rconf).to(torch.bfloat16).eval()
    sd = {}
    for f in os.listdir(out):
        if f.endswith(".safetensors"):
            sd.update(load_file(os.path.join(out, f)))
        elif f.endswith(".bin"):
            sd.update(torch.load(os.path.join(out, f), map_location="cpu"))
    sub = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    res = ref.load_state_dict(sub, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert sorted(res.missing_keys) == [f"decoder.layers.{i}.self_attn.v_proj.bias" for i in range(rconf.num_hidden_layers)]
    own = dict(ref.named_parameters())
    for k in res.missing_keys:
        own[k].data.zero_()              # (what the reference's own from_pretrained does with a missing bias: _init_weights)
    rs = ref.state_dict()
    for k, v in sub.items():
        assert rs[k].shape == v.shape and torch.equal(rs[k], v), k
    ref.config._attn_implementation = "eager"

    class _Wrap:                          # opt_drive reads model.model.decoder and model.lm_head (tied to the embedding)
        model = ref
        lm_head = staticmethod(lambda h: torch.nn.functional.linear(h, ref.decoder.embed_tokens.weight))

    got = opt_drive(_Wrap, ids)
    assert torch.equal(got, want), float((got - want).abs().max())
