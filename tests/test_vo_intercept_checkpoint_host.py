"""CPU: what MODEGPT_VO_INTERCEPT=1 leaves behind, without a GPU.
  * a checkpoint whose o_proj carries the truncation's intercept and whose v_proj carries no bias (config.projection_biases has "o"
    and not "v") round-trips through the modeling file shipped with it -- strict load through shrink_to_config_ranks, the live
    model's logits bit for bit -- for Llama, Qwen3, Qwen2 (whose stock v_proj HAS a bias, which must go) and OPT; the biases are
    random, since a zero bias could be dropped without anybody noticing;
  * convert_model's rules: a vo artefact without o_bias gets an exact zero one, one with a v_bias is refused;
  * the x_mean file of the saved statistics: format, refusals, and "switch off -> the record is what it always was";
  * a sharded run's record carries o_bias (sharding.pack_layer)."""
import json
import os

import numpy as np
import pytest
import torch

KINDS = ("llama", "qwen3", "qwen2", "opt")
CARRIED = {"llama": ["o"], "qwen3": ["o"], "qwen2": ["q", "k", "o"], "opt": ["o"]}
REBUILD = {"llama": "LlamaRebuild.LlamaForCausalLM", "qwen3": "DenseQwenRebuild.Qwen3ForCausalLM", "qwen2": "Qwen2Rebuild.Qwen2ForCausalLM",
           "opt": "OPTRebuild.OPTForCausalLM"}


def _model(kind, scratch):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    if kind == "opt":
        model = transformers.OPTForCausalLM(transformers.OPTConfig(hidden_size=64, ffn_dim=160, num_hidden_layers=2, num_attention_heads=4,
                                                                   vocab_size=97, max_position_embeddings=32, word_embed_proj_dim=64))
    else:
        common = dict(hidden_size=64, intermediate_size=160, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      head_dim=16, vocab_size=97, max_position_embeddings=32)
        cls, cfg = {"llama": (transformers.LlamaForCausalLM, transformers.LlamaConfig), "qwen3": (transformers.Qwen3ForCausalLM, transformers.Qwen3Config),
                    "qwen2": (transformers.Qwen2ForCausalLM, transformers.Qwen2Config)}[kind]
        model = cls(cfg(**common))
    src = os.path.join(str(scratch), "source_" + kind)
    model.to(torch.bfloat16).save_pretrained(src)
    return transformers.AutoModelForCausalLM.from_pretrained(src, dtype=torch.bfloat16).eval()


def _stand_in(kind, scratch):
    """A live 'compressed' model: per-layer shapes that differ between the layers, random bf16 weights, random biases exactly where a
    run with the switch leaves them -- layer 1's o bias an exact zero, what convert_model gives a layer that was not truncated."""
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.patchers import install_compressed_attention
    model = _model(kind, scratch)
    ad = ModelAdapter.from_model(model, None)
    g = torch.Generator().manual_seed(31)
    n_h, n_kv, hd, d = ad.n_heads, ad.n_kv_heads, ad.head_dim, ad.d_model
    has = set(CARRIED[kind])

    def lin(rows, cols, slot, scale=0.3):
        m = torch.nn.Linear(cols, rows, bias=slot in has, dtype=torch.bfloat16)
        m.weight.data.copy_((torch.randn(rows, cols, generator=g) * cols ** -0.5).to(torch.bfloat16))
        if slot in has:
            m.bias.data.copy_((torch.randn(rows, generator=g) * scale).to(torch.bfloat16))
        return m

    masks = []
    for i in range(ad.n_layers):
        r_qk, r_mlp = 8 + 2 * i, 100 + 7 * i
        r_vo = 9 + i if kind == "opt" else r_qk
        ad.replace_attn_layers(i, lin(n_h * r_qk, d, "q"), lin(n_kv * r_qk, d, "k"), lin(n_kv * r_vo, d, "v"),
                               lin(d, n_h * r_vo, "o", scale=0.3 if i == 0 else 0.0))
        ad.replace_mlp_layers(i, lin(r_mlp, d, "up"), lin(d, r_mlp, "down"), None if kind == "opt" else lin(r_mlp, d, "gate"))
        idx = torch.stack([torch.randperm(hd // 2, generator=g)[:r_qk // 2] for _ in range(n_kv)])
        masks.append(torch.cat((idx, idx + hd // 2), dim=1))
    masks = None if kind == "opt" else masks
    install_compressed_attention(ad, masks)
    return ad, masks


@pytest.mark.parametrize("kind", KINDS)
def test_o_bias_without_v_bias_round_trips_through_the_shipped_modeling_file(kind, tmp_path, monkeypatch):
    transformers = pytest.importorskip("transformers")
    from modegpt_amd.model_utils import save_compressed_model
    monkeypatch.setenv("HF_MODULES_CACHE", str(tmp_path / "hf_modules"))
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
    assert cfg["projection_biases"] == CARRIED[kind] and "v" not in cfg["projection_biases"]
    assert cfg["auto_map"]["AutoModelForCausalLM"] == REBUILD[kind]
    loaded, info = transformers.AutoModelForCausalLM.from_pretrained(out, trust_remote_code=True, dtype=torch.bfloat16, output_loading_info=True)
    bad = {k: sorted(v) for k, v in info.items() if k in ("missing_keys", "unexpected_keys", "mismatched_keys") and len(v)}
    assert not bad, bad                                         # strict: the modules hold exactly the parameters the state dict does
    loaded = loaded.eval()
    assert type(loaded).__module__.endswith(REBUILD[kind].split(".")[0])
    got, live = loaded.state_dict(), model.state_dict()
    assert set(got) == set(live), sorted(set(got) ^ set(live))
    for k, v in live.items():
        assert got[k].shape == v.shape and got[k].dtype == v.dtype and torch.equal(got[k], v), k
    o_name = "out_proj" if kind == "opt" else "o_proj"
    assert sum(k.endswith(o_name + ".bias") for k in got) == 2 and not any(k.endswith("v_proj.bias") for k in got)
    assert not bool([v for k, v in got.items() if k.endswith(o_name + ".bias")][1].any())       # layer 1: the exact zero
    loaded.config._attn_implementation = "eager"
    with torch.no_grad():
        logits = loaded(ids).logits.float()
    assert torch.equal(logits, want), float((logits - want).abs().max())
    # the inputs can see the bias: with the o biases zeroed the logits are others
    for name, mod in model.named_modules():
        if name.endswith(o_name):
            mod.bias.data.zero_()
    with torch.no_grad():
        dropped = model(ids).logits.float()
    assert float((dropped - want).abs().max()) > 1e-2 * float(want.abs().max())


def test_convert_model_zero_bias_rule_and_v_bias_refusal(tmp_path, monkeypatch):
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    g = torch.Generator().manual_seed(2)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(torch.bfloat16)      # noqa: E731
    for switch, expect in (("1", ["o"]), (None, [])):
        if switch is None:
            monkeypatch.delenv("MODEGPT_VO_INTERCEPT", raising=False)
        else:
            monkeypatch.setenv("MODEGPT_VO_INTERCEPT", switch)
        ad = ModelAdapter.from_model(_model("llama", tmp_path), None)
        layers = tmp_path / f"layers_{switch}"
        layers.mkdir()
        for i in range(ad.n_layers):
            art = {"v_proj": rnd(2 * 10, 64), "o_proj": rnd(64, 4 * 10)}
            if i == 0 and switch:
                art["o_bias"] = rnd(64)
            torch.save(art, str(layers / f"layer_{i}_vo"))
        ad.convert_model(saved_layers_dir=str(layers), suffixes=("vo",), device="cpu")
        assert [n for n in ad.projection_biases() if n in ("v", "o")] == expect
        b0, b1 = (ad.get_attn_components(i).o_proj.bias for i in (0, 1))
        if switch is None:
            assert b0 is None and b1 is None
        else:
            assert torch.equal(b0, torch.load(str(layers / "layer_0_vo"))["o_bias"])
            assert b1.dtype == torch.bfloat16 and b1.shape == (64,) and not bool(b1.any())
    # an artefact written without the switch by a bias-carrying run (Qwen2: the projected v bias) cannot stand beside the intercept
    monkeypatch.setenv("MODEGPT_VO_INTERCEPT", "1")
    ad = ModelAdapter.from_model(_model("llama", tmp_path), None)
    layers = tmp_path / "layers_v_bias"
    layers.mkdir()
    for i in range(ad.n_layers):
        torch.save({"v_proj": rnd(20, 64), "o_proj": rnd(64, 40), "v_bias": rnd(20)}, str(layers / f"layer_{i}_vo"))
    with pytest.raises(RuntimeError, match=r"MODEGPT_VO_INTERCEPT=1 but the vo artefact of layer 0 carries a v_bias"):
        ad.convert_model(saved_layers_dir=str(layers), suffixes=("vo",), device="cpu")
    monkeypatch.delenv("MODEGPT_VO_INTERCEPT")
    ad.convert_model(saved_layers_dir=str(layers), suffixes=("vo",), device="cpu")       # ... and is what it was without the switch
    assert ad.get_attn_components(0).v_proj.bias is not None and ad.get_attn_components(0).o_proj.bias is None


def test_x_mean_file_format_and_refusals(tmp_path):
    from modegpt_amd import calib_cache as CC
    d = str(tmp_path)
    rng = np.random.default_rng(4)
    mu = rng.standard_normal(64) + 3.0
    entry = CC.write_mean_file(d, 3, mu, 64, kind=CC.X_MEAN_KIND)
    assert entry == {"file": "layer_3_x_mean.f64", "layout": "vector", "n": 64, "bytes": 512, "sum_bits": CC.sum_bits(mu)}
    assert np.array_equal(np.fromfile(os.path.join(d, "layer_3_x_mean.f64"), "<f8"), mu)
    assert not os.path.exists(os.path.join(d, "layer_3_mlp_mean.f64"))                  # (the MLP mean is another file, another switch)
    meta = {"files": {CC.X_MEAN_KIND: entry}}
    assert CC.validate_extra_entry(meta, {"d_model": 64}, 3, CC.X_MEAN_KIND) == entry
    assert np.array_equal(CC.read_mean_file(d, 3, entry, kind=CC.X_MEAN_KIND), mu)
    with pytest.raises(ValueError, match=r"layer 3: field files\.x_mean is missing -- the record was saved without MODEGPT_VO_INTERCEPT=1"):
        CC.validate_extra_entry({"files": {CC.MEAN_KIND: entry}}, {"d_model": 64}, 3, CC.X_MEAN_KIND)
    with pytest.raises(ValueError, match=r"files\.mlp_mean is missing -- the record was saved without MODEGPT_MLP_INTERCEPT=1"):
        CC.validate_extra_entry(meta, {"n_inner": 64}, 3, CC.MEAN_KIND)                                       # (the MLP switch's message is what it was)
    with pytest.raises(ValueError, match=r"files\.x_mean\.n"):
        CC.validate_extra_entry(meta, {"d_model": 65}, 3, CC.X_MEAN_KIND)
    with pytest.raises(ValueError, match=r"files\.x_mean\.sum_bits"):
        CC.validate_extra_entry({"files": {CC.X_MEAN_KIND: dict(entry, sum_bits="7")}}, {"d_model": 64}, 3, CC.X_MEAN_KIND)
    with pytest.raises(ValueError, match="64 entries"):
        CC.write_mean_file(d, 3, mu, 65, kind=CC.X_MEAN_KIND)
    # a flipped bit in the file: the exact sum no longer matches
    path = os.path.join(d, entry["file"])
    raw = bytearray(open(path, "rb").read())
    raw[9] ^= 1
    open(path, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match=r"files\.x_mean\.sum_bits"):
        CC.read_mean_file(d, 3, entry, kind=CC.X_MEAN_KIND)
    open(path, "wb").write(bytes(raw[:-8]))
    with pytest.raises(ValueError, match=r"files\.x_mean\.bytes"):
        CC.read_mean_file(d, 3, entry, kind=CC.X_MEAN_KIND)
    os.remove(path)
    with pytest.raises(FileNotFoundError, match=r"files\.x_mean\.file"):
        CC.read_mean_file(d, 3, entry, kind=CC.X_MEAN_KIND)


def test_switch_off_allocates_no_sums_and_the_switches_are_independent(monkeypatch):
    from modegpt_amd import ops, reports
    assert ops.vo_intercept_enabled is reports.vo_intercept_enabled
    monkeypatch.delenv("MODEGPT_VO_INTERCEPT", raising=False)
    monkeypatch.setenv("MODEGPT_MLP_INTERCEPT", "1")
    assert not ops.vo_intercept_enabled() and ops.mlp_intercept_enabled()
    monkeypatch.setenv("MODEGPT_VO_INTERCEPT", "on")
    monkeypatch.delenv("MODEGPT_MLP_INTERCEPT")
    assert ops.vo_intercept_enabled() and not ops.mlp_intercept_enabled()


def test_sharded_record_carries_the_o_bias():
    from modegpt_amd import sharding
    g = torch.Generator().manual_seed(8)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(torch.bfloat16)      # noqa: E731
    tensors = {"v_proj": rnd(20, 64), "o_proj": rnd(64, 40), "o_bias": rnd(64)}
    layer, out, mask = sharding.unpack_layer(sharding.pack_layer(5, tensors, None))
    assert layer == 5 and mask is None and set(out) == set(tensors)
    for k, v in tensors.items():
        assert out[k].dtype == v.dtype and torch.equal(out[k], v), k
