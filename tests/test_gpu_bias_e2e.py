"""GPU: the projection biases end to end (load_calibs hooks -> compress_nystrom / compress_qk / compress_vo -> convert_model ->
compressed attention) on tiny random-init models whose biases are RANDOM (std 0.15: HF initialises every bias to zero, with which
none of this could fail), and the driver on a local Qwen2 checkpoint."""
import functools
import json
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
KINDS = ("opt", "qwen2", "llama")          # llama: attention_bias=True, mlp_bias=True
U_BF16 = 2.0 ** -8                         # one rounding of the model dtype per entry, as the relative bound the checks below use


def _randomise_biases(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    for mod in model.modules():
        if isinstance(mod, torch.nn.Linear) and mod.bias is not None:
            mod.bias.data.copy_(torch.randn(mod.bias.shape, generator=g) * 0.15)


def _tiny_model(kind, dev):
    """tests/test_gpu_e2e.py's tiny models at init std 0.15 (activations of O(1), so the refit's absolute ridge is negligible)."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    if kind == "opt":
        cfg = transformers.OPTConfig(hidden_size=128, ffn_dim=320, num_hidden_layers=2, num_attention_heads=4, vocab_size=211,
                                     max_position_embeddings=64, word_embed_proj_dim=128, init_std=0.15)
        m = transformers.OPTForCausalLM(cfg)
    else:
        common = dict(hidden_size=128, intermediate_size=320, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      vocab_size=211, max_position_embeddings=64, initializer_range=0.15)
        if kind == "qwen2":
            m = transformers.Qwen2ForCausalLM(transformers.Qwen2Config(**common))
        else:
            m = transformers.LlamaForCausalLM(transformers.LlamaConfig(head_dim=32, attention_bias=True, mlp_bias=True, **common))
    _randomise_biases(m)
    return m.to(dev).to(torch.bfloat16).eval()


def _ids(dev):
    return torch.randint(0, 211, (2, 48), generator=torch.Generator().manual_seed(1)).to(dev)


@functools.lru_cache(maxsize=None)
def _pipeline(kind, keep, switch):
    """One run of the three stages on a fresh tiny model with MODEGPT_KEEP_BIAS = switch ("1" / "0"); shared by the tests below and
    left unchanged by them.  Returns a dict: the original tensors (CPU clones), the reference logits, the artefacts, the masks, the
    converted model and its adapter."""
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.calibration import load_calibs
    from modegpt_amd.compression.compress_mlp import compress_nystrom
    from modegpt_amd.compression.compress_qk import compress_qk
    from modegpt_amd.compression.compress_vo import compress_vo
    from modegpt_amd.patchers import install_compressed_attention
    dev = torch.device("cuda:0")
    before = os.environ.get("MODEGPT_KEEP_BIAS")
    os.environ["MODEGPT_KEEP_BIAS"] = switch
    try:
        model = _tiny_model(kind, dev)
        ad = ModelAdapter.from_model(model, None)
        assert ad.arch == kind
        layers_dir = os.path.join(tempfile.mkdtemp(prefix="bias_e2e_"), "layers")
        ad.config = CompressionConfig(temp_storage_dir=layers_dir, nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5, dataset="synthetic",
                                      order="mlp,qk,vo")
        original = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        with torch.no_grad():
            ref = model(_ids(dev)).logits.float().cpu()
        cov_mlp, cov_q, cov_k, cov_x, _ = load_calibs(ad, n_samples=8, batch_size=4, dataset="synthetic", target_layers=[])
        keeps, layers = [keep] * ad.n_layers, list(range(ad.n_layers))
        compress_nystrom(ad, cov_mlp, keeps, layers)
        masks = compress_qk(ad, (cov_q, cov_k), keeps, target_layers=layers)
        compress_vo(ad, cov_x, keeps, target_layers=layers)
        residuals = getattr(ad, "report_vo_bias_residuals", dict)()      # (code without the reporter: the checks below fail by their numbers)
        arts = {(i, s): torch.load(os.path.join(layers_dir, f"layer_{i}_{s}"), map_location="cpu") for i in layers for s in ("mlp", "qk", "vo")}
        ad.convert_model(saved_layers_dir=layers_dir)
        install_compressed_attention(ad, masks if kind != "opt" else None)
        return dict(original=original, ref=ref, arts=arts, masks=[m.cpu() for m in masks], model=model, adapter=ad, residuals=residuals)
    finally:
        if before is None:
            os.environ.pop("MODEGPT_KEEP_BIAS", None)
        else:
            os.environ["MODEGPT_KEEP_BIAS"] = before


def _logit_error(run, dev):
    with torch.no_grad():
        got = run["model"](_ids(dev)).logits.float().cpu()
    return (got - run["ref"]).abs().max().item() / run["ref"].abs().max().item()


@pytest.mark.parametrize("kind", KINDS)
def test_keep_everything_reproduces_the_model_biases_included(dev, kind):
    """Keep ratio 1.0 with the biases carried: the logits of the original model within the bound
    test_keep_everything_reproduces_the_model holds the bias-free families to (5e-2 of the largest logit)."""
    err = _logit_error(_pipeline(kind, 1.0, "1"), dev)
    print(f"{kind}: keep 1.0, biases carried: logits differ by {err:.3e} of the largest")
    assert err < 5e-2, err


def test_opt_without_the_switch_is_another_network(dev):
    """The inputs can see a dropped bias: the same run with the switch off misses the bound by at least 4 x.  (This is the case the
    code before the switch fails: it is what a compressed OPT was.)"""
    run = _pipeline("opt", 1.0, "0")
    for art in run["arts"].values():
        assert not any(k.endswith("_bias") for k in art)
    err = _logit_error(run, dev)
    print(f"opt: keep 1.0, biases dropped: logits differ by {err:.3e} of the largest")
    assert err >= 4 * 5e-2, err


def _prefix(kind, i):
    return f"model.decoder.layers.{i}." if kind == "opt" else f"model.layers.{i}."


def _names(kind):
    if kind == "opt":
        return dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.out_proj", up="fc1", down="fc2")
    return dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.o_proj", up="mlp.up_proj",
                down="mlp.down_proj", gate="mlp.gate_proj")


def _constant(Wo, b_v, b_o, n_heads, n_kv):
    """W_o b_v + b_o in fp64 from stored tensors: what the attention module adds to every token (softmax rows sum to one), and the
    entry-wise sum of absolute terms.  b_v [n_kv r] is expanded to the query heads."""
    Wo = Wo.double()
    r = Wo.shape[1] // n_heads
    g = n_heads // n_kv
    b = torch.cat([b_v.double()[(h // g) * r:(h // g + 1) * r] for h in range(n_heads)]) if b_v is not None else torch.zeros(Wo.shape[1], dtype=torch.float64)
    c = Wo @ b + (0 if b_o is None else b_o.double())
    return c, Wo.abs() @ b.abs() + (0 if b_o is None else b_o.double().abs())


@pytest.mark.parametrize("kind", KINDS)
def test_bias_isolation_at_keep_0_6(dev, kind):
    """Zero hidden states: every token's v is b_v, so the attention module's output is the constant W_o b_v + b_o whatever the softmax
    does.  Evaluated in fp64 on the host from the stored tensors of the original and of the compressed module: OPT / Llama (the v bias
    folded into o_proj's) agree within one rounding of the model dtype per entry, 2^-8 relative for bf16; Qwen2 (no bias on o_proj:
    v_bias = P b_v) differs by the reported rho within the same rounding of the stored factors.  Then the compressed MODULE is run on
    zeros and gives its constant.  Before the switch: the constant was lost (no bias in the module at all)."""
    run = _pipeline(kind, 0.6, "1")
    ad, names = run["adapter"], _names(kind)
    n_heads, n_kv = ad.n_heads, ad.n_kv_heads
    sd = {k: v.detach().cpu() for k, v in run["model"].state_dict().items()}
    for i in range(ad.n_layers):
        p = _prefix(kind, i)
        get = lambda state, slot, what: state.get(p + names[slot] + "." + what)      # noqa: E731
        c0, _ = _constant(get(run["original"], "o", "weight"), get(run["original"], "v", "bias"), get(run["original"], "o", "bias"), n_heads, n_kv)
        assert c0.abs().max() > 0.05                                                  # (there is a constant to lose)
        v_bias, o_bias = get(sd, "v", "bias"), get(sd, "o", "bias")
        c1, a1 = _constant(get(sd, "o", "weight"), v_bias, o_bias, n_heads, n_kv)
        if kind == "qwen2":
            assert o_bias is None and v_bias is not None
            rep = run["residuals"][i]
            # (W_o' and v_bias are each rounded once, 2^-9 relative per entry: 2^-8 of the absolute terms, and their product 2^-18)
            slack = (U_BF16 * (1 + 2.0 ** -7) * a1).norm().item()
            diff = (c0 - c1).norm().item()
            print(f"{kind} layer {i}: ||c - c'|| = {diff:.6e}, reported ||rho|| = {rep['residual_norm2'] ** 0.5:.6e}, slack {slack:.3e}")
            assert abs(diff - rep["residual_norm2"] ** 0.5) <= slack
            assert abs(rep["constant_norm2"] - float(c0 @ c0)) <= 1e-12 * float(c0 @ c0)
            assert 0 < rep["residual_norm2"] < rep["constant_norm2"]
        else:
            assert v_bias is None and o_bias is not None
            worst = ((c1 - c0).abs() / c0.abs()).max().item()
            print(f"{kind} layer {i}: the folded constant differs from W_o b_v + b_o by {worst:.3e} relative, entry-wise")
            assert torch.all((c1 - c0).abs() <= U_BF16 * c0.abs())
        # the module itself, on zeros: bf16 products accumulated in fp32, the attention output and the result rounded to bf16
        block = ad.get_transformer_blocks()[i]
        x = torch.zeros(1, 3, ad.d_model, dtype=torch.bfloat16, device=dev)
        with torch.no_grad():
            if kind == "opt":
                out = block.self_attn(x, attention_mask=None)[0]
            else:
                pos = torch.arange(3, device=dev)[None]
                out = block.self_attn(x, position_embeddings=run["model"].model.rotary_emb(x, pos), attention_mask=None)[0]
        out = out.double().cpu()[0]
        tol = 3 * 2.0 ** -9 * (a1 + c1.abs())          # (three bf16 roundings: the softmax weights, the attention output, the result)
        assert torch.all((out - c1[None]).abs() <= tol[None]), ((out - c1[None]).abs() / tol[None]).max().item()


@pytest.mark.parametrize("kind", ["opt", "llama"])
def test_switch_changes_no_weight_and_no_mask(dev, kind):
    """With the switch on every weight tensor of every artefact is the same bits as with it off, and the masks are equal; with it off
    the artefacts hold exactly the keys they always held; the carried q / k / up / gate / down biases are bit copies of the original
    entries at the rows the weights were gathered from."""
    on, off = _pipeline(kind, 0.6, "1"), _pipeline(kind, 0.6, "0")
    names = _names(kind)
    weights = {"mlp": {"up", "down"} | ({"gate"} if kind != "opt" else set()), "qk": {"q_proj", "k_proj"}, "vo": {"v_proj", "o_proj"}}
    carried = {"mlp": {"up_bias", "down_bias"} | ({"gate_bias"} if kind != "opt" else set()), "qk": {"q_bias", "k_bias"}, "vo": {"o_bias"}}
    assert len(on["masks"]) == len(off["masks"]) and all(torch.equal(a, b) for a, b in zip(on["masks"], off["masks"]))
    ad = on["adapter"]
    hd, g = ad.head_dim, ad.n_heads // ad.n_kv_heads
    for (i, suffix), art in on["arts"].items():
        base = off["arts"][(i, suffix)]
        assert set(base) == weights[suffix] and set(art) == weights[suffix] | carried[suffix], (suffix, sorted(art))
        for k in base:
            assert art[k].dtype == base[k].dtype and torch.equal(art[k].view(torch.int16), base[k].view(torch.int16)), (i, suffix, k)
        p = _prefix(kind, i)
        orig = lambda slot, what: on["original"][p + names[slot] + "." + what]      # noqa: E731
        bits = lambda t: t.contiguous().view(torch.int16)                            # noqa: E731
        for k in carried[suffix]:
            assert art[k].dim() == 1 and art[k].dtype == torch.bfloat16
        if suffix == "mlp":
            W = orig("up", "weight")
            rows = [int((W == row).all(dim=1).nonzero()[0, 0]) for row in art["up"]]      # the selected columns, from the gathered rows
            assert rows == sorted(rows) and len(set(rows)) == len(rows)
            assert torch.equal(bits(art["up_bias"]), bits(orig("up", "bias")[rows]))
            if kind != "opt":
                assert torch.equal(bits(art["gate_bias"]), bits(orig("gate", "bias")[rows]))
            assert torch.equal(bits(art["down_bias"]), bits(orig("down", "bias")))
        elif suffix == "qk" and kind != "opt":
            mask = on["masks"][i]
            q_rows = torch.cat([h * hd + mask[h // g] for h in range(ad.n_heads)])
            k_rows = torch.cat([h * hd + mask[h] for h in range(ad.n_kv_heads)])
            assert torch.equal(bits(art["q_bias"]), bits(orig("q", "bias")[q_rows]))
            assert torch.equal(bits(art["k_bias"]), bits(orig("k", "bias")[k_rows]))
        elif suffix == "qk":
            W = orig("q", "weight")
            rows = [int((W == row).all(dim=1).nonzero()[0, 0]) for row in art["q_proj"]]
            assert torch.equal(bits(art["q_bias"]), bits(orig("q", "bias")[rows]))
            assert torch.equal(bits(art["k_bias"]), bits(orig("k", "bias")[rows]))       # (one column set for q and k of a head)


def test_run_modegpt_main_on_a_local_qwen2_checkpoint(dev, tmp_path, monkeypatch):
    """The driver on a random-init Qwen2 with random q / k / v biases: compresses, saves, reloads through Qwen2Rebuild, evaluates;
    metrics["vo_bias_residual"] is there; and the same run from saved statistics (MODEGPT_CALIBS_LOAD) writes the same artefacts --
    the biases come from the weights, not from the statistics."""
    transformers = pytest.importorskip("transformers")
    tokenizers = pytest.importorskip("tokenizers")
    from modegpt_amd import run_modegpt
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig

    vocab = {f"w{i}": i for i in range(208)}
    vocab.update({"<unk>": 208, "<s>": 209, "</s>": 210})
    tok = tokenizers.Tokenizer(tokenizers.models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = tokenizers.pre_tokenizers.Whitespace()
    fast = transformers.PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="<unk>", bos_token="<s>", eos_token="</s>")
    torch.manual_seed(0)
    cfg = transformers.Qwen2Config(hidden_size=128, intermediate_size=320, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, vocab_size=211, max_position_embeddings=64, initializer_range=0.15)
    model = transformers.Qwen2ForCausalLM(cfg)
    _randomise_biases(model)
    src = tmp_path / "src_model"
    model.to(torch.bfloat16).save_pretrained(src)
    fast.save_pretrained(src)
    monkeypatch.chdir(tmp_path)   # logs/, metrics/, .mem-usage land in the temp dir
    monkeypatch.delenv("MODEGPT_KEEP_BIAS", raising=False)       # Qwen2 carries its biases whatever the switch says
    stats = str(tmp_path / "stats")
    seen = {}
    real = run_modegpt.save_compressed_model

    def spy(adapter, **kw):
        seen["metrics"] = json.loads(json.dumps(adapter.metrics.get("vo_bias_residual")))
        return real(adapter, **kw)

    monkeypatch.setattr(run_modegpt, "save_compressed_model", spy)

    def run(name, env):
        for var in ("MODEGPT_CALIBS_SAVE", "MODEGPT_CALIBS_LOAD"):
            monkeypatch.delenv(var, raising=False)
        monkeypatch.setenv(env, stats)
        out = tmp_path / name
        conf = CompressionConfig(model=str(src), output_dir=str(out), temp_storage_dir=str(out / "layers"), dataset="synthetic",
                                 order="mlp,qk,vo", calib_size=8, calibs_batch_size=4, compression_ratio=0.3, nystrom_ridge=1e-4,
                                 ridge_qk=1e-2, ridge_vo=1e-5, note="pytest")
        ppl = run_modegpt.main(config=conf)
        assert ppl is not None and ppl > 1.0 and ppl == ppl and ppl != float("inf")
        return out

    out = run("out_save", "MODEGPT_CALIBS_SAVE")
    names = set(os.listdir(out / "model"))
    assert {"Qwen2Rebuild.py", "compressed_attention.py", "rotary_masks.pt", "config.json"} <= names
    c = json.load(open(out / "model" / "config.json"))
    assert c["auto_map"]["AutoModelForCausalLM"] == "Qwen2Rebuild.Qwen2ForCausalLM" and c["projection_biases"] == ["q", "k", "v"]
    rep = seen["metrics"]
    assert rep is not None and sorted(rep) == ["0", "1"]
    for layer in rep.values():
        assert 0 <= layer["residual_norm2"] <= layer["constant_norm2"] and layer["constant_norm2"] > 0
    first = {(i, s): torch.load(out / "layers" / f"layer_{i}_{s}", map_location="cpu") for i in range(2) for s in ("mlp", "qk", "vo")}
    assert set(first[(0, "qk")]) == {"q_proj", "k_proj", "q_bias", "k_bias"} and set(first[(0, "vo")]) == {"v_proj", "o_proj", "v_bias"}
    assert set(first[(0, "mlp")]) == {"up", "gate", "down"}
    again = run("out_load", "MODEGPT_CALIBS_LOAD")
    for key, art in first.items():
        other = torch.load(again / "layers" / f"layer_{key[0]}_{key[1]}", map_location="cpu")
        assert set(other) == set(art)
        for k in art:
            assert torch.equal(art[k].view(torch.int16), other[k].view(torch.int16)), (key, k)
