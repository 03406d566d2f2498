"""GPU: MODEGPT_VO_INTERCEPT=1 end to end on tiny Llama (GQA 4/2 and MHA 4/4), Qwen2 (a v bias, no o bias) and OPT: the hooks' column
sums of x -> calibration's means -> compress_vo's centred truncation and intercept -> convert_model -> the checkpoint and its modeling
file; the saved statistics; MODEGPT_VO_ERROR=1 on the centred statistic; both intercept switches together.

The models are tests/test_gpu_intercept_e2e.py's (max_position_embeddings = 2048, so every calibration text has the 2048 tokens the
statistics' normaliser assumes: mu is the mean over the tokens, S their covariance); a common offset is added to every row of the
embedding table, so that x -- the post-norm hidden state -- has a mean.  The token matrix of every layer is captured by plain torch
hooks beside the engine's."""
import functools
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import vo_mean_model as V

pytestmark = pytest.mark.gpu
KINDS = ("llama", "llama_mha", "qwen2", "opt")
N_SAMPLES, BATCH = 4, 2
TOKENS = N_SAMPLES * 2048
ENV = ("MODEGPT_VO_INTERCEPT", "MODEGPT_MLP_INTERCEPT", "MODEGPT_KEEP_BIAS", "MODEGPT_VO_ERROR", "MODEGPT_OUTPUT_ERROR", "MODEGPT_RANK_CURVE",
       "MODEGPT_CALIBS_SAVE", "MODEGPT_CALIBS_LOAD")


def _tiny_model(kind, dev):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    init = 0.15
    if kind == "opt":
        cfg = transformers.OPTConfig(hidden_size=128, ffn_dim=320, num_hidden_layers=2, num_attention_heads=4, vocab_size=211,
                                     max_position_embeddings=2048, word_embed_proj_dim=128, init_std=init)
        m = transformers.OPTForCausalLM(cfg)
    else:
        common = dict(hidden_size=128, intermediate_size=320, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=4 if kind == "llama_mha" else 2, vocab_size=211, max_position_embeddings=2048,
                      initializer_range=init)
        if kind == "qwen2":
            m = transformers.Qwen2ForCausalLM(transformers.Qwen2Config(**common))
        else:
            m = transformers.LlamaForCausalLM(transformers.LlamaConfig(head_dim=32, **common))
    g = torch.Generator().manual_seed(3)
    for mod in m.modules():                                     # (HF initialises every bias to zero, with which nothing could fail)
        if isinstance(mod, torch.nn.Linear) and mod.bias is not None:
            mod.bias.data.copy_(torch.randn(mod.bias.shape, generator=g) * 0.15)
    emb = m.get_input_embeddings()
    emb.weight.data.add_(torch.randn(emb.weight.shape[1], generator=g) * 2 * init)       # the common offset: x gets a mean
    src = os.path.join(tempfile.mkdtemp(prefix="vo_intercept_src_"), kind)
    m.to(torch.bfloat16).save_pretrained(src)
    m = transformers.AutoModelForCausalLM.from_pretrained(src, dtype=torch.bfloat16).to(dev).eval()
    m.config._attn_implementation = "eager"
    return m


def _ids(dev):
    return torch.randint(0, 211, (2, 48), generator=torch.Generator().manual_seed(1)).to(dev)


class _Env:
    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in ENV}
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in self.values.items() if v is not None})

    def __exit__(self, *exc):
        for k, v in self.before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _norm_of(ad, block):
    return block.self_attn_layer_norm if ad.arch == "opt" else block.input_layernorm


@functools.lru_cache(maxsize=None)
def _pipeline(kind, vo="1", mlp=None, vo_error=None, stats_from=None, stats_to=None):
    """One run of the three stages on a fresh tiny model at keep 0.6; shared by the tests below and left unchanged by them."""
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.calibration import load_calibs
    from modegpt_amd.compression.compress_mlp import compress_nystrom
    from modegpt_amd.compression.compress_qk import compress_qk
    from modegpt_amd.compression.compress_vo import compress_vo, vo_rank_rule
    from modegpt_amd.patchers import install_compressed_attention
    dev = torch.device("cuda:0")
    keep = 0.6
    with _Env(MODEGPT_VO_INTERCEPT=vo, MODEGPT_MLP_INTERCEPT=mlp, MODEGPT_VO_ERROR=vo_error):
        model = _tiny_model(kind, dev)
        ad = ModelAdapter.from_model(model, None)
        root = tempfile.mkdtemp(prefix="vo_intercept_e2e_")
        layers_dir = os.path.join(root, "layers")
        ad.config = CompressionConfig(temp_storage_dir=layers_dir, nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5, dataset="synthetic",
                                      order="mlp,qk,vo", model="tiny-" + kind)
        original = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        X, forwards, handles = {}, [], []
        for i, block in enumerate(ad.get_transformer_blocks()):
            X[i] = []
            handles.append(_norm_of(ad, block).register_forward_hook(
                lambda m, a, out, i=i: X[i].append(out.detach().double().cpu().reshape(-1, out.shape[-1]))))
        handles.append(model.register_forward_pre_hook(lambda m, a: forwards.append(1)))
        cache = {k: v for k, v in (("load_calibs_from", stats_from), ("calibs_save_path", stats_to)) if v}
        try:
            cov_mlp, cov_q, cov_k, cov_x, _ = load_calibs(ad, n_samples=N_SAMPLES, batch_size=BATCH, dataset="synthetic", target_layers=[], **cache)
        finally:
            for h in handles:
                h.remove()
        X = {i: torch.cat(v) for i, v in X.items() if v}
        assert getattr(ad, "x_sums", None) is None
        means = None if getattr(ad, "x_means", None) is None else [m.cpu().clone() for m in ad.x_means]
        covs = [c.cpu().clone() for c in cov_x]
        keeps, layers = [keep] * ad.n_layers, list(range(ad.n_layers))
        compress_nystrom(ad, cov_mlp, keeps, layers)
        masks = compress_qk(ad, (cov_q, cov_k), keeps, target_layers=layers)
        compress_vo(ad, cov_x, keeps, target_layers=layers)
        assert all(torch.equal(c.cpu(), k) for c, k in zip(cov_x, covs))            # the statistic itself is untouched
        report = ad.report_vo_intercepts()
        ad.report_mlp_intercepts()
        ad.report_vo_bias_residuals()
        ad.report_vo_errors()
        vo_errors = dict(getattr(ad, "vo_errors", None) or {})
        ad.flush_artifacts()
        arts = {(i, s): torch.load(os.path.join(layers_dir, f"layer_{i}_{s}"), map_location="cpu") for i in layers for s in ("mlp", "qk", "vo")}
        ad.convert_model(saved_layers_dir=layers_dir)
        install_compressed_attention(ad, masks if kind != "opt" else None)
        return dict(original=original, arts=arts, masks=masks, model=model, adapter=ad, report=report, X=X, means=means, covs=covs,
                    forwards=len(forwards), root=root, vo_errors=vo_errors, rank=vo_rank_rule(ad.head_dim, keep, ad.arch),
                    metrics=json.loads(json.dumps(ad.metrics)))


def _attn_names(kind, i):
    p = f"model.decoder.layers.{i}.self_attn." if kind == "opt" else f"model.layers.{i}.self_attn."
    return p + "v_proj", p + ("out_proj" if kind == "opt" else "o_proj")


@pytest.mark.parametrize("kind", KINDS)
def test_means_artefacts_metrics_and_the_mean_error_on_the_tokens(dev, kind):
    run = _pipeline(kind)
    ad = run["adapter"]
    n_heads, n_kv, hd, rank, d = ad.n_heads, ad.n_kv_heads, ad.head_dim, run["rank"], ad.d_model
    carried = kind == "qwen2"                                   # (MODEGPT_KEEP_BIAS is off: only Qwen2 carries its biases)
    assert run["forwards"] == N_SAMPLES // BATCH and sorted(run["report"]) == [0, 1]
    assert sorted(run["metrics"]["vo_intercept"]) == ["0", "1"] and "vo_bias_residual" not in run["metrics"]
    for i in range(ad.n_layers):
        # the mean is the token matrix's: one fp64 sum per column, scaled once
        X = run["X"][i].numpy()
        assert X.shape == (TOKENS, d)
        mu = run["means"][i].numpy()
        ref = V.ld(X).sum(axis=0) / TOKENS
        assert np.all(np.abs(V.ld(mu) - ref) <= (TOKENS + 1) * 2.0 ** -53 * np.abs(V.ld(X)).sum(axis=0) / TOKENS)
        assert np.abs(mu).max() > 0.1
        art = run["arts"][(i, "vo")]
        assert set(art) == {"v_proj", "o_proj", "o_bias"}
        assert art["o_bias"].dtype == torch.bfloat16 and art["o_bias"].shape == (d,)
        m = run["metrics"]["vo_intercept"][str(i)]
        assert set(m) == {"offset_norm2", "mean_output_norm2", "relative"} and 0 < m["offset_norm2"] and 0 < m["relative"] < 10
        # the live model carries it
        vn, on = _attn_names(kind, i)
        sd = run["model"].state_dict()
        assert torch.equal(sd[on + ".bias"].cpu(), art["o_bias"]) and vn + ".bias" not in sd
        # from the stored tensors and the mean of the token matrix: mean_t (y - y') is one bf16 rounding of the bias
        W_v, W_o = run["original"][vn + ".weight"].double().numpy(), run["original"][on + ".weight"].double().numpy()
        b_v = run["original"][vn + ".bias"].double().numpy() if carried else None
        assert not carried or run["original"].get(on + ".bias") is None
        v, o, bias = art["v_proj"].double().numpy(), art["o_proj"].double().numpy(), art["o_bias"].double().numpy()
        args = (W_v, W_o, v, o, mu, n_heads, n_kv, hd, rank)
        dl, const = V.delta(*args, b_v=b_v)
        terms = d + n_heads * (hd + rank) + 8
        bound = 2.0 ** -8 * np.abs(bias) + V.delta_bound(*args, b_v=b_v) * (terms + TOKENS) / terms
        err = np.abs(V.delta(W_v, W_o, v, o, ref, n_heads, n_kv, hd, rank, b_v=b_v)[0] - V.ld(bias))
        print(f"{kind} layer {i}: |mean y - y'| / bound max {float((err / bound).max()):.3f}; relative offset {m['relative']:.3e}")
        assert np.all(err <= bound)
        assert abs(m["offset_norm2"] - float((dl * dl).sum())) <= 1e-9 * m["offset_norm2"]
        assert abs(m["mean_output_norm2"] - float((const * const).sum())) <= 1e-9 * m["mean_output_norm2"]


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_reloads_through_its_modeling_file_with_the_bias(dev, kind, tmp_path):
    transformers = pytest.importorskip("transformers")
    from modegpt_amd.model_utils import save_compressed_model
    run = _pipeline(kind)
    ad, model = run["adapter"], run["model"]
    with torch.no_grad():
        want = model(_ids(dev)).logits.float().cpu()
    ad.patch_config()
    carried = model.config.projection_biases
    assert "o" in carried and "v" not in carried
    assert set(carried) == ({"q", "k", "o"} if kind == "qwen2" else {"o"})
    out = str(tmp_path / "model")
    save_compressed_model(ad, rotary_masks=run["masks"] if kind != "opt" else None, save_dir=out, source_model_name="none")
    assert json.load(open(os.path.join(out, "config.json")))["projection_biases"] == carried
    loaded, info = transformers.AutoModelForCausalLM.from_pretrained(out, trust_remote_code=True, dtype=torch.bfloat16, output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"], info
    loaded = loaded.to(dev).eval()
    loaded.config._attn_implementation = "eager"
    sd = loaded.state_dict()
    for i in range(ad.n_layers):
        vn, on = _attn_names(kind, i)
        assert torch.equal(sd[on + ".bias"].cpu(), run["arts"][(i, "vo")]["o_bias"]) and vn + ".bias" not in sd
    with torch.no_grad():
        got = loaded(_ids(dev)).logits.float().cpu()
    assert torch.equal(got, want), float((got - want).abs().max())


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_switch_off_changes_nothing_and_on_changes_the_vo_artefact_only(dev):
    on, off = _pipeline("llama"), _pipeline("llama", vo=None)
    assert off["means"] is None and off["report"] == {} and "vo_intercept" not in off["metrics"]
    assert all(torch.equal(a, b) for a, b in zip(on["masks"], off["masks"]))
    for key, base in off["arts"].items():
        art = on["arts"][key]
        assert set(art) == set(base) | ({"o_bias"} if key[1] == "vo" else set())
        for k in base:
            assert _same_bits(art[k], base[k]) != (key[1] == "vo"), (key, k)        # v_proj / o_proj differ (the truncation is on S)
    for a, b in zip(on["covs"], off["covs"]):
        assert torch.equal(a, b)


def test_saved_statistics_round_trip_and_refuse_a_record_without_the_mean(dev, tmp_path):
    stats_on, stats_off = str(tmp_path / "stats_on"), str(tmp_path / "stats_off")
    first = _pipeline("llama", stats_to=stats_on)
    assert {"layer_0_x_mean.f64", "layer_1_x_mean.f64"} <= set(os.listdir(stats_on))
    for i in (0, 1):
        entry = json.load(open(os.path.join(stats_on, f"layer_{i}.json")))["files"]["x_mean"]
        values = np.fromfile(os.path.join(stats_on, entry["file"]), "<f8")
        assert entry["n"] == values.size == 128 and entry["bytes"] == 8 * 128 and np.array_equal(values, first["means"][i].numpy())
    again = _pipeline("llama", stats_from=stats_on)
    assert again["forwards"] == 0
    for key, art in first["arts"].items():
        assert set(again["arts"][key]) == set(art)
        for k in art:
            assert _same_bits(art[k], again["arts"][key][k]), (key, k)
    assert again["metrics"]["vo_intercept"] == first["metrics"]["vo_intercept"]
    # a record written without the switch: today's format (no entry, no file) ...
    plain = _pipeline("llama", vo=None, stats_to=stats_off)
    assert not [n for n in os.listdir(stats_off) if "mean" in n]
    assert all("x_mean" not in json.load(open(os.path.join(stats_off, f"layer_{i}.json")))["files"] for i in (0, 1))
    # ... which a run with the switch refuses, naming layer and field; a run without reads either directory and ignores the means
    with pytest.raises(ValueError, match=r"layer 0: field files\.x_mean is missing"):
        _pipeline("llama", stats_from=stats_off)
    for source in (stats_off, stats_on):
        loaded = _pipeline("llama", vo=None, stats_from=source)
        assert loaded["forwards"] == 0 and loaded["means"] is None
        for key, art in plain["arts"].items():
            assert set(loaded["arts"][key]) == set(art)
            for k in art:
                assert _same_bits(art[k], loaded["arts"][key][k]), (key, k)


@pytest.mark.parametrize("kind", ["llama", "llama_mha"])
def test_vo_error_report_and_curve_identity_on_the_centred_statistic(dev, kind):
    """MODEGPT_VO_ERROR=1 with the switch: the report and the curve are taken on S.  For the fp64 factors sum(e + rho dnorm2) equals
    curve[r] within the report's own noise floor, per kv head; the artefacts are the same bits with and without the report."""
    from modegpt_amd import ops
    run, plain = _pipeline(kind, vo_error="1"), _pipeline(kind)
    ad = run["adapter"]
    n_heads, n_kv, hd, rank = ad.n_heads, ad.n_kv_heads, ad.head_dim, run["rank"]
    ridge = ad.config.ridge_vo
    for i in range(ad.n_layers):
        for k, t in plain["arts"][(i, "vo")].items():
            assert _same_bits(run["arts"][(i, "vo")][k], t)
        m = run["metrics"]["vo_output_error"][str(i)]
        assert m["centred"] is True and m["rank"] == rank
        q, e, dn, curve = run["vo_errors"][i]
        vn, on = _attn_names(kind, i)
        Wv, Wo = run["original"][vn + ".weight"].to(dev), run["original"][on + ".weight"].to(dev)
        S = ops.cov_center(run["covs"][i].to(dev), run["means"][i].to(dev))
        _, _, v64, o64, curve64 = ops.vo_compress(S, Wv, Wo, n_heads, n_kv, hd, rank, ridge, want_f64=True, want_curve=True)
        assert torch.equal(curve64.cpu(), curve)                                   # the report's curve IS the centred one
        q64 = ops.vo_output_error(S, Wv, Wo, n_heads, n_kv, hd, 0, None, None)
        assert torch.allclose(q64.cpu(), q, rtol=1e-12, atol=0.0)
        e64, dn64 = ops.vo_output_error(S, Wv, Wo, n_heads, n_kv, hd, rank, v64, o64, want_dnorm2=True)
        d64 = ops.decode_vo_output_error(e64.cpu().tolist(), q.tolist(), dn64.cpu().tolist(), ridge, rank, n_kv, curve=curve.tolist())
        for g, (h64, hm) in enumerate(zip(d64["heads"], m["heads"])):
            assert hm["predicted_objective"] == float(curve[g, rank])
            print(f"{kind} layer {i} kv head {g}: fp64 objective - curve = {h64['objective'] - h64['predicted_objective']:.3e}, floor "
                  f"{h64['noise_floor']:.3e}; stored factors' excess {hm['excess_over_curve']:.3e}")
            assert abs(h64["objective"] - h64["predicted_objective"]) <= h64["noise_floor"]
            # (no sign is asserted for the STORED factors: grouped, the truncation's subspace ignores W_o, so it is not the minimiser
            #  of the output-weighted objective and a bf16 rounding of the factors can land under the curve as well as over it --
            #  measured here: llama layer 0, kv head 0, 2.1e-5 of the objective UNDER it)
            assert hm["excess_over_curve"] is not None and abs(hm["excess_over_curve"]) < 1.0
            if n_heads == n_kv:           # MHA: the two-SVD truncation IS that minimiser, so rounding its factors can only add
                assert hm["objective"] - hm["predicted_objective"] >= -hm["noise_floor"]
        # the uncentred statistic would say something else: the energy includes the mean's
        q_raw = ops.vo_output_error(run["covs"][i].to(dev), Wv, Wo, n_heads, n_kv, hd, 0, None, None)
        assert float(q_raw.sum()) > float(q.sum())


def test_both_intercept_switches_together_are_each_what_they_are_alone(dev):
    both, vo_only, mlp_only = _pipeline("llama", mlp="1"), _pipeline("llama"), _pipeline("llama", vo=None, mlp="1")
    assert "mlp_intercept" in both["metrics"] and "vo_intercept" in both["metrics"]
    for i in (0, 1):
        for suffix, alone in (("vo", vo_only), ("mlp", mlp_only), ("qk", vo_only)):
            art, want = both["arts"][(i, suffix)], alone["arts"][(i, suffix)]
            assert set(art) == set(want)
            for k in want:
                assert _same_bits(art[k], want[k]), (i, suffix, k)
    both["adapter"].patch_config()
    assert set(both["model"].config.projection_biases) == {"down", "o"}
