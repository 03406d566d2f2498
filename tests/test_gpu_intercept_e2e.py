"""GPU: MODEGPT_MLP_INTERCEPT=1 end to end on a tiny Llama (no mlp_bias) and a tiny OPT (ReLU, fc2 with a random bias): the hooks'
column sums -> calibration's means -> compress_nystrom's centred refit and intercept -> convert_model -> the checkpoint and its
modeling file; the saved statistics; the diagnostics on the centred statistic.

The tiny models have max_position_embeddings = 2048, so every calibration text has the 2048 tokens the statistics' normaliser
1 / (n_texts 2048) assumes: mu is then the mean over the tokens and S their covariance, as in a real run.  The token matrix of every
layer is captured by plain torch hooks beside the engine's, and what the stored tensors do is evaluated on it in fp64."""
import functools
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import mean_model as M

pytestmark = pytest.mark.gpu
KINDS = ("llama", "opt")
N_SAMPLES, BATCH = 4, 2
TOKENS = N_SAMPLES * 2048
ENV = ("MODEGPT_MLP_INTERCEPT", "MODEGPT_KEEP_BIAS", "MODEGPT_OUTPUT_ERROR", "MODEGPT_RANK_CURVE", "MODEGPT_CALIBS_SAVE", "MODEGPT_CALIBS_LOAD")


def _tiny_model(kind, dev, init=0.15):
    """Random init at std `init` (0.15: activations of O(1)), saved and loaded from disk as a run gets it; OPT's biases randomised."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    if kind == "opt":
        cfg = transformers.OPTConfig(hidden_size=128, ffn_dim=320, num_hidden_layers=2, num_attention_heads=4, vocab_size=211,
                                     max_position_embeddings=2048, word_embed_proj_dim=128, init_std=init)
        m = transformers.OPTForCausalLM(cfg)
        g = torch.Generator().manual_seed(3)
        for mod in m.modules():
            if isinstance(mod, torch.nn.Linear) and mod.bias is not None:
                mod.bias.data.copy_(torch.randn(mod.bias.shape, generator=g) * 0.15)
    else:
        cfg = transformers.LlamaConfig(hidden_size=128, intermediate_size=320, num_hidden_layers=2, num_attention_heads=4,
                                       num_key_value_heads=2, head_dim=32, vocab_size=211, max_position_embeddings=2048,
                                       initializer_range=init)
        m = transformers.LlamaForCausalLM(cfg)
    src = os.path.join(tempfile.mkdtemp(prefix="intercept_src_"), kind)
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


def _capture_h(ad, store):
    """Plain torch hooks beside the engine's: the sigma_mlp activation of every layer, as the engine sees it (OPT: before the ReLU)."""
    handles = []
    for i, block in enumerate(ad.get_transformer_blocks()):
        store[i] = []
        if ad.arch == "opt":
            handles.append(block.fc1.register_forward_hook(lambda m, a, out, i=i: store[i].append(torch.relu(out.detach()).double().cpu().reshape(-1, out.shape[-1]))))
        else:
            handles.append(block.mlp.down_proj.register_forward_pre_hook(lambda m, a, i=i: store[i].append(a[0].detach().double().cpu().reshape(-1, a[0].shape[-1]))))
    return handles


@functools.lru_cache(maxsize=None)
def _pipeline(kind, keep, intercept, keep_bias="0", diagnostics="0", stats_from=None, stats_to=None, init=0.15):
    """One run of the three stages on a fresh tiny model; shared by the tests below and left unchanged by them."""
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.calibration import load_calibs
    from modegpt_amd.compression.compress_mlp import compress_nystrom
    from modegpt_amd.compression.compress_qk import compress_qk
    from modegpt_amd.compression.compress_vo import compress_vo
    from modegpt_amd.patchers import install_compressed_attention
    dev = torch.device("cuda:0")
    with _Env(MODEGPT_MLP_INTERCEPT=intercept, MODEGPT_KEEP_BIAS=keep_bias, MODEGPT_OUTPUT_ERROR=diagnostics):
        model = _tiny_model(kind, dev, init)
        ad = ModelAdapter.from_model(model, None)
        assert ad.arch == kind
        root = tempfile.mkdtemp(prefix="intercept_e2e_")
        layers_dir = os.path.join(root, "layers")
        ad.config = CompressionConfig(temp_storage_dir=layers_dir, nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5, dataset="synthetic",
                                      order="mlp,qk,vo", model="tiny-" + kind)
        original = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        H, forwards = {}, []
        handles = _capture_h(ad, H)
        handles.append(model.register_forward_pre_hook(lambda m, a: forwards.append(1)))
        cache = {k: v for k, v in (("load_calibs_from", stats_from), ("calibs_save_path", stats_to)) if v}
        try:
            cov_mlp, cov_q, cov_k, cov_x, _ = load_calibs(ad, n_samples=N_SAMPLES, batch_size=BATCH, dataset="synthetic", target_layers=[], **cache)
        finally:
            for h in handles:
                h.remove()
        H = {i: torch.cat(v) for i, v in H.items() if v}
        means = None if getattr(ad, "mlp_means", None) is None else [m.cpu().clone() for m in ad.mlp_means]
        covs = [c.cpu().clone() for c in cov_mlp]
        keeps, layers = [keep] * ad.n_layers, list(range(ad.n_layers))
        compress_nystrom(ad, cov_mlp, keeps, layers)
        masks = compress_qk(ad, (cov_q, cov_k), keeps, target_layers=layers)
        compress_vo(ad, cov_x, keeps, target_layers=layers)
        report = ad.report_mlp_intercepts()
        errors = ad.report_output_errors()
        output_errors = dict(getattr(ad, "output_errors", None) or {})
        ad.flush_artifacts()
        arts = {(i, s): torch.load(os.path.join(layers_dir, f"layer_{i}_{s}"), map_location="cpu") for i in layers for s in ("mlp", "qk", "vo")}
        ad.convert_model(saved_layers_dir=layers_dir)
        install_compressed_attention(ad, masks if kind != "opt" else None)
        return dict(original=original, arts=arts, masks=masks, model=model, adapter=ad, report=report, H=H, means=means, covs=covs,
                    forwards=len(forwards), root=root, errors=errors, output_errors=output_errors, metrics=json.loads(json.dumps(ad.metrics)))


def _down_names(kind, i):
    p = f"model.decoder.layers.{i}." if kind == "opt" else f"model.layers.{i}."
    return p + ("fc2" if kind == "opt" else "mlp.down_proj"), p + ("fc1" if kind == "opt" else "mlp.up_proj")


def _selection(run, kind, i):
    """The selected columns, from the rows of `up` the artefact gathered."""
    W = run["original"][_down_names(kind, i)[1] + ".weight"]
    rows = [int((W == row).all(dim=1).nonzero()[0, 0]) for row in run["arts"][(i, "mlp")]["up"]]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    return np.asarray(rows)


@pytest.mark.parametrize("kind", KINDS)
def test_artefacts_metrics_and_the_mean_error_on_the_tokens(dev, kind):
    run = _pipeline(kind, 0.6, "1")
    ad = run["adapter"]
    assert run["forwards"] == N_SAMPLES // BATCH and sorted(run["report"]) == [0, 1]
    assert sorted(run["metrics"]["mlp_intercept"]) == ["0", "1"]
    for i in range(ad.n_layers):
        art = run["arts"][(i, "mlp")]
        assert set(art) == {"up", "down", "down_bias"} | ({"gate"} if kind != "opt" else set())      # (KEEP_BIAS off: no up_bias)
        assert art["down_bias"].dtype == torch.bfloat16 and art["down_bias"].shape == (ad.d_model,)
        m = run["metrics"]["mlp_intercept"][str(i)]
        assert set(m) == {"offset_norm2", "mean_output_norm2", "relative"} and 0 < m["offset_norm2"] and 0 < m["relative"] < 10
        # the mean is the token matrix's: one fp64 sum per column, scaled once
        H = run["H"][i]
        assert H.shape == (TOKENS, 320)
        mu = run["means"][i].numpy()
        ref = M.col_sums(H.numpy()) / TOKENS
        assert np.all(np.abs(M.ld(mu) - ref) <= (TOKENS + 1) * 2.0 ** -53 * np.abs(M.ld(H.numpy())).sum(axis=0) / TOKENS)
        # from the stored tensors and the token matrix: the per-channel mean of y - y' is one bf16 rounding of the bias (b_d is not
        # carried here: the switch for that is off, so y has none either)
        W = run["original"][_down_names(kind, i)[0] + ".weight"].double().numpy()
        idx = _selection(run, kind, i)
        D_hat, bias = art["down"].double().numpy(), art["down_bias"].double().numpy()
        mean, _ = M.token_errors(H.numpy(), W, idx, D_hat, bias=bias)
        n, r = W.shape[1], len(idx)
        bound = 2.0 ** -8 * np.abs(bias) + M.bias_bound(W, D_hat, idx, mu) * (n + r + 2 + TOKENS) / (n + r + 2)
        print(f"{kind} layer {i}: |mean y - y'| / bound max {float((np.abs(mean) / bound).max()):.3f}; relative offset {m['relative']:.3e}")
        assert np.all(np.abs(mean) <= bound)
        assert abs(m["offset_norm2"] - float((M.delta(W, D_hat, idx, mu)[0] ** 2).sum())) <= 1e-9 * m["offset_norm2"]


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_reloads_through_its_modeling_file_with_the_bias(dev, kind, tmp_path):
    transformers = pytest.importorskip("transformers")
    from modegpt_amd.model_utils import save_compressed_model
    run = _pipeline(kind, 0.6, "1")
    ad, model = run["adapter"], run["model"]
    with torch.no_grad():
        want = model(_ids(dev)).logits.float().cpu()
    ad.patch_config()
    assert "down" in model.config.projection_biases
    out = str(tmp_path / "model")
    save_compressed_model(ad, rotary_masks=run["masks"] if kind != "opt" else None, save_dir=out, source_model_name="none")
    assert "down" in json.load(open(os.path.join(out, "config.json")))["projection_biases"]
    loaded, info = transformers.AutoModelForCausalLM.from_pretrained(out, trust_remote_code=True, dtype=torch.bfloat16, output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"], info
    loaded = loaded.to(dev).eval()
    loaded.config._attn_implementation = "eager"
    sd = loaded.state_dict()
    for i in range(ad.n_layers):
        key = _down_names(kind, i)[0] + ".bias"
        assert torch.equal(sd[key].cpu(), run["arts"][(i, "mlp")]["down_bias"])
    with torch.no_grad():
        got = loaded(_ids(dev)).logits.float().cpu()
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("kind", KINDS)
def test_keep_everything_returns_the_projections_own_bias(dev, kind):
    """Keep 1.0 with the biases carried: where the stored tensor is W_d itself, delta = 0 up to the bound of its two sums and the bias
    is b_d (Llama has none: zero).  The refit keeps its ridge at r = n, D = W_d (I - eps M^-1), and the stored tensor is W_d only where
    eps |(W_d M^-1)_ij| stays below half a bf16 ulp of W_ij: at init std 0.15 the tiny Llama (lambda_min(S) ~ 1e-4) has 4 of its 40960
    entries one ulp off, and the intercept -- correctly, for the tensor that is stored -- is then 1.3e-8 where b_d is 0 (OPT's bf16
    b_d absorbs that).  The Llama case therefore runs at init std 0.5, S two orders larger, and asserts the premise first."""
    run = _pipeline(kind, 1.0, "1", keep_bias="1", init=0.5 if kind == "llama" else 0.15)
    ad = run["adapter"]
    for i in range(ad.n_layers):
        art = run["arts"][(i, "mlp")]
        name = _down_names(kind, i)[0]
        W = run["original"][name + ".weight"]
        b_d = run["original"].get(name + ".bias")
        idx = np.arange(W.shape[1])
        bound = M.bias_bound(W.double().numpy(), art["down"].double().numpy(), idx, run["means"][i].numpy(),
                             None if b_d is None else b_d.double().numpy())
        want = np.zeros(W.shape[0]) if b_d is None else b_d.double().numpy()
        err = np.abs(M.ld(art["down_bias"].double().numpy()) - M.ld(want))
        if b_d is None:
            assert torch.equal(art["down"], W), "the premise: the stored tensor is W_d"
        print(f"{kind} layer {i}: down == W_d on {float((art['down'] == W).float().mean()):.4f} of the entries; |bias - b_d| max {float(err.max()):.3e}")
        assert np.all(err <= bound)


@pytest.mark.parametrize("kind", KINDS)
def test_switch_off_changes_nothing_and_on_changes_down_and_down_bias_only(dev, kind):
    on, off = _pipeline(kind, 0.6, "1"), _pipeline(kind, 0.6, "0")
    assert off["means"] is None and off["report"] == {} and "mlp_intercept" not in off["metrics"]
    assert all(torch.equal(a, b) for a, b in zip(on["masks"], off["masks"]))
    for key, base in off["arts"].items():
        art = on["arts"][key]
        want = {"mlp": {"up", "down"} | ({"gate"} if kind != "opt" else set()), "qk": {"q_proj", "k_proj"}, "vo": {"v_proj", "o_proj"}}[key[1]]
        assert set(base) == want and set(art) == want | ({"down_bias"} if key[1] == "mlp" else set())
        for k in base:
            same = torch.equal(art[k].view(torch.int16), base[k].view(torch.int16))
            assert same != (k == "down"), (key, k)           # `down` differs (the refit is on S), everything else is the same bits
    for a, b in zip(on["covs"], off["covs"]):
        assert torch.equal(a, b)                             # the statistic itself is untouched


@pytest.mark.parametrize("kind", ["llama"])
def test_saved_statistics_round_trip_without_a_forward_and_refuse_a_record_without_the_mean(dev, kind, tmp_path):
    stats_on, stats_off = str(tmp_path / "stats_on"), str(tmp_path / "stats_off")
    first = _pipeline(kind, 0.6, "1", stats_to=stats_on)
    names = set(os.listdir(stats_on))
    assert {"layer_0_mlp_mean.f64", "layer_1_mlp_mean.f64"} <= names
    for i in (0, 1):
        side = json.load(open(os.path.join(stats_on, f"layer_{i}.json")))
        entry = side["files"]["mlp_mean"]
        values = np.fromfile(os.path.join(stats_on, entry["file"]), "<f8")
        assert entry["n"] == values.size == 320 and entry["bytes"] == 8 * 320
        assert np.array_equal(values, first["means"][i].numpy())
    again = _pipeline(kind, 0.6, "1", stats_from=stats_on)
    assert again["forwards"] == 0
    for key, art in first["arts"].items():
        other = again["arts"][key]
        assert set(other) == set(art)
        for k in art:
            assert torch.equal(art[k].view(torch.int16), other[k].view(torch.int16)), (key, k)
    # a record written without the switch: today's format (no entry, no file) ...
    plain = _pipeline(kind, 0.6, "0", stats_to=stats_off)
    assert not [n for n in os.listdir(stats_off) if "mean" in n]
    assert all("mlp_mean" not in json.load(open(os.path.join(stats_off, f"layer_{i}.json")))["files"] for i in (0, 1))
    # ... which a run with the switch refuses, naming layer and field, and a run without reads as ever -- also from the directory
    # that has the means, which it ignores
    with pytest.raises(ValueError, match=r"layer 0: field files\.mlp_mean is missing"):
        _pipeline(kind, 0.6, "1", stats_from=stats_off)
    for source in (stats_off, stats_on):
        loaded = _pipeline(kind, 0.6, "0", stats_from=source)
        assert loaded["forwards"] == 0 and loaded["means"] is None
        for key, art in plain["arts"].items():
            assert set(loaded["arts"][key]) == set(art)
            for k in art:
                assert torch.equal(art[k].view(torch.int16), loaded["arts"][key][k].view(torch.int16)), (key, k)


@pytest.mark.parametrize("kind", KINDS)
def test_output_error_reports_the_affine_maps_error_on_the_tokens(dev, kind):
    """MODEGPT_OUTPUT_ERROR=1 with the switch on: e_k = u_k S u_k^T is the per-channel error of the affine map -- the stored `down`
    with the OPTIMAL intercept -- over the tokens.  Against the token matrix in long double, relative to a_k = (sum_j |u_kj| sqrt(c_jj))^2 (an upper bound of
    |u_k| |C| |u_k|^T, the scale the fp64 statistic's own entry-wise bound is stated in), within
    tests/test_gpu_output_error.py's forward criterion RATIO * 64 n 2^-53 plus what the statistic itself carries: sigma_mlp and mu are
    fp64 sums over TOKENS tokens ((TOKENS / 4 + 4) 2^-53 and TOKENS 2^-53 relative to the sums of absolute terms)."""
    from tests.test_gpu_output_error import RATIO
    run = _pipeline(kind, 0.6, "1", diagnostics="1")
    plain = _pipeline(kind, 0.6, "1")
    ad = run["adapter"]
    n = ad.get_n_inner()
    for i in range(ad.n_layers):
        assert all(torch.equal(run["arts"][(i, "mlp")][k], v) for k, v in plain["arts"][(i, "mlp")].items())     # diagnostics change nothing
        q, e, _ = run["output_errors"][i]
        H = M.ld(run["H"][i].numpy())
        W = run["original"][_down_names(kind, i)[0] + ".weight"].double().numpy()
        idx = _selection(run, kind, i)
        u = M.residual(W, idx, run["arts"][(i, "mlp")]["down"].double().numpy())
        a_t = H @ u.T                                           # [tokens, d]
        ref = ((a_t - a_t.mean(axis=0)) ** 2).sum(axis=0) / TOKENS
        ref_q = (((H @ M.ld(W).T) - (H @ M.ld(W).T).mean(axis=0)) ** 2).sum(axis=0) / TOKENS
        sd = np.sqrt(M.ld(run["covs"][i].numpy()).diagonal())                       # (|C_ij| <= sqrt(c_ii c_jj): a >= |u| |C| |u|^T)
        a = (np.abs(u) @ sd) ** 2
        tol = (RATIO * 64 * n + (TOKENS / 4 + 4) + 2 * TOKENS + 4) * 2.0 ** -53
        err = np.abs(M.ld(e.numpy()) - ref) / a
        print(f"{kind} layer {i}: |e - token error| / a max {float(err.max()):.3e} (tol {tol:.3e}); relative error {float(ref.sum() / ref_q.sum()):.3e}")
        assert np.all(err <= tol)
        aq = (np.abs(M.ld(W)) @ sd) ** 2
        assert np.all(np.abs(M.ld(q.numpy()) - ref_q) / aq <= tol)
