"""GPU: load_calibs(calibs_save_path=...) / load_calibs(load_calibs_from=...) -- the statistics directory (calib_cache.py) from the
packing kernels up to the driver: a saved calibration loads bit for bit without the model running, compresses to identical
artefacts and certificates, composes over layer subsets, and every mismatch is refused by name."""
import json
import os
import shutil

import pytest
import torch

from tests.test_gpu_e2e import _tiny_model

pytestmark = pytest.mark.gpu
N_SAMPLES, BATCH = 8, 4


def _llama4(dev):
    """The 4-layer Llama of the round trip: d 128, d_ff 320, heads 4/2 x 32."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(hidden_size=128, intermediate_size=320, num_hidden_layers=4, num_attention_heads=4,
                                   num_key_value_heads=2, head_dim=32, vocab_size=211, max_position_embeddings=64)
    return transformers.LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).eval()


def _adapter(model, tmp, calibs=None):
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    ad = ModelAdapter.from_model(model, None)
    ad.config = CompressionConfig(temp_storage_dir=str(tmp), nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5, dataset="synthetic",
                                  calib_size=N_SAMPLES, calibs_batch_size=BATCH, compression_ratio=0.3, order="mlp,qk,vo")
    ad.calibs = calibs
    return ad


def _calibs(ad, **kw):
    from modegpt_amd.calibration import load_calibs
    return load_calibs(ad, n_samples=N_SAMPLES, batch_size=BATCH, dataset="synthetic", **kw)


def _same(a, b):
    for la, lb in zip(a[:4], b[:4]):
        assert len(la) == len(lb)
        for ta, tb in zip(la, lb):
            assert (ta is None) == (tb is None)
            if ta is not None:
                assert torch.equal(ta.view(torch.int64), tb.view(torch.int64))      # bit patterns, both triangles
    assert a[4] == b[4]


def _eps(ad):
    from modegpt_amd.compression.compress_mlp import covariance_error_eps
    from modegpt_amd.compression.compress_qk import attention_error_eps
    return covariance_error_eps(ad, ad.get_n_inner()), attention_error_eps(ad)


class Saved:
    """One calibration of a model, saved: what the tests below load from (computed once, never changed)."""

    def __init__(self, model, root):
        self.model, self.dir = model, str(root / "stats")
        self.ad = _adapter(model, root / "layers_a")
        self.plain = _calibs(self.ad, target_layers=[])
        self.a = _calibs(self.ad, calibs_save_path=self.dir, target_layers=[])
        self.eps = _eps(self.ad)
        self.attrs = (self.ad.calib_tokens, self.ad.cov_routes, getattr(self.ad, "cov_rows_left", None))


@pytest.fixture(scope="module")
def saved(dev, tmp_path_factory):
    return Saved(_llama4(dev), tmp_path_factory.mktemp("calib_llama4"))


def _load(saved, tmp, model=None, directory=None, **kw):
    """A fresh adapter (no tokens, no attributes of an earlier calibration) loading from the saved directory; any forward fails the test."""
    model = saved.model if model is None else model
    ad = _adapter(model, tmp)
    fired = []
    hook = model.register_forward_pre_hook(lambda *a: fired.append(1))
    try:
        out = _calibs(ad, load_calibs_from=directory or saved.dir, **kw)
    finally:
        hook.remove()
    assert not fired, "the model ran"
    assert ad.calibs is None, "the calibration texts were tokenised"
    return ad, out


def test_round_trip(saved, tmp_path):
    _same(saved.plain, saved.a)                                               # saving changes nothing that is returned
    assert sorted(n for n in os.listdir(saved.dir) if ".tmp" in n) == []
    ad, b = _load(saved, tmp_path, target_layers=[])
    _same(saved.a, b)
    for kind in b[:4]:
        for t in kind:
            assert torch.equal(t, t.transpose(-1, -2))
    assert ad.bi_scores == saved.a[4]
    assert (ad.calib_tokens, ad.cov_routes, getattr(ad, "cov_rows_left", None)) == saved.attrs
    assert _eps(ad) == saved.eps
    # both arguments: load, then write to the second directory -- a copy whose files are identical
    copy = str(tmp_path / "copy")
    ad2 = _adapter(saved.model, tmp_path)
    c = _calibs(ad2, load_calibs_from=saved.dir, calibs_save_path=copy, target_layers=[1, 3])
    _same(c, tuple([t if i in (1, 3) else None for i, t in enumerate(lst)] for lst in saved.a[:4]) + (saved.a[4],))
    for name in ("layer_1_mlp.f64", "layer_3_k.f64", "layer_3.json", "bi_scores.json"):
        assert open(os.path.join(copy, name), "rb").read() == open(os.path.join(saved.dir, name), "rb").read(), name
    assert not os.path.exists(os.path.join(copy, "layer_0.json"))


def _compress(ad, calibs, keep_ratio=0.7):
    from modegpt_amd.compression.compress_mlp import compress_nystrom
    from modegpt_amd.compression.compress_qk import compress_qk
    from modegpt_amd.compression.compress_vo import compress_vo
    cov_mlp, cov_q, cov_k, cov_x = ([None if t is None else t.clone() for t in lst] for lst in calibs[:4])   # (the shared reference stays as it is)
    layers = list(range(ad.n_layers))
    keep = [keep_ratio] * ad.n_layers
    compress_nystrom(ad, cov_mlp, keep, layers)
    masks = compress_qk(ad, (cov_q, cov_k), keep, target_layers=layers)
    compress_vo(ad, cov_x, keep, target_layers=layers)
    ad.report_selection_margins()
    ad.report_attention_margins()
    art = {}
    for l in layers:
        for suffix in ("mlp", "qk", "vo"):
            art[(l, suffix)] = torch.load(os.path.join(ad.config.temp_storage_dir, f"layer_{l}_{suffix}"), map_location="cpu")
    return art, masks, {k: ad.metrics.get(k) for k in ("mlp_selection", "qk_selection", "vo_spectrum")}


def _assert_identical_artefacts(saved, tmp):
    art_a, masks_a, metrics_a = _compress(saved.ad, saved.a)
    ad, b = _load(saved, tmp / "layers_b", target_layers=[])
    art_b, masks_b, metrics_b = _compress(ad, b)
    assert art_a.keys() == art_b.keys()
    for key in art_a:
        assert art_a[key].keys() == art_b[key].keys()
        for name in art_a[key]:
            assert torch.equal(art_a[key][name], art_b[key][name]), (key, name)
    assert len(masks_a or []) == len(masks_b or [])
    for ma, mb in zip(masks_a or [], masks_b or []):
        assert (ma is None and mb is None) or torch.equal(ma, mb)
    assert metrics_a["mlp_selection"] is not None and metrics_a["vo_spectrum"] is not None
    assert json.dumps(metrics_a, sort_keys=True) == json.dumps(metrics_b, sort_keys=True)      # (NaN entries compare as text)


def test_artefacts_from_loaded_statistics_are_identical_llama(saved, tmp_path):
    _assert_identical_artefacts(saved, tmp_path)


@pytest.mark.parametrize("kind", ["opt", "llama_128"])
def test_artefacts_from_loaded_statistics_are_identical(dev, tmp_path, kind):
    """opt: fp16 activations and the ReLU statistic; llama_128: every statistic a multiple of 128 wide (the fused int8 launch path)."""
    model = _tiny_model(kind, dev)
    if kind == "opt":
        model = model.to(torch.float16)
    _assert_identical_artefacts(Saved(model, tmp_path), tmp_path)


def test_subsets_compose(saved, tmp_path):
    d = str(tmp_path / "subsets")
    ad = _adapter(saved.model, tmp_path, calibs=saved.ad.calibs)
    _calibs(ad, calibs_save_path=d, target_layers=[0, 1])
    _calibs(ad, calibs_save_path=d, target_layers=[2])
    from modegpt_amd import calib_cache
    assert calib_cache.layers_present(d) == [0, 1, 2]
    _, got = _load(saved, tmp_path, directory=d, target_layers=[1, 2])
    for lst_got, lst_full in zip(got[:4], saved.a[:4]):
        assert lst_got[0] is None and lst_got[3] is None
        for i in (1, 2):
            assert torch.equal(lst_got[i], lst_full[i])
    assert got[4] == saved.a[4]
    with pytest.raises(FileNotFoundError, match=r"layer 3\b"):
        _load(saved, tmp_path, directory=d, target_layers=[3])


def test_refuses_another_width(saved, dev, tmp_path):
    with pytest.raises(ValueError, match="d_model"):
        _load(saved, tmp_path, model=_tiny_model("llama_128", dev), target_layers=[0])


def test_refuses_another_sample_count(saved, tmp_path):
    from modegpt_amd.calibration import load_calibs
    ad = _adapter(saved.model, tmp_path)
    with pytest.raises(ValueError, match="n_samples"):
        load_calibs(ad, n_samples=N_SAMPLES - 2, batch_size=BATCH, dataset="synthetic", load_calibs_from=saved.dir, target_layers=[0])


def test_refuses_changed_weights(saved, tmp_path):
    w = saved.model.model.layers[2].mlp.down_proj.weight.data
    bits = w.view(torch.int16)
    old = bits[3, 5].item()
    bits[3, 5] = old + 1                                                       # one ulp in one element
    try:
        with pytest.raises(ValueError, match=r"layer 2\b.*weights\.down_proj"):
            _load(saved, tmp_path, target_layers=[])
    finally:
        bits[3, 5] = old
    _load(saved, tmp_path, target_layers=[2])


def _damaged_copy(saved, tmp):
    d = str(tmp / "damaged")
    shutil.copytree(saved.dir, d)
    return d


def test_refuses_a_truncated_file(saved, tmp_path):
    d = _damaged_copy(saved, tmp_path)
    path = os.path.join(d, "layer_1_x.f64")
    os.truncate(path, os.path.getsize(path) - 8)
    with pytest.raises(ValueError, match=r"layer 1\b.*files\.x\.bytes"):
        _load(saved, tmp_path, directory=d, target_layers=[])


def test_refuses_a_flipped_diagonal_entry(saved, tmp_path):
    d = _damaged_copy(saved, tmp_path)
    i = 7
    with open(os.path.join(d, "layer_0_mlp.f64"), "r+b") as f:
        f.seek(8 * (i * (i + 3) // 2) + 6)                                     # entry (7, 7) of the packed triangle; byte 6 holds exponent bits
        byte = f.read(1)[0]
        f.seek(-1, 1)
        f.write(bytes([byte ^ 0x10]))                                          # lowest exponent bit: the entry doubles or halves
    with pytest.raises(ValueError, match=r"layer 0\b.*files\.mlp\.trace_bits"):
        _load(saved, tmp_path, directory=d, target_layers=[])


def test_driver_saves_then_loads(dev, tmp_path, monkeypatch):
    """test_run_modegpt_main_on_local_checkpoint twice: MODEGPT_CALIBS_SAVE, then MODEGPT_CALIBS_LOAD.  The two checkpoints are
    identical and the second run's load_calibs never ran the model."""
    transformers = pytest.importorskip("transformers")
    tokenizers = pytest.importorskip("tokenizers")
    from modegpt_amd import run_modegpt
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.model_utils import reload_compressed_model

    vocab = {f"w{i}": i for i in range(208)}
    vocab.update({"<unk>": 208, "<s>": 209, "</s>": 210})
    tok = tokenizers.Tokenizer(tokenizers.models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = tokenizers.pre_tokenizers.Whitespace()
    fast = transformers.PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="<unk>", bos_token="<s>", eos_token="</s>")
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(hidden_size=128, intermediate_size=320, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, head_dim=32, vocab_size=211, max_position_embeddings=64,
                                   initializer_range=0.15)
    src = tmp_path / "src_model"
    transformers.LlamaForCausalLM(cfg).to(torch.bfloat16).save_pretrained(src)
    fast.save_pretrained(src)
    monkeypatch.chdir(tmp_path)
    stats = str(tmp_path / "stats")

    forwards = []
    real = run_modegpt.load_calibs

    def counting(adapter, **kw):
        n = []
        hook = adapter.model.register_forward_pre_hook(lambda *a: n.append(1))
        try:
            return real(adapter=adapter, **kw)
        finally:
            hook.remove()
            forwards.append(len(n))

    monkeypatch.setattr(run_modegpt, "load_calibs", counting)

    def run(name, env):
        for var in ("MODEGPT_CALIBS_SAVE", "MODEGPT_CALIBS_LOAD"):
            monkeypatch.delenv(var, raising=False)
        monkeypatch.setenv(env, stats)
        out = tmp_path / name
        conf = CompressionConfig(model=str(src), output_dir=str(out), temp_storage_dir=str(out / "layers"), dataset="synthetic",
                                 order="mlp,qk,vo", calib_size=8, calibs_batch_size=4, compression_ratio=0.3, nystrom_ridge=1e-4,
                                 ridge_qk=1e-2, ridge_vo=1e-5, note="pytest")
        ppl = run_modegpt.main(config=conf)
        assert ppl is not None and ppl > 1.0 and ppl == ppl
        return ppl, out / "model"

    ppl_save, dir_save = run("out_save", "MODEGPT_CALIBS_SAVE")
    assert len(forwards) == 1 and forwards[0] > 0 and os.path.exists(os.path.join(stats, "layer_1.json")) and os.path.exists(os.path.join(stats, "bi_scores.json"))
    ppl_load, dir_load = run("out_load", "MODEGPT_CALIBS_LOAD")
    assert len(forwards) == 2 and forwards[1] == 0, "the loading run ran the model inside load_calibs"
    assert ppl_save == ppl_load
    masks_a, masks_b = torch.load(dir_save / "rotary_masks.pt"), torch.load(dir_load / "rotary_masks.pt")
    assert len(masks_a) == len(masks_b) == 2 and all(torch.equal(x, y) for x, y in zip(masks_a, masks_b))
    sd_a = reload_compressed_model(str(dir_save))[0].state_dict()
    sd_b = reload_compressed_model(str(dir_load))[0].state_dict()
    assert sd_a.keys() == sd_b.keys()
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
