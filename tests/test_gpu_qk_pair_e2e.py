"""MODEGPT_QK_SEQ=1 -- the within-sequence Q/K statistic through the calibration hooks (ops.qk_pair_accum on the rotated rows), the
report metrics["qk_logit_error_seq"], the cache entries and MODEGPT_QK_SEQ_SELECT=1, on tiny Llama (GQA, MHA) and Qwen2 models.

Criteria (a priori):
  IDENTITY  per kv head, error (raw_error) of metrics["qk_logit_error_seq"] against the brute-force sum over sequences, queries and
            keys of the variance over keys (the mean square) of e_ij = q'_iD . k'_jD in long double, from the rows the model's own
            apply_rotary_pos_emb returned (a spy), over n_texts 2048^2, within
              ((4T + n_texts + 8) + 1 + (g hd^2 + 2)) 2^-53 sum_{h in group} sum_{a,b in D} scale_h[a,b] / (n_texts 2048^2):
            the kernel's entry-wise bound (the fold over the batches of a layer is one chain of n_texts additions), one rounding of
            the normaliser, and mdg_qk_rank_curve's own summation bound; |P_ab| <= scale_ab
  ONE TEXT  raw_error against the error of metrics["qk_logit_error_rope"]: the same quantity when there is one sequence; both sides
            within their bounds of it, ((4T + 10) + (2T + 4) + 2 (g hd^2 + 2)) 2^-53 of the same scale
  SELECT    a Llama whose key rows carry a near-constant component in the lowest-frequency pair: the post-RoPE rule keeps that pair
            first, the within-sequence rule drops it, shift_share > 0.9 there, the masks differ, and E_seq of the within-sequence
            mask is no larger than E_seq of the post-RoPE mask on the same P

MEASURED on an MI355X: IDENTITY largest |report - brute force| / bound 4.5e-4 (Llama GQA), 5.1e-4 (Llama MHA), 4.4e-4 (Qwen2); SELECT
shift_share 0.99945 .. 0.99961 over both layers and kv heads."""
import contextlib
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import qk_pair_model as M

pytestmark = pytest.mark.gpu
LD, U = M.LD, M.U
N_TEXTS, SEQ, SEED = 3, 24, 0
SWITCHES = ("MODEGPT_QK_ROPE", "MODEGPT_QK_ROPE_SELECT", "MODEGPT_QK_ERROR", "MODEGPT_QK_SEQ", "MODEGPT_QK_SEQ_SELECT")


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def env(**switches):
    """The switches exactly as given (absent = unset), restored afterwards."""
    before = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in switches.items():
            os.environ["MODEGPT_" + k] = v
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int64 if t.element_size() == 8 else torch.int16)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def tiny(dev, kind="llama", **over):
    import transformers
    torch.manual_seed(SEED)
    kw = dict(hidden_size=64, intermediate_size=160, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=16,
              vocab_size=211, max_position_embeddings=64)
    kw.update(over)
    if kind == "qwen3":
        m = transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**kw))
    elif kind == "qwen2":
        kw.pop("head_dim")
        m = transformers.Qwen2ForCausalLM(transformers.Qwen2Config(**kw))
    elif kind == "opt":
        m = transformers.OPTForCausalLM(transformers.OPTConfig(hidden_size=64, ffn_dim=160, num_hidden_layers=2, num_attention_heads=4,
                                                               vocab_size=211, max_position_embeddings=64, word_embed_proj_dim=64))
    else:
        m = transformers.LlamaForCausalLM(transformers.LlamaConfig(**kw))
    return m.to(dev).to(torch.bfloat16).eval()


def adapter_for(model, dev, store, n_texts=N_TEXTS):
    """A fresh adapter with n_texts texts of 24 tokens in batches of 2 (the last batch may be ragged) already in place."""
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    ad = ModelAdapter.from_model(model, None)
    ad.config = CompressionConfig(temp_storage_dir=str(store), nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5, dataset="synthetic",
                                  calib_size=n_texts, calibs_batch_size=2, compression_ratio=0.3, order="mlp,qk,vo")
    ids = torch.randint(0, 211, (n_texts, SEQ), generator=torch.Generator().manual_seed(SEED + 1)).to(dev)
    ad.calibs = [ids[i:i + 2] for i in range(0, n_texts, 2)]
    return ad


def calibrate(ad, n_texts=N_TEXTS, **kw):
    from modegpt_amd.calibration import load_calibs
    return load_calibs(ad, n_samples=n_texts, batch_size=2, dataset="synthetic", target_layers=[], **kw)


def compress(ad, calibs, keep=0.5):
    from modegpt_amd.compression import compress_qk as CQ
    rank = CQ.qk_rank_rule(ad.head_dim, keep, ad.arch)
    return [CQ.compress_layer(ad, l, rank, cov_q_list=calibs[1][l], cov_k_list=calibs[2][l], rotary_masks=[]).cpu()
            for l in range(ad.n_layers)], rank


def artefacts(store, n_layers):
    return [torch.load(os.path.join(str(store), f"layer_{l}_qk"), map_location="cpu") for l in range(n_layers)]


@pytest.fixture(scope="module")
def model(dev):
    return tiny(dev)


def spied_calibration(monkeypatch, module, ad, n_texts=N_TEXTS, **switches):
    """Calibrates under the switches with a spy on the model's own rotary function; returns (calibs, rows): rows[l] = (q', k') of
    layer l over all texts, [n_texts * T, heads * hd] bf16 on the CPU, sequences in calibration order."""
    seen, real = [], module.apply_rotary_pos_emb

    def spy(q, k, cos, sin, *a, **kw):
        out = real(q, k, cos, sin, *a, **kw)
        seen.append(tuple(t.detach().cpu() for t in out))                   # ([B, H, T, hd], [B, KV, T, hd]) per layer and batch
        return out
    monkeypatch.setattr(module, "apply_rotary_pos_emb", spy)
    with env(**switches):
        calibs = calibrate(ad, n_texts)
    monkeypatch.setattr(module, "apply_rotary_pos_emb", real)
    L, nb = ad.n_layers, len(ad.calibs)
    assert len(seen) == nb * L
    rows = []
    for l in range(L):
        rows.append(tuple(torch.cat([seen[b * L + l][i].transpose(1, 2).reshape(-1, seen[b * L + l][i].shape[1] * ad.head_dim)
                                     for b in range(nb)]) for i in (0, 1)))
    return calibs, rows


def dropped(order_row, m, ns):
    units = np.asarray(order_row[m:], dtype=np.int64)
    return np.concatenate([units, units + ns])


# ---------------------------------------------------------------- the report against the brute-force sums, through the hooks
@pytest.mark.parametrize("kind,over", [("llama", {}), ("llama", {"num_key_value_heads": 4}), ("qwen2", {})])
def test_report_equals_the_brute_force_variance_sum(ops, dev, tmp_path, monkeypatch, kind, over):
    import importlib
    module = importlib.import_module("transformers.models.%s.modeling_%s" % (kind, kind))
    ad = adapter_for(tiny(dev, kind, **over), dev, tmp_path / "layers")
    calibs, rows = spied_calibration(monkeypatch, module, ad, QK_ROPE="1", QK_SEQ="1", QK_ERROR="1")
    assert ad.qk_pair_stats is not None and getattr(ad, "qk_pair_sums", None) is None
    with env(QK_ROPE="1", QK_SEQ="1", QK_ERROR="1"):
        masks, rank = compress(ad, calibs)
        ad.report_qk_errors()
    H, KV, hd = ad.n_heads, ad.n_kv_heads, ad.head_dim
    g, ns, m = H // KV, hd // 2, rank // 2
    s2 = LD(N_TEXTS) * LD(2048) ** 2
    c = (4 * SEQ + N_TEXTS + 8) + 1 + (g * hd * hd + 2)
    report = ad.metrics["qk_logit_error_seq"]
    json.dumps(report, allow_nan=False)
    assert sorted(report) == ["0", "1"]
    worst = 0.0
    for l in range(ad.n_layers):
        q, k = rows[l]
        P, R, scale = M.longdouble_pair(q, k, N_TEXTS, SEQ, H, KV, hd)
        # the collected statistic itself, entry-wise (the fold over the two batches is one chain) and symmetric to the bit
        for got, ref in ((ad.qk_pair_stats[0][l], P), (ad.qk_pair_stats[1][l], R)):
            assert same(got, got.transpose(1, 2))
            err = np.abs(got.cpu().numpy().astype(LD) - ref / s2)
            assert bool((err <= (4 * SEQ + N_TEXTS + 9) * U * scale / s2).all())
        order = ad.qk_errors_seq[l][6]
        assert torch.equal(order, ad.qk_errors[l][6]) and torch.equal(order, ad.qk_errors_rope[l][6])       # the same order everywhere
        e = report[str(l)]
        assert e["statistic"] == "within_sequence" and e["rank"] == rank and len(e["heads"]) == KV
        for kv in range(KV):
            D = dropped(order[kv].tolist(), m, ns)
            var, ms = M.brute_force(q, k, N_TEXTS, SEQ, H, KV, hd, D)
            grp = slice(kv * g, (kv + 1) * g)
            tol = c * U * sum(scale[h][np.ix_(D, D)].sum() for h in range(kv * g, (kv + 1) * g)) / s2
            head = e["heads"][kv]
            for name, got, want in (("error", head["error"], var[grp].sum() / s2), ("raw_error", head["raw_error"], ms[grp].sum() / s2)):
                err = abs(LD(got) - want)
                assert err <= tol, ("IDENTITY", kind, l, kv, name, float(err), float(tol))
                worst = max(worst, float(err / tol))
            assert 0.0 <= head["shift_share"] <= 1.0
            assert head["shift_share"] == 1.0 - head["error"] / head["raw_error"]
        assert e["shift_share"] == 1.0 - e["error"] / e["raw_error"]
    print("IDENTITY %s %s: largest |report - brute force| / bound = %.3e" % (kind, over, worst))


def test_one_text_raw_error_equals_the_post_rope_logit_error(ops, dev, model, tmp_path, monkeypatch):
    from transformers.models.llama import modeling_llama as ML
    ad = adapter_for(model, dev, tmp_path / "layers", n_texts=1)
    calibs, rows = spied_calibration(monkeypatch, ML, ad, n_texts=1, QK_ROPE="1", QK_SEQ="1", QK_ERROR="1")
    with env(QK_ROPE="1", QK_SEQ="1", QK_ERROR="1"):
        _, rank = compress(ad, calibs)
        ad.report_qk_errors()
    H, KV, hd = ad.n_heads, ad.n_kv_heads, ad.head_dim
    g, ns, m = H // KV, hd // 2, rank // 2
    c = (4 * SEQ + 10) + (2 * SEQ + 4) + 2 * (g * hd * hd + 2)
    for l in range(ad.n_layers):
        scale = M.longdouble_pair(rows[l][0], rows[l][1], 1, SEQ, H, KV, hd)[2]
        order = ad.qk_errors_seq[l][6]
        for kv in range(KV):
            D = dropped(order[kv].tolist(), m, ns)
            tol = c * U * sum(scale[h][np.ix_(D, D)].sum() for h in range(kv * g, (kv + 1) * g)) / LD(2048) ** 2
            raw = ad.metrics["qk_logit_error_seq"][str(l)]["heads"][kv]["raw_error"]
            rope = ad.metrics["qk_logit_error_rope"][str(l)]["heads"][kv]["error"]
            assert rope > 0 and abs(LD(raw) - LD(rope)) <= tol, (l, kv, raw, rope, float(tol))


# ---------------------------------------------------------------- switches off / on
def test_switch_off_launches_nothing_and_on_changes_no_other_bit(ops, dev, model, tmp_path, monkeypatch):
    calls = []
    real = ops.qk_pair_accum
    monkeypatch.setattr(ops, "qk_pair_accum", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    off = adapter_for(model, dev, tmp_path / "off")
    stats_off = str(tmp_path / "stats_off")
    with env(QK_ROPE="1", QK_ERROR="1"):
        c_off = calibrate(off, calibs_save_path=stats_off)
        m_off, rank = compress(off, c_off)
        off.report_qk_errors()
        off.report_attention_margins()
    assert not calls, "ops.qk_pair_accum ran with MODEGPT_QK_SEQ unset"
    assert off.qk_pair_stats is None and "qk_logit_error_seq" not in off.metrics
    assert not any("qk_pair" in name for name in os.listdir(stats_off))
    assert sorted(json.load(open(os.path.join(stats_off, "layer_0.json")))["files"]) == ["k", "k_rope", "mlp", "q", "q_rope", "x"]
    on = adapter_for(model, dev, tmp_path / "on")
    with env(QK_ROPE="1", QK_SEQ="1", QK_ERROR="1"):
        c_on = calibrate(on)
        assert len(calls) == 2 * on.n_layers                                # one call per layer and batch
        m_on, _ = compress(on, c_on)
        on.report_qk_errors()
        on.report_attention_margins()
    for a, b in zip(c_off[:4], c_on[:4]):
        assert all(same(x, y) for x, y in zip(a, b))
    assert c_off[4] == c_on[4]
    for i in (0, 1):
        assert all(same(x, y) for x, y in zip(off.qk_rope_stats[i], on.qk_rope_stats[i]))
    assert all(torch.equal(a, b) for a, b in zip(m_off, m_on))
    for a, b in zip(artefacts(tmp_path / "off", 2), artefacts(tmp_path / "on", 2)):
        assert sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    assert sorted(set(on.metrics) - set(off.metrics)) == ["qk_logit_error_seq"]
    for key in off.metrics:
        assert json.dumps(off.metrics[key], sort_keys=True) == json.dumps(on.metrics[key], sort_keys=True), key


def test_seq_without_rope_raises_before_the_first_forward(dev, model, tmp_path):
    ad = adapter_for(model, dev, tmp_path / "layers")
    fired = []
    hook = model.register_forward_pre_hook(lambda *args: fired.append(1))
    try:
        with env(QK_SEQ="1"):
            with pytest.raises(RuntimeError, match="MODEGPT_QK_SEQ=1 needs MODEGPT_QK_ROPE=1"):
                calibrate(ad)
    finally:
        hook.remove()
    assert not fired


@pytest.mark.parametrize("kind", ["qwen3", "opt"])
def test_other_architectures_collect_nothing_and_say_why(ops, dev, kind, tmp_path, monkeypatch, caplog):
    calls = []
    real = ops.qk_pair_accum
    monkeypatch.setattr(ops, "qk_pair_accum", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    ad = adapter_for(tiny(dev, kind), dev, tmp_path / "layers")
    stats = str(tmp_path / "stats")
    with env(QK_SEQ="1"), caplog.at_level(logging.INFO, logger="MoDeGPT"):
        calibrate(ad, calibs_save_path=stats)
    assert not calls and ad.qk_pair_stats is None
    assert not any("qk_pair" in name for name in os.listdir(stats))
    said = [r for r in caplog.records if "MODEGPT_QK_SEQ=1" in r.getMessage()]
    assert len(said) == 1 and said[0].levelno == (logging.WARNING if kind == "qwen3" else logging.INFO)


# ---------------------------------------------------------------- cache
def test_cache_round_trip_and_refusal(ops, dev, model, tmp_path):
    stats_on, stats_off = str(tmp_path / "stats_on"), str(tmp_path / "stats_off")
    a = adapter_for(model, dev, tmp_path / "a")
    with env(QK_ROPE="1", QK_SEQ="1", QK_ERROR="1"):
        ca = calibrate(a, calibs_save_path=stats_on)
        ma, _ = compress(a, ca)
        a.report_qk_errors()
    for l in range(a.n_layers):
        meta = json.load(open(os.path.join(stats_on, f"layer_{l}.json")))
        for kind in ("qk_pair", "qk_pair_raw"):
            assert os.path.getsize(os.path.join(stats_on, f"layer_{l}_{kind}.f64")) == meta["files"][kind]["bytes"]
            assert {k: meta["files"][kind][k] for k in ("n", "batch", "bytes", "layout")} == \
                {k: meta["files"]["q"][k] for k in ("n", "batch", "bytes", "layout")}
    c = adapter_for(model, dev, tmp_path / "c")
    with env(QK_ROPE="1"):
        calibrate(c, calibs_save_path=stats_off)
    fired = []
    hook = model.register_forward_pre_hook(lambda *args: fired.append(1))
    try:
        b = adapter_for(model, dev, tmp_path / "b")
        with env(QK_ROPE="1", QK_SEQ="1", QK_ERROR="1"):
            cb = calibrate(b, load_calibs_from=stats_on)
            mb, _ = compress(b, cb)
            b.report_qk_errors()
        for i in (0, 1):
            assert all(same(x, y) for x, y in zip(a.qk_pair_stats[i], b.qk_pair_stats[i]))
        assert all(torch.equal(x, y) for x, y in zip(ma, mb))
        assert a.metrics["qk_logit_error_seq"] == b.metrics["qk_logit_error_seq"]
        d = adapter_for(model, dev, tmp_path / "d")
        with env(QK_ROPE="1", QK_SEQ="1"):
            with pytest.raises(ValueError, match=r"layer 0.*qk_pair.*MODEGPT_QK_SEQ=1"):
                calibrate(d, load_calibs_from=stats_off)
        with env(QK_ROPE="1"):                                               # a record WITH the entries, loaded without the switch
            e = adapter_for(model, dev, tmp_path / "e")
            ce = calibrate(e, load_calibs_from=stats_on)
            assert e.qk_pair_stats is None and all(same(p, q) for p, q in zip(ca[1], ce[1]))
        assert not fired, "the model ran"
    finally:
        hook.remove()


# ---------------------------------------------------------------- MODEGPT_QK_SEQ_SELECT=1
def biased_llama(dev):
    """A Llama whose key rows carry a large, nearly position-independent component in the lowest-frequency rotary pair: k_proj.bias
    = 16 on column ns - 1 of every kv head, the weight rows of that pair scaled down; at T = 24 the pair turns by under 0.01 rad."""
    m = tiny(dev, attention_bias=True)
    hd, ns = 16, 8
    with torch.no_grad():
        for layer in m.model.layers:
            kp = layer.self_attn.k_proj
            kp.bias.zero_()
            layer.self_attn.q_proj.bias.zero_()
            for kv in range(2):
                for col in (ns - 1, hd - 1):
                    kp.weight[kv * hd + col] *= 0.01
                kp.bias[kv * hd + ns - 1] = 16.0
    return m


def e_seq(P, mask, g, hd):
    """sum over a kv head's group of 1^T P_h[D,D] 1, D = the columns the mask drops; per kv head."""
    out = []
    for kv in range(mask.shape[0]):
        D = sorted(set(range(hd)) - set(mask[kv].tolist()))
        out.append(sum(float(P[h][np.ix_(D, D)].sum()) for h in range(kv * g, (kv + 1) * g)))
    return out


def test_selection_on_the_within_sequence_statistic(ops, dev, tmp_path):
    import transformers
    from modegpt_amd.compression import compress_qk as CQ
    from modegpt_amd.compression.compress_mlp import compress_nystrom
    from modegpt_amd.compression.compress_vo import compress_vo
    from modegpt_amd.model_utils import save_compressed_model
    own = biased_llama(dev)
    ad = adapter_for(own, dev, tmp_path / "layers")
    layers, keep = list(range(ad.n_layers)), [0.5] * ad.n_layers
    H, KV, hd = ad.n_heads, ad.n_kv_heads, ad.head_dim
    g, ns = H // KV, hd // 2
    with env(QK_ROPE="1", QK_SEQ_SELECT="1"):
        c0 = calibrate(ad)
        with pytest.raises(RuntimeError, match="MODEGPT_QK_SEQ_SELECT=1.*MODEGPT_QK_SEQ=1"):
            compress(ad, c0)
    with env(QK_ROPE="1", QK_SEQ="1", QK_ROPE_SELECT="1", QK_SEQ_SELECT="1"):
        c = calibrate(ad)
        with pytest.raises(RuntimeError, match="MODEGPT_QK_SEQ_SELECT=1 and MODEGPT_QK_ROPE_SELECT=1"):
            compress(ad, c)
    with env(QK_ROPE="1", QK_SEQ="1", QK_ROPE_SELECT="1", QK_ERROR="1"):
        rope_masks, rank = compress(ad, c)
        ad.report_qk_errors()
        ad.report_attention_margins()
    rope_sel = dict(ad.metrics["qk_selection"])
    with env(QK_ROPE="1", QK_SEQ="1", QK_SEQ_SELECT="1", QK_ERROR="1"):
        compress_nystrom(ad, c[0], keep, layers)
        masks = CQ.compress_qk(ad, (c[1], c[2]), keep, target_layers=layers)
        compress_vo(ad, c[3], keep, target_layers=layers)
        ad.report_qk_errors()
        ad.report_attention_margins()
    mode = CQ.qk_mode_and_ridges(ad.arch, True, ad.config.ridge_qk)[0]
    ones = torch.ones(KV, hd, hd, dtype=torch.float64, device=dev)
    for l in layers:
        P = ad.qk_pair_stats[0][l]
        assert torch.equal(masks[l], ops.qk_select(P, ones, rank, mode, 0.0, 0.0)[0])
        assert torch.equal(ad.qk_errors_seq[l][6], ops.qk_select(P, ones, hd, mode, 0.0, 0.0)[0][:, :ns].cpu())
        seq_mask, rope_mask = masks[l].cpu(), rope_masks[l]
        assert not torch.equal(seq_mask, rope_mask)
        for kv in range(KV):
            assert int(rope_mask[kv][0]) == ns - 1, "the post-RoPE rule keeps the near-constant pair first"
            assert ns - 1 not in seq_mask[kv].tolist() and hd - 1 not in seq_mask[kv].tolist(), "the within-sequence rule drops it"
            share = ad.metrics["qk_logit_error_seq"][str(l)]["heads"][kv]["shift_share"]
            print("SELECT layer %d kv %d: shift_share %.6f" % (l, kv, share))
            assert share > 0.9
        Ph = P.cpu().numpy()
        for a, b in zip(e_seq(Ph, seq_mask, g, hd), e_seq(Ph, rope_mask, g, hd)):
            assert a <= b
        # the entry says which statistic, and that no certificate exists; the post-RoPE run had one
        sel = ad.metrics["qk_selection"][str(l)]
        assert sel["statistic"] == "within_sequence" and sel["certificate"] is None and sel["certified"] is None and "heads" not in sel
        assert rope_sel[str(l)]["statistic"] == "post_rope" and "heads" in rope_sel[str(l)]
    # the artefact through the existing rebuild path: a mask is a mask
    ad.convert_model(saved_layers_dir=ad.config.temp_storage_dir)
    ad.patch_config()
    out = str(tmp_path / "ckpt")
    save_compressed_model(ad, rotary_masks=masks, save_dir=out, source_model_name="none")
    loaded = transformers.AutoModelForCausalLM.from_pretrained(out, trust_remote_code=True, dtype=torch.bfloat16).to(dev).eval()
    assert "Rebuild" in type(loaded).__module__
    ids = torch.randint(0, 211, (2, 20), generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        assert bool(torch.isfinite(loaded(ids).logits.float()).all())
