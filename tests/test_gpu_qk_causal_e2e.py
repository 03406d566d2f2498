"""MODEGPT_QK_CAUSAL=1 -- the causal Q/K statistic through the calibration hooks (ops.qk_causal_accum on the rotated rows), the report
metrics["qk_logit_error_causal"], the cache entries and MODEGPT_QK_CAUSAL_SELECT=1, on tiny random-weight Llama (GQA, MHA) and Qwen2
models: three texts of 24 tokens in batches of 2 + 1.

Criteria (a priori):
  IDENTITY  per kv head, error (raw_error) of metrics["qk_logit_error_causal"] against the brute-force sum over sequences and queries
            of the variance (the mean square) over the keys j <= i of e_ij = q'_iD . k'_jD in long double, from the rows the model's
            own apply_rotary_pos_emb returned (a spy), over n_texts 2048, within
              ((4T + n_texts + 8) + 1 + (g hd^2 + 2)) 2^-53 sum_{h in group} sum_{a,b in D} A_h[a,b] / (n_texts 2048):
            the kernel's entry-wise bound (the fold over the batches of a layer is one chain of n_texts additions), one rounding of
            the normaliser, and mdg_qk_rank_curve's own summation bound; |P_ab| <= A_ab
  OVER_FULL over_full = error / (the seq entry's error) exactly, when MODEGPT_QK_SEQ=1 runs beside it; absent without it
  SELECT    MODEGPT_QK_CAUSAL_SELECT=1: the masks are ops.qk_select's on (P^c, ones); metrics["qk_selection"] says
            within_sequence_causal with no certificate; the checkpoint loads through the shipped modeling file
  CACHE     save, then load with no forward pass: the same statistic bits, masks and report; a record without the entries is refused
  OFF       switches unset: ops.qk_causal_accum is never called, no file, no metric; switching it on changes no other bit
"""
import contextlib
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import qk_causal_model as C
from tests.test_gpu_qk_pair_e2e import N_TEXTS, SEQ, adapter_for, artefacts, calibrate, compress, dropped, same, spied_calibration, tiny

pytestmark = pytest.mark.gpu
LD, U = C.LD, C.U
SWITCHES = ("MODEGPT_QK_ROPE", "MODEGPT_QK_ROPE_SELECT", "MODEGPT_QK_ERROR", "MODEGPT_QK_SEQ", "MODEGPT_QK_SEQ_SELECT", "MODEGPT_QK_CAUSAL",
            "MODEGPT_QK_CAUSAL_SELECT")


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def env(**switches):
    """The switches exactly as given (absent = unset), restored afterwards.  (spied_calibration's own env() clears and sets the
    five older switches; the causal ones are handled here, around it.)"""
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


@pytest.fixture(scope="module")
def model(dev):
    return tiny(dev)


def count_calls(ops, monkeypatch):
    calls = []
    real = ops.qk_causal_accum
    monkeypatch.setattr(ops, "qk_causal_accum", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    return calls


# ---------------------------------------------------------------- the report against the brute-force sums, through the hooks
@pytest.mark.parametrize("kind,over", [("llama", {}), ("llama", {"num_key_value_heads": 4}), ("qwen2", {})])
def test_report_equals_the_brute_force_causal_sums(ops, dev, tmp_path, monkeypatch, kind, over):
    import importlib
    module = importlib.import_module("transformers.models.%s.modeling_%s" % (kind, kind))
    ad = adapter_for(tiny(dev, kind, **over), dev, tmp_path / "layers")
    with env(QK_CAUSAL="1"):                                    # (the spy's env sets the older three inside)
        calibs, rows = spied_calibration(monkeypatch, module, ad, QK_ROPE="1", QK_SEQ="1", QK_ERROR="1")
    assert ad.qk_causal_stats is not None and getattr(ad, "qk_causal_sums", None) is None
    with env(QK_ROPE="1", QK_SEQ="1", QK_CAUSAL="1", QK_ERROR="1"):
        masks, rank = compress(ad, calibs)
        ad.report_qk_errors()
    H, KV, hd = ad.n_heads, ad.n_kv_heads, ad.head_dim
    g, ns, m = H // KV, hd // 2, rank // 2
    s1 = LD(N_TEXTS) * LD(2048)
    c = (4 * SEQ + N_TEXTS + 8) + 1 + (g * hd * hd + 2)
    report = ad.metrics["qk_logit_error_causal"]
    json.dumps(report, allow_nan=False)
    assert sorted(report) == ["0", "1"]
    worst = 0.0
    for l in range(ad.n_layers):
        q, k = rows[l]
        P, R, A = C.longdouble_causal(q, k, N_TEXTS, SEQ, H, KV, hd)
        # the collected statistic itself, entry-wise (the fold over the two batches is one chain) and symmetric to the bit
        for got, ref in ((ad.qk_causal_stats[0][l], P), (ad.qk_causal_stats[1][l], R)):
            assert same(got, got.transpose(1, 2))
            err = np.abs(got.cpu().numpy().astype(LD) - ref / s1)
            assert bool((err <= (4 * SEQ + N_TEXTS + 9) * U * A / s1).all())
        order = ad.qk_errors_causal[l][6]
        assert torch.equal(order, ad.qk_errors[l][6]) and torch.equal(order, ad.qk_errors_seq[l][6])        # the same order everywhere
        e, seq = report[str(l)], ad.metrics["qk_logit_error_seq"][str(l)]
        assert e["statistic"] == "within_sequence_causal" and e["rank"] == rank and len(e["heads"]) == KV
        for kv in range(KV):
            D = dropped(order[kv].tolist(), m, ns)
            var, ms = C.brute_force_causal(q, k, N_TEXTS, SEQ, H, KV, hd, D)
            grp = slice(kv * g, (kv + 1) * g)
            tol = c * U * sum(A[h][np.ix_(D, D)].sum() for h in range(kv * g, (kv + 1) * g)) / s1
            head = e["heads"][kv]
            for name, got, want in (("error", head["error"], var[grp].sum() / s1), ("raw_error", head["raw_error"], ms[grp].sum() / s1)):
                err = abs(LD(got) - want)
                assert err <= tol, ("IDENTITY", kind, l, kv, name, float(err), float(tol))
                worst = max(worst, float(err / tol))
            assert 0.0 <= head["shift_share"] <= 1.0
            assert head["shift_share"] == 1.0 - head["error"] / head["raw_error"]
            assert head["over_full"] == head["error"] / seq["heads"][kv]["error"]
        assert e["shift_share"] == 1.0 - e["error"] / e["raw_error"] and e["over_full"] == e["error"] / seq["error"]
        print("E2E %s %s layer %d (random weights): over_full %.4f shift_share %.4f" % (kind, over, l, e["over_full"], e["shift_share"]))
    print("IDENTITY %s %s: largest |report - brute force| / bound = %.3e" % (kind, over, worst))


# ---------------------------------------------------------------- switches off / on
def test_switch_off_launches_nothing_and_on_changes_no_other_bit(ops, dev, model, tmp_path, monkeypatch):
    calls = count_calls(ops, monkeypatch)
    off = adapter_for(model, dev, tmp_path / "off")
    stats_off = str(tmp_path / "stats_off")
    with env(QK_ROPE="1", QK_SEQ="1", QK_ERROR="1"):
        c_off = calibrate(off, calibs_save_path=stats_off)
        m_off, rank = compress(off, c_off)
        off.report_qk_errors()
        off.report_attention_margins()
    assert not calls, "ops.qk_causal_accum ran with MODEGPT_QK_CAUSAL unset"
    assert off.qk_causal_stats is None and "qk_logit_error_causal" not in off.metrics
    assert not any("qk_causal" in name for name in os.listdir(stats_off))
    assert sorted(json.load(open(os.path.join(stats_off, "layer_0.json")))["files"]) == \
        ["k", "k_rope", "mlp", "q", "q_rope", "qk_pair", "qk_pair_raw", "x"]
    on = adapter_for(model, dev, tmp_path / "on")
    with env(QK_ROPE="1", QK_SEQ="1", QK_CAUSAL="1", QK_ERROR="1"):
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
        assert all(same(x, y) for x, y in zip(off.qk_pair_stats[i], on.qk_pair_stats[i]))
    assert all(torch.equal(a, b) for a, b in zip(m_off, m_on))
    for a, b in zip(artefacts(tmp_path / "off", 2), artefacts(tmp_path / "on", 2)):
        assert sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    assert sorted(set(on.metrics) - set(off.metrics)) == ["qk_logit_error_causal"]
    for key in off.metrics:
        assert json.dumps(off.metrics[key], sort_keys=True) == json.dumps(on.metrics[key], sort_keys=True), key
    # independent of MODEGPT_QK_SEQ: without it the same causal statistic bits, and a report without over_full
    alone = adapter_for(model, dev, tmp_path / "alone")
    with env(QK_ROPE="1", QK_CAUSAL="1", QK_ERROR="1"):
        c_alone = calibrate(alone)
        compress(alone, c_alone)
        alone.report_qk_errors()
    assert alone.qk_pair_stats is None and "qk_logit_error_seq" not in alone.metrics
    for i in (0, 1):
        assert all(same(x, y) for x, y in zip(alone.qk_causal_stats[i], on.qk_causal_stats[i]))
    for l in ("0", "1"):
        e = alone.metrics["qk_logit_error_causal"][l]
        assert "over_full" not in e and e["error"] == on.metrics["qk_logit_error_causal"][l]["error"]


def test_causal_without_rope_raises_before_the_first_forward(dev, model, tmp_path):
    ad = adapter_for(model, dev, tmp_path / "layers")
    fired = []
    hook = model.register_forward_pre_hook(lambda *args: fired.append(1))
    try:
        with env(QK_CAUSAL="1"):
            with pytest.raises(RuntimeError, match="MODEGPT_QK_CAUSAL=1 needs MODEGPT_QK_ROPE=1"):
                calibrate(ad)
    finally:
        hook.remove()
    assert not fired


@pytest.mark.parametrize("kind", ["qwen3", "opt"])
def test_other_architectures_collect_nothing_and_say_why(ops, dev, kind, tmp_path, monkeypatch, caplog):
    calls = count_calls(ops, monkeypatch)
    ad = adapter_for(tiny(dev, kind), dev, tmp_path / "layers")
    stats = str(tmp_path / "stats")
    with env(QK_CAUSAL="1"), caplog.at_level(logging.INFO, logger="MoDeGPT"):
        calibrate(ad, calibs_save_path=stats)
    assert not calls and ad.qk_causal_stats is None
    assert not any("qk_causal" in name for name in os.listdir(stats))
    said = [r for r in caplog.records if "MODEGPT_QK_CAUSAL=1" in r.getMessage()]
    assert len(said) == 1 and said[0].levelno == (logging.WARNING if kind == "qwen3" else logging.INFO)


# ---------------------------------------------------------------- cache
def test_cache_round_trip_and_refusal(ops, dev, model, tmp_path):
    stats_on, stats_off = str(tmp_path / "stats_on"), str(tmp_path / "stats_off")
    a = adapter_for(model, dev, tmp_path / "a")
    with env(QK_ROPE="1", QK_CAUSAL="1", QK_ERROR="1"):
        ca = calibrate(a, calibs_save_path=stats_on)
        ma, _ = compress(a, ca)
        a.report_qk_errors()
    for l in range(a.n_layers):
        meta = json.load(open(os.path.join(stats_on, f"layer_{l}.json")))
        for kind in ("qk_causal", "qk_causal_raw"):
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
        with env(QK_ROPE="1", QK_CAUSAL="1", QK_ERROR="1"):
            cb = calibrate(b, load_calibs_from=stats_on)
            mb, _ = compress(b, cb)
            b.report_qk_errors()
        for i in (0, 1):
            assert all(same(x, y) for x, y in zip(a.qk_causal_stats[i], b.qk_causal_stats[i]))
        assert all(torch.equal(x, y) for x, y in zip(ma, mb))
        assert a.metrics["qk_logit_error_causal"] == b.metrics["qk_logit_error_causal"]
        d = adapter_for(model, dev, tmp_path / "d")
        with env(QK_ROPE="1", QK_CAUSAL="1"):
            with pytest.raises(ValueError, match=r"layer 0.*qk_causal.*MODEGPT_QK_CAUSAL=1"):
                calibrate(d, load_calibs_from=stats_off)
        with env(QK_ROPE="1"):                                               # a record WITH the entries, loaded without the switch
            e = adapter_for(model, dev, tmp_path / "e")
            ce = calibrate(e, load_calibs_from=stats_on)
            assert e.qk_causal_stats is None and all(same(p, q) for p, q in zip(ca[1], ce[1]))
        assert not fired, "the model ran"
    finally:
        hook.remove()


# ---------------------------------------------------------------- MODEGPT_QK_CAUSAL_SELECT=1
def test_selection_on_the_causal_statistic(ops, dev, tmp_path):
    import transformers
    from modegpt_amd.compression import compress_qk as CQ
    from modegpt_amd.compression.compress_mlp import compress_nystrom
    from modegpt_amd.compression.compress_vo import compress_vo
    from modegpt_amd.model_utils import save_compressed_model
    ad = adapter_for(tiny(dev), dev, tmp_path / "layers")          # (its own model: convert_model rebuilds it in place)
    layers, keep = list(range(ad.n_layers)), [0.5] * ad.n_layers
    KV, hd = ad.n_kv_heads, ad.head_dim
    ns = hd // 2
    with env(QK_ROPE="1", QK_CAUSAL_SELECT="1"):
        c0 = calibrate(ad)
        with pytest.raises(RuntimeError, match="MODEGPT_QK_CAUSAL_SELECT=1.*MODEGPT_QK_CAUSAL=1"):
            compress(ad, c0)
    with env(QK_ROPE="1", QK_SEQ="1", QK_CAUSAL="1", QK_CAUSAL_SELECT="1", QK_SEQ_SELECT="1"):
        c = calibrate(ad)
        with pytest.raises(RuntimeError, match="MODEGPT_QK_CAUSAL_SELECT=1 and MODEGPT_QK_SEQ_SELECT=1 are both set"):
            compress(ad, c)
    with env(QK_ROPE="1", QK_SEQ="1", QK_CAUSAL="1", QK_CAUSAL_SELECT="1", QK_ROPE_SELECT="1"):
        with pytest.raises(RuntimeError, match="MODEGPT_QK_CAUSAL_SELECT=1 and MODEGPT_QK_ROPE_SELECT=1 are both set"):
            compress(ad, c)
    with env(QK_ROPE="1", QK_SEQ="1", QK_CAUSAL="1", QK_CAUSAL_SELECT="1", QK_ERROR="1"):
        compress_nystrom(ad, c[0], keep, layers)
        masks = CQ.compress_qk(ad, (c[1], c[2]), keep, target_layers=layers)
        compress_vo(ad, c[3], keep, target_layers=layers)
        ad.report_qk_errors()
        ad.report_attention_margins()
    rank = CQ.qk_rank_rule(hd, 0.5, ad.arch)
    mode = CQ.qk_mode_and_ridges(ad.arch, True, ad.config.ridge_qk)[0]
    ones = torch.ones(KV, hd, hd, dtype=torch.float64, device=dev)
    for l in layers:
        P = ad.qk_causal_stats[0][l]
        assert torch.equal(masks[l], ops.qk_select(P, ones, rank, mode, 0.0, 0.0)[0])
        assert torch.equal(ad.qk_errors_causal[l][6], ops.qk_select(P, ones, hd, mode, 0.0, 0.0)[0][:, :ns].cpu())
        sel = ad.metrics["qk_selection"][str(l)]
        assert sel["statistic"] == "within_sequence_causal" and sel["certificate"] is None and sel["certified"] is None
        assert "heads" not in sel
    json.dumps(ad.metrics["qk_selection"], allow_nan=False)
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
