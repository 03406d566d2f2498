"""MODEGPT_QK_ROPE=1 -- the post-RoPE statistics sigma_q', sigma_k' (ops.rope_rows into ops.cov_accum_multi), the report on them
(metrics["qk_logit_error_rope"]), the cache entries and MODEGPT_QK_ROPE_SELECT=1.

Criteria (a priori; nothing here is fitted to what the kernels give, every test prints the share of its bound it used under -s):
  LATTICE   lattice rows and quarter-turn tables: every product and every partial sum is exact in fp64 -> bit equality with
            cov_ref.exact_cov of the CPU-rotated rows, also for a second call accumulating onto the first
  GENERIC   |sigma' - long double| <= tokens 2^-53 sqrt(sigma_ii sigma_jj) (1 + 1e-3): fp64 sums of exact products
            (tests/test_gpu_cov.py::test_rounding_bound)
  IDENTITY  curve_h[h][m] of ops.qk_rank_curve on the collected statistics against sum_i sum_j delta_ij^2 / s^2 in long double from
            the rows modeling_llama.apply_rotary_pos_emb itself returned (a spy: independent of the hook plumbing), within
            (hd^2 + 2) 2^-53 A_h  +  (2 nu + nu^2) (sum_{a in D} sqrt(sigma_q'_aa sigma_k'_aa))^2,  nu = (N + 4) 2^-53:
            the header's curve bound plus what the statistics' own rounding (|sigma'_ab - exact| <= nu sqrt(sigma'_aa sigma'_bb), N
            tokens and the normaliser) can move a product sigma_q'_ab sigma_k'_ab, summed over D x D.

MEASURED on an MI355X: LATTICE bit-equal at hd 16 and 128; GENERIC 0.033 (bf16, hd 128, 4 heads), 0.052 (bf16, hd 16, 2 heads), 0.025
(f16, hd 64, 3 heads) of the bound; IDENTITY largest error / bound 5.6e-3 over both layers, all heads and ranks, the pre-RoPE statistic
misses the brute-force value by up to 1.1e-1 relative (8.5e-2 on the CPU); REPORT at keep 0.5: post-RoPE relative_error 4.74e-1 / 4.82e-1
(layers 0 / 1) beside pre-RoPE 4.78e-1 / 4.63e-1; SELECT at keep 0.5 the post-RoPE selection equals the pre-RoPE one on this model."""
import contextlib
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import cov_ref as CR
from tests import qk_error_model as QK
from tests import rope_rows_ref as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
LD, U = QK.LD, QK.U
N_TEXTS, SEQ, SEED = 3, 24, 0
SWITCHES = ("MODEGPT_QK_ROPE", "MODEGPT_QK_ROPE_SELECT", "MODEGPT_QK_ERROR")


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def env(**switches):
    """The three switches exactly as given (absent = unset), restored afterwards."""
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


# ---------------------------------------------------------------- a. exact lattice
@pytest.mark.parametrize("hd", [16, 128])
def test_lattice_rows_give_the_exact_statistic_bit_for_bit(ops, dev, hd):
    n_heads, n_kv, tokens = 4, 2, 53
    for heads, seed in ((n_heads, 11), (n_kv, 12)):
        x1, cos, sin = R.lattice_case(hd, heads, tokens, seed + hd)
        x2 = R.lattice_case(hd, heads, tokens, seed + hd + 100)[0]
        r1, r2 = (R.rope_rows(x, cos, sin, heads, hd) for x in (x1, x2))
        # every rotated value is +- a lattice value: the rotation itself is a permutation with signs
        assert torch.equal(r1.float().abs().reshape(-1, hd).sort(-1).values, x1.float().abs().reshape(-1, hd).sort(-1).values)
        sigma = torch.zeros(heads, hd, hd, dtype=F64, device=dev)
        want = None
        for x, r in ((x1, r1), (x2, r2)):                                   # the second call accumulates onto the first
            got_rows = ops.rope_rows(x.to(dev), cos.to(dev), sin.to(dev), heads, hd, out=ops.rope_scratch(x.to(dev), "q"))
            assert R.same_bits(got_rows.cpu(), r)
            ops.cov_accum_multi([(sigma, got_rows, heads)])
            want = CR.exact_cov(r.reshape(tokens, heads * hd), heads=heads, sigma0=want)
            low = torch.tril(torch.ones(hd, hd, dtype=torch.bool))
            assert torch.equal(bits(sigma)[:, low], bits(want)[:, low]), "LATTICE hd %d heads %d" % (hd, heads)
        ops.cov_finalize(sigma, 1.0)
        assert same(sigma, want)
    print("LATTICE hd %d: sigma' equals the exact statistic bit for bit, two accumulating calls, 4 and 2 heads" % hd)


# ---------------------------------------------------------------- b. generic data
@pytest.mark.parametrize("dt,hd,heads", [("bf16", 128, 4), ("bf16", 16, 2), ("f16", 64, 3)])
def test_generic_rows_within_the_fp64_rounding_bound(ops, dev, dt, hd, heads):
    B, T = 2, 70
    c = R.make_case(dt, hd, heads, B, T, "shared")
    tokens = B * T
    sigma = torch.zeros(heads, hd, hd, dtype=F64, device=dev)
    x = c.x.to(dev)
    rows = ops.rope_rows(x, c.cos.to(dev), c.sin.to(dev), heads, hd, out=ops.rope_scratch(x, "k"))
    ops.cov_accum_multi([(sigma, rows, heads)])
    got = sigma.cpu().numpy().astype(LD)
    ref, scale = CR.longdouble_cov(c.want.reshape(tokens, heads * hd), heads=heads)
    bound = tokens * U * scale * (1 + 1e-3)
    il = np.tril_indices(hd)
    live = bound[:, il[0], il[1]] > 0
    frac = (np.abs(got - ref)[:, il[0], il[1]][live] / bound[:, il[0], il[1]][live])
    print("GENERIC %s hd %d heads %d: max |sigma' - long double| / bound = %.4f" % (dt, hd, heads, float(frac.max())))
    assert float(frac.max()) <= 1.0
    assert bool((np.abs(got - ref)[:, il[0], il[1]][~live] == 0).all())


# ---------------------------------------------------------------- the tiny Llama of c .. g
def tiny_llama(dev, kind="llama"):
    import transformers
    torch.manual_seed(SEED)
    kw = dict(hidden_size=64, intermediate_size=160, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=16,
              vocab_size=211, max_position_embeddings=64)
    if kind == "qwen3":
        m = transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**kw))
    elif kind == "opt":
        m = transformers.OPTForCausalLM(transformers.OPTConfig(hidden_size=64, ffn_dim=160, num_hidden_layers=2, num_attention_heads=4,
                                                               vocab_size=211, max_position_embeddings=64, word_embed_proj_dim=64))
    else:
        m = transformers.LlamaForCausalLM(transformers.LlamaConfig(**kw))
    return m.to(dev).to(torch.bfloat16).eval()


def adapter_for(model, dev, store):
    """A fresh adapter with the three texts of 24 tokens in batches of 2 + 1 (the last batch is ragged) already in place."""
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    ad = ModelAdapter.from_model(model, None)
    ad.config = CompressionConfig(temp_storage_dir=str(store), nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5, dataset="synthetic",
                                  calib_size=N_TEXTS, calibs_batch_size=2, compression_ratio=0.3, order="mlp,qk,vo")
    ids = torch.randint(0, 211, (N_TEXTS, SEQ), generator=torch.Generator().manual_seed(SEED + 1)).to(dev)
    ad.calibs = [ids[:2], ids[2:]]
    return ad


def calibrate(ad, **kw):
    from modegpt_amd.calibration import load_calibs
    return load_calibs(ad, n_samples=N_TEXTS, batch_size=2, dataset="synthetic", target_layers=[], **kw)


def compress(ad, calibs, keep=0.5):
    """compress_qk layer by layer, keeping every layer's mask."""
    from modegpt_amd.compression import compress_qk as CQ
    rank = CQ.qk_rank_rule(ad.head_dim, keep, ad.arch)
    return [CQ.compress_layer(ad, l, rank, cov_q_list=calibs[1][l], cov_k_list=calibs[2][l], rotary_masks=[]).cpu()
            for l in range(ad.n_layers)], rank


def artefacts(store, n_layers):
    return [torch.load(os.path.join(str(store), f"layer_{l}_qk"), map_location="cpu") for l in range(n_layers)]


@pytest.fixture(scope="module")
def model(dev):
    return tiny_llama(dev)


# ---------------------------------------------------------------- c. the identity, through the hooks
def test_identity_against_the_brute_force_double_sum(ops, dev, model, tmp_path, monkeypatch):
    from transformers.models.llama import modeling_llama as ML
    from modegpt_amd.compression import compress_qk as CQ
    seen = []
    real = ML.apply_rotary_pos_emb

    def spy(q, k, cos, sin, *a, **kw):
        out = real(q, k, cos, sin, *a, **kw)
        seen.append(tuple(t.detach().cpu() for t in out))                   # ([B, H, T, hd], [B, KV, T, hd]) per layer and batch
        return out
    monkeypatch.setattr(ML, "apply_rotary_pos_emb", spy)
    ad = adapter_for(model, dev, tmp_path / "layers")
    with env(QK_ROPE="1"):
        calibs = calibrate(ad)
    monkeypatch.setattr(ML, "apply_rotary_pos_emb", real)
    L, H, KV, hd = ad.n_layers, ad.n_heads, ad.n_kv_heads, ad.head_dim
    assert len(seen) == 2 * L and ad.qk_rope_stats is not None and getattr(ad, "qk_rope_sums", None) is None
    g, ns, N = H // KV, hd // 2, N_TEXTS * SEQ
    s = LD(N_TEXTS * 2048)
    mode, rq, rk = CQ.qk_mode_and_ridges(ad.arch, KV != H, ad.config.ridge_qk)
    nu = LD((N + 4) * U)
    worst, pre_miss = 0.0, 0.0
    for l in range(L):
        rows = lambda i: torch.cat([seen[b * L + l][i].transpose(1, 2).reshape(-1, seen[b * L + l][i].shape[1], hd)       # noqa: E731
                                    for b in range(2)]).double().numpy().astype(LD)
        qr, kr = rows(0), rows(1)                                           # [N, H, hd], [N, KV, hd]
        assert qr.shape == (N, H, hd) and kr.shape == (N, KV, hd)
        sq, sk = ad.qk_rope_stats[0][l], ad.qk_rope_stats[1][l]
        assert same(sq, sq.transpose(1, 2)) and same(sk, sk.transpose(1, 2))          # finalised: mirrored
        order = ops.qk_select(calibs[1][l], calibs[2][l], hd, mode, rq, rk)[0][:, :ns].contiguous()
        curve_h = ops.qk_rank_curve(sq, sk, mode, 0.0, 0.0, order)[0].cpu().numpy().astype(LD)
        pre_h = ops.qk_rank_curve(calibs[1][l], calibs[2][l], mode, 0.0, 0.0, order)[0].cpu().numpy().astype(LD)
        o = order.cpu().numpy()
        A_h = QK.model(sq.cpu().numpy(), sk.cpu().numpy(), mode, 0.0, 0.0, o)["A_h"]
        for h in range(H):
            kv = h // g
            dq = (qr[:, h] ** 2).sum(0) / s                                  # the exact diagonals of sigma_q'[h], sigma_k'[kv]
            dk = (kr[:, kv] ** 2).sum(0) / s
            for m in range(ns + 1):
                units = o[kv][m:]
                D = np.concatenate([units, units + ns]).astype(np.int64)
                delta = qr[:, h][:, D] @ kr[:, kv][:, D].T                   # [N, N]: every token pair, causal or not, across texts
                brute = (delta ** 2).sum() / (s * s)
                tol = (hd * hd + 2) * U * A_h[h][m] + (2 * nu + nu * nu) * np.sqrt(dq[D] * dk[D]).sum() ** 2
                err = abs(curve_h[h][m] - brute)
                assert err <= tol, ("IDENTITY", l, h, m, float(err), float(tol))
                worst = max(worst, float(err / tol) if tol > 0 else 0.0)
                if brute > 0:
                    pre_miss = max(pre_miss, float(abs(pre_h[h][m] - brute) / brute))
    print("IDENTITY post-RoPE curve against the brute-force double sum: largest error / bound %.3e; the pre-RoPE statistic misses it "
          "by up to %.3e relative" % (worst, pre_miss))
    # a condition on the inputs (seed): the rotation matters here, the pre-RoPE figure is NOT the logit error
    assert pre_miss > 1e-6


# ---------------------------------------------------------------- d, e. the switch off; on or off, the same bits elsewhere
def test_switch_off_launches_and_reports_nothing_and_on_changes_no_other_bit(ops, dev, model, tmp_path, monkeypatch):
    calls = []
    real = ops.rope_rows
    monkeypatch.setattr(ops, "rope_rows", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    off = adapter_for(model, dev, tmp_path / "off")
    with env(QK_ERROR="1"):
        c_off = calibrate(off)
        m_off, rank = compress(off, c_off)
        off.report_qk_errors()
        off.report_attention_margins()
    assert not calls, "ops.rope_rows ran with the switch unset"
    assert off.qk_rope_stats is None and "qk_logit_error_rope" not in off.metrics
    assert all("statistic" not in v for v in off.metrics["qk_selection"].values())
    on = adapter_for(model, dev, tmp_path / "on")
    with env(QK_ROPE="1", QK_ERROR="1"):
        c_on = calibrate(on)
        assert len(calls) == 2 * 2 * on.n_layers                            # q and k, per layer and batch
        m_on, _ = compress(on, c_on)
        on.report_qk_errors()
        on.report_attention_margins()
    for a, b in zip(c_off[:4], c_on[:4]):
        assert all(same(x, y) for x, y in zip(a, b))
    assert c_off[4] == c_on[4]
    assert all(torch.equal(a, b) for a, b in zip(m_off, m_on))
    for a, b in zip(artefacts(tmp_path / "off", 2), artefacts(tmp_path / "on", 2)):
        assert sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    assert json.dumps(off.metrics["qk_logit_error"], sort_keys=True) == json.dumps(on.metrics["qk_logit_error"], sort_keys=True)
    # ... and the new report: the unchanged decoder's entry plus the two fields, the pre-RoPE figure being the sibling's
    rope = on.metrics["qk_logit_error_rope"]
    json.dumps(rope, allow_nan=False)
    assert sorted(rope) == ["0", "1"]
    for l, e in rope.items():
        sib = on.metrics["qk_logit_error"][l]
        assert e["statistic"] == "post_rope" and e["pre_rope_relative_error"] == sib["relative_error"]
        assert sorted(set(e) - {"statistic", "pre_rope_relative_error"}) == sorted(sib) and e["rank"] == rank
        assert 0.0 < e["relative_error"] < 1.0 and e["relative_error"] != sib["relative_error"]
        host = on.qk_errors_rope[int(l)]
        assert len(host) == 7 and torch.equal(host[6], on.qk_errors[int(l)][6])          # the same order as the existing report
        print("REPORT layer %s: post-RoPE relative_error %.3e, pre-RoPE %.3e" % (l, e["relative_error"], sib["relative_error"]))
    assert all(v["statistic"] == "pre_rope" for v in on.metrics["qk_selection"].values())


# ---------------------------------------------------------------- f. cache
def test_cache_round_trip_and_refusals(ops, dev, model, tmp_path):
    stats_on, stats_off = str(tmp_path / "stats_on"), str(tmp_path / "stats_off")
    a = adapter_for(model, dev, tmp_path / "a")
    with env(QK_ROPE="1", QK_ERROR="1"):
        ca = calibrate(a, calibs_save_path=stats_on)
        ma, _ = compress(a, ca)
        a.report_qk_errors()
    for l in range(a.n_layers):
        meta = json.load(open(os.path.join(stats_on, f"layer_{l}.json")))
        for kind, like in (("q_rope", "q"), ("k_rope", "k")):
            assert os.path.getsize(os.path.join(stats_on, f"layer_{l}_{kind}.f64")) == meta["files"][kind]["bytes"]
            assert sorted(meta["files"][kind]) == sorted(meta["files"][like])
            assert {k: meta["files"][kind][k] for k in ("n", "batch", "bytes", "layout")} == \
                {k: meta["files"][like][k] for k in ("n", "batch", "bytes", "layout")}
    c = adapter_for(model, dev, tmp_path / "c")          # ... and a record saved without the switch (the last forward pass of this test)
    with env():
        cc = calibrate(c, calibs_save_path=stats_off)
    b = adapter_for(model, dev, tmp_path / "b")
    fired = []
    hook = model.register_forward_pre_hook(lambda *args: fired.append(1))
    try:
        with env(QK_ROPE="1", QK_ERROR="1"):
            cb = calibrate(b, load_calibs_from=stats_on)
            mb, _ = compress(b, cb)
            b.report_qk_errors()
        assert not fired, "the model ran"
        for i in (0, 1):
            assert all(same(x, y) for x, y in zip(a.qk_rope_stats[i], b.qk_rope_stats[i]))
        assert all(torch.equal(x, y) for x, y in zip(ma, mb))
        assert a.metrics["qk_logit_error_rope"] == b.metrics["qk_logit_error_rope"]
        # a record saved without the switch: refused with it (never recalibrated), loaded as always without it
        assert not any("rope" in name for name in os.listdir(stats_off))
        for l in range(c.n_layers):          # ... and its sidecars name no such entry: byte for byte what a run before the switch wrote
            assert sorted(json.load(open(os.path.join(stats_off, f"layer_{l}.json")))["files"]) == ["k", "mlp", "q", "x"]
        d = adapter_for(model, dev, tmp_path / "d")
        with env(QK_ROPE="1"):
            with pytest.raises(ValueError, match=r"layer 0.*q_rope"):
                calibrate(d, load_calibs_from=stats_off)
        with env():
            cd = calibrate(d, load_calibs_from=stats_off)
            assert d.qk_rope_stats is None
            for x, y in zip(cc[:4], cd[:4]):
                assert all(same(p, q) for p, q in zip(x, y))
            # a record WITH the entries, loaded without the switch: they are ignored
            e = adapter_for(model, dev, tmp_path / "e")
            ce = calibrate(e, load_calibs_from=stats_on)
            assert e.qk_rope_stats is None and all(same(p, q) for p, q in zip(ca[1], ce[1]))
        assert not fired, "the model ran"
    finally:
        hook.remove()


# ---------------------------------------------------------------- g. MODEGPT_QK_ROPE_SELECT=1
def test_selection_on_the_rope_statistics(ops, dev, tmp_path):
    import transformers
    from modegpt_amd.compression import compress_qk as CQ
    from modegpt_amd.compression.compress_mlp import compress_nystrom
    from modegpt_amd.compression.compress_vo import compress_vo
    from modegpt_amd.model_utils import save_compressed_model
    own = tiny_llama(dev)                                                   # convert_model below rebuilds it in place
    ad = adapter_for(own, dev, tmp_path / "layers")
    layers = list(range(ad.n_layers))
    keep = [0.5] * ad.n_layers
    with env(QK_ROPE_SELECT="1"):
        c0 = calibrate(ad)
        with pytest.raises(RuntimeError, match="MODEGPT_QK_ROPE_SELECT=1.*MODEGPT_QK_ROPE=1"):
            compress(ad, c0)
    with env(QK_ROPE="1", QK_ROPE_SELECT="1", QK_ERROR="1"):
        c = calibrate(ad)
        compress_nystrom(ad, c[0], keep, layers)
        masks = CQ.compress_qk(ad, (c[1], c[2]), keep, target_layers=layers)
        compress_vo(ad, c[3], keep, target_layers=layers)
        ad.report_qk_errors()
        ad.report_attention_margins()
    mode, rq, rk = CQ.qk_mode_and_ridges(ad.arch, True, ad.config.ridge_qk)
    rank = CQ.qk_rank_rule(ad.head_dim, keep[0], ad.arch)
    differs = False
    for l in layers:
        direct = ops.qk_select(ad.qk_rope_stats[0][l], ad.qk_rope_stats[1][l], rank, mode, rq, rk)
        assert torch.equal(masks[l], direct[0])
        art = artefacts(tmp_path / "layers", ad.n_layers)[l]
        differs |= not torch.equal(masks[l], ops.qk_select(c[1][l], c[2][l], rank, mode, rq, rk)[0])
        assert ad.metrics["qk_selection"][str(l)]["statistic"] == "post_rope"
        # the report's order is the rope statistics' order too
        ns = ad.head_dim // 2
        assert torch.equal(ad.qk_errors[l][6], ops.qk_select(ad.qk_rope_stats[0][l], ad.qk_rope_stats[1][l], ad.head_dim, mode, rq, rk)[0][:, :ns].cpu())
        assert art["q_proj"].shape == (ad.n_heads * rank, ad.d_model) and art["k_proj"].shape == (ad.n_kv_heads * rank, ad.d_model)
    print("SELECT the post-RoPE selection %s the pre-RoPE one on this model" % ("differs from" if differs else "equals"))
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


# ---------------------------------------------------------------- h. other architectures
@pytest.mark.parametrize("kind", ["qwen3", "opt"])
def test_other_architectures_collect_nothing(ops, dev, kind, tmp_path, monkeypatch, caplog):
    calls = []
    real = ops.rope_rows
    monkeypatch.setattr(ops, "rope_rows", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    ad = adapter_for(tiny_llama(dev, kind), dev, tmp_path / "layers")
    stats = str(tmp_path / "stats")
    with env(QK_ROPE="1"), caplog.at_level(logging.INFO, logger="MoDeGPT"):
        calibrate(ad, calibs_save_path=stats)
    assert not calls and ad.qk_rope_stats is None
    assert not any("rope" in name for name in os.listdir(stats))
    said = [r for r in caplog.records if "MODEGPT_QK_ROPE=1" in r.getMessage()]
    assert len(said) == 1 and said[0].levelno == (logging.WARNING if kind == "qwen3" else logging.INFO)
