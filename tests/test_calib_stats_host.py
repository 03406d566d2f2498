"""CPU: the table of optional calibration statistics (modegpt_amd/calib_stats.py) and what is derived from it -- the records
themselves, calib_cache's kind constants, the collection rules of calibration.py with their messages, the per-layer fetch the
hooks and compress_qk share, and a saved record of all five statistics, entry by entry.  Every expected value is a literal."""
import logging
import re
from types import SimpleNamespace

import numpy as np
import pytest

from modegpt_amd import calib_cache as cc
from modegpt_amd import calib_stats as cs

Q_ARCHS = ("llama", "qwen2")
# name: (switch, members, layout, sums_attr, stats_attr, needs, archs, entry, mirror, token_power, noun)
TABLE = {
    "mlp_mean": ("MODEGPT_MLP_INTERCEPT", (("mlp_mean", "n_inner"),), "vector", "mlp_sums", "mlp_means", None, None, None, False, 1,
                 "activation means"),
    "x_mean": ("MODEGPT_VO_INTERCEPT", (("x_mean", "d_model"),), "vector", "x_sums", "x_means", None, None, None, False, 1, "input means"),
    "qk_rope": ("MODEGPT_QK_ROPE", (("q_rope", "q"), ("k_rope", "k")), "full", "qk_rope_sums", "qk_rope_stats", None, Q_ARCHS, None, True, 1,
                "post-RoPE statistics"),
    "qk_pair": ("MODEGPT_QK_SEQ", (("qk_pair", "q"), ("qk_pair_raw", "q")), "full", "qk_pair_sums", "qk_pair_stats", "qk_rope", Q_ARCHS,
                "mdg_qk_pair_accum", False, 2, "within-sequence statistic"),
    "qk_causal": ("MODEGPT_QK_CAUSAL", (("qk_causal", "q"), ("qk_causal_raw", "q")), "full", "qk_causal_sums", "qk_causal_stats", "qk_rope",
                  Q_ARCHS, "mdg_qk_causal_accum", False, 1, "causal statistic"),
}


def test_the_table_is_the_five_statistics_in_order():
    assert tuple(s.name for s in cs.STATS) == ("mlp_mean", "x_mean", "qk_rope", "qk_pair", "qk_causal") == tuple(cs.BY_NAME)
    for s in cs.STATS:
        assert (s.switch, s.members, s.layout, s.sums_attr, s.stats_attr, s.needs, s.archs, s.entry, s.mirror, s.token_power,
                s.noun) == TABLE[s.name], s.name
    assert tuple(cs.KIND_STAT) == ("mlp_mean", "x_mean", "q_rope", "k_rope", "qk_pair", "qk_pair_raw", "qk_causal", "qk_causal_raw")
    assert cs.KIND_STAT["k_rope"] is cs.BY_NAME["qk_rope"] and cs.KIND_SHAPE["k_rope"] == "k"


def test_the_switch_is_read_when_asked(monkeypatch):
    for s in cs.STATS:
        monkeypatch.delenv(s.switch, raising=False)
        assert s.enabled() is False
        monkeypatch.setenv(s.switch, "1")
        assert s.enabled() is True
        monkeypatch.setenv(s.switch, "0")
        assert s.enabled() is False


def test_the_constants_calib_cache_derives():
    assert cc.ROPE_KINDS == {"q_rope": "q", "k_rope": "k"} and tuple(cc.ROPE_KINDS) == ("q_rope", "k_rope")
    assert cc.PAIR_KINDS == {"qk_pair": "q", "qk_pair_raw": "q"} and tuple(cc.PAIR_KINDS) == ("qk_pair", "qk_pair_raw")
    assert cc.CAUSAL_KINDS == {"qk_causal": "q", "qk_causal_raw": "q"} and tuple(cc.CAUSAL_KINDS) == ("qk_causal", "qk_causal_raw")
    assert cc.EXTRA_KINDS == {"q_rope": "q", "k_rope": "k", "qk_pair": "q", "qk_pair_raw": "q", "qk_causal": "q", "qk_causal_raw": "q"}
    assert tuple(cc.EXTRA_KINDS) == ("q_rope", "k_rope", "qk_pair", "qk_pair_raw", "qk_causal", "qk_causal_raw")      # the order files are written in
    assert cc.MEAN_KIND == "mlp_mean" and cc.X_MEAN_KIND == "x_mean"
    assert cc.VECTOR_KINDS == {"mlp_mean": "n_inner", "x_mean": "d_model"} and tuple(cc.VECTOR_KINDS) == ("mlp_mean", "x_mean")


# ---------------------------------------------------------------- the collection rules
# wrapper, switch, what the "needs" message calls it, the head_dim limit's entry point, the two log lines on another architecture
RULES = (
    ("qk_rope_collected", "MODEGPT_QK_ROPE", None, None,
     "MODEGPT_QK_ROPE=1 ignored for qwen3: the compressed model renormalises q / k over the kept columns (masked RMSNorm), so the "
     "dropped-column identity of the post-RoPE statistic does not hold; nothing is collected",
     "MODEGPT_QK_ROPE=1: opt has no rotary embedding, the pre-RoPE statistic is already the exact one; nothing more is collected"),
    ("qk_seq_collected", "MODEGPT_QK_SEQ", "within-sequence Q/K statistic", "mdg_qk_pair_accum",
     "MODEGPT_QK_SEQ=1 ignored for qwen3: the compressed model renormalises q / k over the kept columns (masked RMSNorm), so the "
     "dropped-column identity of the within-sequence statistic does not hold; nothing is collected",
     "MODEGPT_QK_SEQ=1: opt has no rotary embedding and separate q / k hooks; the within-sequence statistic is not collected for it"),
    ("qk_causal_collected", "MODEGPT_QK_CAUSAL", "causal Q/K statistic", "mdg_qk_causal_accum",
     "MODEGPT_QK_CAUSAL=1 ignored for qwen3: the compressed model renormalises q / k over the kept columns (masked RMSNorm), so the "
     "dropped-column identity of the causal statistic does not hold; nothing is collected",
     "MODEGPT_QK_CAUSAL=1: opt has no rotary embedding and separate q / k hooks; the causal statistic is not collected for it"),
)
SWITCHES = ("MODEGPT_QK_ROPE", "MODEGPT_QK_SEQ", "MODEGPT_QK_CAUSAL", "MODEGPT_MLP_INTERCEPT", "MODEGPT_VO_INTERCEPT")


@pytest.mark.parametrize("wrapper,switch,needs_noun,entry,qwen_line,opt_line", RULES)
def test_collected_rules_and_messages(monkeypatch, caplog, wrapper, switch, needs_noun, entry, qwen_line, opt_line):
    from modegpt_amd import calibration
    rule = getattr(calibration, wrapper)
    log = logging.getLogger("test_calib_stats")
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    llama, qwen2, wide = (SimpleNamespace(arch=a, head_dim=h) for a, h in (("llama", 64), ("qwen2", 128), ("llama", 256)))
    others = [SimpleNamespace(arch=a, head_dim=64) for a in ("qwen3", "opt")]
    # switch off: nothing, silently, whatever else is set
    monkeypatch.setenv("MODEGPT_QK_ROPE" if switch != "MODEGPT_QK_ROPE" else "MODEGPT_QK_SEQ", "1")
    for ad in (llama, qwen2, wide, *others):
        assert rule(ad, log) is False
    monkeypatch.delenv("MODEGPT_QK_ROPE", raising=False)
    monkeypatch.delenv("MODEGPT_QK_SEQ", raising=False)
    # switch on, MODEGPT_QK_ROPE off
    monkeypatch.setenv(switch, "1")
    if needs_noun is not None:
        msg = (f"{switch}=1 needs MODEGPT_QK_ROPE=1: the {needs_noun} is accumulated from the post-RoPE rows, which are only produced "
               "when the post-RoPE statistics are collected")
        for ad in (llama, qwen2, wide):
            with pytest.raises(RuntimeError, match="^" + re.escape(msg) + "$"):
                rule(ad)
        monkeypatch.setenv("MODEGPT_QK_ROPE", "1")
    # collected on the two rotary architectures; the head_dim limit of the sequence kernels
    assert rule(llama) is True and rule(qwen2) is True
    if entry is None:
        assert rule(wide) is True
    else:
        with pytest.raises(RuntimeError, match="^" + re.escape(f"{switch}=1: head_dim 256 > 128 is not supported by {entry}") + "$"):
            rule(wide)
    # independent of the other statistics' switches
    for name, fn in (("MODEGPT_QK_SEQ", calibration.qk_seq_collected), ("MODEGPT_QK_CAUSAL", calibration.qk_causal_collected)):
        if name != switch:
            assert fn(llama) is False
    # another architecture: nothing is collected, one line with a logger, none without
    for ad, level, line in zip(others, (logging.WARNING, logging.INFO), (qwen_line, opt_line)):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="test_calib_stats"):
            assert rule(ad) is False and not caplog.records
            assert rule(ad, log) is False
        assert [(r.levelno, r.getMessage()) for r in caplog.records] == [(level, line)]


def test_the_means_are_collected_on_every_architecture(monkeypatch):
    from modegpt_amd import calibration
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, switch in (("mlp_mean", "MODEGPT_MLP_INTERCEPT"), ("x_mean", "MODEGPT_VO_INTERCEPT")):
        for arch in ("llama", "qwen2", "qwen3", "opt"):
            ad = SimpleNamespace(arch=arch, head_dim=256)
            assert calibration.collected(cs.BY_NAME[name], ad) is False
            monkeypatch.setenv(switch, "1")
            assert calibration.collected(cs.BY_NAME[name], ad) is True
            monkeypatch.delenv(switch)


# ---------------------------------------------------------------- the per-layer fetch
def test_layer_value_is_none_when_absent_unset_empty_or_without_what_it_needs():
    v, q, k, p, r = object(), object(), object(), object(), object()
    ad = SimpleNamespace()
    assert all(cs.layer_value(ad, name, 1) is None for name in cs.BY_NAME)                       # attribute absent
    ad.mlp_means, ad.qk_rope_stats, ad.qk_pair_stats, ad.qk_causal_stats = [None, v], ([None, q], [None, k]), ([None, p], [None, r]), None
    assert cs.layer_value(ad, "mlp_mean", 1) is v and cs.layer_value(ad, "mlp_mean", 0) is None  # the layer's entry is None
    assert cs.layer_value(ad, "qk_rope", 1) == (q, k) and cs.layer_value(ad, "qk_rope", 0) is None
    assert cs.layer_value(ad, "qk_pair", 1) == (p, r) and cs.layer_value(ad, "qk_pair", 0) is None
    assert cs.layer_value(ad, "qk_causal", 1) is None                                            # attribute None
    ad.qk_rope_stats = None
    assert cs.layer_value(ad, "qk_pair", 1) is None                                              # what it needs is None
    assert cs.layer_value(ad, "mlp_mean", 1, "sums_attr") is None                                # the sweep's attribute is another one
    ad.mlp_sums = [None, v]
    assert cs.layer_value(ad, "mlp_mean", 1, "sums_attr") is v


# ---------------------------------------------------------------- a record of all five statistics
ARCH = {"arch": "llama", "d_model": 8, "n_inner": 8, "n_heads": 2, "n_kv_heads": 1, "head_dim": 4, "n_layers": 3, "dtype": "torch.bfloat16"}


def bits_of_two_to(k):
    """The bit pattern of the double 2^k."""
    return (1023 + k) << 52


# every member holds one constant, 2^i for the i-th kind of the table: its exact sum (n entries) or trace (batch * n entries) is a
# power of two too
FILES = {
    "mlp_mean": {"file": "layer_2_mlp_mean.f64", "layout": "vector", "n": 8, "bytes": 64, "sum_bits": bits_of_two_to(3)},
    "x_mean": {"file": "layer_2_x_mean.f64", "layout": "vector", "n": 8, "bytes": 64, "sum_bits": bits_of_two_to(4)},
    "q_rope": {"file": "layer_2_q_rope.f64", "layout": "full", "n": 4, "batch": 2, "bytes": 256, "trace_bits": bits_of_two_to(5)},
    "k_rope": {"file": "layer_2_k_rope.f64", "layout": "full", "n": 4, "batch": 1, "bytes": 128, "trace_bits": bits_of_two_to(5)},
    "qk_pair": {"file": "layer_2_qk_pair.f64", "layout": "full", "n": 4, "batch": 2, "bytes": 256, "trace_bits": bits_of_two_to(7)},
    "qk_pair_raw": {"file": "layer_2_qk_pair_raw.f64", "layout": "full", "n": 4, "batch": 2, "bytes": 256, "trace_bits": bits_of_two_to(8)},
    "qk_causal": {"file": "layer_2_qk_causal.f64", "layout": "full", "n": 4, "batch": 2, "bytes": 256, "trace_bits": bits_of_two_to(9)},
    "qk_causal_raw": {"file": "layer_2_qk_causal_raw.f64", "layout": "full", "n": 4, "batch": 2, "bytes": 256, "trace_bits": bits_of_two_to(10)},
}


def test_a_record_of_all_five_statistics_entry_by_entry(tmp_path):
    d = str(tmp_path)
    files, values = {}, {}
    for i, (kind, stat) in enumerate(cs.KIND_STAT.items()):
        if stat.layout == "vector":
            n = ARCH[cs.KIND_SHAPE[kind]]
            values[kind] = np.full(n, 2.0 ** i)
            files[kind] = cc.write_mean_file(d, 2, values[kind], n, kind=kind)
        else:
            n, batch = cc.stat_shapes(ARCH)[cs.KIND_SHAPE[kind]]
            values[kind] = np.full(batch * n * n, 2.0 ** i)
            files[kind] = cc.write_data_file(d, 2, kind, values[kind], n, batch)
    meta = cc.make_sidecar(2, ARCH, {"dataset": "synthetic"}, "m", {"down_proj": 1, "q_proj": 2}, files, {})
    assert meta["files"] == FILES
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(e["file"] for e in FILES.values())
    for kind in FILES:
        entry = cc.validate_extra_entry(meta, ARCH, 2, kind)
        assert entry == FILES[kind]
        if entry["layout"] == "vector":
            back = cc.read_mean_file(d, 2, entry, kind=kind)
        else:
            back = np.empty(values[kind].size)
            cc.read_data_file(d, 2, kind, entry, back)
        assert back.tobytes() == values[kind].tobytes()
    # a record saved without a switch is refused under that switch's name, for every member
    for kind, stat in cs.KIND_STAT.items():
        without = {"files": {k: v for k, v in FILES.items() if k != kind}}
        with pytest.raises(ValueError, match=rf"layer 2: field files\.{kind} is missing -- the record was saved without {stat.switch}=1 and"):
            cc.validate_extra_entry(without, ARCH, 2, kind)
    # ... and one of another shape under the field that differs
    for kind, field, arch in (("mlp_mean", "n", dict(ARCH, n_inner=9)), ("x_mean", "n", dict(ARCH, d_model=9)),
                              ("q_rope", "batch", dict(ARCH, n_heads=4)), ("k_rope", "batch", dict(ARCH, n_kv_heads=2)),
                              ("qk_pair", "n", dict(ARCH, head_dim=8)), ("qk_causal_raw", "batch", dict(ARCH, n_heads=4))):
        with pytest.raises(ValueError, match=rf"layer 2: field files\.{kind}\.{field} is"):
            cc.validate_extra_entry(meta, arch, 2, kind)
