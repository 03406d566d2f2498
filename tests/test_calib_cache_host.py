"""CPU: the statistics directory's host half (modegpt_amd/calib_cache.py) -- the file format read with numpy alone, the sidecar
schema and every refusal of its validation on metadata alone, the commit-marker rule, one writer per file."""
import copy
import json
import math
import os
import struct

import numpy as np
import pytest

from modegpt_amd import calib_cache as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calib_cache_n5")

ARCH = {"arch": "llama", "d_model": 6, "n_inner": 9, "n_heads": 2, "n_kv_heads": 1, "head_dim": 3, "n_layers": 4,
        "dtype": "torch.bfloat16"}
CALIBRATION = {"dataset": "synthetic", "n_samples": 8, "batch_size": 4, "n_texts": 8, "n_tokens": 512}
CERTIFICATES = {"calib_tokens": 512, "cov_routes": {"i8_5": 0, "i8_6": 0, "fallback_f64": 0, "fp64_columns": 0, "exact": 0},
                "cov_rows_left": None, "cov_mode": "i8", "i8_tolerance": 1.0, "i8_rows": False, "i8_exact": "auto", "i8_fuse": True}


def bits(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


def test_golden_record_reads_with_numpy_alone():
    """tests/golden/calib_cache_n5 was written once by the device code (sym_pack_lower -> pinned host -> file) from
    mlp[i][j] = 1 / (1 + i + j) + [i == j], x[i][j] = 1 / (2 + i + j) + 3 [i == j]: it reads back through np.fromfile and
    np.tril_indices into exactly the matrix its sidecar describes."""
    meta = json.load(open(os.path.join(GOLDEN, "layer_0.json")))
    assert meta["format_version"] == 1 and meta["layer"] == 0
    i = np.arange(5.0)
    want = {"mlp": 1.0 / (1.0 + i[:, None] + i[None, :]) + np.eye(5), "x": 1.0 / (2.0 + i[:, None] + i[None, :]) + 3.0 * np.eye(5)}
    for kind in ("mlp", "x"):
        entry = meta["files"][kind]
        assert entry["layout"] == "packed_lower" and entry["n"] == 5 == meta["arch"]["n_inner"]
        path = os.path.join(GOLDEN, entry["file"])
        assert os.path.getsize(path) == entry["bytes"] == 15 * 8
        packed = np.fromfile(path, "<f8")
        full = np.zeros((5, 5))
        full[np.tril_indices(5)] = packed
        full = full + np.tril(full, -1).T
        assert np.array_equal(full.view(np.int64), want[kind].view(np.int64))
        assert bits(math.fsum(np.diag(full).tolist())) == entry["trace_bits"]
    for kind, m in (("q", [[2.0, 0.25], [0.25, 1.0]]), ("k", [[4.0, -0.5], [-0.5, 3.0]])):
        entry = meta["files"][kind]
        assert entry["layout"] == "full" and (entry["batch"], entry["n"]) == (1, 2)
        got = np.fromfile(os.path.join(GOLDEN, entry["file"]), "<f8").reshape(1, 2, 2)
        assert np.array_equal(got[0], np.array(m))
    assert json.load(open(os.path.join(GOLDEN, "bi_scores.json")))["bi_scores"] == [0.125]
    # ... and through the module's own reader
    expect = {"arch": meta["arch"], "dataset": "synthetic", "n_samples": 2, "model": "fixture", "weights": {"down_proj": 0, "q_proj": 0},
              "cov_mode": "f64", "i8_tolerance": 1.0}
    cc.validate_sidecar(cc.read_sidecar(GOLDEN, 0), expect, 0)
    out = np.empty(15)
    cc.read_data_file(GOLDEN, 0, "mlp", meta["files"]["mlp"], out)
    assert np.array_equal(out, want["mlp"][np.tril_indices(5)])
    assert cc.read_bi_scores(GOLDEN, expect) == [0.125]


def stats(seed):
    g = np.random.default_rng(seed)
    out = {}
    for kind, (n, batch) in cc.stat_shapes(ARCH).items():
        a = g.standard_normal((batch, n, 2 * n))
        s = a @ a.transpose(0, 2, 1)
        out[kind] = (s[0][np.tril_indices(n)] if kind in cc.PACKED_KINDS else s.reshape(-1), n, batch)
    return out


def write_record(directory, layer, seed, sidecar=True):
    files = {kind: cc.write_data_file(directory, layer, kind, v, n, batch) for kind, (v, n, batch) in stats(seed).items()}
    meta = cc.make_sidecar(layer, ARCH, CALIBRATION, "some/model", {"down_proj": 11 + layer, "q_proj": -7}, files, CERTIFICATES)
    if sidecar:
        cc.write_sidecar(directory, meta)
    return meta


def expect_for(layer):
    return {"arch": dict(ARCH), "dataset": "synthetic", "n_samples": 8, "model": "some/model",
            "weights": {"down_proj": 11 + layer, "q_proj": -7}, "cov_mode": "i8", "i8_tolerance": 1.0}


def test_sidecar_schema_and_round_trip(tmp_path):
    d = str(tmp_path)
    meta = write_record(d, 2, seed=5)
    assert set(meta) == {"format_version", "layer", "arch", "calibration", "model", "weights", "files", "certificates"}
    assert set(meta["arch"]) == set(cc.ARCH_FIELDS)
    assert {"dataset", "n_samples", "n_texts", "n_tokens", "batch_size"} <= set(meta["calibration"])
    assert {"calib_tokens", "cov_routes", "cov_rows_left", "cov_mode", "i8_tolerance"} <= set(meta["certificates"])
    for kind in cc.KINDS:
        assert set(meta["files"][kind]) == {"file", "layout", "n", "batch", "bytes", "trace_bits"}
    back = cc.read_sidecar(d, 2)
    assert back == meta
    cc.validate_sidecar(back, expect_for(2), 2)
    cc.validate_sidecar(back, dict(expect_for(2), batch_size=999), 2)           # batch_size is recorded, not checked
    for kind, (v, n, batch) in stats(5).items():
        out = np.empty(v.size)
        cc.read_data_file(d, 2, kind, back["files"][kind], out)
        assert np.array_equal(out.view(np.int64), v.view(np.int64))


def _set(meta, path, value):
    node = meta
    for key in path[:-1]:
        node = node[key]
    node[path[-1]] = value


REFUSALS = [(("format_version",), 2, "format_version"), (("layer",), 3, "layer"),
            (("arch", "arch"), "opt", r"arch\.arch"), (("arch", "d_model"), 8, r"arch\.d_model"), (("arch", "n_inner"), 10, r"arch\.n_inner"),
            (("arch", "n_heads"), 4, r"arch\.n_heads"), (("arch", "n_kv_heads"), 2, r"arch\.n_kv_heads"),
            (("arch", "head_dim"), 4, r"arch\.head_dim"), (("arch", "n_layers"), 5, r"arch\.n_layers"),
            (("arch", "dtype"), "torch.float16", r"arch\.dtype"),
            (("calibration", "dataset"), "wikitext", r"calibration\.dataset"), (("calibration", "n_samples"), 16, r"calibration\.n_samples"),
            (("calibration", "n_texts"), None, r"calibration\.n_texts"), (("calibration", "n_tokens"), "many", r"calibration\.n_tokens"),
            (("model",), "another/model", "model"),
            (("weights", "down_proj"), 14, r"weights\.down_proj"), (("weights", "q_proj"), -6, r"weights\.q_proj"),
            (("files", "mlp", "n"), 10, r"files\.mlp\.n"), (("files", "x", "bytes"), 8, r"files\.x\.bytes"),
            (("files", "q", "batch"), 1, r"files\.q\.batch"), (("files", "k", "layout"), "packed_lower", r"files\.k\.layout"),
            (("files", "mlp", "trace_bits"), 1.5, r"files\.mlp\.trace_bits"), (("files", "x"), None, r"files\.x"),
            (("certificates", "cov_mode"), "f64", r"certificates\.cov_mode"), (("certificates", "i8_tolerance"), 64.0, r"certificates\.i8_tolerance"),
            (("certificates",), None, "certificates")]


@pytest.mark.parametrize("path,value,field", REFUSALS, ids=[".".join(r[0]) for r in REFUSALS])
def test_validation_refuses_and_names_the_field(tmp_path, path, value, field):
    meta = copy.deepcopy(write_record(str(tmp_path), 2, seed=5))
    cc.validate_sidecar(meta, expect_for(2), 2)
    _set(meta, path, value)
    with pytest.raises(ValueError, match=rf"layer 2\b.*field {field}\b"):
        cc.validate_sidecar(meta, expect_for(2), 2)


def test_data_file_checks(tmp_path):
    d = str(tmp_path)
    meta = write_record(d, 1, seed=3)
    v, n, batch = stats(3)["mlp"]
    out = np.empty(v.size)
    path = cc.data_path(d, 1, "mlp")
    os.truncate(path, v.size * 8 - 8)
    with pytest.raises(ValueError, match=r"layer 1\b.*files\.mlp\.bytes"):
        cc.read_data_file(d, 1, "mlp", meta["files"]["mlp"], out)
    flipped = v.copy()
    flipped[4 * 7 // 2] *= 2.0                                                  # the diagonal entry (4, 4)
    flipped.tofile(path)
    with pytest.raises(ValueError, match=r"layer 1\b.*files\.mlp\.trace_bits"):
        cc.read_data_file(d, 1, "mlp", meta["files"]["mlp"], out)
    os.remove(path)
    with pytest.raises(FileNotFoundError, match=r"layer 1\b"):
        cc.read_data_file(d, 1, "mlp", meta["files"]["mlp"], out)


def test_a_layer_without_sidecar_is_absent(tmp_path):
    d = str(tmp_path)
    write_record(d, 0, seed=1)
    write_record(d, 1, seed=2, sidecar=False)                                   # data files only: a write that never finished
    assert os.path.exists(cc.data_path(d, 1, "mlp"))
    assert cc.layers_present(d) == [0]
    with pytest.raises(FileNotFoundError, match=r"layer 1\b"):
        cc.read_sidecar(d, 1)
    assert cc.layers_present(str(tmp_path / "nowhere")) == []


def test_two_ranks_write_disjoint_layers(tmp_path):
    d = str(tmp_path)
    mine = {0: [0, 1], 1: [2, 3]}                                                # rank -> the layers it owns: one writer per file
    written = {}
    for step in range(2):                                                        # interleaved, as two processes would be
        for rank in (0, 1):
            layer = mine[rank][step]
            written[layer] = write_record(d, layer, seed=10 + layer)
    cc.write_bi_scores(d, [0.1, 0.2, 0.3, 0.4], ARCH, CALIBRATION, "some/model")  # (the rank that computed them)
    assert cc.layers_present(d) == [0, 1, 2, 3]
    for layer in range(4):
        meta = cc.read_sidecar(d, layer)
        assert meta == written[layer]
        cc.validate_sidecar(meta, expect_for(layer), layer)
        for kind, (v, n, batch) in stats(10 + layer).items():
            out = np.empty(v.size)
            cc.read_data_file(d, layer, kind, meta["files"][kind], out)
            assert np.array_equal(out, v)
    assert cc.read_bi_scores(d, expect_for(0)) == [0.1, 0.2, 0.3, 0.4]
    names = os.listdir(d)
    assert len(names) == 4 * 5 + 1 and not [n for n in names if "tmp" in n]


def test_certificates_of_one_run_come_back_as_they_are_and_several_add_up():
    one = dict(CERTIFICATES, cov_routes={"i8_5": 3, "i8_6": 1, "fallback_f64": 0, "fp64_columns": 2, "exact": 1})
    assert cc.merge_certificates([one, dict(one), dict(one)]) == one
    two = dict(CERTIFICATES, cov_routes={"i8_5": 0, "i8_6": 0, "fallback_f64": 1, "fp64_columns": 0, "exact": 0})
    merged = cc.merge_certificates([one, two])
    assert merged["cov_routes"] == {"i8_5": 3, "i8_6": 1, "fallback_f64": 1, "fp64_columns": 2, "exact": 1}
    with pytest.raises(ValueError, match="calib_tokens"):
        cc.merge_certificates([one, dict(two, calib_tokens=1024)])
