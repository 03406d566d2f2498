"""The calibration statistics on disk: what load_calibs(calibs_save_path=...) writes and load_calibs(load_calibs_from=...) reads
instead of running the model (reference: src/calibration.py:23-24 declares both parameters and never reads them).

One directory, one self-contained record per layer, so chunks of layers, target_layers subsets and sharded ranks compose:

    layer_<i>_mlp.f64, layer_<i>_x.f64     raw little-endian fp64, the LOWER triangle in row-major packed order (row r holds its
                                           entries 0..r at offset r(r+1)/2; ops.sym_pack_lower).  numpy alone reads one:
                                           full[np.tril_indices(n)] = np.fromfile(path, "<f8")
    layer_<i>_q.f64, layer_<i>_k.f64       raw little-endian fp64, full [heads, head_dim, head_dim]
    layer_<i>_<kind>.f64                   one per member of every optional statistic this run collects (calib_stats.STATS: which
                                           kinds, under which switch, of which shape).  Layout "vector" (the means): n raw
                                           little-endian fp64, np.fromfile(path, "<f8") reads it; its sidecar entry files.<kind> holds
                                           the length, n and the bit pattern of its exact sum.  Layout "full" (the Q/K statistics):
                                           the format and sidecar entry fields of layer_<i>_q.f64 / _k.f64.  A run with the switch
                                           refuses a record without the entry (it never recalibrates); a run without ignores file
                                           and entry; records written without the switch are what they always were
    layer_<i>.json                         the sidecar, written LAST: the commit marker -- a layer without it does not exist
    bi_scores.json                         the Block-Influence scores of all layers, written by the rank that computed them

Every file goes to a temporary name and then through os.replace, and has one writer (the rank that owns the layer).  The sidecar
records what the statistics depend on -- architecture, calibration samples, the source model string, a fingerprint of the layer's
weights -- and per data file its length, size and the bit pattern of its trace; the loader compares all of it and raises a
ValueError / FileNotFoundError naming the layer and the field.  It never recalibrates on its own.  The sidecar also carries what
the selection certificates are taken against (calib_tokens, cov_routes, cov_rows_left, the covariance mode and tolerance), which
the loader puts back on the adapter: a compression from loaded statistics reports the same metrics.

The host half of this module (paths, sidecars, validation, raw files) needs numpy only; the device half moves a statistic
device -> pinned host -> file through two pinned buffers of the largest packed statistic (the copy of one statistic runs while
the previous one is written; synchronous otherwise: save() returns with every file in place) and one device buffer of the same
size for the packed triangle.  No second copy of the statistics exists in HBM.
"""
from __future__ import annotations

import json
import logging
import math
import os
import re
import struct
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

from .calib_stats import BY_NAME, KIND_SHAPE, KIND_STAT, STATS

logger = logging.getLogger("MoDeGPT")

FORMAT_VERSION = 1
PACKED_KINDS = ("mlp", "x")      # 2-D statistics: packed lower triangle
FULL_KINDS = ("q", "k")          # per-head statistics: full (tiny)
KINDS = PACKED_KINDS + FULL_KINDS
# the optional statistics (calib_stats.STATS), in table order.  Layout "full": file kind -> the statistic whose shape and layout it has
ROPE_KINDS, PAIR_KINDS, CAUSAL_KINDS = (dict(BY_NAME[name].members) for name in ("qk_rope", "qk_pair", "qk_causal"))
EXTRA_KINDS = {kind: shape for kind, shape in KIND_SHAPE.items() if KIND_STAT[kind].layout == "full"}
# ... layout "vector" (the activation means): file kind -> the arch field that is its length
VECTOR_KINDS = {kind: shape for kind, shape in KIND_SHAPE.items() if KIND_STAT[kind].layout == "vector"}
MEAN_KIND, X_MEAN_KIND = VECTOR_KINDS
ARCH_FIELDS = ("arch", "d_model", "n_inner", "n_heads", "n_kv_heads", "head_dim", "n_layers", "dtype")
BI_FILE = "bi_scores.json"


# ------------------------------------------------------------------ host half: names, atomic writes
def data_path(directory: str, layer: int, kind: str) -> str:
    return os.path.join(directory, f"layer_{int(layer)}_{kind}.f64")


def sidecar_path(directory: str, layer: int) -> str:
    return os.path.join(directory, f"layer_{int(layer)}.json")


def _replace_into(path: str, write) -> None:
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        write(tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _write_json(path: str, obj: dict) -> None:
    def write(tmp):
        with open(tmp, "w") as f:
            json.dump(obj, f, indent=1, sort_keys=True)
    _replace_into(path, write)


def layers_present(directory: str) -> List[int]:
    """The layers that exist in `directory`: those with a sidecar.  Data files without one are a write that never finished."""
    if not os.path.isdir(directory):
        return []
    found = (re.fullmatch(r"layer_(\d+)\.json", name) for name in os.listdir(directory))
    return sorted(int(m.group(1)) for m in found if m)


# ------------------------------------------------------------------ host half: one data file
def packed_numel(n: int) -> int:
    return n * (n + 1) // 2


def stat_numel(kind: str, n: int, batch: int) -> int:
    return packed_numel(n) if kind in PACKED_KINDS else batch * n * n


def trace_bits(values: np.ndarray, kind: str, n: int, batch: int) -> int:
    """The bit pattern (as int64) of the statistic's trace, summed exactly (math.fsum: one rounding, no summation order), from the
    file's flat contents."""
    if kind in PACKED_KINDS:
        i = np.arange(n, dtype=np.int64)
        diag = values[i * (i + 3) // 2]
    else:
        diag = values.reshape(batch, n, n).diagonal(axis1=1, axis2=2).ravel()
    return struct.unpack("<q", struct.pack("<d", math.fsum(diag.tolist())))[0]


def write_data_file(directory: str, layer: int, kind: str, values: np.ndarray, n: int, batch: int) -> dict:
    """`values`: the file's flat fp64 contents.  Returns the sidecar's entry for the file."""
    values = np.ascontiguousarray(values, dtype="<f8").reshape(-1)
    if values.size != stat_numel(kind, n, batch):
        raise ValueError(f"layer {layer}: statistic {kind} has {values.size} elements, n = {n} and batch = {batch} make "
                         f"{stat_numel(kind, n, batch)}")
    path = data_path(directory, layer, kind)
    _replace_into(path, values.tofile)
    return {"file": os.path.basename(path), "layout": "packed_lower" if kind in PACKED_KINDS else "full", "n": int(n),
            "batch": int(batch), "bytes": int(values.size * 8), "trace_bits": trace_bits(values, kind, n, batch)}


def read_data_file(directory: str, layer: int, kind: str, entry: dict, out: np.ndarray) -> None:
    """Fills `out` (flat fp64, exactly the statistic's size) from the file and checks the length and the trace the sidecar holds."""
    path = os.path.join(directory, entry["file"])
    if not os.path.exists(path):
        raise FileNotFoundError(f"calibration statistics, layer {layer}: data file {path} (field files.{kind}.file) is missing")
    want = out.size * 8
    size = os.path.getsize(path)
    if size != want or entry["bytes"] != want:
        raise ValueError(f"calibration statistics, layer {layer}: field files.{kind}.bytes -- {path} holds {size} bytes, the "
                         f"sidecar says {entry['bytes']}, the statistic takes {want}")
    with open(path, "rb") as f:
        got = f.readinto(memoryview(out).cast("B"))
    if got != want:
        raise ValueError(f"calibration statistics, layer {layer}: field files.{kind}.bytes -- read {got} of {want} bytes of {path}")
    if sys.byteorder != "little":
        out.byteswap(inplace=True)
    bits = trace_bits(out, kind, entry["n"], entry["batch"])
    if bits != entry["trace_bits"]:
        raise ValueError(f"calibration statistics, layer {layer}: field files.{kind}.trace_bits -- the trace of {path} has the bit "
                         f"pattern {bits}, the sidecar recorded {entry['trace_bits']}")


# ------------------------------------------------------------------ host half: the optional statistics (calib_stats.STATS)
def sum_bits(values: np.ndarray) -> int:
    """The bit pattern (as int64) of the exact sum of the vector, rounded once (math.fsum: no summation order)."""
    return struct.unpack("<q", struct.pack("<d", math.fsum(np.asarray(values, dtype=np.float64).ravel().tolist())))[0]


def write_mean_file(directory: str, layer: int, values: np.ndarray, n: int, kind: str = MEAN_KIND) -> dict:
    """layer_<i>_<kind>.f64 from the n means; returns the sidecar's entry for it."""
    values = np.ascontiguousarray(values, dtype="<f8").reshape(-1)
    if values.size != n:
        raise ValueError(f"layer {layer}: the activation mean has {values.size} entries, {VECTOR_KINDS[kind]} is {n}")
    path = data_path(directory, layer, kind)
    _replace_into(path, values.tofile)
    return {"file": os.path.basename(path), "layout": "vector", "n": int(n), "bytes": int(n * 8), "sum_bits": sum_bits(values)}


def validate_extra_entry(meta: dict, arch: dict, layer: int, kind: str) -> dict:
    """Metadata alone: the record must carry files.<kind> for a member of an optional statistic, with the shape `arch` gives it -- a
    vector of the arch field it names, or the shape of files.q / files.k.  Returns the entry."""
    entry = meta.get("files", {}).get(kind)
    if not isinstance(entry, dict):
        raise ValueError(f"calibration statistics, layer {layer}: field files.{kind} is missing -- the record was saved without "
                         f"{KIND_STAT[kind].switch}=1 and this run has the switch on; save the statistics again with it (nothing is "
                         "recalibrated on load)")
    if kind in VECTOR_KINDS:
        n = int(arch[VECTOR_KINDS[kind]])
        want, bits = {"n": n, "bytes": 8 * n, "layout": "vector"}, "sum_bits"
    else:
        n, batch = stat_shapes(arch)[EXTRA_KINDS[kind]]
        want, bits = {"n": n, "batch": batch, "bytes": 8 * stat_numel(kind, n, batch), "layout": "full"}, "trace_bits"
    for name, value in want.items():
        if entry.get(name) != value:
            _refuse(layer, f"files.{kind}.{name}", entry.get(name), value)
    if not isinstance(entry.get(bits), int) or not isinstance(entry.get("file"), str):
        _refuse(layer, f"files.{kind}.{bits}", entry.get(bits), "an integer")
    return entry


def read_mean_file(directory: str, layer: int, entry: dict, kind: str = MEAN_KIND) -> np.ndarray:
    """The n means of the file, checked against the length and the exact sum the sidecar holds."""
    path = os.path.join(directory, entry["file"])
    if not os.path.exists(path):
        raise FileNotFoundError(f"calibration statistics, layer {layer}: data file {path} (field files.{kind}.file) is missing")
    size = os.path.getsize(path)
    if size != entry["bytes"]:
        raise ValueError(f"calibration statistics, layer {layer}: field files.{kind}.bytes -- {path} holds {size} bytes, the "
                         f"sidecar says {entry['bytes']}")
    values = np.fromfile(path, dtype="<f8").astype(np.float64)
    bits = sum_bits(values)
    if bits != entry["sum_bits"]:
        raise ValueError(f"calibration statistics, layer {layer}: field files.{kind}.sum_bits -- the sum of {path} has the bit "
                         f"pattern {bits}, the sidecar recorded {entry['sum_bits']}")
    return values


# ------------------------------------------------------------------ host half: the sidecar
def make_sidecar(layer: int, arch: dict, calibration: dict, model: str, weights: dict, files: dict, certificates: dict) -> dict:
    return {"format_version": FORMAT_VERSION, "layer": int(layer), "arch": dict(arch), "calibration": dict(calibration),
            "model": str(model), "weights": dict(weights), "files": dict(files), "certificates": dict(certificates)}


def write_sidecar(directory: str, meta: dict) -> None:
    _write_json(sidecar_path(directory, meta["layer"]), meta)


def read_sidecar(directory: str, layer: int) -> dict:
    path = sidecar_path(directory, layer)
    if not os.path.exists(path):
        raise FileNotFoundError(f"calibration statistics: layer {layer} has no sidecar in {directory} (layers there: "
                                f"{layers_present(directory)})")
    with open(path) as f:
        return json.load(f)


def _refuse(layer, field: str, got, want) -> None:
    raise ValueError(f"calibration statistics, layer {layer}: field {field} is {got!r}, this run has {want!r}")


def stat_shapes(arch: dict) -> Dict[str, tuple]:
    """kind -> (n, batch) of the statistics of a layer (src/calibration.py:82-96)."""
    return {"mlp": (arch["n_inner"], 1), "x": (arch["d_model"], 1), "q": (arch["head_dim"], arch["n_heads"]),
            "k": (arch["head_dim"], arch["n_kv_heads"])}


def validate_sidecar(meta: dict, expect: dict, layer: int) -> None:
    """Metadata alone.  `expect` holds what THIS run has: "arch" (ARCH_FIELDS), "dataset", "n_samples", "model", "weights"
    ({"down_proj", "q_proj"}: the layer's fingerprints), "cov_mode", "i8_tolerance".  batch_size is recorded, not checked (it only
    reorders fp64 sums)."""
    if meta.get("format_version") != FORMAT_VERSION:
        _refuse(layer, "format_version", meta.get("format_version"), FORMAT_VERSION)
    if meta.get("layer") != layer:
        _refuse(layer, "layer", meta.get("layer"), layer)
    for group in ("arch", "calibration", "weights", "files", "certificates"):
        if not isinstance(meta.get(group), dict):
            _refuse(layer, group, meta.get(group), "a record")
    for name in ARCH_FIELDS:
        if meta["arch"].get(name) != expect["arch"][name]:
            _refuse(layer, f"arch.{name}", meta["arch"].get(name), expect["arch"][name])
    for name in ("dataset", "n_samples"):
        if meta["calibration"].get(name) != expect[name]:
            _refuse(layer, f"calibration.{name}", meta["calibration"].get(name), expect[name])
    for name in ("n_texts", "n_tokens"):
        if not isinstance(meta["calibration"].get(name), int):
            _refuse(layer, f"calibration.{name}", meta["calibration"].get(name), "an integer")
    if meta.get("model") != expect["model"]:
        _refuse(layer, "model", meta.get("model"), expect["model"])
    for name in ("down_proj", "q_proj"):
        if meta["weights"].get(name) != expect["weights"][name]:
            _refuse(layer, f"weights.{name}", meta["weights"].get(name), expect["weights"][name])
    for kind, (n, batch) in stat_shapes(expect["arch"]).items():
        entry = meta["files"].get(kind)
        if not isinstance(entry, dict):
            _refuse(layer, f"files.{kind}", entry, "a record")
        want = {"n": n, "batch": batch, "bytes": 8 * stat_numel(kind, n, batch),
                "layout": "packed_lower" if kind in PACKED_KINDS else "full"}
        for name, value in want.items():
            if entry.get(name) != value:
                _refuse(layer, f"files.{kind}.{name}", entry.get(name), value)
        if not isinstance(entry.get("trace_bits"), int) or not isinstance(entry.get("file"), str):
            _refuse(layer, f"files.{kind}.trace_bits", entry.get("trace_bits"), "an integer")
    # the certificates read ops.COV_MODE / ops.i8_tolerance() of the running process beside what the adapter carries: statistics of
    # another mode or tolerance would be certified against the wrong bound
    for name in ("cov_mode", "i8_tolerance"):
        if meta["certificates"].get(name) != expect[name]:
            _refuse(layer, f"certificates.{name}", meta["certificates"].get(name), expect[name])
    if "calib_tokens" not in meta["certificates"] or "cov_routes" not in meta["certificates"]:
        _refuse(layer, "certificates.calib_tokens", None, "recorded")


# ------------------------------------------------------------------ host half: the BI scores
def write_bi_scores(directory: str, bi_scores: Sequence[float], arch: dict, calibration: dict, model: str) -> None:
    _write_json(os.path.join(directory, BI_FILE),
                {"format_version": FORMAT_VERSION, "arch": dict(arch), "calibration": dict(calibration), "model": str(model),
                 "bi_scores": [float(v) for v in bi_scores]})     # (json writes repr(float): reads back bit for bit)


def read_bi_scores(directory: str, expect: dict) -> List[float]:
    path = os.path.join(directory, BI_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"calibration statistics: {path} (the BI scores of all layers) is missing")
    with open(path) as f:
        meta = json.load(f)
    who = "all (bi_scores)"
    if meta.get("format_version") != FORMAT_VERSION:
        _refuse(who, "format_version", meta.get("format_version"), FORMAT_VERSION)
    for name in ARCH_FIELDS:
        if meta.get("arch", {}).get(name) != expect["arch"][name]:
            _refuse(who, f"arch.{name}", meta.get("arch", {}).get(name), expect["arch"][name])
    for name in ("dataset", "n_samples"):
        if meta.get("calibration", {}).get(name) != expect[name]:
            _refuse(who, f"calibration.{name}", meta.get("calibration", {}).get(name), expect[name])
    if meta.get("model") != expect["model"]:
        _refuse(who, "model", meta.get("model"), expect["model"])
    scores = meta.get("bi_scores")
    if not isinstance(scores, list) or len(scores) != expect["arch"]["n_layers"]:
        _refuse(who, "bi_scores", scores, f"{expect['arch']['n_layers']} scores")
    return [float(v) for v in scores]


def merge_certificates(records: Sequence[dict]) -> dict:
    """What goes back on the adapter after loading layers whose sidecars hold `records`.  Layers of ONE saving run carry one
    record: it comes back as it is.  Layers of several runs (subsets saved one after the other): the route counts add up, which
    keeps every distinction the error bounds draw (none / some on the int8 route, any fp64 fallback or column)."""
    distinct = []
    for r in records:
        if r not in distinct:
            distinct.append(r)
    if not distinct:
        return {}
    out = dict(distinct[0])
    for r in distinct[1:]:
        if r["calib_tokens"] != out["calib_tokens"]:
            raise ValueError(f"calibration statistics: field certificates.calib_tokens differs between the loaded layers "
                             f"({out['calib_tokens']} and {r['calib_tokens']})")
        if (r["cov_routes"] is None) != (out["cov_routes"] is None):
            raise ValueError("calibration statistics: field certificates.cov_routes is recorded for some loaded layers only")
        if r["cov_routes"] is not None:
            out["cov_routes"] = {k: out["cov_routes"].get(k, 0) + r["cov_routes"].get(k, 0)
                                 for k in sorted(set(out["cov_routes"]) | set(r["cov_routes"]))}
        if r.get("cov_rows_left") is not None or out.get("cov_rows_left") is not None:
            out["cov_rows_left"] = (out.get("cov_rows_left") or 0) + (r.get("cov_rows_left") or 0)
    return out


# ------------------------------------------------------------------ device half
def arch_fingerprint(adapter) -> dict:
    return {"arch": str(adapter.arch), "d_model": int(adapter.d_model), "n_inner": int(adapter.get_n_inner()),
            "n_heads": int(adapter.n_heads), "n_kv_heads": int(adapter.n_kv_heads), "head_dim": int(adapter.head_dim),
            "n_layers": int(adapter.n_layers), "dtype": str(next(adapter.model.parameters()).dtype)}


def _bits_sum(w) -> int:
    import torch
    w = w.detach().contiguous()
    as_int = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[w.element_size()]
    return int(w.view(as_int).sum(dtype=torch.int64).item())


def weight_fingerprint(adapter, layer: int) -> dict:
    """The int64 sums (wrapping) of the raw bit patterns of the layer's down-projection and q-projection weights: exact, whatever
    order the device adds them in, and one ulp in one element moves it."""
    return {"down_proj": _bits_sum(adapter.get_mlp_tensors(layer).down_proj),
            "q_proj": _bits_sum(adapter.get_qk_tensors(layer).query_proj)}


def resolve_targets(adapter, target_layers) -> List[int]:
    """The layers a load_calibs call is about (calibration._calibrate_model's rule)."""
    if getattr(adapter, "calib_no_hooks", False):
        return []
    return list(target_layers) if target_layers else list(range(adapter.n_layers))


def _model_string(adapter) -> str:
    return str(getattr(getattr(adapter, "config", None), "model", "") or "")


def certificates_in_force(adapter) -> dict:
    """What the certificates of a compression from these statistics are taken against, as calibration left it on the adapter."""
    from . import ops
    i8 = ops.COV_MODE == "i8"
    return {"calib_tokens": int(adapter.calib_tokens), "cov_routes": getattr(adapter, "cov_routes", None),
            "cov_rows_left": int(adapter.cov_rows_left) if i8 and ops.I8_ROWS and hasattr(adapter, "cov_rows_left") else None,
            "cov_mode": ops.COV_MODE, "i8_tolerance": float(ops.i8_tolerance()),
            "i8_rows": bool(ops.I8_ROWS), "i8_exact": ops.I8_EXACT, "i8_fuse": bool(ops.I8_FUSE)}


class Staging:
    """The bounded staging area: two pinned host buffers of `numel` doubles, taken in turn, and one device buffer of the same size
    for a packed triangle.  A buffer is handed out again only after the copy that last used it has finished."""

    def __init__(self, numel: int, device):
        import torch
        self.numel = numel
        self.device = device
        self.dev = torch.empty(numel, dtype=torch.float64, device=device)
        self._host = [None, None]
        self._busy = [None, None]
        self._turn = 0

    def take(self, numel: int):
        """(slot, pinned flat fp64 tensor of `numel` elements)."""
        import torch
        slot, self._turn = self._turn, self._turn ^ 1
        if self._busy[slot] is not None:
            self._busy[slot].synchronize()
            self._busy[slot] = None
        if self._host[slot] is None:
            self._host[slot] = torch.empty(self.numel, dtype=torch.float64, pin_memory=True)
        return slot, self._host[slot][:numel]

    def mark(self, slot: int):
        """Record, on the current stream, the end of the copy that uses `slot`; returns the event."""
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._busy[slot] = ev
        return ev


def _staging_for(arch: dict, device) -> Staging:
    return Staging(max(stat_numel(kind, n, batch) for kind, (n, batch) in stat_shapes(arch).items()), device)


def write_layer(directory: str, layer: int, tensors: dict, staging: Staging, arch: dict, calibration: dict, model: str,
                weights: dict, certificates: dict, extra: Optional[dict] = None) -> dict:
    """One layer's record from its four device tensors ({"mlp", "x": [n, n]; "q", "k": [heads, hd, hd]}): data files first, the
    sidecar last.  The device -> host copy of a statistic runs while the one before it is written to its file.  extra: file kind ->
    the layer's device tensor, for the members of the optional statistics the record is to hold (calib_stats.STATS) -- the files and
    entries of the "full" ones follow those of the four through the same staging, in table order, then the vectors."""
    import torch
    from . import ops
    os.makedirs(directory, exist_ok=True)
    files, waiting = {}, None
    extra = extra or {}
    staged = tuple(kind for kind in EXTRA_KINDS if kind in extra)
    tensors = dict(tensors, **extra)

    def finish(item):
        kind, n, batch, host, ev = item
        ev.synchronize()
        files[kind] = write_data_file(directory, layer, kind, host.numpy(), n, batch)

    for kind in KINDS + staged:
        t = tensors[kind]
        n, batch = t.shape[-1], (1 if t.dim() == 2 else t.shape[0])
        numel = stat_numel(kind, n, batch)
        slot, host = staging.take(numel)
        with torch.cuda.device(t.device):
            src = ops.sym_pack_lower(t, out=staging.dev[:numel]) if kind in PACKED_KINDS else t.contiguous().view(-1)
            host.copy_(src, non_blocking=True)
            ev = staging.mark(slot)
        if waiting is not None:
            finish(waiting)
        waiting = (kind, n, batch, host, ev)
    finish(waiting)
    for kind, field in VECTOR_KINDS.items():
        if kind in extra:
            files[kind] = write_mean_file(directory, layer, extra[kind].detach().cpu().numpy(), arch[field], kind=kind)
    meta = make_sidecar(layer, arch, calibration, model, weights, files, certificates)
    write_sidecar(directory, meta)
    return meta


def read_layer(directory: str, layer: int, tensors: dict, staging: Staging, expect: dict, extra: Optional[dict] = None) -> dict:
    """The inverse: checks the sidecar against `expect`, fills the four device tensors, returns the sidecar.  The file of a
    statistic is read while the one before it is copied to the device and unpacked.  extra: file kind -> the fp64 device tensor to
    fill from layer_<i>_<kind>.f64, for the members of the optional statistics this run demands (calib_stats.STATS); a record
    without the entry is refused before any data is read."""
    import torch
    from . import ops
    meta = read_sidecar(directory, layer)
    validate_sidecar(meta, expect, layer)
    extra = extra or {}
    entries = {kind: validate_extra_entry(meta, expect["arch"], layer, kind) for kind in KIND_STAT if kind in extra}
    tensors = dict(tensors, **extra)
    for kind in KINDS + tuple(kind for kind in EXTRA_KINDS if kind in extra):
        t = tensors[kind]
        entry = meta["files"][kind]
        numel = stat_numel(kind, entry["n"], entry["batch"])
        slot, host = staging.take(numel)
        read_data_file(directory, layer, kind, entry, host.numpy())
        with torch.cuda.device(t.device):
            if kind in PACKED_KINDS:
                staging.dev[:numel].copy_(host, non_blocking=True)
                ops.sym_unpack_lower(staging.dev[:numel], t)
            else:
                t.view(-1).copy_(host, non_blocking=True)
            staging.mark(slot)
    for kind in VECTOR_KINDS:
        if kind in extra:
            extra[kind].copy_(torch.from_numpy(read_mean_file(directory, layer, entries[kind], kind=kind)))
    return meta


def expectation(adapter, dataset: str, n_samples: int) -> dict:
    """What a sidecar must say to be loaded into THIS run, but for the layer's weight fingerprint."""
    from . import ops
    return {"arch": arch_fingerprint(adapter), "dataset": str(dataset), "n_samples": int(n_samples),
            "model": _model_string(adapter), "cov_mode": ops.COV_MODE, "i8_tolerance": float(ops.i8_tolerance())}


def save(adapter, directory: str, calibs, n_samples: int, batch_size: int, dataset: str, target_layers,
         loaded: Optional[Dict[int, dict]] = None) -> None:
    """Write the record of every target layer of `calibs` (load_calibs' five-tuple) into `directory`, and the BI scores if this
    call has them to write.  loaded: the sidecars the statistics came from when they were loaded (a copy / subset of another
    directory); else they were calibrated just now and the adapter carries what the records need."""
    import torch
    directory = os.path.expandvars(directory)
    cov = dict(zip(("mlp", "q", "k", "x"), calibs[:4]))
    bi_scores = calibs[4]
    targets = resolve_targets(adapter, target_layers)
    arch, model = arch_fingerprint(adapter), _model_string(adapter)
    os.makedirs(directory, exist_ok=True)
    calibration = None
    if loaded is None:
        calibration = {"dataset": str(dataset), "n_samples": int(n_samples), "batch_size": int(batch_size),
                       "n_texts": int(sum(len(b) for b in adapter.calibs)), "n_tokens": int(adapter.calib_tokens)}
        certificates = certificates_in_force(adapter)
    nbytes = 0
    from .calibration import collected
    extra = {}      # file kind -> per-layer list, for the optional statistics this run collects (none: today's record, bit for bit)
    for stat in STATS:
        if not collected(stat, adapter):
            continue
        value = getattr(adapter, stat.stats_attr, None)
        lists = None if value is None else (value,) if len(stat.kinds) == 1 else tuple(value)
        if targets and (lists is None or any(lst[i] is None for i in targets for lst in lists)):
            raise RuntimeError(f"{stat.switch}=1 but the adapter carries no {stat.noun} (adapter.{stat.stats_attr}) to save")
        if lists is not None:
            extra.update(zip(stat.kinds, lists))
    if targets:
        staging = _staging_for(arch, cov["mlp"][targets[0]].device)
        for i in targets:
            cal = calibration if loaded is None else loaded[i]["calibration"]
            cert = certificates if loaded is None else loaded[i]["certificates"]
            meta = write_layer(directory, i, {k: cov[k][i] for k in KINDS}, staging, arch, cal, model,
                               weight_fingerprint(adapter, i), cert, extra={kind: lst[i] for kind, lst in extra.items()})
            nbytes += sum(e["bytes"] for e in meta["files"].values())
        torch.cuda.synchronize(staging.device)
    if bi_scores is not None and getattr(adapter, "calib_want_bi", True):
        write_bi_scores(directory, bi_scores, arch, {"dataset": str(dataset), "n_samples": int(n_samples),
                                                     "batch_size": int(batch_size)}, model)
    logger.info(f"Saved the calibration statistics of layers {targets} to {directory} ({nbytes} bytes)")


def load(adapter, directory: str, n_samples: int, batch_size: int, dataset: str, target_layers):
    """load_calibs without the model: no tokenisation, no forward, no hooks.  Returns (five-tuple, {layer: sidecar})."""
    import torch
    from .calibration import SigmaBuffers
    directory = os.path.expandvars(directory)
    targets = resolve_targets(adapter, target_layers)
    logger.info(f"Detected architecture: {adapter.arch}")
    logger.info(f"target_layers = {targets}")
    logger.info(f"Loading calibration statistics from {directory}")
    expect = expectation(adapter, dataset, n_samples)
    if not os.path.isdir(directory):
        raise FileNotFoundError(f"calibration statistics: directory {directory} (load_calibs_from) does not exist")
    bi_scores = read_bi_scores(directory, expect)
    missing = [i for i in targets if not os.path.exists(sidecar_path(directory, i))]
    if missing:
        read_sidecar(directory, missing[0])      # raises, naming the layer
    sig = SigmaBuffers(adapter, targets)
    metas: Dict[int, dict] = {}
    for stat in STATS:                         # (filled below from the statistic's files; None when this run does not collect it)
        setattr(adapter, stat.stats_attr, sig.value(stat.name))
    if targets:
        staging = _staging_for(expect["arch"], sig.lists["mlp"][targets[0]].device)
        for i in targets:
            metas[i] = read_layer(directory, i, {k: sig.lists[k][i] for k in KINDS}, staging,
                                  dict(expect, weights=weight_fingerprint(adapter, i)),
                                  extra={kind: lst[i] for kind, lst in sig.extra.items()})
        torch.cuda.synchronize(staging.device)
    adapter.bi_scores = bi_scores
    cert = merge_certificates([m["certificates"] for m in metas.values()])
    if cert:
        adapter.calib_tokens = cert["calib_tokens"]
        adapter.cov_routes = cert["cov_routes"]
        if cert.get("cov_rows_left") is not None:
            adapter.cov_rows_left = cert["cov_rows_left"]
        adapter.calib_cov_settings = {k: cert.get(k) for k in ("cov_mode", "i8_tolerance", "i8_rows", "i8_exact", "i8_fuse")}
    logger.info("Finished loading the calibration statistics and BI scores.")
    return (sig.lists["mlp"], sig.lists["q"], sig.lists["k"], sig.lists["x"], bi_scores), metas
