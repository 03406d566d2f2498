"""torch-tensor front ends of the C ABI: pointer/stride extraction, workspace allocation, stream hand-off.

PyTorch is plumbing here (device memory + the current HIP stream); all arithmetic happens in
libmodegpt_hip.so.  Every function requires CUDA(HIP) tensors and raises otherwise.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check
# the host side of the reports (switches, constants, decoders) lives in reports.py; every name stays reachable as ops.<name>
from .reports import (MARGIN_FIELDS, OUTPUT_ERROR_LEVELS, QK_ERROR_TARGETS, QK_MARGIN_FIELDS, RANK_CURVE_KEEP,  # noqa: F401
                      RANK_CURVE_TARGETS, VO_ERROR_TARGETS, VO_SPECTRUM_FIELDS, decode_margin, decode_output_error, decode_qk_logit_error,
                      decode_mlp_greedy, decode_qk_margin, decode_qk_seq_error, decode_rank_curve, decode_vo_output_error, decode_vo_spectrum,
                      greedy_partition, keep_bias_enabled, mlp_greedy_rounds, mlp_intercept_enabled, output_error_enabled, qk_error_enabled, qk_rope_enabled, qk_rope_select_enabled, qk_seq_enabled,
                      qk_causal_enabled, qk_causal_select_enabled, qk_select_statistic, decode_qk_causal_error,
                      qk_seq_select_enabled,                      rank_curve_enabled, vo_error_enabled, vo_intercept_enabled)

_DT = {torch.bfloat16: _lib.MDG_BF16, torch.float16: _lib.MDG_F16, torch.float32: _lib.MDG_F32,
       torch.float64: _lib.MDG_F64}


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_gpu(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("modegpt_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")


def _ws(nbytes: int, device) -> Tuple[Optional[torch.Tensor], int]:
    if nbytes == 0:
        return None, 0
    t = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t, t.data_ptr()


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _as_weight(W: torch.Tensor) -> torch.Tensor:
    """Weights enter the fp64 GEMMs either as bf16 (converted exactly on load) or as fp64; fp16 / fp32 checkpoints are
    widened to fp64 first, exactly, instead of being squeezed through bf16."""
    W = W.detach()
    if W.dtype not in (torch.bfloat16, torch.float64):
        W = W.to(torch.float64)
    return W if W.stride(-1) == 1 else W.contiguous()


# ------------------------------------------------------------------ deferred status of a decomposition chain
class DeferredStatus:
    """`with ops.DeferredStatus(device) as st: <ridge_scores / nystrom_down / vo_compress / potrf_lower ...>` -- inside the block
    the decomposition entry points do not wait for the host to read their status word (Cholesky pivot, Jacobi convergence):
    they merge it into a device-side int[2] and return at once (mdg_deferred_status_begin / _end).  `st.check()` -- any time
    later -- copies the two ints to the host (the one synchronisation of the chain) and raises what the synchronising call
    would have raised: torch.linalg.LinAlgError for a matrix that is not positive definite, RuntimeError otherwise."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.status = torch.empty(2, dtype=torch.int32, device=self.device)
        self.checked = False

    def __enter__(self):
        with torch.cuda.device(self.device):
            check(_lib.load().mdg_deferred_status_begin(self.status.data_ptr(), _stream(self.status)), "mdg_deferred_status_begin")
        return self

    def __exit__(self, *exc):
        _lib.load().mdg_deferred_status_end()
        return False

    def check(self) -> None:
        if self.checked:
            return
        self.checked = True
        host = (C.c_int * 2)(*self.status.cpu().tolist())
        check(_lib.load().mdg_deferred_status_decode(host), "decomposition chain")


# ------------------------------------------------------------------ covariance
_I8_DTYPES = (torch.bfloat16, torch.float16)       # element types the int8 digit-plane kernels split (include/modegpt_hip.h, MDG_I8_F16)


def _cov_problem(sigma: torch.Tensor, x: torch.Tensor, n_heads: int = 1, i8: Optional[str] = None, dtype=None):
    """The prologue of every covariance front end: checks the pair and returns (x as [tokens, n_heads * feat] with contiguous rows,
    its mdg_cov_problem with sigma's leading dimension feat and batch stride feat * feat).  i8: the int8 entry that asks
    ("cov_accum_i8": sigma is one matrix; "cov_accum_i8_multi": per-head statistics need a [n_heads, feat, feat] sigma) -- x must
    then be bf16 or fp16, and of `dtype` when the call already has an element type."""
    _need_gpu(sigma, x)
    single = i8 == "cov_accum_i8"
    if sigma.dtype != torch.float64 or not sigma.is_contiguous() or (single and sigma.dim() != 2):
        raise ValueError(f"sigma must be a contiguous {'2-D ' if single else ''}float64 tensor")
    if i8 and (x.dtype not in _I8_DTYPES or x.dtype != (dtype or x.dtype)):
        raise ValueError(f"{i8} takes bf16 or fp16 activations" + ("" if single else ", one element type per call"))
    x2 = x.detach().reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    shape, (n_tok, width) = sigma.shape, x2.shape
    feat = shape[-1]
    per_head_ok = not i8 or n_heads == 1 or (len(shape) == 3 and shape[0] == n_heads)
    if shape[-2] != feat or width != n_heads * feat or not per_head_ok:
        raise ValueError(f"shape mismatch: sigma {tuple(shape)}, x {tuple(x2.shape)}" if single else
                         f"shape mismatch: x {tuple(x.shape)} vs sigma {tuple(shape)} with n_heads={n_heads}")
    if len(shape) == 3 and shape[0] != n_heads:
        raise ValueError("sigma batch dimension must equal n_heads")
    return x2, _lib.CovProblem(x2.data_ptr(), n_tok, feat, n_heads, x2.stride(0), sigma.data_ptr(), feat, feat * feat)


def cov_accum(sigma: torch.Tensor, x: torch.Tensor, n_heads: int = 1, relu: bool = False) -> None:
    """sigma (lower triangle) += X^T X in fp64.  x: [..., n_heads*feat] (bf16/f16/f32/f64, last dim
    contiguous, viewed as [tokens, n_heads*feat]); sigma: [feat, feat] or [n_heads, feat, feat] fp64.
    Only the lower triangle is valid until cov_finalize()."""
    _cov_f64_call(*_cov_problem(sigma, x, n_heads), relu)


def _cov_f64_call(x2: torch.Tensor, p: "_lib.CovProblem", relu: bool = False) -> None:
    """mdg_cov_accum on one problem _cov_problem built (x2: the activation p.x points into)."""
    lib = _lib.load()
    n_tok, feat, n_heads = p.n_tokens, p.n_feat, p.batch
    nbytes = lib.mdg_cov_accum_ws_bytes(n_tok, feat, n_heads)
    ws, wsp = _ws(nbytes, x2.device)
    with torch.cuda.device(x2.device):
        check(lib.mdg_cov_accum(p.x, _DT[x2.dtype], n_tok, feat, n_heads, p.ld, int(relu), p.sigma, p.ld_sigma, p.sigma_batch_stride,
                                wsp, nbytes, _stream(x2)), "mdg_cov_accum")


def cov_accum_i8(sigma: torch.Tensor, x: torch.Tensor, events=None, mfma_stats: Optional[dict] = None,
                 report: bool = True, route_info: Optional[dict] = None, tolerance: Optional[float] = None,
                 relu: bool = False, rows: Optional[bool] = None) -> Optional[int]:
    """sigma (lower triangle) += X^T X for one bf16 or fp16 matrix (relu=True: of max(x, 0), applied on load) through the int8 digit-plane kernel (csrc/cov_i8.hip): error-free
    split into digit planes, truncated plane-pair product.  The route -- five planes or six, which columns leave the int8 path
    for the fp64 column kernel (at most 32), or the fp64 kernel for the whole statistic -- is derived on the device from a
    per-call error bound (guaranteed <= 1.1e-11 of sqrt(sigma_ii sigma_jj) entry-wise, typically 1e-13; include/modegpt_hip.h);
    the result is valid either way.  tolerance: the factor on the route's thresholds for THIS call (None: i8_tolerance(), the
    calling thread's default).  report=True (tests, measurements) returns the route of this
    call (5, 6, or 0 for the fp64 kernel) at the price of one stream synchronisation and books it in I8_STATS;
    report=False (the hooks: cov_accum_multi) only enqueues and returns None -- the per-device counters behind
    i8_route_counts() are updated by the kernels themselves in both modes.  Feature count must be a multiple of 128.
    route_info: optional dict, filled with {"planes", "columns" (those the fp64 column kernel computed), "sq", "x" (the two parts
    of the bound for the columns that stayed), "bound" (their sum), "exact" (the call ran the exact route: no plane pair dropped,
    the bound is the rounded-element term + fp64 rounding), "remainder" ("tiles" / "wide": which implementation of the exact
    route's remainder products the device picked; None off the exact route)} -- implies report.
    events: optional pair of torch.cuda.Event(enable_timing=True), each recorded once already, re-recorded around the product
    launches alone.  mfma_stats: optional dict; its "executed" entry is increased by the number of v_mfma instructions the
    product kernel issued (it skips digit planes that are all-zero over a tile panel) and "dense" by what a kernel without
    that skipping issues -- costs a stream synchronisation, for measurement only (implies report).
    rows: let up to 64 outlier token rows leave the int8 path for the fp64 row kernel (MDG_I8_ROWS, include/modegpt_hip.h; None:
    ops.I8_ROWS); route_info then also holds "rows", the tokens that left, ascending."""
    x2, p = _cov_problem(sigma, x, i8="cov_accum_i8")
    nbytes = _lib.load().mdg_cov_accum_i8_ws_bytes(p.n_tokens, p.n_feat)
    used, infos = _cov_i8_call("mdg_cov_accum_i8", (x2.data_ptr(), p.n_tokens, p.n_feat, p.ld, sigma.data_ptr(), sigma.stride(0)),
                               (_lib.CovProblem * 1)(p), nbytes, x2, events, mfma_stats, report, route_info is not None, tolerance,
                               relu, rows)
    if route_info is not None:
        route_info.update(infos[0])
    return used


def _cov_i8_call(entry: str, head: tuple, arr, nbytes: int, x2: torch.Tensor, events, mfma_stats: Optional[dict], report: bool,
                 want_infos: bool, tolerance: Optional[float], relu: bool, rows: Optional[bool]):
    """An int8 covariance call once its problems are built: lib.<entry>(*head, workspace, tolerance, flags, route, counters, events,
    stream) on x2's device and stream, then the read-backs that were asked for.  arr: the call's mdg_cov_problem array (the
    read-backs address a statistic through it), nbytes: its workspace.  Returns (the route -- None unless the call reports --, one
    route dict per statistic -- None unless want_infos or mfma_stats) and does the mfma_stats / I8_STATS bookkeeping described at
    cov_accum_i8."""
    lib = _lib.load()
    count, dev = len(arr), x2.device
    ws, wsp = _ws(nbytes, dev)
    report = report or mfma_stats is not None or want_infos
    used = C.c_int(0)
    flags = _i8_flags(x2.dtype, relu, rows)
    infos = None
    with torch.cuda.device(dev):
        stream = _stream(x2)
        check(getattr(lib, entry)(*head, wsp, nbytes, i8_tolerance() if tolerance is None else float(tolerance), flags,
                                  C.byref(used) if report else None, _route_counters(dev).data_ptr(),
                                  None if events is None else events[0].cuda_event,
                                  None if events is None else events[1].cuda_event, stream), entry)
        if want_infos or mfma_stats is not None:
            infos = [_read_route(lib, count, arr, i, wsp, stream, flags) for i in range(count)]
        if mfma_stats is not None and used.value in (5, 6):
            done = C.c_ulonglong(0)
            check(lib.mdg_cov_accum_i8_stats(wsp, 0, 0, C.byref(done), stream), "mdg_cov_accum_i8_stats")    # (the whole launch's count)
            ran = 3 if any(i_["exact"] for i_ in infos) else used.value      # (the exact route: the three-plane product launch, all nine pairs)
            mfma_stats["executed"] = mfma_stats.get("executed", 0) + done.value
            mfma_stats["dense"] = mfma_stats.get("dense", 0) + sum(i8_dense_mfma_count(q.n_tokens, q.n_feat, ran, q.batch) for q in arr)
            mfma_stats["planes_run"] = ran
    if not report:
        return None, infos
    I8_STATS[{5: "i8_5", 6: "i8_6"}.get(used.value, "fallback_f64")] += count
    return used.value, infos


def _read_route(lib, count, arr, stat, wsp, stream, flags: int = 0) -> dict:
    planes, ncol, exact = C.c_int(0), C.c_int(0), C.c_int(0)
    cols = (C.c_int * 32)()
    bound = (C.c_double * 2)()
    check(lib.mdg_cov_accum_i8_route(count, arr, stat, wsp, C.byref(planes), C.byref(ncol), cols, bound, C.byref(exact), stream),
          "mdg_cov_accum_i8_route")
    info = {"planes": planes.value, "columns": [cols[i] for i in range(ncol.value)], "sq": bound[0], "x": bound[1],
            "bound": bound[0] + bound[1], "exact": bool(exact.value),
            "remainder": {0: None, 1: "tiles", 2: "wide"}.get(exact.value)}
    if flags & _lib.MDG_I8_ROWS:       # the token rows the fp64 row kernel computed
        n_rows = C.c_int(0)
        rows = (C.c_int * _lib.MDG_I8_MAX_ROWS)()
        check(lib.mdg_cov_accum_i8_rows(count, arr, stat, wsp, C.byref(n_rows), rows, stream), "mdg_cov_accum_i8_rows")
        info["rows"] = [rows[i] for i in range(n_rows.value)]
    return info


# The exact route of the int8 covariance (include/modegpt_hip.h, "THE EXACT ROUTE"): "auto" (default) takes it where it is the
# faster product -- launches of the six-plane class (the MLP statistic of a gated model) and five-plane launches of a statistic of
# 4096 features and more; "always" (True) wherever the remainder lists fit (fp64-rounding accuracy for every int8 statistic);
# "never" (False) keeps every call on the truncated five- / six-plane product with its bound.  MODEGPT_I8_EXACT=auto|1|0.
I8_EXACT = {"1": True, "always": True, "0": False, "never": False}.get(os.environ.get("MODEGPT_I8_EXACT", "auto").lower(), "auto")


# Outlier token rows (include/modegpt_hip.h, "OUTLIER TOKEN ROWS"): when on, a handful of tokens that are large across many columns
# leave the int8 path for an fp64 row kernel instead of dragging the whole statistic to the fp64 kernel.  Opt-in: MODEGPT_I8_ROWS=1.
I8_ROWS = os.environ.get("MODEGPT_I8_ROWS", "0").lower() in ("1", "on", "true")


def _i8_flags(dtype=torch.bfloat16, relu: bool = False, rows: Optional[bool] = None) -> int:
    return ({True: _lib.MDG_I8_EXACT_ALWAYS, False: _lib.MDG_I8_NO_EXACT}.get(I8_EXACT, 0)
            | (_lib.MDG_I8_F16 if dtype == torch.float16 else 0) | (_lib.MDG_I8_RELU if relu else 0)
            | (_lib.MDG_I8_ROWS if (I8_ROWS if rows is None else rows) else 0))


def cov_accum_i8_multi(items, events=None, mfma_stats: Optional[dict] = None, report: bool = False,
                       route_info: Optional[list] = None, tolerance: Optional[float] = None, relu: bool = False,
                       rows: Optional[bool] = None) -> Optional[int]:
    """Several statistics of ONE calibration batch through the int8 digit-plane kernels in one persistent product launch
    (mdg_cov_accum_i8_multi): items = sequence of (sigma, x, n_heads), largest first, at most 4, all bf16 or all fp16, with the same
    token count (relu=True: max(x, 0) on load, for every statistic of the call).  n_heads == 1: sigma [n, n], n a multiple of 128; n_heads > 1: per-head Grams, sigma [n_heads, 128, 128] of an
    activation [tokens, n_heads * 128].  The tiles of all statistics share one tile schedule -- the small ones fill what the
    large one's last round leaves idle -- and one route: the deepest any column of any of them asks for (more planes are
    never less exact); a statistic too heavy-tailed for six planes leaves the launch alone (fp64 kernel).  events / mfma_stats /
    report as in cov_accum_i8 (report: the planes of the statistics that stayed, 0 if none did; the executed / dense counts cover
    all statistics and assume none fell back).  route_info: optional list, extended by one dict per statistic (see cov_accum_i8).
    rows as in cov_accum_i8, for every statistic of the call."""
    items = list(items)
    built = [_cov_problem(sigma, x, n_heads, i8="cov_accum_i8_multi", dtype=items[0][1].dtype) for sigma, x, n_heads in items]
    arr = (_lib.CovProblem * len(built))(*(p for _, p in built))
    x2 = built[0][0]                 # (`built` keeps every row-contiguous copy alive until the launch is enqueued)
    nbytes = _lib.load().mdg_cov_accum_i8_multi_ws_bytes(len(built), arr)
    if nbytes == 0 and x2.shape[0] > 0:
        raise ValueError("these statistics cannot share an int8 launch (token counts differ, widths not multiples of 128, or "
                         "per-head statistics with head_dim != 128)")
    used, infos = _cov_i8_call("mdg_cov_accum_i8_multi", (len(built), arr), arr, nbytes, x2, events, mfma_stats, report,
                               route_info is not None, tolerance, relu, rows)
    if route_info is not None:
        route_info.extend(infos)
    return used


def _device_index(device=None) -> int:
    """The index of a CUDA device; None and a device without an index ("cuda") stand for the current device."""
    index = None if device is None else torch.device(device).index
    return torch.cuda.current_device() if index is None else index


_ROUTE_COUNTERS = {}


def _route_counters(device) -> torch.Tensor:
    """Per-device int32[6] the kernels bump: [five planes, six planes, fp64 fallback of a whole statistic, columns handed to the
    fp64 column kernel, statistics on the exact route, token rows handed to the fp64 row kernel (MDG_I8_ROWS calls only)]
    (mdg_cov_accum_i8 route_counts)."""
    key = _device_index(device)
    if key not in _ROUTE_COUNTERS:
        _ROUTE_COUNTERS[key] = torch.zeros(6, dtype=torch.int32, device=torch.device("cuda", key))
    return _ROUTE_COUNTERS[key]


# The accuracy / speed dial of the int8 covariance route is an ARGUMENT of every call (mdg_cov_accum_i8's `tolerance`, ABI 9); the
# library keeps no accuracy state.  What is kept here, on the Python side, is only the default a call without an explicit
# `tolerance=` uses: a process default (set_i8_tolerance; initialised from the environment variable MODEGPT_I8_TOLERANCE when this
# module is imported) that a thread can override for itself (i8_tolerance_scope) without touching any other caller's arithmetic.
def _checked_tolerance(factor) -> float:
    f = float(factor)
    if not (1.0 <= f <= 1e6):
        raise ValueError(f"int8 route tolerance factor {f!r} outside [1, 1e6] (1 = guaranteed <= 1.1e-11)")
    return f


_I8_TOLERANCE_DEFAULT = _checked_tolerance(os.environ.get("MODEGPT_I8_TOLERANCE", "1") or "1")
_I8_TOLERANCE_LOCAL = threading.local()


def i8_tolerance() -> float:
    """The tolerance factor a cov_accum_i8 / cov_accum_i8_multi / cov_accum_multi call made by THIS thread uses when it is not
    given one: the innermost i8_tolerance_scope of the thread, else the process default."""
    stack = getattr(_I8_TOLERANCE_LOCAL, "stack", None)
    return stack[-1] if stack else _I8_TOLERANCE_DEFAULT


def set_i8_tolerance(factor: float) -> float:
    """Sets the process DEFAULT of the int8 route's tolerance factor (`factor` >= 1 on both thresholds of the per-call error bound;
    1 = guaranteed <= 1.1e-11 of sqrt(sigma_ii sigma_jj)) and returns the previous default.  A Python-side default only: every
    library call carries its factor as an argument."""
    global _I8_TOLERANCE_DEFAULT
    prev, _I8_TOLERANCE_DEFAULT = _I8_TOLERANCE_DEFAULT, _checked_tolerance(factor)
    return prev


@contextlib.contextmanager
def i8_tolerance_scope(factor: float):
    """`with ops.i8_tolerance_scope(64): ...` -- the calling THREAD's default inside the block (hooks enqueued from it included);
    other threads keep theirs."""
    stack = getattr(_I8_TOLERANCE_LOCAL, "stack", None)
    if stack is None:
        stack = _I8_TOLERANCE_LOCAL.stack = []
    stack.append(_checked_tolerance(factor))
    try:
        yield
    finally:
        stack.pop()


def i8_route_counts(device=None, reset: bool = False) -> dict:
    """How the int8-route requests on `device` (default: the current one) were served so far, counted on the device by the
    kernels that ran: {"i8_5", "i8_6", "fallback_f64"} count statistics (by the class the route kernel gave them), "fp64_columns"
    the single columns the route handed to the fp64 column kernel, "exact" how many of the i8_5 / i8_6 statistics ran the exact
    route (nine plane pairs + the fp64 remainder products) instead of the truncated product.  One small device -> host copy;
    calibration reads it once, at the end.  (The sixth counter, the rows of MDG_I8_ROWS calls, is read by i8_rows_left; reset
    clears it too.)"""
    t = _route_counters(device)
    v = t.cpu().tolist()
    if reset:
        t.zero_()
    return {"i8_5": v[0], "i8_6": v[1], "fallback_f64": v[2], "fp64_columns": v[3], "exact": v[4]}


def i8_rows_left(device=None, reset: bool = False) -> int:
    """Token rows the int8 covariance calls on `device` (default: the current one) handed to the fp64 row kernel so far (calls with
    the rows option, MDG_I8_ROWS; counted on the device).  reset clears this counter only."""
    t = _route_counters(device)
    v = int(t[5].item())
    if reset:
        t[5] = 0
    return v


def i8_dense_mfma_count(n_tokens: int, n: int, planes: int, n_heads: int = 1) -> int:
    """v_mfma_i32_32x32x32_i8 instructions of the digit-plane product without zero-plane skipping: every 32 x 32 block of
    the tiles covering the lower triangle (128 x 128 tiles for five planes, 128 x 64 for six; the diagonal tiles whole), per
    k-step of 32 tokens, planes (planes + 1) / 2 plane pairs.  n_heads > 1: per-head statistics of width n = 128 each -- one
    diagonal 128 x 128 tile (16 blocks) per head."""
    rb, nk = n // 128, -(-n_tokens // 32)
    if n_heads > 1:
        blocks = n_heads * 16
    else:
        blocks = rb * (rb + 1) * 8 if planes == 6 else rb * (rb + 1) // 2 * 16
    return blocks * nk * {3: 9, 5: 15, 6: 21}[planes]       # (3: the exact route's product -- three planes, all nine pairs)


# Which matrix cores accumulate the large covariances of a layer: "f64" (v_mfma_f64, the accumulation order of the
# reference's fp64 matmul) or "i8" (error-free digit-plane split, truncated product on the int8 cores, csrc/cov_i8.hip; what it
# cannot take stays on the fp64 kernel, and every call derives its route -- planes, columns for the fp64 column kernel, or the
# fp64 kernel -- from its own error bound).
COV_MODE = os.environ.get("MODEGPT_COV_MODE", "i8")
I8_MIN_FEATURES = 2048
I8_STATS = {"i8_5": 0, "i8_6": 0, "fallback_f64": 0}      # routes of the REPORTING cov_accum_i8 calls (tests, bench); all calls: i8_route_counts()


def takes_i8_planes(width: int, dtype=torch.bfloat16, n_heads: int = 1, relu: bool = False, min_features: Optional[int] = None) -> bool:
    """Whether a statistic runs on the int8 digit planes when the mode is "i8" -- the one rule the launch plan, cov_accum_fc_relu
    and the error bound the selection certificate is taken against (compress_mlp.covariance_error_eps) share.  width: the side of
    one Gram matrix (the head_dim of a per-head statistic).  bf16 / fp16 only; per-head statistics (which run beside a plane, as
    diagonal tiles of its launch) need head_dim 128; a single matrix a multiple of 128 of at least min_features (default
    ops.I8_MIN_FEATURES) features, with ReLU on load (OPT's fc1 statistic) of at least FC_I8_MIN_FEATURES.
    Below ~2048 features the 128 x 128 tiles do not fill the 256 CUs and the fp64 kernel is the faster one
    (scripts/probes/i8_small_n.py: 1536 features 1.35 vs 1.23 ms, 2048 features 1.40 vs 2.14 ms)."""
    if dtype not in _I8_DTYPES:
        return False
    if n_heads > 1:
        return width == 128
    least = FC_I8_MIN_FEATURES if relu else I8_MIN_FEATURES if min_features is None else min_features
    return width % 128 == 0 and width >= least


class CovStat(NamedTuple):
    """What the launch plan looks at of one statistic (sigma, x, n_heads)."""
    width: int          # sigma.shape[-1]
    n_heads: int
    dtype: torch.dtype  # of x
    sigma_dim: int
    tokens: int


COV_JOIN = ("join",)       # the step of a plan at which the caller's stream waits for the side stream


def plan_cov_launches(stats: Sequence[CovStat], mode: str, *, fuse: bool, overlap: bool, fusable_device: bool,
                      min_features: int) -> list:
    """The launches of cov_accum_multi for the statistics `stats` (largest first), in the order they are enqueued -- a pure
    function of its arguments (the ops.* switches come in as arguments).  Steps, over indices into stats:
    ("i8", [i]) one statistic in an int8 launch of its own, ("i8_multi", [i, ...]) two to four in one persistent int8 launch,
    ("f64", [i, ...], on_side_stream) the fp64 kernel -- on the side stream, forked off the caller's stream at this step, or on
    the caller's --, COV_JOIN the caller's stream waits for the side stream.  tests/test_cov_plan_host.py is the table of cases.
    Fused (fuse, on a device the persistent launch's tile schedule is cut for): the largest plane (sigma_mlp) keeps a launch and a
    route of its own -- on a real gated MLP it is the heavy-tailed one (six planes) while the others take five, and a shared launch
    would drag them along (measured: -2 % on SiLU-gated data); the other planes and the per-head statistics of head_dim 128 share
    ONE launch (one tile schedule, one k-split last round, no fp64 launch for the heads) when they are at most four of one
    element type and all int8 statistics have one token count; what is left runs on fp64 beside all of that.  Otherwise every
    plane has its launch and the heads join the rest, which runs beside the LAST -- smallest -- plane, whose few hundred tiles
    leave CUs idle in their final round; the large planes keep the chip to themselves."""
    if mode not in ("f64", "i8"):
        raise ValueError(f"covariance mode must be 'f64' or 'i8', got {mode!r}")
    planes, heads, rest = [], [], []
    for i, s in enumerate(stats):
        takes = mode == "i8" and s.sigma_dim == (2 if s.n_heads == 1 else 3) and \
            takes_i8_planes(s.width, s.dtype, s.n_heads, min_features=min_features)
        (rest if not takes else planes if s.n_heads == 1 else heads).append(i)
    group = ((planes[1:] if len(planes) > 1 else planes) + heads) if planes else []
    fused = bool(planes) and fuse and fusable_device and len(group) <= 4 and len({stats[i].dtype for i in group}) == 1 and \
        len({stats[i].tokens for i in planes + heads}) == 1
    if fused:
        i8 = ([("i8", planes[:1])] if len(planes) > 1 else []) + [("i8_multi" if len(group) > 1 else "i8", group)]
    else:
        i8, rest = [("i8", [i]) for i in planes], heads + rest
    if not rest:
        return i8
    if not (planes and overlap):
        return i8 + [("f64", rest, False)]
    before = 0 if fused else len(i8) - 1
    return i8[:before] + [("f64", rest, True)] + i8[before:] + [COV_JOIN]


def cov_accum_multi(items, mode: Optional[str] = None) -> None:
    """The covariance problems of one calibration batch.  items: sequence of (sigma, x, n_heads), largest problem first.
    mode (default ops.COV_MODE): "f64" sends all of them through the fp64 kernel; "i8" sends every bf16 or fp16 statistic the int8
    digit-plane kernels can take (takes_i8_planes: single matrices of at least I8_MIN_FEATURES features, a multiple of 128, and,
    beside one of those, per-head statistics of head_dim 128) through them and only the rest through the fp64 kernel.  Which
    launches that makes, in which order and on which stream: plan_cov_launches.  The fp64 part is one launch, or one cov_accum call
    per item when the fused kernel's preconditions do not hold (mixed dtypes, feature count not a multiple of 128, unaligned rows)."""
    items = [(s_, x_, h_) for (s_, x_, h_) in items if x_.numel() > 0]
    if not items:
        return
    mode = mode or COV_MODE
    dev = items[0][1].device
    stats = [CovStat(s_.shape[-1], h_, x_.dtype, s_.dim(), x_.numel() // x_.shape[-1]) for s_, x_, h_ in items]
    steps = plan_cov_launches(stats, mode, fuse=I8_FUSE, overlap=COV_OVERLAP_SMALL, min_features=I8_MIN_FEATURES,
                              fusable_device=mode == "i8" and I8_FUSE and _fusable_device(dev))
    main = side = None
    for step in steps:
        if step == COV_JOIN:
            main.wait_stream(side)       # later work on the caller's stream (and any reuse of these buffers) is ordered after both
            continue
        chosen = [items[i] for i in step[1]]
        if step[0] == "i8":
            cov_accum_i8(chosen[0][0], chosen[0][1], report=False)
        elif step[0] == "i8_multi":
            cov_accum_i8_multi(chosen, report=False)
        elif step[2]:
            main, side = torch.cuda.current_stream(dev), _side_stream(dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                _cov_accum_fused(chosen)
        else:
            _cov_accum_fused(chosen)


# Width from which OPT's fc1 statistic (ReLU on load) takes the int8 digit planes: where the exact route is offered by default
# (cov_i8_exact.hip LO_AUTO_MIN_N), i.e. where the statistic keeps fp64-rounding accuracy whenever its remainder lists fit.
FC_I8_MIN_FEATURES = 4096


def cov_accum_fc_relu(sigma: torch.Tensor, x: torch.Tensor, mode: Optional[str] = None) -> None:
    """sigma += ReLU(x)^T ReLU(x), the ReLU fused into the kernels' loads (OPT's fc1 statistic): bf16 / fp16 activations of at
    least FC_I8_MIN_FEATURES features (a multiple of 128) through the int8 digit planes (cov_accum_i8(relu=True)) unless mode is
    "f64"; everything else through the fp64 kernel (cov_accum(relu=True))."""
    if (mode or COV_MODE) == "i8" and takes_i8_planes(x.shape[-1], x.dtype, relu=True) and x.numel() > 0:
        cov_accum_i8(sigma, x, report=False, relu=True)
    else:
        cov_accum(sigma, x, relu=True)


_SIDE_STREAMS = {}
I8_FUSE = os.environ.get("MODEGPT_I8_FUSE", "1") != "0"      # one int8 launch for all eligible statistics of a batch (cov_accum_i8_multi)


def _fusable_device(device) -> bool:
    """The fused int8 launch is a persistent launch over a tile schedule cut for 8 XCDs x 32 CUs."""
    return torch.cuda.get_device_properties(device).multi_processor_count == 256


COV_OVERLAP_SMALL = os.environ.get("MODEGPT_COV_OVERLAP", "1") != "0"
NYSTROM_OVERLAP = os.environ.get("MODEGPT_NYSTROM_OVERLAP", "1") != "0"   # cross product of the Nystrom refit beside the factorisation of C_kk


def _side_stream(device, purpose: str = "cov", beside=None) -> "torch.cuda.Stream":
    """One helper stream per (device, purpose[, the stream it runs beside]): two layers' chains on two streams of the caller's
    get a helper each and stay independent of one another."""
    dev = _device_index(device)
    key = (dev, purpose, None if beside is None else beside.cuda_stream)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _SIDE_STREAMS[key]


def _cov_accum_fused(items) -> None:
    """The fp64 part of cov_accum_multi: one fused launch when the preconditions hold, else one mdg_cov_accum call per item."""
    built = [_cov_problem(sigma, x, n_heads) for sigma, x, n_heads in items]
    x0 = built[0][0]
    if not (len(built) <= 4 and all(x2.dtype == x0.dtype and p.n_feat % 128 == 0 and x2.data_ptr() % 16 == 0 and
                                    (x2.stride(0) * x2.element_size()) % 16 == 0 and x2.device == x0.device for x2, p in built)):
        for x2, p in built:
            _cov_f64_call(x2, p)
        return
    lib = _lib.load()
    arr = (_lib.CovProblem * len(built))(*(p for _, p in built))
    nbytes = lib.mdg_cov_accum_multi_ws_bytes(len(built), arr, _DT[x0.dtype])
    ws, wsp = _ws(nbytes, x0.device)
    with torch.cuda.device(x0.device):
        check(lib.mdg_cov_accum_multi(len(built), arr, _DT[x0.dtype], wsp, nbytes, _stream(x0)), "mdg_cov_accum_multi")


def cov_finalize(sigma: torch.Tensor, scale: float) -> None:
    """sigma <- scale * sigma (lower) mirrored into the upper triangle."""
    _need_gpu(sigma)
    lib = _lib.load()
    n = sigma.shape[-1]
    batch = 1 if sigma.dim() == 2 else sigma.shape[0]
    with torch.cuda.device(sigma.device):
        check(lib.mdg_cov_finalize(sigma.data_ptr(), n, batch, n, n * n, float(scale), _stream(sigma)),
              "mdg_cov_finalize")


COL_SUM_CHUNK = 128        # tokens per workgroup of mdg_col_sum_accum (one partial row each)
COV_CENTER_TILE = 64       # tile edge of mdg_cov_center


def col_sum_accum(sum_: torch.Tensor, x: torch.Tensor, relu: bool = False) -> None:
    """sum_[j] += sum_t f(x[t, j]) in fp64 (mdg_col_sum_accum): x [..., n] of bf16 / fp16 / fp32 / fp64, read in place when its rows are
    contiguous and equally spaced (any leading dimension, any element-aligned offset); f = ReLU with relu=True.  sum_: fp64 [n],
    contiguous.  Deterministic, no atomics.  The call only enqueues."""
    _need_gpu(sum_, x)
    lib = _lib.load()
    n = x.shape[-1]
    if sum_.dtype != torch.float64 or sum_.dim() != 1 or sum_.numel() != n or not sum_.is_contiguous():
        raise ValueError(f"col_sum_accum: sum must be a contiguous float64 vector of {n} entries")
    if x.dtype not in _DT:
        raise ValueError(f"col_sum_accum: unsupported dtype {x.dtype}")
    x2 = x.detach()
    if x2.dim() != 2:
        x2 = x2.reshape(-1, n)              # (a view when the leading dimensions collapse, as the hooks' [batch, T, n] does)
    if x2.shape[0] == 0:
        return
    if x2.stride(1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < n):
        x2 = x2.contiguous()
    tokens = x2.shape[0]
    ld = x2.stride(0) if tokens > 1 else n
    nbytes = lib.mdg_col_sum_ws_bytes(tokens, n)
    ws, wsp = _ws(nbytes, x2.device)
    with torch.cuda.device(x2.device):
        check(lib.mdg_col_sum_accum(x2.data_ptr(), _DT[x2.dtype], tokens, n, ld, int(bool(relu)), sum_.data_ptr(), wsp, nbytes,
                                    _stream(x2)), "mdg_col_sum_accum")


def cov_center(Cm: torch.Tensor, mu: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """S = C - mu mu^T, S_ij = fma(-mu_i, mu_j, C_ij) (mdg_cov_center): C fp64 [n, n] with contiguous rows (any row stride), read at
    and below its diagonal; mu fp64 [n]; the result is written in both triangles from one value, symmetric bit for bit.  out: an fp64
    [n, n] view with contiguous rows to write into (default: a new tensor); C itself is not modified.  The call only enqueues."""
    _need_gpu(Cm, mu, out)
    lib = _lib.load()
    n, _, ldc, _ = _sym_view(Cm)
    if Cm.dim() != 2 or mu.dtype != torch.float64 or mu.numel() != n:
        raise ValueError(f"cov_center: C must be [n, n] and mu a float64 vector of {n} entries")
    mu = mu.contiguous()
    if out is None:
        out = torch.empty(n, n, dtype=torch.float64, device=Cm.device)
    n_o, _, lds, _ = _sym_view(out)
    if out.dim() != 2 or n_o != n:
        raise ValueError("cov_center: out must be [n, n] like C")
    with torch.cuda.device(Cm.device):
        check(lib.mdg_cov_center(Cm.data_ptr(), n, ldc, mu.data_ptr(), out.data_ptr(), lds, _stream(Cm)), "mdg_cov_center")
    return out


def _sym_view(full: torch.Tensor):
    """(n, batch, ld, batch stride) of a [n, n] or [batch, n, n] fp64 view whose rows are contiguous."""
    if full.dtype != torch.float64 or full.dim() not in (2, 3) or full.shape[-1] != full.shape[-2] or full.stride(-1) != 1:
        raise ValueError("a symmetric statistic is a float64 [n, n] or [batch, n, n] tensor with contiguous rows")
    n = full.shape[-1]
    batch = 1 if full.dim() == 2 else full.shape[0]
    ld = full.stride(-2) if n > 1 else max(full.stride(-2), 1)
    bs = full.stride(0) if full.dim() == 3 and batch > 1 else n * ld
    if ld < n or (batch > 1 and bs < (n - 1) * ld + n):
        raise ValueError("the matrices of a symmetric statistic must not overlap")
    return n, batch, ld, bs


def sym_pack_lower(full: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The lower triangle (diagonal included) of `full` -- fp64 [n, n] or [batch, n, n], any row / batch stride -- as n(n+1)/2
    contiguous doubles per matrix in row-major packed order (row i at offset i(i+1)/2): out[np.tril_indices(n)] order.  Nothing
    above the diagonal is read; bit patterns are moved, not values.  out: a contiguous fp64 device tensor of batch * n(n+1)/2
    elements to write into (default: a new one).  Returns it, shaped [n(n+1)/2] or [batch, n(n+1)/2]."""
    _need_gpu(full, out)
    n, batch, ld, bs = _sym_view(full)
    m = n * (n + 1) // 2
    shape = (m,) if full.dim() == 2 else (batch, m)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=full.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != batch * m or out.device != full.device:
        raise ValueError(f"out must be a contiguous float64 tensor of {batch * m} elements on {full.device}")
    with torch.cuda.device(full.device):
        check(_lib.load().mdg_sym_pack_lower(full.data_ptr(), n, batch, ld, bs, out.data_ptr(), _stream(full)),
              "mdg_sym_pack_lower")
    return out.view(shape)


def sym_unpack_lower(packed: torch.Tensor, full: torch.Tensor) -> torch.Tensor:
    """The inverse of sym_pack_lower: both triangles of `full` (fp64 [n, n] or [batch, n, n], any row / batch stride) from the
    packed lower triangles in `packed` (contiguous, batch * n(n+1)/2 doubles).  Only the n x n entries are written."""
    _need_gpu(packed, full)
    n, batch, ld, bs = _sym_view(full)
    m = n * (n + 1) // 2
    if packed.dtype != torch.float64 or not packed.is_contiguous() or packed.numel() != batch * m or packed.device != full.device:
        raise ValueError(f"packed must be a contiguous float64 tensor of {batch * m} elements on {full.device}")
    with torch.cuda.device(full.device):
        check(_lib.load().mdg_sym_unpack_lower(packed.data_ptr(), n, batch, full.data_ptr(), ld, bs, _stream(full)),
              "mdg_sym_unpack_lower")
    return full


def bi_accum(out: torch.Tensor, x_in: torch.Tensor, x_out: torch.Tensor) -> None:
    """out[0] += sum_tokens (1 - cos(x_in, x_out)); out: 1-element fp64 device tensor."""
    _need_gpu(out, x_in, x_out)
    lib = _lib.load()
    a = x_in.detach().reshape(-1, x_in.shape[-1])
    b = x_out.detach().reshape(-1, x_out.shape[-1])
    if a.dtype != b.dtype or a.shape != b.shape:
        raise ValueError("x_in / x_out must match in dtype and shape")
    a = a if a.is_contiguous() else a.contiguous()
    b = b if b.is_contiguous() else b.contiguous()
    nbytes = lib.mdg_bi_ws_bytes(a.shape[0])
    ws, wsp = _ws(nbytes, a.device)
    with torch.cuda.device(a.device):
        check(lib.mdg_bi_accum(a.data_ptr(), b.data_ptr(), _DT[a.dtype], a.shape[0], a.shape[1], a.stride(0),
                               out.data_ptr(), wsp, nbytes, _stream(a)), "mdg_bi_accum")


# ------------------------------------------------------------------ dense blocks
def gemm(A: torch.Tensor, B: torch.Tensor, C_out: torch.Tensor, alpha: float = 1.0, beta: float = 0.0,
         trans_a: bool = False, trans_b: bool = False, a_rows: Optional[torch.Tensor] = None, flags: int = 0) -> None:
    """C_out = alpha * op(A) @ op(B) + beta * C_out for 2-D row-major tensors (f64 or bf16)."""
    _need_gpu(A, B, C_out)
    lib = _lib.load()
    M, N = C_out.shape
    K = A.shape[0] if trans_a else A.shape[1]
    sa_i, sa_k = (A.stride(1), A.stride(0)) if trans_a else (A.stride(0), A.stride(1))
    sb_k, sb_j = (B.stride(1), B.stride(0)) if trans_b else (B.stride(0), B.stride(1))
    with torch.cuda.device(A.device):
        check(lib.mdg_gemm_f64(M, N, K, alpha, A.data_ptr(), _DT[A.dtype], sa_i, sa_k, _p(a_rows), B.data_ptr(),
                               _DT[B.dtype], sb_k, sb_j, beta, C_out.data_ptr(), _DT[C_out.dtype], C_out.stride(0),
                               1, 0, 0, 0, flags, _stream(A)), "mdg_gemm_f64")


def potrf_lower(A: torch.Tensor) -> torch.Tensor:
    """In-place lower Cholesky of the square fp64 matrix A; returns the inverted-diagonal-block buffer."""
    _need_gpu(A)
    lib = _lib.load()
    n = A.shape[0]
    inv = torch.empty(lib.mdg_potrf_inv_diag_elems(n), dtype=torch.float64, device=A.device)
    with torch.cuda.device(A.device):
        check(lib.mdg_potrf_lower(A.data_ptr(), n, A.stride(0), inv.data_ptr(), _stream(A)), "mdg_potrf_lower")
    return inv


def potrs_lower(L: torch.Tensor, inv: torch.Tensor, X: torch.Tensor) -> None:
    """X <- (L L^T)^-1 X in place."""
    _need_gpu(L, inv, X)
    lib = _lib.load()
    nbytes = lib.mdg_potrs_lower_ws_bytes(L.shape[0], X.shape[1])
    ws, wsp = _ws(nbytes, L.device)
    with torch.cuda.device(L.device):
        check(lib.mdg_potrs_lower(L.data_ptr(), L.shape[0], L.stride(0), inv.data_ptr(), X.data_ptr(), X.shape[1],
                                  X.stride(0), wsp, nbytes, _stream(L)), "mdg_potrs_lower")


def syevj(A: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eigen-decomposition of a batch of symmetric matrices [b, n, n] (n <= 128, even).
    Returns (evals descending [b, n], evecs [b, n, n], eigenvector j in column j).  A is not modified."""
    _need_gpu(A)
    lib = _lib.load()
    A3 = A.reshape(-1, A.shape[-2], A.shape[-1]).to(torch.float64).clone()
    b, n, _ = A3.shape
    evals = torch.empty(b, n, dtype=torch.float64, device=A.device)
    evecs = torch.empty(b, n, n, dtype=torch.float64, device=A.device)
    with torch.cuda.device(A.device):
        check(lib.mdg_syevj_batched(A3.data_ptr(), n, b, evals.data_ptr(), evecs.data_ptr(), _stream(A)),
              "mdg_syevj_batched")
    return evals, evecs


def sqrt_psd_small(M: torch.Tensor, ridge: float, scaled: bool, want_inverse: bool):
    """Batched sqrt_M for n <= 128: returns (root, inv_root or None, evals descending pre-ridge)."""
    _need_gpu(M)
    lib = _lib.load()
    M3 = M.reshape(-1, M.shape[-2], M.shape[-1]).to(torch.float64).contiguous()
    b, n, _ = M3.shape
    root = torch.empty_like(M3)
    inv_root = torch.empty_like(M3) if want_inverse else None
    evals = torch.empty(b, n, dtype=torch.float64, device=M.device)
    nbytes = lib.mdg_sqrt_psd_small_ws_bytes(n, b)
    ws, wsp = _ws(nbytes, M.device)
    with torch.cuda.device(M.device):
        check(lib.mdg_sqrt_psd_small(M3.data_ptr(), n, b, float(ridge), int(scaled), root.data_ptr(), _p(inv_root),
                                     evals.data_ptr(), wsp, nbytes, _stream(M)), "mdg_sqrt_psd_small")
    return root.reshape(M.shape), (None if inv_root is None else inv_root.reshape(M.shape)), evals


def sqrt_psd_large(M: torch.Tensor, ridge: float, scaled: bool, want_inverse: bool, want_evals: bool = True):
    """sqrt_M for one symmetric matrix of any size: returns (root, inv_root or None, evals unsorted or None).
    With want_evals=False and scaled=False the library takes the GEMM-only Newton-Schulz route for sqrt(M + ridge I)
    (falling back to block Jacobi by itself when the input is not positive definite); eigenvalues need block Jacobi.
    Only the lower triangle is read; the same input gives the same bits on every call; a NaN or Inf there raises with the
    non-finite-input message (include/modegpt_hip.h)."""
    _need_gpu(M)
    lib = _lib.load()
    if M.dim() != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("sqrt_psd_large expects one square matrix")
    M2 = M if (M.dtype == torch.float64 and M.stride(1) == 1) else M.to(torch.float64).contiguous()
    n = M2.shape[0]
    root = torch.empty(n, n, dtype=torch.float64, device=M.device)
    inv_root = torch.empty(n, n, dtype=torch.float64, device=M.device) if want_inverse else None
    evals = torch.empty(n, dtype=torch.float64, device=M.device) if want_evals else None
    nbytes = lib.mdg_sqrt_psd_large_ws_bytes(n)
    ws, wsp = _ws(nbytes, M.device)
    with torch.cuda.device(M.device):
        check(lib.mdg_sqrt_psd_large(M2.data_ptr(), n, M2.stride(0), float(ridge), int(scaled), root.data_ptr(),
                                     _p(inv_root), _p(evals), wsp, nbytes, _stream(M)), "mdg_sqrt_psd_large")
    return root, inv_root, evals


# ------------------------------------------------------------------ MLP
def ridge_scores(Cm: torch.Tensor, ridge: float, want_sens: bool = False):
    """diag((C + ridge I)^-1) for a symmetric PD fp64 matrix.  want_sens: also the first-order sensitivities `sens` of the scores to
    an entry-wise relative perturbation of C (|delta score_j| <= eps sens_j for |E_ab| <= eps sqrt(c_aa c_bb); mdg_ridge_scores)
    -> (scores, sens)."""
    _need_gpu(Cm)
    lib = _lib.load()
    if Cm.dtype != torch.float64 or Cm.stride(1) != 1:
        raise ValueError("C must be float64 with unit column stride")
    n = Cm.shape[0]
    scores = torch.empty(n, dtype=torch.float64, device=Cm.device)
    sens = torch.empty(n, dtype=torch.float64, device=Cm.device) if want_sens else None
    nbytes = lib.mdg_ridge_scores_ws_bytes(n)
    ws, wsp = _ws(nbytes, Cm.device)
    with torch.cuda.device(Cm.device):
        check(lib.mdg_ridge_scores(Cm.data_ptr(), n, Cm.stride(0), float(ridge), scores.data_ptr(), _p(sens), wsp, nbytes,
                                   _stream(Cm)), "mdg_ridge_scores")
    return (scores, sens) if want_sens else scores


def select_smallest_sorted(scores: torch.Tensor, k: int) -> torch.Tensor:
    """Indices of the k smallest scores in ascending index order (topk(largest=False) + sort)."""
    _need_gpu(scores)
    lib = _lib.load()
    s = scores.to(torch.float64).contiguous()
    idx = torch.empty(k, dtype=torch.int64, device=s.device)
    with torch.cuda.device(s.device):
        check(lib.mdg_select_smallest_sorted(s.data_ptr(), s.numel(), k, idx.data_ptr(), _stream(s)),
              "mdg_select_smallest_sorted")
    return idx


def select_margin(scores: torch.Tensor, sens: torch.Tensor, idx: torch.Tensor, eps: float) -> torch.Tensor:
    """The certificate of a k-smallest selection (mdg_select_margin): 8 fp64 numbers ON THE DEVICE (MARGIN_FIELDS), enqueued only --
    read them when the stream is waited for anyway (decode_margin)."""
    _need_gpu(scores, sens, idx)
    lib = _lib.load()
    s = scores if (scores.dtype == torch.float64 and scores.is_contiguous()) else scores.to(torch.float64).contiguous()
    b = sens if (sens.dtype == torch.float64 and sens.is_contiguous()) else sens.to(torch.float64).contiguous()
    idx = idx.to(torch.int64).contiguous()
    out = torch.empty(8, dtype=torch.float64, device=s.device)
    with torch.cuda.device(s.device):
        check(lib.mdg_select_margin(s.data_ptr(), b.data_ptr(), idx.data_ptr() if idx.numel() else None, s.numel(), idx.numel(),
                                    float(eps), out.data_ptr(), _stream(s)), "mdg_select_margin")
    return out


def gather_rows(W: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """W[rows, :] for a 2-byte dtype (bf16/f16) row-major matrix."""
    _need_gpu(W, rows)
    lib = _lib.load()
    if W.element_size() != 2 or W.stride(1) != 1:
        raise ValueError("gather_rows needs a 2-byte dtype with unit column stride")
    rows = rows.to(torch.int64).contiguous()
    out = torch.empty(rows.numel(), W.shape[1], dtype=W.dtype, device=W.device)
    with torch.cuda.device(W.device):
        check(lib.mdg_gather_rows_16(W.data_ptr(), W.stride(0), rows.data_ptr(), rows.numel(), W.shape[1],
                                     out.data_ptr(), out.stride(0), _stream(W)), "mdg_gather_rows_16")
    return out


def nystrom_down(Cm: torch.Tensor, idx: torch.Tensor, W_down: torch.Tensor, eps: float = 1e-6,
                 want_f64: bool = False):
    """down' [d, r] bf16 = ((C[idx,idx] + eps I)^-1 C[idx,:] W_down^T)^T;  W_down: [d, n], bf16 as is, any other
    dtype widened exactly to fp64 (what the reference's .to(float64) does; bf16 would lose bits of an fp16 weight)."""
    _need_gpu(Cm, idx, W_down)
    lib = _lib.load()
    W_down = _as_weight(W_down)
    n, r, d = Cm.shape[0], idx.numel(), W_down.shape[0]
    idx = idx.to(torch.int64).contiguous()
    out = torch.empty(d, r, dtype=torch.bfloat16, device=Cm.device)
    f64 = torch.empty(r, d, dtype=torch.float64, device=Cm.device) if want_f64 else None
    nbytes = lib.mdg_nystrom_down_ws_bytes(n, r, d)
    ws, wsp = _ws(nbytes, Cm.device)
    with torch.cuda.device(Cm.device):
        if NYSTROM_OVERLAP:
            # the gathered cross product on a side stream beside the factorisation of C_kk (independent; the factorisation's
            # 128-column steps leave most of the chip idle between their GEMMs): 36 -> 27 ms for the two at Llama-3-8B shapes
            main = torch.cuda.current_stream(Cm.device)
            side = _side_stream(Cm.device, "nystrom", beside=main)
            side.wait_stream(main)                       # (inputs and workspace were produced / allocated on `main`)
            fork, join = torch.cuda.Event(), torch.cuda.Event()
            fork.record(main)                            # materialise the HIP events; the library re-records them
            join.record(main)
            check(lib.mdg_nystrom_down_overlapped(Cm.data_ptr(), n, Cm.stride(0), idx.data_ptr(), r, W_down.data_ptr(), d,
                                                  W_down.stride(0), _DT[W_down.dtype], float(eps), out.data_ptr(), out.stride(0),
                                                  _p(f64), wsp, nbytes, side.cuda_stream, fork.cuda_event, join.cuda_event,
                                                  main.cuda_stream), "mdg_nystrom_down_overlapped")
            for t in (Cm, W_down, idx, ws):
                t.record_stream(side)                    # read (workspace: written) there
        else:
            check(lib.mdg_nystrom_down(Cm.data_ptr(), n, Cm.stride(0), idx.data_ptr(), r, W_down.data_ptr(), d,
                                       W_down.stride(0), _DT[W_down.dtype], float(eps), out.data_ptr(), out.stride(0), _p(f64), wsp, nbytes,
                                       _stream(Cm)), "mdg_nystrom_down")
    return (out, f64) if want_f64 else out


def nystrom_intercept(W_down: torch.Tensor, down_hat: torch.Tensor, idx: torch.Tensor, mu: torch.Tensor,
                      b_d: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None):
    """The intercept of the mean-aware refit (mdg_nystrom_intercept): delta = W_down mu - down_hat mu[idx] in fp64 with exact products;
    W_down [d, n] as nystrom_down takes it, down_hat [d, r] the bf16 tensor nystrom_down RETURNED for the selection idx, mu fp64 [n].
    Returns (bias, bias_f64, norms): bias_f64 [d] = b_d + delta (b_d None: 0), bias = its one rounding to out_dtype (default: b_d's
    dtype, else bf16 for a bf16 weight and W_down's own dtype otherwise), norms [2] = (||delta||^2, ||W_down mu||^2), fp64 ON THE
    DEVICE.  The call only enqueues."""
    _need_gpu(W_down, down_hat, idx, mu, b_d)
    lib = _lib.load()
    if out_dtype is None:
        out_dtype = b_d.dtype if b_d is not None else W_down.dtype
    W = _as_weight(W_down)
    if down_hat.dtype != torch.bfloat16 or down_hat.dim() != 2 or down_hat.stride(1) != 1:
        raise ValueError("nystrom_intercept: down_hat must be the stored bf16 [d, r] tensor with contiguous rows")
    d, n = W.shape
    r = idx.numel()
    if down_hat.shape[0] != d or down_hat.shape[1] != r or mu.numel() != n or mu.dtype != torch.float64:
        raise ValueError(f"nystrom_intercept: shapes disagree (W_down {tuple(W.shape)}, down_hat {tuple(down_hat.shape)}, "
                         f"idx {r}, mu {mu.numel()} {mu.dtype})")
    if out_dtype not in _DT or (b_d is not None and (b_d.dtype not in _DT or b_d.numel() != d)):
        raise ValueError("nystrom_intercept: unsupported bias dtype or length")
    idx = idx.to(torch.int64).contiguous()
    mu = mu.contiguous()
    bd = None if b_d is None else b_d.detach().contiguous()
    dev = W.device
    bias = torch.empty(d, dtype=out_dtype, device=dev)
    bias_f64 = torch.empty(d, dtype=torch.float64, device=dev)
    norms = torch.empty(2, dtype=torch.float64, device=dev)
    nbytes = lib.mdg_nystrom_intercept_ws_bytes(d)
    ws, wsp = _ws(nbytes, dev)
    with torch.cuda.device(dev):
        check(lib.mdg_nystrom_intercept(W.data_ptr(), d, n, W.stride(0), _DT[W.dtype], down_hat.data_ptr(), r, down_hat.stride(0),
                                        idx.data_ptr(), mu.data_ptr(), _p(bd), _DT[bd.dtype] if bd is not None else 0, bias.data_ptr(),
                                        _DT[out_dtype], bias_f64.data_ptr(), norms.data_ptr(), wsp, nbytes, _stream(W)),
              "mdg_nystrom_intercept")
    return bias, bias_f64, norms


def nystrom_rank_curve(Cm: torch.Tensor, order: torch.Tensor, W_down: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """curve [n + 1] fp64 ON THE DEVICE: curve[r] = tr(W (M - M[:, S] M_SS^-1 M[S, :]) W^T), M = C + eps I, S = order[:r] -- the
    residual energy of the Nystrom refit that keeps the first r columns of `order`, for every r from one factorisation.  `order`:
    a permutation of 0 .. n-1 (the ridge-score order: torch.argsort(scores, stable=True)).  W_down [d, n] as in nystrom_down.
    Inside an ops.DeferredStatus the call only enqueues; outside it raises torch.linalg.LinAlgError for a matrix that is not
    positive definite (a repeated index in `order` makes one).  Read it with decode_rank_curve."""
    _need_gpu(Cm, order, W_down)
    lib = _lib.load()
    if Cm.dtype != torch.float64 or Cm.dim() != 2 or Cm.shape[0] != Cm.shape[1] or Cm.stride(1) != 1:
        raise ValueError("C must be a square float64 matrix with unit column stride")
    W_down = _as_weight(W_down)
    n, d = Cm.shape[0], W_down.shape[0]
    if order.numel() != n or W_down.dim() != 2 or W_down.shape[1] != n:
        raise ValueError(f"nystrom_rank_curve: order needs {n} entries and W_down {n} columns")
    order = order.to(torch.int64).contiguous()
    curve = torch.empty(n + 1, dtype=torch.float64, device=Cm.device)
    nbytes = lib.mdg_nystrom_rank_curve_ws_bytes(n, d)
    ws, wsp = _ws(nbytes, Cm.device)
    with torch.cuda.device(Cm.device):
        check(lib.mdg_nystrom_rank_curve(Cm.data_ptr(), n, Cm.stride(0), order.data_ptr(), W_down.data_ptr(), d, W_down.stride(0),
                                         _DT[W_down.dtype], float(eps), curve.data_ptr(), wsp, nbytes, _stream(Cm)),
              "mdg_nystrom_rank_curve")
    return curve


def nystrom_greedy_select(Cm: torch.Tensor, W_down: torch.Tensor, r: int, rounds: int, eps: float = 1e-6):
    """(order [r] int64, objective [rounds + 1] fp64, cut [rounds, 2] fp64, n_dead [1] int64), all ON THE DEVICE: the r columns that
    `rounds` rounds of block-greedy descent on tr(W (M - M[:, S] M_SS^-1 M[S, :]) W^T), M = C + eps I, select
    (mdg_nystrom_greedy_select; include/modegpt_hip.h states the algorithm) -- order round by round and ascending within a round,
    the objective before the first round and after each, per round the smallest picked and the largest unpicked eligible gain,
    and the number of dead picks.  W_down [d, n] as in nystrom_down; only the lower triangle of C is read.  Inside an
    ops.DeferredStatus the call only enqueues; outside it raises torch.linalg.LinAlgError when a round's pivot block is not
    positive definite.  Read the numbers with decode_mlp_greedy."""
    _need_gpu(Cm, W_down)
    lib = _lib.load()
    if Cm.dtype != torch.float64 or Cm.dim() != 2 or Cm.shape[0] != Cm.shape[1] or Cm.stride(1) != 1:
        raise ValueError("C must be a square float64 matrix with unit column stride")
    W_down = _as_weight(W_down)
    n, d, r, rounds = Cm.shape[0], W_down.shape[0], int(r), int(rounds)
    if W_down.dim() != 2 or W_down.shape[1] != n:
        raise ValueError(f"nystrom_greedy_select: W_down needs {n} columns")
    if not 0 <= r <= n or rounds < 1:
        raise ValueError(f"nystrom_greedy_select: need 0 <= r <= {n} and rounds >= 1, got r = {r}, rounds = {rounds}")
    dev = Cm.device
    order = torch.empty(r, dtype=torch.int64, device=dev)
    objective = torch.empty(rounds + 1, dtype=torch.float64, device=dev)
    cut = torch.full((rounds, 2), float("nan"), dtype=torch.float64, device=dev)
    n_dead = torch.zeros(1, dtype=torch.int64, device=dev)
    nbytes = lib.mdg_nystrom_greedy_ws_bytes(n, d, r, rounds)
    ws, wsp = _ws(nbytes, dev)
    with torch.cuda.device(dev):
        check(lib.mdg_nystrom_greedy_select(Cm.data_ptr(), n, Cm.stride(0), W_down.data_ptr(), d, W_down.stride(0), _DT[W_down.dtype],
                                            float(eps), r, rounds, order.data_ptr() if r else None, objective.data_ptr(), cut.data_ptr(),
                                            n_dead.data_ptr(), wsp, nbytes, _stream(Cm)), "mdg_nystrom_greedy_select")
    return order, objective, cut, n_dead


def mlp_output_error(Cm: torch.Tensor, W_down: torch.Tensor, idx: Optional[torch.Tensor], down: Optional[torch.Tensor],
                     want_unorm2: bool = False):
    """e [d] fp64 ON THE DEVICE: e[k] = u_k C u_k^T, u_k = row k of W_down with down[k, p] subtracted at column idx[p] -- what output
    channel k of the MLP loses on the statistic C when `down` replaces W_down at the kept columns `idx`.  Only the lower triangle of C
    is read.  W_down [d, n] as in nystrom_down.  down: the stored [d, r] bf16 tensor, or an fp64 tensor [d, r] of any strides
    (nystrom_down's f64 solution [r, d] goes in as `f64.T`); any other dtype is widened exactly to fp64.  down=None (or an empty
    idx): nothing is subtracted and e[k] = q_k, the channel's output energy.  want_unorm2: -> (e, unorm2), unorm2[k] = ||u_k||^2.
    The call only enqueues; an index that occurs twice subtracts its highest position, entries outside 0 .. n-1 are clamped."""
    _need_gpu(Cm, W_down, idx, down)
    lib = _lib.load()
    if Cm.dtype != torch.float64 or Cm.dim() != 2 or Cm.shape[0] != Cm.shape[1] or Cm.stride(1) != 1:
        raise ValueError("C must be a square float64 matrix with unit column stride")
    W_down = _as_weight(W_down)
    n, d = Cm.shape[0], W_down.shape[0]
    if W_down.dim() != 2 or W_down.shape[1] != n:
        raise ValueError(f"mlp_output_error: W_down needs {n} columns")
    r = 0 if (down is None or idx is None) else idx.numel()
    if r:
        if down.dim() != 2 or tuple(down.shape) != (d, r):
            raise ValueError(f"mlp_output_error: down must be [{d}, {r}], got {tuple(down.shape)}")
        down = down.detach()
        if down.dtype not in (torch.bfloat16, torch.float64):
            down = down.to(torch.float64)
        idx = idx.to(torch.int64).contiguous()
    e = torch.empty(d, dtype=torch.float64, device=Cm.device)
    u2 = torch.empty(d, dtype=torch.float64, device=Cm.device) if want_unorm2 else None
    nbytes = lib.mdg_mlp_output_error_ws_bytes(n, d)
    ws, wsp = _ws(nbytes, Cm.device)
    with torch.cuda.device(Cm.device):
        check(lib.mdg_mlp_output_error(Cm.data_ptr(), n, Cm.stride(0), W_down.data_ptr(), d, W_down.stride(0), _DT[W_down.dtype],
                                       idx.data_ptr() if r else None, r, down.data_ptr() if r else None,
                                       down.stride(0) if r else 0, down.stride(1) if r else 0, _DT[down.dtype] if r else _lib.MDG_BF16,
                                       e.data_ptr(), _p(u2), wsp, nbytes, _stream(Cm)), "mdg_mlp_output_error")
    return (e, u2) if want_unorm2 else e


NYSTROM_EPS = 1e-6          # the ridge of the refit compress_weights computes (compress_mlp.py:52,56): the eps of `objective`


# ------------------------------------------------------------------ QK / VO
def qk_select(cov_q: torch.Tensor, cov_k: torch.Tensor, rank: int, mode: int, ridge_q: float, ridge_k: float):
    """Returns (mask [n_kv, rank] int64, q_rows [n_heads*rank], k_rows [n_kv*rank])."""
    _need_gpu(cov_q, cov_k)
    lib = _lib.load()
    cq = cov_q.to(torch.float64).contiguous()
    ck = cov_k.to(torch.float64).contiguous()
    n_heads, hd, _ = cq.shape
    n_kv = ck.shape[0]
    dev = cq.device
    mask = torch.empty(n_kv, rank, dtype=torch.int64, device=dev)
    q_rows = torch.empty(n_heads * rank, dtype=torch.int64, device=dev)
    k_rows = torch.empty(n_kv * rank, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.mdg_qk_select(cq.data_ptr(), ck.data_ptr(), n_heads, n_kv, hd, float(ridge_q), float(ridge_k), rank,
                                mode, mask.data_ptr(), q_rows.data_ptr(), k_rows.data_ptr(), _stream(cq)),
              "mdg_qk_select")
    return mask, q_rows, k_rows


def qk_select_margin(cov_q: torch.Tensor, cov_k: torch.Tensor, rank: int, mode: int, ridge_q: float, ridge_k: float,
                     mask: torch.Tensor, eps_rel: float, eps_abs: float) -> torch.Tensor:
    """The certificate of a qk_select selection (mdg_qk_select_margin): [n_kv, 8] fp64 ON THE DEVICE (QK_MARGIN_FIELDS), enqueued
    only -- read it when the stream is waited for anyway (decode_qk_margin).  mask: what qk_select returned for these arguments.
    Every diagonal entry c of a sigma_q / sigma_k head is taken as known to within eps_rel |c| + eps_abs (||C||_inf + ridge)."""
    _need_gpu(cov_q, cov_k, mask)
    lib = _lib.load()
    cq = cov_q.to(torch.float64).contiguous()
    ck = cov_k.to(torch.float64).contiguous()
    n_heads, hd, _ = cq.shape
    n_kv = ck.shape[0]
    if mask.dtype != torch.int64 or tuple(mask.shape) != (n_kv, rank):
        raise ValueError(f"qk_select_margin: mask must be int64 [{n_kv}, {rank}], got {mask.dtype} {tuple(mask.shape)}")
    mask = mask.contiguous()
    out = torch.empty(n_kv, 8, dtype=torch.float64, device=cq.device)
    with torch.cuda.device(cq.device):
        check(lib.mdg_qk_select_margin(cq.data_ptr(), ck.data_ptr(), n_heads, n_kv, hd, float(ridge_q), float(ridge_k), rank, mode,
                                       mask.data_ptr(), float(eps_rel), float(eps_abs), out.data_ptr(), _stream(cq)),
              "mdg_qk_select_margin")
    return out


def qk_units(mode: int, hd: int):
    """(ns, columns per unit) of a scoring mode: RoPE pairs {u, u + hd/2} or, for OPT, single columns."""
    return (hd, 1) if mode == _lib.MDG_QK_OPT else (hd // 2, 2)


def qk_rank_curve(cov_q: torch.Tensor, cov_k: torch.Tensor, mode: int, ridge_q: float, ridge_k: float, order: torch.Tensor,
                  want_greedy: bool = True, terms_ridges=None):
    """Returns (curve_h [n_heads, ns + 1], curve [n_kv, ns + 1], terms [n_kv, ns], scale [n_kv], greedy_curve [n_kv, ns + 1] or None,
    greedy_order [n_kv, ns] int64 or None), all ON THE DEVICE, enqueued only (mdg_qk_rank_curve; decode_qk_logit_error reads them).
    curve_h[h][m]: the mean-square change of query head h's logits over all token pairs of the calibration set when only the first m
    units of `order` are kept, under (cov_q + ridge_q I) (.) (cov_k + ridge_k I); curve: the kv group's sums.  order: int64 [n_kv, ns],
    keep-first -- qk_select(..., rank=hd)[0][:, :ns].  terms: the diagonal share of every unit in that order, what qk_select's score
    is made of, with terms_ridges = (ridge_q, ridge_k) of its own (None: the same ridges).  scale: the abs-sum the values are accurate
    relative to.  want_greedy: the comparison order built on the full objective and its curve."""
    _need_gpu(cov_q, cov_k, order)
    lib = _lib.load()
    if cov_q.dim() != 3 or cov_k.dim() != 3 or cov_q.shape[1] != cov_q.shape[2] or tuple(cov_k.shape[1:]) != tuple(cov_q.shape[1:]):
        raise ValueError(f"qk_rank_curve: cov_q / cov_k must be [heads, hd, hd], got {tuple(cov_q.shape)} / {tuple(cov_k.shape)}")
    if mode not in (_lib.MDG_QK_ROPE_GROUPED, _lib.MDG_QK_ROPE_MHA, _lib.MDG_QK_OPT):
        raise ValueError(f"qk_rank_curve: unknown mode {mode!r}")
    cq = cov_q.to(torch.float64).contiguous()
    ck = cov_k.to(torch.float64).contiguous()
    n_heads, hd, _ = cq.shape
    n_kv = ck.shape[0]
    ns, _ = qk_units(mode, hd)
    if order.dtype != torch.int64 or tuple(order.shape) != (n_kv, ns):
        raise ValueError(f"qk_rank_curve: order must be int64 [{n_kv}, {ns}], got {order.dtype} {tuple(order.shape)}")
    order = order.contiguous()
    tq, tk = (ridge_q, ridge_k) if terms_ridges is None else terms_ridges
    dev = cq.device
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)      # noqa: E731
    curve_h, curve, terms, scale = new(n_heads, ns + 1), new(n_kv, ns + 1), new(n_kv, ns), new(n_kv)
    g_curve = new(n_kv, ns + 1) if want_greedy else None
    g_order = torch.empty(n_kv, ns, dtype=torch.int64, device=dev) if want_greedy else None
    with torch.cuda.device(dev):
        check(lib.mdg_qk_rank_curve(cq.data_ptr(), ck.data_ptr(), n_heads, n_kv, hd, float(ridge_q), float(ridge_k), mode,
                                    order.data_ptr(), float(tq), float(tk), curve_h.data_ptr(), curve.data_ptr(), terms.data_ptr(),
                                    scale.data_ptr(), _p(g_curve), _p(g_order), _stream(cq)), "mdg_qk_rank_curve")
    return curve_h, curve, terms, scale, g_curve, g_order


def vo_bias(ws: torch.Tensor, W_o: torch.Tensor, b_v: torch.Tensor, b_o: Optional[torch.Tensor], n_heads: int, n_kv: int, hd: int,
            rank: int):
    """The v_proj / o_proj biases through the truncation the LAST mdg_vo_compress call on workspace `ws` computed (mdg_vo_bias; same
    stream, same shapes and rank).  W_o: the ORIGINAL [d, n_heads*hd] weight (bf16 / fp16 as they are, anything else widened exactly to
    fp64); b_v [n_kv*hd], b_o [d] or None.  Returns (o_bias, v_bias, resid), fp64 ON THE DEVICE: with b_o, o_bias [d] = b_o + sum_h
    W_o,h b_v,kv(h) and v_bias is None (v_proj becomes bias-free, nothing is lost at any rank); without, v_bias [n_kv*rank] = P_g b_v,g
    and o_bias is None.  resid [2] = (||rho||^2, ||sum_h W_o,h b_v||^2), rho the part of the constant the second form cannot carry.
    The call only enqueues."""
    _need_gpu(ws, W_o, b_v, b_o)
    lib = _lib.load()
    Wo = W_o.detach()
    if Wo.dtype not in (torch.bfloat16, torch.float16, torch.float64):
        Wo = Wo.to(torch.float64)
    if Wo.stride(-1) != 1:
        Wo = Wo.contiguous()
    d = Wo.shape[0]
    if Wo.dim() != 2 or Wo.shape[1] != n_heads * hd:
        raise ValueError(f"vo_bias: W_o must be [d, {n_heads * hd}], got {tuple(Wo.shape)}")
    bv = b_v.detach().contiguous()
    bo = None if b_o is None else b_o.detach().to(bv.dtype).contiguous()
    if bv.numel() != n_kv * hd or (bo is not None and bo.numel() != d):
        raise ValueError(f"vo_bias: b_v must hold {n_kv * hd} entries and b_o {d}")
    dev = Wo.device
    o_bias = torch.empty(d, dtype=torch.float64, device=dev) if bo is not None else None
    v_bias = torch.empty(n_kv * rank, dtype=torch.float64, device=dev) if bo is None else None
    resid = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.mdg_vo_bias(ws.data_ptr(), ws.numel() * ws.element_size(), Wo.data_ptr(), Wo.stride(0), _DT[Wo.dtype], d,
                              bv.data_ptr(), _p(bo), _DT[bv.dtype], n_heads, n_kv, hd, rank, _p(o_bias), _p(v_bias), resid.data_ptr(),
                              _stream(Wo)), "mdg_vo_bias")
    return o_bias, v_bias, resid


def vo_intercept(W_v: torch.Tensor, W_o: torch.Tensor, v_new: Optional[torch.Tensor], o_new: Optional[torch.Tensor], mu: torch.Tensor,
                 n_heads: int, n_kv: int, hd: int, rank: int, b_v: Optional[torch.Tensor] = None, b_o: Optional[torch.Tensor] = None,
                 out_dtype: Optional[torch.dtype] = None):
    """The intercept of the mean-aware V/O truncation (mdg_vo_intercept): delta = sum_h (W_o,h a_kv(h) - o^_h a'_kv(h)) in fp64 with
    exact products, a_g = W_v,g mu + b_v,g, a'_g = v^_g mu.  W_v [n_kv*hd, d] / W_o [d, n_heads*hd] as vo_compress takes them, v_new
    [n_kv*rank, d] / o_new [d, n_heads*rank] the stored bf16 tensors vo_compress RETURNED or its v_f64 / o_f64 (row-strided views are
    taken as they are; any other dtype is widened exactly to fp64); mu fp64 [d]; rank 0 (or v_new None): nothing is subtracted.
    Returns (bias, bias_f64, norms): bias_f64 [d] = b_o + delta (b_o None: 0), bias = its one rounding to out_dtype (default: b_o's
    dtype, else the dtype of W_o), norms [2] = (||delta||^2, ||sum_h W_o,h a_kv(h)||^2), fp64 ON THE DEVICE.  The call only enqueues."""
    _need_gpu(W_v, W_o, v_new, o_new, mu, b_v, b_o)
    lib = _lib.load()
    if out_dtype is None:
        out_dtype = b_o.dtype if b_o is not None else W_o.dtype
    Wv, Wo = _as_weight(W_v), _as_weight(W_o)
    if Wv.dtype != Wo.dtype:
        Wv, Wo = Wv.to(torch.float64), Wo.to(torch.float64)
    d = Wv.shape[1]
    if Wv.dim() != 2 or Wo.dim() != 2 or tuple(Wv.shape) != (n_kv * hd, d) or tuple(Wo.shape) != (d, n_heads * hd):
        raise ValueError(f"vo_intercept: W_v must be [{n_kv * hd}, d] and W_o [d, {n_heads * hd}], got {tuple(Wv.shape)} and {tuple(Wo.shape)}")
    if mu.dtype != torch.float64 or mu.numel() != d:
        raise ValueError(f"vo_intercept: mu must be a float64 vector of {d} entries")
    r = 0 if (v_new is None or o_new is None) else int(rank)
    vn = on = None
    if r:
        if tuple(v_new.shape) != (n_kv * r, d) or tuple(o_new.shape) != (d, n_heads * r):
            raise ValueError(f"vo_intercept: v_new must be [{n_kv * r}, {d}] and o_new [{d}, {n_heads * r}], got "
                             f"{tuple(v_new.shape)} and {tuple(o_new.shape)}")
        vn, on = _as_weight(v_new), _as_weight(o_new)
        if vn.dtype != on.dtype:
            vn, on = vn.to(torch.float64), on.to(torch.float64)
    bv = None if b_v is None else b_v.detach().contiguous()
    bo = None if b_o is None else b_o.detach().contiguous()
    if bv is not None and bo is not None and bv.dtype != bo.dtype:        # (one b_dtype for both: widen exactly)
        bv, bo = bv.to(torch.float64), bo.to(torch.float64)
    bdt = bv.dtype if bv is not None else (bo.dtype if bo is not None else torch.float64)
    if out_dtype not in _DT or bdt not in _DT or (bv is not None and bv.numel() != n_kv * hd) or (bo is not None and bo.numel() != d):
        raise ValueError(f"vo_intercept: unsupported bias dtype, or b_v does not hold {n_kv * hd} entries / b_o {d}")
    mu = mu.contiguous()
    dev = Wv.device
    bias = torch.empty(d, dtype=out_dtype, device=dev)
    bias_f64 = torch.empty(d, dtype=torch.float64, device=dev)
    norms = torch.empty(2, dtype=torch.float64, device=dev)
    nbytes = lib.mdg_vo_intercept_ws_bytes(d, n_kv, hd, r)
    ws, wsp = _ws(nbytes, dev)
    with torch.cuda.device(dev):
        check(lib.mdg_vo_intercept(Wv.data_ptr(), Wv.stride(0), Wo.data_ptr(), Wo.stride(0), _DT[Wv.dtype], _p(vn),
                                   vn.stride(0) if r else 0, _p(on), on.stride(0) if r else 0, _DT[vn.dtype] if r else _lib.MDG_BF16, d,
                                   n_heads, n_kv, hd, r, mu.data_ptr(), _p(bv), _p(bo), _DT[bdt], bias.data_ptr(), _DT[out_dtype],
                                   bias_f64.data_ptr(), norms.data_ptr(), wsp, nbytes, _stream(Wv)), "mdg_vo_intercept")
    return bias, bias_f64, norms


def vo_compress(cov_x: torch.Tensor, W_v: torch.Tensor, W_o: torch.Tensor, n_heads: int, n_kv: int, hd: int, rank: int,
                ridge: float, want_f64: bool = False, want_spectrum: bool = False, spectrum_eps: Optional[float] = None,
                want_curve: bool = False, bias=None, spectrum_cov: Optional[torch.Tensor] = None):
    """Returns (v_proj [n_kv*rank, d] bf16, o_proj [d, n_heads*rank] bf16[, v_f64, o_f64][, spectrum][, curve][, bias]).
    spectrum_cov: the statistic whose DIAGONAL mdg_vo_spectrum's Weyl bound reads (default: cov_x).  The mean-aware truncation passes
    the centred S = C - mu mu^T as cov_x and the uncentred C here: S was computed from C, so an entry-wise relative error eps of C
    leaves |E_ab| <= eps sqrt(c_aa c_bb) in S as well (up to the fp64 rounding of mu), and c_aa >= s_aa -- the bound stays a bound.
    bias: (b_v, b_o or None) -- vo_bias's (o_bias, v_bias, resid) for this truncation comes last in the tuple, enqueued behind
    everything else while the workspace is alive; the factors are the same bits with or without it.
    want_curve: what the truncation costs the attention output at every rank (mdg_vo_rank_curve: [n_kv, hd + 1] fp64 ON THE DEVICE;
    decode_vo_output_error reads it), enqueued like the spectrum, behind the factorisation while its workspace is alive.
    want_spectrum: what the truncation at `rank` did to the spectrum (mdg_vo_spectrum: [n_kv, 8] fp64 ON THE DEVICE,
    VO_SPECTRUM_FIELDS; decode_vo_spectrum), enqueued behind the factorisation on the same stream while its workspace is alive;
    spectrum_eps: the entry-wise relative error bound of cov_x its Weyl bound is taken against (None: 0, the gap alone).  The
    factors are the same bits with or without it."""
    _need_gpu(cov_x, W_v, W_o)
    lib = _lib.load()
    Wv, Wo = _as_weight(W_v), _as_weight(W_o)
    if Wv.dtype != Wo.dtype:
        Wv, Wo = Wv.to(torch.float64), Wo.to(torch.float64)
    Cx = cov_x if (cov_x.dtype == torch.float64 and cov_x.stride(1) == 1) else cov_x.to(torch.float64).contiguous()
    d = Cx.shape[0]
    dev = Cx.device
    v_out = torch.empty(n_kv * rank, d, dtype=torch.bfloat16, device=dev)
    o_out = torch.empty(d, n_heads * rank, dtype=torch.bfloat16, device=dev)
    v64 = torch.empty(n_kv * rank, d, dtype=torch.float64, device=dev) if want_f64 else None
    o64 = torch.empty(d, n_heads * rank, dtype=torch.float64, device=dev) if want_f64 else None
    spectrum = torch.empty(n_kv, 8, dtype=torch.float64, device=dev) if want_spectrum else None
    nbytes = lib.mdg_vo_compress_ws_bytes(d, n_heads, n_kv, hd)
    ws, wsp = _ws(nbytes, dev)
    with torch.cuda.device(dev):
        check(lib.mdg_vo_compress(Cx.data_ptr(), d, Cx.stride(0), Wv.data_ptr(), Wv.stride(0), Wo.data_ptr(),
                                  Wo.stride(0), _DT[Wv.dtype], n_heads, n_kv, hd, rank, float(ridge), v_out.data_ptr(),
                                  v_out.stride(0), o_out.data_ptr(), o_out.stride(0), _p(v64), _p(o64), wsp, nbytes,
                                  _stream(Cx)), "mdg_vo_compress")
        if want_spectrum:
            Cd = Cx
            if spectrum_cov is not None:
                Cd = spectrum_cov
                if Cd.dtype != torch.float64 or Cd.dim() != 2 or Cd.stride(1) != 1 or tuple(Cd.shape) != (d, d) or Cd.device != dev:
                    raise ValueError(f"vo_compress: spectrum_cov must be a float64 [{d}, {d}] matrix with unit column stride beside cov_x")
            check(lib.mdg_vo_spectrum(wsp, nbytes, Cd.data_ptr(), d, Cd.stride(0), Wv.data_ptr(), Wv.stride(0), _DT[Wv.dtype],
                                      n_heads, n_kv, hd, rank, float(ridge), float(spectrum_eps or 0.0), spectrum.data_ptr(),
                                      _stream(Cx)), "mdg_vo_spectrum")
        if want_curve:
            curve = torch.empty(n_kv, hd + 1, dtype=torch.float64, device=dev)
            cbytes = lib.mdg_vo_rank_curve_ws_bytes(d, n_heads, n_kv, hd)
            cws, cwsp = _ws(cbytes, dev)
            check(lib.mdg_vo_rank_curve(wsp, nbytes, Wo.data_ptr(), Wo.stride(0), _DT[Wo.dtype], d, n_heads, n_kv, hd,
                                        curve.data_ptr(), cwsp, cbytes, _stream(Cx)), "mdg_vo_rank_curve")
        if bias is not None:
            carried = vo_bias(ws, W_o, bias[0], bias[1], n_heads, n_kv, hd, rank)
    out = (v_out, o_out, v64, o64) if want_f64 else (v_out, o_out)
    out = out + (spectrum,) if want_spectrum else out
    out = out + (curve,) if want_curve else out
    return out + (carried,) if bias is not None else out


def vo_output_error(cov_x: torch.Tensor, W_v: torch.Tensor, W_o: torch.Tensor, n_heads: int, n_kv: int, hd: int, rank: int,
                    v_new: Optional[torch.Tensor], o_new: Optional[torch.Tensor], want_dnorm2: bool = False):
    """e [n_heads, d] fp64 ON THE DEVICE: e[h][k] = delta C delta^T, delta = W_o,h[k, :] W_v,g - o'_h[k, :] v'_g -- what output
    channel k of query head h (kv group g) loses on the statistic C = cov_x when v_new [n_kv*rank, d] / o_new [d, n_heads*rank] replace
    W_v [n_kv*hd, d] / W_o [d, n_heads*hd].  v_new / o_new: the stored bf16 tensors or vo_compress's v_f64 / o_f64 (row-strided views
    are taken as they are; any other dtype is widened exactly to fp64).  v_new=None or rank=0: nothing is subtracted and e = q, the
    channel's output energy.  want_dnorm2: -> (e, dnorm2), dnorm2[h][k] = ||delta||^2, so that e + ridge * dnorm2 is the channel's
    objective under C + ridge I.  e is accurate relative to the scale a of include/modegpt_hip.h, not to itself (decode_vo_output_error
    reports the floor).  The call only enqueues."""
    _need_gpu(cov_x, W_v, W_o, v_new, o_new)
    lib = _lib.load()
    if cov_x.dtype != torch.float64 or cov_x.dim() != 2 or cov_x.shape[0] != cov_x.shape[1] or cov_x.stride(1) != 1:
        raise ValueError("cov_x must be a square float64 matrix with unit column stride")
    Wv, Wo = _as_weight(W_v), _as_weight(W_o)
    if Wv.dtype != Wo.dtype:
        Wv, Wo = Wv.to(torch.float64), Wo.to(torch.float64)
    d = cov_x.shape[0]
    if tuple(Wv.shape) != (n_kv * hd, d) or tuple(Wo.shape) != (d, n_heads * hd):
        raise ValueError(f"vo_output_error: W_v must be [{n_kv * hd}, {d}] and W_o [{d}, {n_heads * hd}]")
    r = 0 if (v_new is None or o_new is None) else int(rank)
    if r:
        if tuple(v_new.shape) != (n_kv * r, d) or tuple(o_new.shape) != (d, n_heads * r):
            raise ValueError(f"vo_output_error: v_new must be [{n_kv * r}, {d}] and o_new [{d}, {n_heads * r}], got "
                             f"{tuple(v_new.shape)} and {tuple(o_new.shape)}")
        vn, on = _as_weight(v_new), _as_weight(o_new)
        if vn.dtype != on.dtype:
            vn, on = vn.to(torch.float64), on.to(torch.float64)
    e = torch.empty(n_heads, d, dtype=torch.float64, device=cov_x.device)
    dn = torch.empty(n_heads, d, dtype=torch.float64, device=cov_x.device) if want_dnorm2 else None
    nbytes = lib.mdg_vo_output_error_ws_bytes(d, n_heads, n_kv, hd, r)
    ws, wsp = _ws(nbytes, cov_x.device)
    with torch.cuda.device(cov_x.device):
        check(lib.mdg_vo_output_error(cov_x.data_ptr(), d, cov_x.stride(0), Wv.data_ptr(), Wv.stride(0), Wo.data_ptr(), Wo.stride(0),
                                      _DT[Wv.dtype], n_heads, n_kv, hd, r, vn.data_ptr() if r else None, vn.stride(0) if r else 0,
                                      on.data_ptr() if r else None, on.stride(0) if r else 0, _DT[vn.dtype] if r else _lib.MDG_BF16,
                                      e.data_ptr(), _p(dn), wsp, nbytes, _stream(cov_x)), "mdg_vo_output_error")
    return (e, dn) if want_dnorm2 else e


ROPE_PLAN_FIELDS = ("route", "hpt", "vec", "norm", "half_even", "iters", "one_shot", "cs_vec16", "nw_vec16", "tt", "wi", "wo",
                    "hp1", "lds", "lds_attr", "grid_x", "grid_y", "grid_z", "t_tiles", "n_tiles")   # include/modegpt_hip.h


def rope_plan_at(dtype, B: int, T: int, n_heads: int, n_kv: int, r: int, head_dim: int, ld_x: int, x: int, cos: int, sin: int,
                 cs_batch_stride: int, mask: Optional[int], norm_weight: Optional[int], out: int) -> dict:
    """mdg_rope_gather_plan on plain integers: what mdg_rope_gather launches for operands at the ADDRESSES x, cos, sin,
    mask, norm_weight (None = absent) and out.  Nothing is dereferenced, no device is needed.  "route" is "direct" or
    "tile", "grid" a tuple; every other field of the header's layout is an int under its name."""
    lib = _lib.load()
    arr = (C.c_int64 * len(ROPE_PLAN_FIELDS))()
    check(lib.mdg_rope_gather_plan(x, _DT[dtype], ld_x, B, T, n_heads, n_kv, r, head_dim, cos, sin, cs_batch_stride, mask or None,
                                   norm_weight or None, 0.0, out, None, arr), "mdg_rope_gather_plan")
    p = dict(zip(ROPE_PLAN_FIELDS, (int(v) for v in arr)))
    p["route"] = "tile" if p["route"] else "direct"
    p["grid"] = (p.pop("grid_x"), p.pop("grid_y"), p.pop("grid_z"))
    return p


def _rope_operands(x, cos, sin, mask, n_heads, n_kv, head_dim, norm_weight, out):
    """The operands of mdg_rope_gather as it receives them (shared by rope_gather and rope_gather_plan)."""
    B, T, width = x.shape
    r = width // n_heads
    if r * n_heads != width:
        raise ValueError(f"rope_gather: projection width {width} is not a multiple of n_heads={n_heads}")
    if x.stride(2) != 1 or x.stride(0) != T * x.stride(1):
        x = x.contiguous()
    cos = cos.to(x.dtype).contiguous()
    sin = sin.to(x.dtype).contiguous()
    if cos.shape != sin.shape or cos.shape[-2:] != (T, head_dim) or cos.shape[0] not in (1, B):
        raise ValueError(f"rope_gather: cos/sin {tuple(cos.shape)} / {tuple(sin.shape)} do not fit [B or 1, {T}, {head_dim}]")
    if mask is not None:
        if mask.dtype != torch.int64 or tuple(mask.shape) != (n_kv, r):
            raise ValueError(f"rope_gather: mask must be int64 [{n_kv}, {r}], got {mask.dtype} {tuple(mask.shape)}")
        mask = mask.contiguous()
    if norm_weight is not None:
        norm_weight = norm_weight.detach().to(x.dtype).contiguous()
    if out is None:
        out = torch.empty(B, n_heads, T, r, dtype=x.dtype, device=x.device)
    elif (tuple(out.shape) != (B, n_heads, T, r) or out.dtype != x.dtype or out.device != x.device
          or not out.is_contiguous()):
        raise ValueError(f"rope_gather: out must be a contiguous {x.dtype} [{B}, {n_heads}, {T}, {r}] on {x.device}, got "
                         f"{out.dtype} {tuple(out.shape)} strides {out.stride()} on {out.device}")
    return x, cos, sin, mask, norm_weight, out, (B, T, r)


def rope_gather(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mask: Optional[torch.Tensor], n_heads: int,
                n_kv: int, head_dim: int, norm_weight: Optional[torch.Tensor] = None, eps: float = 1e-6,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rotary embedding of a compressed q / k projection.  x: [B, T, n_heads*r] (bf16 / f16 / f32, last dim
    contiguous); cos, sin: [B or 1, T, head_dim]; mask: int64 [n_kv, r] or None; returns [B, n_heads, T, r].
    With `norm_weight` ([head_dim]) the Qwen3 masked RMSNorm runs first (DenseQwenRebuild.py:262-286).
    `out`: a caller-owned contiguous [B, n_heads, T, r] tensor of x's dtype to write into (it is returned)."""
    _need_gpu(x, cos, sin)
    lib = _lib.load()
    x, cos, sin, mask, norm_weight, out, (B, T, r) = _rope_operands(x, cos, sin, mask, n_heads, n_kv, head_dim, norm_weight, out)
    with torch.cuda.device(x.device):
        check(lib.mdg_rope_gather(x.data_ptr(), _DT[x.dtype], x.stride(1), B, T, n_heads, n_kv, r, head_dim,
                                  cos.data_ptr(), sin.data_ptr(), 0 if cos.shape[0] == 1 else T * head_dim, _p(mask),
                                  _p(norm_weight), float(eps), out.data_ptr(), _stream(x)), "mdg_rope_gather")
    return out


def rope_gather_plan(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mask: Optional[torch.Tensor], n_heads: int,
                     n_kv: int, head_dim: int, norm_weight: Optional[torch.Tensor] = None, eps: float = 1e-6,
                     out: Optional[torch.Tensor] = None) -> dict:
    """The kernel variant rope_gather(same arguments) launches, as rope_plan_at's dict.  The plan depends on the operands'
    alignment: pass the `out` the call will use (without one, the plan is that of a freshly allocated output)."""
    x, cos, sin, mask, norm_weight, out, (B, T, r) = _rope_operands(x, cos, sin, mask, n_heads, n_kv, head_dim, norm_weight, out)
    return rope_plan_at(x.dtype, B, T, n_heads, n_kv, r, head_dim, x.stride(1), x.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                        0 if cos.shape[0] == 1 else T * head_dim, _p(mask), _p(norm_weight), out.data_ptr())


def rope_rows(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, n_heads: int, head_dim: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rotary embedding of a projection output in its own layout (mdg_rope_rows): x [B, T, n_heads*head_dim] (bf16 / f16 / f32,
    last dim contiguous, rows of one pitch) -> x's shape, bit-identical to torch's eager x * cos + rotate_half(x) * sin.  cos, sin:
    [B or 1, T, head_dim], full width.  `out`: a caller-owned tensor of x's shape and dtype with a contiguous last dim and rows of one
    pitch (it is returned); it must not overlap x -- the model still needs x."""
    _need_gpu(x, cos, sin, out)
    lib = _lib.load()
    if x.dim() != 3 or x.shape[2] != n_heads * head_dim:
        raise ValueError(f"rope_rows: x must be [B, T, n_heads*head_dim = {n_heads * head_dim}], got {tuple(x.shape)}")
    B, T, width = x.shape
    x = x.detach()
    if x.stride(2) != 1 or (B > 1 and x.stride(0) != T * x.stride(1)):
        x = x.contiguous()
    cos = cos.detach().to(x.dtype).contiguous()
    sin = sin.detach().to(x.dtype).contiguous()
    if cos.dim() != 3 or cos.shape != sin.shape or tuple(cos.shape[-2:]) != (T, head_dim) or cos.shape[0] not in (1, B):
        raise ValueError(f"rope_rows: cos/sin {tuple(cos.shape)} / {tuple(sin.shape)} do not fit [B or 1, {T}, {head_dim}]")
    if out is None:
        out = torch.empty(B, T, width, dtype=x.dtype, device=x.device)
    elif (tuple(out.shape) != (B, T, width) or out.dtype != x.dtype or out.device != x.device or out.stride(2) != 1
          or (B > 1 and out.stride(0) != T * out.stride(1))):
        raise ValueError(f"rope_rows: out must be a {x.dtype} [{B}, {T}, {width}] on {x.device} with a contiguous last dim and rows of "
                         f"one pitch, got {out.dtype} {tuple(out.shape)} strides {out.stride()} on {out.device}")
    if x.numel() == 0:
        return out
    with torch.cuda.device(x.device):
        check(lib.mdg_rope_rows(x.data_ptr(), _DT[x.dtype], x.stride(1), B, T, n_heads, head_dim, cos.data_ptr(), sin.data_ptr(),
                                0 if cos.shape[0] == 1 else T * head_dim, out.data_ptr(), out.stride(1), _stream(x)), "mdg_rope_rows")
    return out


def _attn_operands(fn: str, q, k, v, out, scale, causal):
    """The tensor checks attn_fwd and attn_decode share, and what their calls share: (q, k, v, out, the extents (B, T, S, n_heads, n_kv,
    r_qk, r_vo), the 19 arguments every mdg_attn_* entry begins with -- q .. causal --, and out, ld_out, stream that follow the entry's
    own)."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError(f"{fn}: q, k, v must be 4-D, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if q.dtype not in (torch.bfloat16, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"{fn}: q, k, v must share bf16 or f16, got {q.dtype}, {k.dtype}, {v.dtype}")
    B, n_heads, T, r_qk = q.shape
    n_kv, S, r_vo = k.shape[1], k.shape[2], v.shape[3]
    if tuple(k.shape) != (B, n_kv, S, r_qk) or tuple(v.shape) != (B, n_kv, S, r_vo):
        raise ValueError(f"{fn}: k {tuple(k.shape)} / v {tuple(v.shape)} do not fit q {tuple(q.shape)}: "
                         f"k [B, n_kv, S, r_qk], v [B, n_kv, S, r_vo]")
    q, k, v = q.detach(), k.detach(), v.detach()
    if not q.is_contiguous():
        q = q.contiguous()
    for name, t in (("k", k), ("v", v)):
        if t.shape[3] > 1 and t.stride(3) != 1:
            raise ValueError(f"{fn}: {name} must have a contiguous last dimension, got strides {t.stride()}")
    if out is None:
        out = torch.empty(B, T, n_heads, r_vo, dtype=q.dtype, device=q.device)
    elif (tuple(out.shape) != (B, T, n_heads, r_vo) or out.dtype != q.dtype or out.device != q.device
          or (r_vo > 1 and out.stride(3) != 1) or (n_heads > 1 and out.stride(2) != r_vo)
          or (B > 1 and T > 1 and out.stride(0) != T * out.stride(1))):
        raise ValueError(f"{fn}: out must be a {q.dtype} [{B}, {T}, {n_heads}, {r_vo}] on {q.device} with contiguous heads and rows "
                         f"of one pitch, got {out.dtype} {tuple(out.shape)} strides {out.stride()} on {out.device}")
    # the stride of an axis of extent 1 is arbitrary in torch: the pitch of the [B*T] rows comes from an axis that has one
    ld_out = out.stride(1) if T > 1 else out.stride(0) if B > 1 else n_heads * r_vo
    k_ts = k.stride(2) if S > 1 else r_qk
    v_ts = v.stride(2) if S > 1 else r_vo
    dims = (B, T, S, n_heads, n_kv, r_qk, r_vo)
    head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), _DT[q.dtype], *dims, k.stride(0), k.stride(1), k_ts, v.stride(0), v.stride(1), v_ts,
            float(scale), 1 if causal else 0)
    return q, k, v, out, dims, head, (out.data_ptr(), ld_out, _stream(q))


def _attn_mask(fn: str, mask, q, k):
    """The checks of a bool mask for attn_fwd / attn_decode: torch.bool, 4-D, on q's device, [B or 1, 1 or n_heads, T, S] with a unit
    last stride.  Returns (Hm, batch stride, head stride, query stride) in bytes -- torch.bool has one byte per element; an axis
    of extent 1 (or an expanded one) has stride 0."""
    B, n_heads, T = q.shape[0], q.shape[1], q.shape[2]
    S = k.shape[2]
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.dim() != 4:
        raise ValueError(f"{fn}: mask must be a 4-D torch.bool tensor, got "
                         f"{getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
    if mask.device != q.device:
        raise ValueError(f"{fn}: mask on {mask.device}, q on {q.device}")
    if (mask.shape[0] not in (1, B) or mask.shape[1] not in (1, n_heads) or mask.shape[2] != T or mask.shape[3] != S):
        raise ValueError(f"{fn}: mask {tuple(mask.shape)} is not [{B} or 1, 1 or {n_heads}, {T}, {S}]")
    if S > 1 and mask.stride(3) != 1:
        raise ValueError(f"{fn}: mask must have a contiguous last dimension, got strides {mask.stride()}")
    if any(mask.stride(d) < 0 for d in range(3)):
        raise ValueError(f"{fn}: mask with a negative stride {mask.stride()}")
    st = [0 if mask.shape[d] == 1 else mask.stride(d) for d in range(3)]
    return mask.shape[1], st[0], st[1], st[2]


def _attn_mask_summary(mask, B, Hm, T, S, strides):
    """The mdg_attn_mask_summary launch of attn_mask_summary and attn_fwd, on the mask's device and its current stream: (a flat uint8
    buffer of at least one byte, the bytes of it that hold the summary); nothing is launched for an empty summary."""
    lib = _lib.load()
    n = int(lib.mdg_attn_mask_summary_bytes(B, Hm, T, S))
    summary = torch.empty(max(n, 1), dtype=torch.uint8, device=mask.device)
    if n:
        with torch.cuda.device(mask.device):
            check(lib.mdg_attn_mask_summary(mask.data_ptr(), B, Hm, T, S, *strides, summary.data_ptr(), n, _stream(mask)),
                  "mdg_attn_mask_summary")
    return summary, n


def attn_mask_summary(mask: torch.Tensor, B: Optional[int] = None) -> torch.Tensor:
    """The tile summary attn_fwd reads (mdg_attn_mask_summary): bool mask [B or 1, Hm, T, S] with a unit last stride -> uint8
    [B, Hm, ceil(T / 32), ceil(S / 64)], 0 = the 32-query x 64-key tile admits nothing, 1 = everything, 2 = mixed."""
    _need_gpu(mask)
    if mask.dtype != torch.bool or mask.dim() != 4 or (mask.shape[3] > 1 and mask.stride(3) != 1):
        raise ValueError(f"attn_mask_summary: mask must be a 4-D torch.bool tensor with a contiguous last dimension, got {mask.dtype} "
                         f"{tuple(mask.shape)} strides {mask.stride()}")
    B = mask.shape[0] if B is None else int(B)
    if mask.shape[0] not in (1, B):
        raise ValueError(f"attn_mask_summary: mask batch {mask.shape[0]} is not {B} or 1")
    Hm, T, S = mask.shape[1], mask.shape[2], mask.shape[3]
    summary, n = _attn_mask_summary(mask, B, Hm, T, S, [0 if mask.shape[d] == 1 else mask.stride(d) for d in range(3)])
    return summary[:n].view(B, Hm, -(-T // 32), -(-S // 64))


def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, causal: bool = True,
             out: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused attention forward for compressed heads (mdg_attn_fwd): q [B, n_heads, T, r_qk], k [B, n_kv, S, r_qk], v [B, n_kv, S, r_vo]
    (bf16 / f16; r_qk even, r_qk != r_vo allowed, both <= 256) -> [B, T, n_heads, r_vo], the token-major layout o_proj reads.  With
    `causal`, query i sees the keys j <= i + (S - T).  k and v may be views of longer buffers (a static cache): their strides are
    taken as they are, only a non-unit last stride is refused.  `out`: a caller-owned [B, T, n_heads, r_vo] tensor of q's dtype whose
    last two dimensions are contiguous and whose rows have one pitch (it is returned); it must not overlap q, k or v.
    `mask`: a torch.bool [B or 1, 1 or n_heads, T, S] tensor with a unit last stride, taken as it is (expanded axes included): key j
    is admitted for query (b, h, i) iff the mask says so (and the causal rule, with `causal`); a query with no admitted key gets
    zeros; v must be finite at masked keys.  The call then builds the mask's tile summary (mdg_attn_mask_summary, a launch of its
    own on the same stream) and runs mdg_attn_fwd_masked.  Nothing is cached across calls and nothing synchronises."""
    _need_gpu(q, k, v, out)
    lib = _lib.load()
    q, k, v, out, (B, T, S, *_), head, tail = _attn_operands("attn_fwd", q, k, v, out, scale, causal)
    entry, masked = "mdg_attn_fwd", ()
    if mask is not None:
        Hm, *m_strides = _attn_mask("attn_fwd", mask, q, k)
        summary, n_sum = _attn_mask_summary(mask, B, Hm, T, S, m_strides)
        entry, masked = "mdg_attn_fwd_masked", (mask.data_ptr(), Hm, *m_strides, summary.data_ptr(), n_sum)
    with torch.cuda.device(q.device):
        check(getattr(lib, entry)(*head, *tail, *masked), entry)
    return out


ATTN_DECODE_COLUMNS = 32     # mdg_attn_decode's domain: T * (n_heads / n_kv) query columns of one MFMA tile
ATTN_DECODE_MAX_SPLITS = 256  # the most chunks mdg_attn_decode cuts the keys into (its combine kernel has one thread per chunk)


def attn_decode_splits(B: int, n_kv: int, S: int, device) -> int:
    """The default split count of attn_decode for a shape on `device` (mdg_attn_decode_splits with the device's CU count)."""
    n_cu = torch.cuda.get_device_properties(device).multi_processor_count
    return int(_lib.load().mdg_attn_decode_splits(int(B), int(n_kv), int(S), int(n_cu)))


def attn_decode(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, causal: bool = True,
                splits: Optional[int] = None, out: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attn_fwd's product on the split-key decode schedule (mdg_attn_decode), for T * (n_heads / n_kv) <= 32: same operands, same
    `out` contract, same result within the same bound.  The keys are cut into `splits` chunks, one workgroup each per (batch, kv
    head), and a second kernel combines the fp32 partials; `splits=None` asks mdg_attn_decode_splits with the device's CU count.
    The workspace is a torch.empty on q's device.  `mask`: attn_fwd's, read directly by mdg_attn_decode_masked (no summary)."""
    _need_gpu(q, k, v, out)
    lib = _lib.load()
    q, k, v, out, (B, T, S, n_heads, n_kv, _, r_vo), head, tail = _attn_operands("attn_decode", q, k, v, out, scale, causal)
    if n_kv <= 0 or n_heads % n_kv or T * (n_heads // n_kv) > ATTN_DECODE_COLUMNS:
        raise ValueError(f"attn_decode: T={T} queries x a group of n_heads={n_heads} / n_kv={n_kv} heads must fit "
                         f"{ATTN_DECODE_COLUMNS} columns (attn_fwd takes the rest)")
    if splits is None:
        splits = attn_decode_splits(B, n_kv, S, q.device)
    splits = int(splits)
    if not 1 <= splits <= ATTN_DECODE_MAX_SPLITS:
        raise ValueError(f"attn_decode: splits={splits} must be within 1 .. {ATTN_DECODE_MAX_SPLITS}")
    if B == 0 or T == 0:
        return out
    ws_bytes = int(lib.mdg_attn_decode_ws_bytes(B, T, n_heads, r_vo, splits))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=q.device)
    entry, masked = "mdg_attn_decode", ()
    if mask is not None:
        entry, masked = "mdg_attn_decode_masked", (mask.data_ptr(), *_attn_mask("attn_decode", mask, q, k))
    with torch.cuda.device(q.device):
        check(getattr(lib, entry)(*head, splits, ws.data_ptr(), ws_bytes, *tail, *masked), entry)
    return out


def _qk_seq_accum(stem: str, pair, pair_raw, q_rows, k_rows, B, T, n_heads, n_kv, head_dim) -> None:
    """The body qk_pair_accum and qk_causal_accum share (stem "qk_pair" / "qk_causal"): the argument checks, with messages under
    the caller's name, the two row matrices as [B*T, width] views, then mdg_<stem>_accum on a workspace of mdg_<stem>_ws_bytes."""
    fn = stem + "_accum"
    _need_gpu(pair, pair_raw, q_rows, k_rows)
    B, T, n_heads, n_kv, head_dim = int(B), int(T), int(n_heads), int(n_kv), int(head_dim)
    if B < 0 or T < 0:
        raise ValueError(f"{fn}: negative extent (B={B}, T={T})")
    if n_heads <= 0 or n_kv <= 0 or n_heads % n_kv:
        raise ValueError(f"{fn}: n_heads={n_heads} must be a positive multiple of n_kv={n_kv}")
    if not 1 <= head_dim <= 128:
        raise ValueError(f"{fn}: head_dim={head_dim} must be within 1 .. 128")
    rows = []
    for name, x, width in (("q_rows", q_rows, n_heads * head_dim), ("k_rows", k_rows, n_kv * head_dim)):
        x = x.detach()
        if x.dim() == 3 and tuple(x.shape) == (B, T, width) and (B <= 1 or T == 0 or x.stride(0) == T * x.stride(1)):
            x = x.as_strided((B * T, width), (x.stride(1), x.stride(2)), x.storage_offset()) if B * T else x.reshape(0, width)
        if x.dim() != 2 or tuple(x.shape) != (B * T, width):
            raise ValueError(f"{fn}: {name} must be [B*T = {B * T}, {width}] (or [B, T, {width}] rows of one pitch), got "
                             f"{tuple(x.shape)}")
        if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise ValueError(f"{fn}: {name} must be bf16, f16 or f32, got {x.dtype}")
        if B * T and x.stride(1) != 1:
            raise ValueError(f"{fn}: {name} needs a contiguous last dim, got strides {x.stride()}")
        rows.append(x)
    q2, k2 = rows
    if q2.dtype != k2.dtype or q2.device != k2.device:
        raise ValueError(f"{fn}: q_rows and k_rows differ in dtype or device ({q2.dtype} on {q2.device}, {k2.dtype} on {k2.device})")
    for name, p in (("pair", pair), ("pair_raw", pair_raw)):
        if p is None and name == "pair_raw":
            continue
        if (p is None or p.dtype != torch.float64 or tuple(p.shape) != (n_heads, head_dim, head_dim) or not p.is_contiguous()
                or p.device != q2.device):
            raise ValueError(f"{fn}: {name} must be a contiguous fp64 [{n_heads}, {head_dim}, {head_dim}] on {q2.device}")
    if B * T == 0:
        return
    lib = _lib.load()
    need = getattr(lib, f"mdg_{stem}_ws_bytes")(B, n_heads, head_dim, int(pair_raw is not None))
    ws, wsp = _ws(need, q2.device)
    with torch.cuda.device(q2.device):
        check(getattr(lib, "mdg_" + fn)(q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0), _DT[q2.dtype], B, T, n_heads, n_kv,
                                        head_dim, pair.data_ptr(), _p(pair_raw), wsp, need, _stream(q2)), "mdg_" + fn)


def qk_pair_accum(pair: torch.Tensor, pair_raw: Optional[torch.Tensor], q_rows: torch.Tensor, k_rows: torch.Tensor, B: int, T: int,
                  n_heads: int, n_kv: int, head_dim: int) -> None:
    """The within-sequence Q/K statistic of one calibration batch (mdg_qk_pair_accum), enqueued only: for the B sequences of T rows
    each in q_rows [B*T, n_heads*head_dim] and k_rows [B*T, n_kv*head_dim] (bf16 / f16 / f32, one dtype, last dim contiguous, rows
    of one pitch; [B, T, width] views of such rows are taken too -- the rows rope_rows writes), in ascending order,
    pair[h] += G^q (.) (G^k - m m^T / T) and, unless pair_raw is None, pair_raw[h] += G^q (.) G^k.  pair, pair_raw: fp64
    [n_heads, head_dim, head_dim], contiguous, accumulated into."""
    _qk_seq_accum("qk_pair", pair, pair_raw, q_rows, k_rows, B, T, n_heads, n_kv, head_dim)


def qk_causal_accum(pair: torch.Tensor, pair_raw: Optional[torch.Tensor], q_rows: torch.Tensor, k_rows: torch.Tensor, B: int, T: int,
                    n_heads: int, n_kv: int, head_dim: int) -> None:
    """The causal Q/K statistic of one calibration batch (mdg_qk_causal_accum), enqueued only: for the B sequences of T rows each,
    starting at position 0, in q_rows and k_rows (the layouts of qk_pair_accum), in ascending order,
    pair[h] += sum_i (q_i q_i^T) (.) (K_i - m_i m_i^T / n_i) / n_i with the prefix sums K_i, m_i over the keys j <= i, n_i = i + 1,
    and, unless pair_raw is None, pair_raw[h] += sum_i (q_i q_i^T) (.) K_i / n_i.  pair, pair_raw: fp64 [n_heads, head_dim,
    head_dim], contiguous, accumulated into."""
    _qk_seq_accum("qk_causal", pair, pair_raw, q_rows, k_rows, B, T, n_heads, n_kv, head_dim)


_ROPE_SCRATCH = {}


def rope_scratch(like: torch.Tensor, slot: str) -> torch.Tensor:
    """A scratch tensor of `like`'s shape and dtype on its device for the rotated rows of a calibration batch (slot "q" / "k"):
    one flat buffer per (device, slot), grown on demand and reused across layers and batches.  Reuse is ordered by the caller's
    stream: whoever reads the scratch enqueues on the stream the next rope_rows call into it is enqueued on."""
    key = (_device_index(like.device), slot)
    need = like.numel() * like.element_size()
    buf = _ROPE_SCRATCH.get(key)
    if buf is None or buf.numel() < need:
        buf = _ROPE_SCRATCH[key] = torch.empty(need, dtype=torch.uint8, device=like.device)
    return buf[:need].view(like.dtype).view(like.shape)


def cast_transpose(x: torch.Tensor) -> torch.Tensor:
    """bf16(x^T) for an fp64 matrix, with torch's double->float->bf16 rounding."""
    _need_gpu(x)
    lib = _lib.load()
    out = torch.empty(x.shape[1], x.shape[0], dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.mdg_cast_transpose_f64_bf16(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), out.data_ptr(),
                                              out.stride(0), _stream(x)), "mdg_cast_transpose_f64_bf16")
    return out


def probe_mfma_f64(iters: int = 4096) -> float:
    """Measured fp64-MFMA issue rate of this device in TFLOP/s (register-resident operands)."""
    lib = _lib.load()
    out = C.c_double(0.0)
    check(lib.mdg_probe_mfma_f64(iters, C.byref(out), torch.cuda.current_stream().cuda_stream), "mdg_probe_mfma_f64")
    return out.value


def probe_mfma_i8(iters: int = 200000, random_operands: bool = True) -> float:
    """Measured int8-MFMA rate of this device in TOP/s from register-resident operands that change every MFMA: all zero (full
    clock) or random bytes (power-capped clock) -- the ceiling of any int8 kernel on such data."""
    lib = _lib.load()
    out = C.c_double(0.0)
    check(lib.mdg_probe_mfma_i8(iters, int(random_operands), C.byref(out), torch.cuda.current_stream().cuda_stream),
          "mdg_probe_mfma_i8")
    return out.value


def probe_mfma_i8_shape(shape: int, iters: int = 200000, random_operands: bool = True, waves_per_simd: int = 1) -> float:
    """probe_mfma_i8's loop on either int8 MFMA shape (32: v_mfma_i32_32x32x32_i8, 16: v_mfma_i32_16x16x64_i8) at the same
    int8 op count per wave, in TOP/s: under the power cap the chip may hold a different clock on the two shapes."""
    lib = _lib.load()
    out = C.c_double(0.0)
    check(lib.mdg_probe_mfma_i8_shape(shape, waves_per_simd, iters, int(random_operands), C.byref(out),
                                      torch.cuda.current_stream().cuda_stream), "mdg_probe_mfma_i8_shape")
    return out.value


def device_info(device: int = 0):
    lib = _lib.load()
    name = C.create_string_buffer(64)
    n_cu = C.c_int(0)
    hbm = C.c_int64(0)
    check(lib.mdg_device_info(device, name, 64, C.byref(n_cu), C.byref(hbm)), "mdg_device_info")
    return name.value.decode(), n_cu.value, hbm.value
