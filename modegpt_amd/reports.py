"""The host side of the opt-in reports: the environment switches that turn them on and the decoders that read what the kernels left
(lists of Python numbers in, plain dicts out).  No torch, no library: ops.py launches and re-exports every name here."""
import math
import os

RANK_CURVE_TARGETS = QK_ERROR_TARGETS = VO_ERROR_TARGETS = (1e-1, 1e-2, 1e-3)      # the relative errors a rank is looked up for
RANK_CURVE_KEEP = tuple(k / 100 for k in range(5, 101, 5))          # 0.05, 0.10, ..., 1.00
OUTPUT_ERROR_LEVELS = (1e-1, 1e-2, 1e-3)
MARGIN_FIELDS = ("s_selected_max", "s_unselected_min", "selected_upper", "unselected_lower", "sens_selected_max", "sens_unselected_max",
                 "scores_at_risk", "certified")
QK_MARGIN_FIELDS = ("s_selected_min", "s_unselected_max", "selected_lower", "unselected_upper", "score_halfwidth", "units_at_risk",
                    "order_at_risk", "certified")
VO_SPECTRUM_FIELDS = ("lambda_r", "lambda_next", "gap", "energy", "bound", "separated", "lambda_max", "lambda_min")


# ------------------------------------------------------------------ the switches (read when asked: per layer, not frozen at import)
def _switch(name: str) -> bool:
    return os.environ.get(name, "0").lower() in ("1", "on", "true")


# The mean-aware MLP refit ("The MLP intercept").  Opt-in: MODEGPT_MLP_INTERCEPT=1 makes calibration collect the
# column sums of the sigma_mlp activation and compress_nystrom refit on the centred statistic and store an intercept as down_bias.
def mlp_intercept_enabled() -> bool:
    """MODEGPT_MLP_INTERCEPT as it stands when calibration or a compressor asks (per layer; not frozen at import)."""
    return _switch("MODEGPT_MLP_INTERCEPT")


# The mean-aware V/O truncation ("The V/O intercept").  Opt-in: MODEGPT_VO_INTERCEPT=1 makes calibration collect the
# column sums of x (the post-norm hidden state) and compress_vo truncate on the centred statistic and store an intercept as o_bias.
def vo_intercept_enabled() -> bool:
    """MODEGPT_VO_INTERCEPT as it stands when calibration or a compressor asks (per layer; not frozen at import)."""
    return _switch("MODEGPT_VO_INTERCEPT")


# The Nystrom refit's error at every rank (mdg_nystrom_rank_curve).  Opt-in: MODEGPT_RANK_CURVE=1 makes compress_nystrom compute
# it for every layer (one more factorisation of sigma_mlp and a triangular product per layer; DESIGN.md section 7, "The error-versus-rank curve").
def rank_curve_enabled() -> bool:
    """MODEGPT_RANK_CURVE as it stands when compress_nystrom asks (per layer; not frozen at import)."""
    return _switch("MODEGPT_RANK_CURVE")


# The realised output error of the STORED down projection (mdg_mlp_output_error).  Opt-in: MODEGPT_OUTPUT_ERROR=1 makes
# compress_nystrom compute it for every layer from the bf16 tensor it saves (two launches of d n (n + 1) flop per layer; DESIGN.md
# section 7, "The realised output error of the stored MLP weights").
def output_error_enabled() -> bool:
    """MODEGPT_OUTPUT_ERROR as it stands when compress_nystrom asks (per layer; not frozen at import)."""
    return _switch("MODEGPT_OUTPUT_ERROR")


# What the Q/K selection costs the attention logits on the calibration statistic, per query head and at every rank
# (mdg_qk_rank_curve).  Opt-in: MODEGPT_QK_ERROR=1 makes compress_qk compute it for every layer from the statistics it holds anyway
# ("What the Q/K selection costs the attention logits").
def qk_error_enabled() -> bool:
    """MODEGPT_QK_ERROR as it stands when compress_qk asks (per layer; not frozen at import)."""
    return _switch("MODEGPT_QK_ERROR")


# The realised output error of the STORED v_proj / o_proj (mdg_vo_output_error) and the truncation's cost at every rank
# (mdg_vo_rank_curve).  Opt-in: MODEGPT_VO_ERROR=1 makes compress_vo compute both for every layer from the bf16 tensors it saves
# ("The realised output error of the stored V/O factors").
def vo_error_enabled() -> bool:
    """MODEGPT_VO_ERROR as it stands when compress_vo asks (per layer; not frozen at import)."""
    return _switch("MODEGPT_VO_ERROR")


# The post-RoPE Q/K statistics ("Post-RoPE Q/K statistics").  Opt-in: MODEGPT_QK_ROPE=1 makes calibration of a
# rotary model (Llama, Qwen2) rotate the parked q / k rows (mdg_rope_rows) and accumulate sigma_q', sigma_k' beside the pre-RoPE
# pair; with MODEGPT_QK_ERROR=1 compress_qk then reports the logit error on them, which is exact for a rotary model.
def qk_rope_enabled() -> bool:
    """MODEGPT_QK_ROPE as it stands when calibration, the cache or compress_qk asks (not frozen at import)."""
    return _switch("MODEGPT_QK_ROPE")


# Opt-in: MODEGPT_QK_ROPE_SELECT=1 makes compress_qk score, certify and order the pair selection on the post-RoPE statistics instead
# of the reference's pre-RoPE pair.  Needs the statistics (MODEGPT_QK_ROPE=1 at calibration or in the loaded record).
def qk_rope_select_enabled() -> bool:
    """MODEGPT_QK_ROPE_SELECT as it stands when compress_qk asks (per layer; not frozen at import)."""
    return _switch("MODEGPT_QK_ROPE_SELECT")


# The within-sequence, shift-invariant Q/K statistic ("The within-sequence Q/K statistic").  Opt-in:
# MODEGPT_QK_SEQ=1 makes calibration of a rotary model (Llama, Qwen2) that collects the post-RoPE statistics (MODEGPT_QK_ROPE=1)
# also accumulate P_h = sum_s G^q_s (.) (G^k_s - m m^T / T) and its uncentred twin per layer (mdg_qk_pair_accum); with
# MODEGPT_QK_ERROR=1 compress_qk then reports metrics["qk_logit_error_seq"].
def qk_seq_enabled() -> bool:
    """MODEGPT_QK_SEQ as it stands when calibration, the cache or compress_qk asks (not frozen at import)."""
    return _switch("MODEGPT_QK_SEQ")


# Opt-in: MODEGPT_QK_SEQ_SELECT=1 makes compress_qk score and order the pair selection on the within-sequence statistic.  Needs the
# statistic (MODEGPT_QK_SEQ=1 at calibration or in the loaded record); excludes MODEGPT_QK_ROPE_SELECT; no certificate is issued.
def qk_seq_select_enabled() -> bool:
    """MODEGPT_QK_SEQ_SELECT as it stands when compress_qk asks (per layer; not frozen at import)."""
    return _switch("MODEGPT_QK_SEQ_SELECT")


# The causal Q/K statistic ("The causal Q/K statistic").  Opt-in: MODEGPT_QK_CAUSAL=1 makes calibration of a
# rotary model (Llama, Qwen2) that collects the post-RoPE statistics (MODEGPT_QK_ROPE=1) also accumulate, per layer,
# P^c_h = sum_s sum_i (q_i q_i^T) (.) (K_i / n_i - m_i m_i^T / n_i^2) over the keys j <= i each query can see, and its uncentred
# twin (mdg_qk_causal_accum); with MODEGPT_QK_ERROR=1 compress_qk then reports metrics["qk_logit_error_causal"].  Independent of
# MODEGPT_QK_SEQ.
def qk_causal_enabled() -> bool:
    """MODEGPT_QK_CAUSAL as it stands when calibration, the cache or compress_qk asks (not frozen at import)."""
    return _switch("MODEGPT_QK_CAUSAL")


# Opt-in: MODEGPT_QK_CAUSAL_SELECT=1 makes compress_qk score and order the pair selection on the causal statistic.  Needs the
# statistic (MODEGPT_QK_CAUSAL=1 at calibration or in the loaded record); excludes MODEGPT_QK_SEQ_SELECT and MODEGPT_QK_ROPE_SELECT;
# no certificate is issued.
def qk_causal_select_enabled() -> bool:
    """MODEGPT_QK_CAUSAL_SELECT as it stands when compress_qk asks (per layer; not frozen at import)."""
    return _switch("MODEGPT_QK_CAUSAL_SELECT")


def qk_select_statistic() -> str:
    """Which statistic the pair selection is scored on, from the three select switches as they stand: "causal", "seq", "rope" or
    "default".  At most one of MODEGPT_QK_CAUSAL_SELECT, MODEGPT_QK_SEQ_SELECT, MODEGPT_QK_ROPE_SELECT may be set: the selection
    takes one statistic."""
    on = [(name, kind) for name, kind, fn in (("MODEGPT_QK_CAUSAL_SELECT", "causal", qk_causal_select_enabled),
                                              ("MODEGPT_QK_SEQ_SELECT", "seq", qk_seq_select_enabled),
                                              ("MODEGPT_QK_ROPE_SELECT", "rope", qk_rope_select_enabled)) if fn()]
    if len(on) > 1:
        raise RuntimeError(" and ".join(f"{name}=1" for name, _ in on) + (" are both set" if len(on) == 2 else " are all set") +
                           ": the pair selection takes one statistic")
    return on[0][1] if on else "default"


# Greedy MLP selection (mdg_nystrom_greedy_select; DESIGN.md section 7, "Greedy MLP selection").  Opt-in: MODEGPT_MLP_GREEDY=T makes
# compress_nystrom select each layer's columns by T rounds of block-greedy descent on the objective the refit minimises, instead of
# the reference's ridge-leverage rule.  No certificate is issued for that selection.
def mlp_greedy_rounds() -> int:
    """MODEGPT_MLP_GREEDY as it stands when compress_nystrom asks (per layer; not frozen at import): 0 (off) when unset or "0",
    the number of rounds for a positive integer, ValueError for anything else."""
    raw = os.environ.get("MODEGPT_MLP_GREEDY")
    if raw is None:
        return 0
    rounds = int(raw) if raw.strip().isdigit() else -1
    if rounds < 0:
        raise ValueError(f"MODEGPT_MLP_GREEDY must be unset, 0 or a positive number of rounds, got {raw!r}")
    return rounds


def greedy_partition(r: int, rounds: int) -> list:
    """The picks per round of mdg_nystrom_greedy_select: m_t = floor(r (t + 1) / T) - floor(r t / T) with T = min(rounds, r), then
    zeros for the rounds beyond r.  Sums to r."""
    r, rounds = int(r), int(rounds)
    if r < 0 or rounds < 1:
        raise ValueError(f"greedy_partition: need r >= 0 and rounds >= 1, got {r}, {rounds}")
    T = min(rounds, r)
    return [r * (t + 1) // T - r * t // T for t in range(T)] + [0] * (rounds - T)


def keep_bias_enabled(arch=None) -> bool:
    """Whether the compressors carry the projection biases into the artefacts ("Projection biases"): always
    for Qwen2 / Qwen2.5 (model_type "qwen2": nothing of the reference's to preserve, and dropping q/k/v biases is never right),
    otherwise MODEGPT_KEEP_BIAS as it stands when a compressor asks (per layer; not frozen at import).  Off: the reference's
    behaviour, every rebuilt Linear bias-free (model_adapter.py:199-208)."""
    return arch == "qwen2" or _switch("MODEGPT_KEEP_BIAS")


# ------------------------------------------------------------------ what the decoders share
def _vec(t):
    return [float(x) for x in t]


def _mat(t):
    return [[float(x) for x in row] for row in t]


def _fin(x):                               # x, or None where it is missing or not finite
    return x if x is not None and math.isfinite(x) else None


def _total(v):                             # the exactly rounded sum of a flat or nested list; NaN if an entry is missing or not finite
    flat = [x for row in v for x in row] if v and isinstance(v[0], list) else list(v)
    return math.fsum(flat) if all(_fin(x) is not None for x in flat) else float("nan")


def _ratio(a, b):                          # a / b for finite a and finite b > 0, else None
    return a / b if _fin(a) is not None and _fin(b) is not None and b > 0 else None


# ------------------------------------------------------------------ MLP
def decode_margin(out8, eps: float) -> dict:
    """Host-side reading of select_margin's 8 numbers (a list / CPU tensor): the relative margin of the selection threshold, the
    bound on what a perturbation of relative size eps can do to a score there, and whether the selected set is certified."""
    v = _vec(out8)
    s_k, s_k1 = v[0], v[1]
    finite = s_k > float("-inf") and s_k1 < float("inf")
    margin = (s_k1 - s_k) / abs(s_k) if finite and s_k != 0 else float("inf")
    spread = v[4] + v[5]
    return {"margin": margin, "score_bound": eps * max(v[4], v[5]) / abs(s_k) if finite and s_k != 0 else 0.0,
            "eps": eps, "eps_certifiable": (s_k1 - s_k) / spread if finite and spread > 0 else float("inf"),
            "scores_at_risk": int(v[6]), "certified": bool(v[7] == 1.0), **{k: x for k, x in zip(MARGIN_FIELDS[:4], v[:4])}}


def decode_rank_curve(curve, rank: int) -> dict:
    """Host-side reading of a rank curve (a list / CPU tensor of n + 1 numbers) for a layer compressed to `rank`:
    n, rank, energy = curve[0] (the output energy tr(W (C + eps I) W^T) of the uncompressed MLP), rel_error = curve[rank] / energy,
    keep = RANK_CURVE_KEEP with rel_error_at_keep = the relative error at rank int(n * keep) (compress_weights' rounding), and
    rank_for_rel_error = {target: the smallest rank whose relative error is at or under it} for RANK_CURVE_TARGETS.  A zero or
    non-finite energy gives None in every relative field; the energy itself and a non-finite curve entry are passed through raw."""
    v = _vec(curve)
    n, rank, energy = len(v) - 1, int(rank), v[0]
    if n < 0 or not 0 <= rank <= n:
        raise ValueError(f"decode_rank_curve: rank {rank} outside 0 .. {n}")
    ok = energy > 0 and energy < float("inf")         # (False for NaN)
    rel = (lambda r: v[r] / energy) if ok else (lambda r: None)

    def smallest_rank(target):       # the curve is non-increasing: bisect for the first rank at or under the target
        if not ok:
            return None
        lo, hi = 0, n                # invariant: rel(hi) <= target (rel(n) = 0)
        if not v[n] / energy <= target:
            return None
        while lo < hi:
            mid = (lo + hi) // 2
            if v[mid] / energy <= target:
                hi = mid
            else:
                lo = mid + 1
        return hi
    return {"n": n, "rank": rank, "energy": energy, "rel_error": rel(rank), "keep": list(RANK_CURVE_KEEP),
            "rel_error_at_keep": [rel(int(n * k)) for k in RANK_CURVE_KEEP],
            "rank_for_rel_error": {"%g" % t: smallest_rank(t) for t in RANK_CURVE_TARGETS}}


def decode_mlp_greedy(objective, cut, n_dead, rank: int, ridge_at_rank=None, greedy_at_rank=None) -> dict:
    """Host-side reading of nystrom_greedy_select's numbers (lists / CPU tensors: objective [rounds + 1], cut [rounds][2] or None,
    n_dead a number) for a layer that keeps `rank` columns:
    rounds, rank, objective (a non-finite entry as None), objective_over_total = objective[-1] / objective[0], dead_picks,
    min_cut_gap = the smallest (picked - unpicked) / picked over the rounds that have both sides of their cut -- how far the weakest
    pick stood above the strongest column left behind (None without such a round).  With the rank curves' two values at `rank`
    (MODEGPT_RANK_CURVE=1): ridge_at_rank (the ridge-leverage rule's residual energy), greedy_at_rank (this selection's, by the
    rank curve's independent route) and greedy_over_ridge, their ratio.  Non-finite figures become None."""
    obj = _vec(objective)
    if len(obj) < 2:
        raise ValueError("decode_mlp_greedy: objective needs rounds + 1 >= 2 entries")
    gaps = []
    for row in ([] if cut is None else _mat(cut)):
        lo, hi = _fin(row[0]), _fin(row[1])
        if lo is not None and hi is not None and lo > 0:
            gaps.append((lo - hi) / lo)
    out = {"rounds": len(obj) - 1, "rank": int(rank), "objective": [_fin(x) for x in obj],
           "objective_over_total": _ratio(obj[-1], obj[0]) if _fin(obj[-1]) is not None and obj[-1] >= 0 else None,
           "dead_picks": int(n_dead), "min_cut_gap": min(gaps) if gaps else None}
    if ridge_at_rank is not None or greedy_at_rank is not None:
        ridge = None if ridge_at_rank is None else float(ridge_at_rank)
        greedy = None if greedy_at_rank is None else float(greedy_at_rank)
        out.update({"ridge_at_rank": _fin(ridge), "greedy_at_rank": _fin(greedy),
                    "greedy_over_ridge": _ratio(greedy, ridge) if greedy is not None and greedy >= 0 else None})
    return out


def decode_output_error(e, q, unorm2, eps: float, rank: int, curve=None) -> dict:
    """Host-side reading of a layer's output error (lists / CPU tensors of d numbers each: e and unorm2 of the stored tensor, q of
    the uncompressed weights; eps: the ridge of the refit; rank: the columns kept):
    rank, energy = sum q, error = sum e, relative_error = error / energy, objective = error + eps sum unorm2 (what the refit
    minimises, compress_mlp.py:52-62), worst_channel = the channel with the largest e_k / q_k among those with q_k > 0 and
    worst_channel_relative_error that ratio, channels_above = {level: how many such channels exceed it} for OUTPUT_ERROR_LEVELS.
    With the layer's rank curve (n + 1 numbers): predicted_objective = curve[rank], the minimum of the objective over all refits,
    and excess_over_optimum = (objective - curve[rank]) / curve[0] -- what rounding to bf16 and solving with C[S, :] instead of
    M[S, :] cost beyond the best refit.  A non-finite sum gives None in the fields derived from it."""
    ev, qv, uv = _vec(e), _vec(q), _vec(unorm2)
    if not len(ev) == len(qv) == len(uv):
        raise ValueError("decode_output_error: e, q and unorm2 must have one entry per output channel")
    energy, error, u2 = _total(qv), _total(ev), _total(uv)
    objective = error + float(eps) * u2
    ratios = [(ek / qk, k) for k, (ek, qk) in enumerate(zip(ev, qv)) if qk > 0 and math.isfinite(qk) and math.isfinite(ek)]
    worst = max(ratios, key=lambda t: (t[0], -t[1])) if ratios and math.isfinite(error) and math.isfinite(energy) else None
    out = {"rank": int(rank), "energy": _fin(energy), "error": _fin(error), "relative_error": _ratio(error, energy),
           "objective": _fin(objective),
           "worst_channel": None if worst is None else worst[1],
           "worst_channel_relative_error": None if worst is None else worst[0],
           "channels_above": {"%g" % t: (None if worst is None else sum(1 for x, _ in ratios if x > t)) for t in OUTPUT_ERROR_LEVELS}}
    if curve is not None:
        cv = _vec(curve)
        if not 0 <= int(rank) < len(cv):
            raise ValueError(f"decode_output_error: rank {rank} outside the curve's 0 .. {len(cv) - 1}")
        ok = math.isfinite(cv[int(rank)]) and math.isfinite(cv[0]) and cv[0] > 0
        out["predicted_objective"] = cv[int(rank)] if ok else None
        out["excess_over_optimum"] = (objective - cv[int(rank)]) / cv[0] if ok and math.isfinite(objective) else None
    return out


# ------------------------------------------------------------------ Q/K
def decode_qk_margin(rows, eps_rel: float, eps_abs: float) -> dict:
    """Host-side reading of qk_select_margin's [n_kv, 8] numbers (nested list / CPU tensor).  Per kv head: the relative margin
    between the weakest selected and the strongest unselected unit, the relative half-width a score can move within the error
    model, how many units sit within reach of the threshold, how many neighbours of the selected order could swap, and whether set
    and order are certified.  Layer summary: the weakest head (smallest margin among the uncertified heads, else among all), its
    margin and half-width, and whether every head is certified.  Infinite margins are passed through raw."""
    heads = []
    for v in _mat(rows):
        s_sel, s_unsel = v[0], v[1]
        separable = s_unsel > float("-inf") and s_sel < float("inf")
        margin = (s_sel - s_unsel) / s_sel if separable and s_sel > 0 else (float("inf") if not separable else float("-inf"))
        certified = v[7] == 1.0
        heads.append({"margin": margin, "score_halfwidth": v[4], "units_at_risk": int(v[5]), "order_at_risk": int(v[6]),
                      "certified": certified, "order_certified": certified and v[6] == 0.0,
                      **{k: x for k, x in zip(QK_MARGIN_FIELDS[:4], v[:4])}})
    weakest = min(range(len(heads)), key=lambda i: (heads[i]["certified"], heads[i]["margin"])) if heads else None
    return {"heads": heads, "eps_rel": float(eps_rel), "eps_abs": float(eps_abs), "weakest_head": weakest,
            "margin": heads[weakest]["margin"] if heads else float("inf"),
            "score_halfwidth": heads[weakest]["score_halfwidth"] if heads else 0.0,
            "certified": all(h["certified"] for h in heads), "order_certified": all(h["order_certified"] for h in heads)}


def decode_qk_logit_error(curve_h, curve, rank: int, cols_per_unit: int, terms=None, scale=None, greedy_curve=None) -> dict:
    """Host-side reading of qk_rank_curve's numbers (nested lists / CPU tensors: curve_h [n_heads][ns + 1], curve and greedy_curve
    [n_kv][ns + 1], terms [n_kv][ns], scale [n_kv]); rank: the columns kept per head, cols_per_unit: 2 for the RoPE modes, 1 for OPT.
    With m = rank / cols_per_unit units kept, per kv head under "heads":
    energy = curve[0] (the mean-square logit of the group's heads), error = curve[m], relative_error = error / energy;
    diagonal_estimate = sum_{i >= m} terms[i] (what the reference's rule believes the cost is) and diagonal_ratio = diagonal_estimate /
    error (far from 1: the off-diagonal correlations the rule ignores matter); greedy_relative_error = greedy_curve[m] / energy;
    rank_for_rel_error = {"selection" / "greedy": {target: the fewest columns per head at which the curve is at or under target x
    energy}} for QK_ERROR_TARGETS (the curve need not be monotone: the FIRST such rank; None without a usable energy);
    head_relative_error = [curve_h[h][m] / curve_h[h][0]] over the group's query heads; noise_floor = (g hd^2 + 2) 2^-53 scale / energy,
    below which a relative value says nothing; non_monotone = some curve[i + 1] > curve[i] by more than that floor.
    The layer: the sums over the kv heads (energy-weighted), non_monotone = any head's.  Values are reported raw, never clamped; a
    non-finite figure, or one derived from an unusable energy, is None."""
    ch, cv = _mat(curve_h), _mat(curve)
    n_heads, n_kv, rank, cols = len(ch), len(cv), int(rank), int(cols_per_unit)
    if n_kv <= 0 or n_heads % n_kv or cols not in (1, 2) or any(len(row) != len(cv[0]) for row in cv + ch) or len(cv[0]) < 1:
        raise ValueError("decode_qk_logit_error: curve_h must be [n_heads][ns + 1] and curve [n_kv][ns + 1], n_heads a multiple of n_kv")
    ns, group = len(cv[0]) - 1, n_heads // n_kv
    if rank % cols or not 0 <= rank // cols <= ns:
        raise ValueError(f"decode_qk_logit_error: rank {rank} is not a whole number of units within 0 .. {ns * cols}")
    m, hd = rank // cols, ns * cols
    tv, gv, sv = (None if terms is None else _mat(terms), None if greedy_curve is None else _mat(greedy_curve),
                  None if scale is None else _vec(scale))
    if (tv is not None and (len(tv) != n_kv or any(len(r) != ns for r in tv))) or (sv is not None and len(sv) != n_kv) or \
            (gv is not None and (len(gv) != n_kv or any(len(r) != ns + 1 for r in gv))):
        raise ValueError(f"decode_qk_logit_error: terms must be [{n_kv}][{ns}], scale [{n_kv}] and greedy_curve [{n_kv}][{ns + 1}]")
    unit = (group * hd * hd + 2) * 2.0 ** -53

    def first_under(c, energy):      # linearly, in columns per head: the unit index times cols_per_unit
        if _fin(energy) is None or energy <= 0 or not all(map(math.isfinite, c)):
            return {"%g" % t: None for t in QK_ERROR_TARGETS}
        return {"%g" % t: next((i * cols for i, x in enumerate(c) if x <= t * energy), None) for t in QK_ERROR_TARGETS}

    heads = []
    for g in range(n_kv):
        c = cv[g]
        energy, error = c[0], c[m]
        floor_abs = unit * sv[g] if sv is not None and _fin(sv[g]) is not None else None
        diag = None if tv is None else _total(tv[g][m:])
        heads.append({"energy": _fin(energy), "error": _fin(error), "relative_error": _ratio(error, energy),
                      "diagonal_estimate": _fin(diag), "diagonal_ratio": _ratio(diag, error),
                      "greedy_relative_error": None if gv is None else _ratio(gv[g][m], energy),
                      "rank_for_rel_error": {"selection": first_under(c, energy),
                                             "greedy": None if gv is None else first_under(gv[g], energy)},
                      "head_relative_error": [_ratio(ch[q][m], ch[q][0]) for q in range(g * group, (g + 1) * group)],
                      "noise_floor": _ratio(floor_abs, energy),
                      "non_monotone": (any(b > a + (floor_abs or 0.0) for a, b in zip(c, c[1:]))
                                       if all(map(math.isfinite, c)) else None)})

    energy, error, diag = (_fin(_total([h[key] for h in heads])) for key in ("energy", "error", "diagonal_estimate"))
    greedy = None if gv is None else _fin(_total([gv[g][m] for g in range(n_kv)]))
    floors = None if sv is None else _fin(_total([unit * s for s in sv]))
    flags = [h["non_monotone"] for h in heads]
    return {"rank": rank, "units_kept": m, "n_kv": n_kv, "head_dim": hd, "energy": energy, "error": error,
            "relative_error": _ratio(error, energy), "diagonal_estimate": diag, "diagonal_ratio": _ratio(diag, error),
            "greedy_relative_error": _ratio(greedy, energy), "noise_floor": _ratio(floors, energy),
            "non_monotone": None if any(f is None for f in flags) else any(flags), "heads": heads}


def decode_qk_seq_error(curve_h, curve, raw_curve, rank: int, cols_per_unit: int, terms=None, scale=None, greedy_curve=None) -> dict:
    """decode_qk_logit_error of the curves taken on the within-sequence statistic P, plus the same error on the uncentred P_raw
    (raw_curve [n_kv][ns + 1], same order): per kv head and for the layer, raw_error = raw_curve[m] and
    shift_share = 1 - error / raw_error, the share of the within-sequence logit change at the kept rank that depends on the query
    alone and that softmax therefore cannot see (None where raw_error is not a usable positive number)."""
    out = decode_qk_logit_error(curve_h, curve, rank, cols_per_unit, terms=terms, scale=scale, greedy_curve=greedy_curve)
    rv = _mat(raw_curve)
    if len(rv) != out["n_kv"] or any(len(r) != len(rv[0]) for r in rv) or len(rv[0]) != out["head_dim"] // int(cols_per_unit) + 1:
        raise ValueError("decode_qk_seq_error: raw_curve must have curve's shape")
    m = out["units_kept"]

    def share(error, raw):
        r = _ratio(error, raw)
        return None if r is None or raw <= 0 else 1.0 - r

    for g, h in enumerate(out["heads"]):
        h["raw_error"] = _fin(rv[g][m])
        h["shift_share"] = share(h["error"], rv[g][m])
    raw = _fin(_total([rv[g][m] for g in range(out["n_kv"])]))
    out["raw_error"] = raw
    out["shift_share"] = None if raw is None else share(out["error"], raw)
    return out


def decode_qk_causal_error(curve_h, curve, raw_curve, rank: int, cols_per_unit: int, terms=None, scale=None, greedy_curve=None,
                           seq=None) -> dict:
    """decode_qk_seq_error of the curves taken on the causal statistic P^c and its uncentred twin: error is then the mean over the
    queries of the variance of the logit change over the keys each query can see, raw_error the mean square over them, shift_share
    the share of raw_error that softmax cannot see.  seq: the layer's metrics["qk_logit_error_seq"] entry at the same rank, or None;
    with it, per kv head and for the layer, over_full = error / (seq error), what the causal mask makes of the figure that pairs every
    query with every key of its sequence (None where the seq error is not a usable positive number)."""
    out = decode_qk_seq_error(curve_h, curve, raw_curve, rank, cols_per_unit, terms=terms, scale=scale, greedy_curve=greedy_curve)
    if seq is not None:
        if seq.get("rank") != out["rank"] or len(seq.get("heads", ())) != out["n_kv"]:
            raise ValueError("decode_qk_causal_error: seq must be the within-sequence entry of the same layer at the same rank")
        for h, hs in zip(out["heads"], seq["heads"]):
            h["over_full"] = _ratio(h["error"], hs.get("error"))
        out["over_full"] = _ratio(out["error"], seq.get("error"))
    return out


# ------------------------------------------------------------------ V/O
def decode_vo_spectrum(rows, eps: float) -> dict:
    """Host-side reading of vo_compress(want_spectrum=True)'s [n_kv, 8] numbers.  Per kv head VO_SPECTRUM_FIELDS ("separated": True /
    False for the grouped variant, None for the two-SVD MHA variant, whose second spectrum has no bound here).  Layer summary: the
    head with the smallest relative gap, that gap, the smallest retained energy, and "separated" (False as soon as one grouped head
    is not; None for MHA)."""
    heads = []
    for v in _mat(rows):
        sep = None if v[5] != v[5] else v[5] == 1.0
        heads.append({**{k: x for k, x in zip(VO_SPECTRUM_FIELDS, v)}, "bound": None if v[4] != v[4] else v[4], "separated": sep})
    weakest = min(range(len(heads)), key=lambda i: heads[i]["gap"]) if heads else None
    seps = [h["separated"] for h in heads]
    return {"heads": heads, "eps": float(eps), "weakest_head": weakest, "gap": heads[weakest]["gap"] if heads else float("inf"),
            "energy_min": min((h["energy"] for h in heads), default=1.0),
            "separated": None if (not seps or any(x is None for x in seps)) else all(seps)}


def decode_vo_output_error(e, q, dnorm2, ridge: float, rank: int, n_kv: int, curve=None, hd=None) -> dict:
    """Host-side reading of a layer's V/O output error (nested lists / CPU tensors [n_heads][d]: e and dnorm2 of the stored factors, q
    of the uncompressed weights; ridge: the ridge vo_compress was called with; rank: the components kept per head).  Layer and, under
    "heads", per kv head (a kv head's numbers are the sums over its group's query heads):
    energy = sum q, error = sum e, relative_error = error / energy, objective = error + ridge sum dnorm2 (what the truncation is
    judged by under C + ridge I), noise_floor = 64 (d + hd + rank) 2^-53 energy -- e is accurate relative to a scale a >= q, not to
    itself, so an error below the floor (of either sign) says nothing; hd is taken from the curve, else from `hd`, else as rank.
    worst_head = the QUERY head with the largest error / energy, worst_head_relative_error, and worst_channel /
    worst_channel_relative_error = the channel of that head with the largest e / q among those with q > 0.
    With the layer's curve ([n_kv][hd + 1], vo_compress(want_curve=True)), per kv head: predicted_objective = curve[g][rank],
    excess_over_curve = (objective - curve[g][rank]) / curve[g][0] (what rounding the factors to bf16 costs beyond the fp64
    truncation; rounding noise of either sign for fp64 factors), relative_curve = curve[g][r] / curve[g][0] for every r, and
    rank_for_rel_error = {target: the smallest rank at or under it} for VO_ERROR_TARGETS; the layer gets predicted_objective and
    excess_over_curve of the sums.  A zero or non-finite sum gives None in the fields derived from it."""
    ev, qv, nv = _mat(e), _mat(q), _mat(dnorm2)
    n_heads, rank, n_kv = len(ev), int(rank), int(n_kv)
    if not (len(qv) == len(nv) == n_heads) or n_kv <= 0 or n_heads % n_kv or any(len(a) != len(b) or len(a) != len(c)
                                                                                 for a, b, c in zip(ev, qv, nv)):
        raise ValueError("decode_vo_output_error: e, q and dnorm2 must be [n_heads][d] with n_heads a multiple of n_kv")
    group, d = n_heads // n_kv, (len(ev[0]) if n_heads else 0)
    cv = None
    if curve is not None:
        cv = _mat(curve)
        if len(cv) != n_kv or any(len(row) != len(cv[0]) or not 0 <= rank < len(row) for row in cv):
            raise ValueError(f"decode_vo_output_error: the curve must be [{n_kv}][hd + 1] with rank {rank} <= hd")
        hd = len(cv[0]) - 1
    hd = rank if hd is None else int(hd)
    unit = 64.0 * (d + hd + rank) * 2.0 ** -53

    def summary(heads_of, curves):
        energy, error, n2 = (_total([t[h] for h in heads_of]) for t in (qv, ev, nv))
        objective = error + float(ridge) * n2
        out = {"energy": _fin(energy), "error": _fin(error), "objective": _fin(objective),
               "relative_error": _ratio(error, energy),
               "noise_floor": unit * energy if math.isfinite(energy) and energy > 0 else None}
        if curves is not None:
            at, top = math.fsum(c[rank] for c in curves), math.fsum(c[0] for c in curves)
            ok = math.isfinite(at) and math.isfinite(top) and top > 0
            out["predicted_objective"] = at if ok else None
            out["excess_over_curve"] = (objective - at) / top if ok and math.isfinite(objective) else None
        return out

    heads = []
    for g in range(n_kv):
        m = summary(range(g * group, (g + 1) * group), None if cv is None else [cv[g]])
        if cv is not None:
            c = cv[g]
            ok = math.isfinite(c[0]) and c[0] > 0 and all(math.isfinite(x) for x in c)
            m["relative_curve"] = [x / c[0] for x in c] if ok else None
            # (non-increasing, and its last entry is +0.0: the first rank at or under the target, taken linearly)
            m["rank_for_rel_error"] = {"%g" % t: (next(r for r, x in enumerate(c) if x / c[0] <= t) if ok else None)
                                       for t in VO_ERROR_TARGETS}
        heads.append(m)
    out = {"rank": rank, "n_kv": n_kv, **summary(range(n_heads), cv), "heads": heads}
    ratios = []
    for h in range(n_heads):
        eh, qh = _total(ev[h]), _total(qv[h])
        if math.isfinite(eh) and math.isfinite(qh) and qh > 0:
            ratios.append((eh / qh, -h))
    worst = max(ratios) if ratios and out["relative_error"] is not None else None
    out["worst_head"] = None if worst is None else -worst[1]
    out["worst_head_relative_error"] = None if worst is None else worst[0]
    chan = None
    if worst is not None:
        h = -worst[1]
        per = [(ek / qk, -k) for k, (ek, qk) in enumerate(zip(ev[h], qv[h])) if qk > 0]
        chan = max(per) if per else None
    out["worst_channel"] = None if chan is None else -chan[1]
    out["worst_channel_relative_error"] = None if chan is None else chan[0]
    return out
