"""CPU: the host side of the attention certificates (QK pair selection, VO spectral gap) on hand-made numbers, the one measured
constant of the QK certificate against the CPU oracle, and the torch restatement of the interval rule the GPU tests compare
mdg_qk_select_margin with (tests/test_gpu_attn_certificate.py imports `qk_margin_host`, `eigh_route_family`, `ladder_heads`)."""
import logging
import math

import pytest
import torch

from oracle import modegpt_oracle as O
from tests.golden_util import CASES, Case

F64 = torch.float64
INF = float("inf")
ROPE_GROUPED, ROPE_MHA, OPT = 0, 1, 2


# ---------------------------------------------------------------- the interval rule, restated
def qk_margin_host(cov_q, cov_k, rank, mode, ridge_q, ridge_k, mask, eps_rel, eps_abs):
    """mdg_qk_select_margin in torch fp64 on the CPU: [n_kv, 8].  Every diagonal entry c of a head matrix C is known to within
    delta = eps_rel |c| + eps_abs (||C||_inf + rho); the scores are monotone in every diagonal entry, so the score formula at
    max(c - delta + rho, 0) / max(c + delta + rho, 0) gives the ends of each score's interval."""
    cov_q, cov_k, mask = cov_q.to(F64).cpu(), cov_k.to(F64).cpu(), mask.cpu()
    n_heads, hd, _ = cov_q.shape
    n_kv = cov_k.shape[0]
    g, half = n_heads // n_kv, hd // 2
    take = rank if mode == OPT else rank // 2

    def ends(Cm, ridge):                                    # [3, hd]: centre, low, high of C_jj + rho
        c = torch.diagonal(Cm)
        delta = eps_rel * c.abs() + eps_abs * (Cm.abs().sum(dim=1).max() + ridge)
        return torch.stack([c + ridge, c - delta + ridge, c + delta + ridge]).clamp(min=0)

    out = torch.empty(n_kv, 8, dtype=F64)
    for h in range(n_kv):
        K = ends(cov_k[h], ridge_k)
        if mode == OPT:
            s = torch.sqrt(ends(cov_q[h], ridge_q)) * torch.sqrt(K)
        else:
            s = torch.zeros(3, half, dtype=F64)
            for q in range(h * g, (h + 1) * g):
                Q = ends(cov_q[q], ridge_q)
                s = s + (Q[:, :half] * K[:, :half] + Q[:, half:] * K[:, half:])
            s = torch.sqrt(s) if mode == ROPE_GROUPED else s
        c, lo, hi = s
        order = mask[h, :take]
        sel = torch.zeros(c.numel(), dtype=torch.bool)
        sel[order] = True
        rest = bool((~sel).any())
        out[h, 0], out[h, 1] = c[sel].min(), (c[~sel].max() if rest else -INF)
        out[h, 2], out[h, 3] = lo[sel].min(), (hi[~sel].max() if rest else -INF)
        out[h, 4] = ((hi - lo) / (2 * c)).max()
        mid = 0.5 * (out[h, 0] + out[h, 1])
        out[h, 5] = int(((lo <= mid) & (mid <= hi)).sum()) if rest else 0
        out[h, 6] = int((~(lo[order[:-1]] > hi[order[1:]])).sum())
        out[h, 7] = 1.0 if bool(torch.isfinite(s).all()) and out[h, 2] > out[h, 3] else 0.0
    return out


def ladder_heads(n_heads, n_kv, hd, mode, gen, ridge_k, step=0.01, scale=1e-3):
    """sigma_q [n_heads, hd, hd] / sigma_k [n_kv, hd, hd]: weak off-diagonals under an exactly prescribed diagonal -- sigma_k's + ridge_k is
    a geometric ladder (the two partners of a rotary pair equal, shuffled), sigma_q's is 1 -- so the scores of neighbouring units are
    `step` apart in every mode.  Returns (cov_q, cov_k, perm) with perm[h][i] = the unit holding
    the i-th LARGEST score of kv head h."""
    ns = hd if mode == OPT else hd // 2
    fac = (1 + step) if mode == ROPE_MHA else ((1 + step) ** 2)     # (ROPE_MHA scores are not square-rooted)

    def weak(n):
        H = torch.randn(n, 4 * hd, hd, generator=gen, dtype=F64) * scale
        Cm = H.transpose(1, 2) @ H / (4 * hd)
        return Cm - torch.diag_embed(torch.diagonal(Cm, dim1=1, dim2=2))
    cov_q = weak(n_heads) + torch.eye(hd, dtype=F64)
    cov_k = weak(n_kv)
    perms = []
    for h in range(n_kv):
        perm = torch.randperm(ns, generator=gen)
        vals = torch.empty(ns, dtype=F64)
        vals[perm] = 0.5 * fac ** (-torch.arange(ns, dtype=F64))
        cov_k[h] += torch.diag((vals if mode == OPT else torch.cat((vals, vals))) - ridge_k)
        perms.append(perm)
    return cov_q, cov_k, perms


# ---------------------------------------------------------------- the one measured number: eps_abs
def eigh_route_family():
    """The family EIGH_ROUTE_EPS_ABS is measured over: yields (name, C [hd, hd] fp64, rho).  Every sigma_q / sigma_k head of
    tests/golden/ at rho in {1e-4, 1e-2}, and 96 seeded synthetic matrices: hd in {64, 128}, C = X^T X / T (T = 4 hd) with column
    scales spread log-uniformly over 0, 2, 4, 6 decades (shuffled) and mild mixing (I + 0.1 G / sqrt(hd)), rho in {1e-4, 1e-2},
    6 seeds each."""
    for name in CASES:
        c = Case(name)
        for key in ("sigma_q", "sigma_k"):
            for h, Cm in enumerate(c.f64[key]):
                for rho in (1e-4, 1e-2):
                    yield f"{name}/{key}[{h}]/rho={rho:g}", Cm, rho
    for hd in (64, 128):
        for decades in (0, 2, 4, 6):
            for rho in (1e-4, 1e-2):
                for seed in range(6):
                    gen = torch.Generator().manual_seed(100000 * hd + 1000 * decades + 10 * seed + (rho > 1e-3))
                    X = torch.randn(4 * hd, hd, generator=gen, dtype=F64)
                    X = X @ (torch.eye(hd, dtype=F64) + 0.1 * torch.randn(hd, hd, generator=gen, dtype=F64) / math.sqrt(hd))
                    scales = 10.0 ** (-decades * torch.linspace(0, 1, hd, dtype=F64))[torch.randperm(hd, generator=gen)]
                    X = X * scales
                    yield f"synthetic/hd={hd}/decades={decades}/rho={rho:g}/seed={seed}", X.T @ X / (4 * hd), rho


def eigh_route_error(Cm, rho):
    """| ||col_j(sqrt_M(C, rho))||^2 - (C_jj + rho) | / (||C||_inf + rho), worst column: how far the reference's route to a squared
    column norm (eigh -> sqrt -> V diag V^T -> column norm) lands from the identity the engine scores with."""
    S = O.sqrt_M(Cm, ridge_lambda=rho)
    got = torch.norm(S, dim=0) ** 2
    return ((got - (torch.diagonal(Cm) + rho)).abs().max() / (Cm.abs().sum(dim=1).max() + rho)).item()


def test_eigh_route_stays_inside_eps_abs():
    """The condition behind the committed constant, one the reference's arithmetic alone has to satisfy: over the whole family the
    oracle's eigh route stays within EIGH_ROUTE_EPS_ABS (= 4 x the worst case measured when the constant was written) of the
    identity, relative to ||C||_inf + rho."""
    from modegpt_amd.compression import compress_qk as cq
    assert cq.EIGH_ROUTE_EPS_ABS == cq.EIGH_ROUTE_SAFETY * cq.EIGH_ROUTE_MEASURED_ULPS * 2.0 ** -53 and cq.EIGH_ROUTE_SAFETY == 4
    worst, where, count = 0.0, None, 0
    for name, Cm, rho in eigh_route_family():
        e = eigh_route_error(Cm, rho)
        count += 1
        if e > worst:
            worst, where = e, name
    print(f"eigh route vs identity: worst {worst * 2.0 ** 53:.2f} x 2^-53 at {where} over {count} matrices; "
          f"committed {cq.EIGH_ROUTE_MEASURED_ULPS} x 2^-53 (x {cq.EIGH_ROUTE_SAFETY})")
    assert count >= 96 + 2 * len(CASES)
    assert 0 < worst <= cq.EIGH_ROUTE_EPS_ABS, (worst, where)


# ---------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("mode,n_heads,n_kv", [(ROPE_GROUPED, 8, 2), (ROPE_MHA, 3, 3), (OPT, 3, 3)])
def test_interval_rule_restatement(mode, n_heads, n_kv):
    """On a 1 % ladder the restated rule certifies set and order and its centre scores rank as the oracle's eigh route does; with
    the two units at the threshold 2e-13 apart that head -- and only that head -- is flagged."""
    from modegpt_amd.compression.compress_qk import EIGH_ROUTE_EPS_ABS
    hd, rank, eps_rel = 64, 44, 1.2e-11
    take = rank if mode == OPT else rank // 2
    gen = torch.Generator().manual_seed(11 + mode)
    ridge_k = 1e-2 if mode == ROPE_GROUPED else 1e-4
    cov_q, cov_k, perms = ladder_heads(n_heads, n_kv, hd, mode, gen, ridge_k)
    arch = "opt" if mode == OPT else "llama"
    W = torch.zeros(n_heads * hd, 8), torch.zeros(n_kv * hd, 8)
    _, mask = O.compress_qk_layer(W[0], W[1], cov_q, cov_k, n_heads, n_kv, hd, rank, arch, ridge_k)
    for h in range(n_kv):
        assert torch.equal(mask[h, :take], perms[h][:take])
    rows = qk_margin_host(cov_q, cov_k, rank, mode, 1e-4, ridge_k, mask, eps_rel, EIGH_ROUTE_EPS_ABS)
    assert bool((rows[:, 7] == 1).all()) and bool((rows[:, 6] == 0).all()) and bool((rows[:, 5] == 0).all())
    assert bool((rows[:, 4] < 1e-10).all()) and bool(((rows[:, 0] - rows[:, 1]) / rows[:, 0] > 5e-3).all())
    # near-tie in head 1: the unit just below the threshold moved to 2e-13 under the one just above it
    a, b = perms[1][take - 1].item(), perms[1][take].item()
    for j in ((b,) if mode == OPT else (b, b + hd // 2)):
        cov_k[1, j, j] = (cov_k[1, a, a] + ridge_k) * (1 - 2e-13 if mode == ROPE_MHA else 1 - 4e-13) - ridge_k
    rows = qk_margin_host(cov_q, cov_k, rank, mode, 1e-4, ridge_k, mask, eps_rel, EIGH_ROUTE_EPS_ABS)
    assert rows[1, 7] == 0 and rows[1, 5] >= 2 and 0 < (rows[1, 0] - rows[1, 1]) / rows[1, 0] < 1e-12
    assert rows[0, 7] == 1 and rows[2 if n_kv > 2 else 0, 7] == 1


# ---------------------------------------------------------------- decode + report on hand-made numbers
def _qk_row(s_sel, s_unsel, half, at_risk, order, certified):
    return [s_sel, s_unsel, s_sel * (1 - half), s_unsel * (1 + half) if s_unsel > -INF else -INF, half, at_risk, order, certified]


def test_decode_and_report_attention_margins(caplog):
    from modegpt_amd import engine, ops
    eps_rel, eps_abs = 1.2e-11, 2e-14
    good = [_qk_row(2.0, 2.0 * (1 - 1e-2), 3e-11, 0., 0., 1.), _qk_row(3.0, 3.0 * (1 - 2e-2), 3e-11, 0., 1., 1.)]
    tied = [_qk_row(2.0, 2.0 * (1 - 1e-2), 3e-11, 0., 0., 1.), _qk_row(5.0, 5.0 * (1 - 2e-13), 3e-11, 2., 1., 0.)]
    m = ops.decode_qk_margin(good, eps_rel, eps_abs)
    assert m["certified"] and not m["order_certified"] and m["weakest_head"] == 0 and abs(m["margin"] - 1e-2) < 1e-15
    assert m["heads"][0]["order_certified"] and not m["heads"][1]["order_certified"] and m["heads"][1]["order_at_risk"] == 1
    assert set(m["heads"][0]) >= {"margin", "score_halfwidth", "units_at_risk", "order_at_risk", "certified", "order_certified"}
    m = ops.decode_qk_margin(tied, eps_rel, eps_abs)
    assert not m["certified"] and m["weakest_head"] == 1 and 0 < m["margin"] < 1e-12 and m["score_halfwidth"] == 3e-11
    assert m["heads"][0]["certified"] and m["heads"][1]["units_at_risk"] == 2
    full = ops.decode_qk_margin([_qk_row(2.0, -INF, 3e-11, 0., 0., 1.)], eps_rel, eps_abs)          # rank == number of units
    assert full["certified"] and full["margin"] == INF
    nan = float("nan")
    sep = [[4.0, 1.0, 0.5, 0.9, 1e-9, 1.0, 9.0, 0.1], [4.0, 3.0, 1 - math.sqrt(0.75), 0.8, 1e-9, 1.0, 9.0, 0.1]]
    close = [[4.0, 1.0, 0.5, 0.9, 1e-9, 1.0, 9.0, 0.1], [4.0, 4.0 - 1e-12, 1.25e-13, 0.8, 1e-9, 0.0, 9.0, 0.1]]
    mha = [[4.0, 1.0, 0.5, 0.9, nan, nan, 9.0, 0.1]]
    v = ops.decode_vo_spectrum(sep, 1.2e-11)
    assert v["separated"] is True and v["weakest_head"] == 1 and abs(v["gap"] - (1 - math.sqrt(0.75))) < 1e-15 and v["energy_min"] == 0.8
    assert v["heads"][0]["lambda_r"] == 4.0 and v["heads"][0]["lambda_next"] == 1.0 and v["heads"][0]["lambda_max"] == 9.0
    v = ops.decode_vo_spectrum(close, 1.2e-11)
    assert v["separated"] is False and v["heads"][0]["separated"] is True and v["heads"][1]["separated"] is False
    v = ops.decode_vo_spectrum(mha, 1.2e-11)
    assert v["separated"] is None and v["heads"][0]["bound"] is None and v["gap"] == 0.5

    ad = engine.TensorAdapter(dict(engine.SHAPES["tiny"]), {})
    t = lambda rows: torch.tensor(rows, dtype=F64)                                              # noqa: E731
    mlp8 = torch.tensor([2.0, 2.0 * (1 + 1e-6), 2.0 + 1e-9, 2.0 * (1 + 1e-6) - 1e-9, 40., 60., 0., 1.], dtype=F64)
    ad.selection_margin(3, mlp8, 1.1e-11)
    ad.attention_margin(0, "qk", t(good), eps_rel, eps_abs)
    ad.attention_margin(5, "qk", t(tied), eps_rel, eps_abs)
    ad.attention_margin(0, "vo", t(sep), 1.2e-11)
    ad.attention_margin(5, "vo", t(close), 1.2e-11)
    ad.attention_margin(6, "vo", t(mha), 1.2e-11)
    with pytest.raises(ValueError):
        ad.attention_margin(0, "mlp", t(good), eps_rel)
    # the MLP report neither reads nor disturbs the pending attention records, and keeps its return value
    with caplog.at_level(logging.WARNING, logger="MoDeGPT"):
        caplog.clear()
        rep = ad.report_selection_margins()
        assert set(rep) == {3} and set(rep[3]) == {"margin", "score_bound", "eps", "eps_certifiable", "scores_at_risk", "certified"}
        assert rep[3]["certified"] and not caplog.records
        assert set(ad.metrics) == {"mlp_selection"} and set(ad.metrics["mlp_selection"]) == {"3"}
        mlp_before = dict(ad.metrics["mlp_selection"]["3"])
        rep = ad.report_attention_margins()
    msgs = [r.getMessage() for r in caplog.records]
    assert len(msgs) == 2, msgs
    assert "[QK] Layer 5" in msgs[0] and "NOT certified" in msgs[0] and "kv head 1" in msgs[0] and f"{rep['qk'][5]['margin']:.3e}" in msgs[0] \
        and "3.000e-11" in msgs[0]
    assert "[VO] Layer 5" in msgs[1] and "NOT separated" in msgs[1] and "kv head 1" in msgs[1]
    assert set(rep) == {"qk", "vo"} and set(rep["qk"]) == {0, 5} and set(rep["vo"]) == {0, 5, 6}
    assert rep["qk"][0]["certified"] and not rep["qk"][5]["certified"] and rep["vo"][6]["separated"] is None
    assert set(ad.metrics["qk_selection"]) == {"0", "5"} and set(ad.metrics["vo_spectrum"]) == {"0", "5", "6"}
    assert ad.metrics["qk_selection"]["5"]["certified"] is False and ad.metrics["qk_selection"]["5"]["weakest_head"] == 1
    assert ad.metrics["vo_spectrum"]["5"]["separated"] is False and ad.metrics["vo_spectrum"]["0"]["separated"] is True
    assert ad.metrics["mlp_selection"] == {"3": mlp_before}
    assert ad.report_attention_margins() == {"qk": {}, "vo": {}}                                # (read once)
    assert ad.report_selection_margins() == {}
    import json
    json.dumps(ad.metrics)                                                                      # (the metrics file stays writable)


def test_attention_error_eps():
    from modegpt_amd import engine, ops
    from modegpt_amd.compression.compress_qk import attention_error_eps
    ad = engine.TensorAdapter(dict(engine.SHAPES["tiny"]), {})
    ad.cov_error_eps = 5e-12
    assert attention_error_eps(ad) == 5e-12
    ad.cov_error_eps = None
    ad.calib_tokens = 1 << 10
    i8 = 1.1e-11 + 64 * 2.0 ** -53
    assert attention_error_eps(ad) == i8                                # few tokens: the int8 guarantee is the larger
    ad.calib_tokens = 1 << 22
    assert attention_error_eps(ad) == ((1 << 22) / 4 + 4) * 2.0 ** -53 > i8
    with ops.i8_tolerance_scope(64.0):
        assert attention_error_eps(ad) == 64 * 1.1e-11 + 64 * 2.0 ** -53
