"""GPU: the certificates of the attention half -- mdg_qk_select_margin (is the rotary-pair selection determined, given the error
bound of the covariance route and the rounding of the reference's eigh route?) and mdg_vo_spectrum (sigma_r against sigma_r+1 of
the spectrum compress_vo truncated) -- from the kernels up to ModelAdapter.report_attention_margins."""
import logging
import math

import pytest
import torch

from oracle import modegpt_oracle as O
from tests.golden_util import CASES, Case
from tests.test_attn_certificate_host import OPT, ROPE_GROUPED, ROPE_MHA, ladder_heads, qk_margin_host

pytestmark = pytest.mark.gpu
F64 = torch.float64
ULPS = 8 * 2.0 ** -52          # "a few ulps": the kernel contracts a*b + c*d into an fma and orders the row sums differently
MODES = [(ROPE_GROUPED, "llama", 8, 2), (ROPE_MHA, "llama", 3, 3), (OPT, "opt", 3, 3)]
HD, RANK, KEEP = 64, 44, 0.7   # int(64 * 0.7) = 44 (even)
EPS_REL = 1.1e-11 + 64 * 2.0 ** -53


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def _shape(arch, n_heads, n_kv, hd=HD, d=128):
    return dict(arch=arch, n_layers=1, d=d, d_ff=256, n_heads=n_heads, n_kv_heads=n_kv, head_dim=hd)


def _ridge_k(mode):
    from modegpt_amd import engine
    return engine.RECIPE_RIDGES["ridge_qk"] if mode == ROPE_GROUPED else 1e-4


def _oracle_scores(mode, cov_q, cov_k, h, ridge_k):
    g = cov_q.shape[0] // cov_k.shape[0]
    if mode == OPT:
        return O.qk_scores_opt(cov_q[h], cov_k[h])
    return O.qk_scores_rope([cov_q[j] for j in range(h * g, (h + 1) * g)], cov_k[h], ridge_k=ridge_k, ridge_q=1e-4,
                            take_sqrt=mode == ROPE_GROUPED)


def _oracle_order(mode, cov_q, cov_k, h, ridge_k, take):
    return torch.topk(_oracle_scores(mode, cov_q, cov_k, h, ridge_k), k=take).indices


def _run_driver(arch, n_heads, n_kv, cov_q, cov_k, dev, caplog, adapter_cls=None):
    from modegpt_amd import engine
    from modegpt_amd.compression.compress_qk import compress_qk
    shape = _shape(arch, n_heads, n_kv)
    weights = engine.make_layer_weights(shape, 3, dev)
    adapter = (adapter_cls or engine.TensorAdapter)(shape, {0: weights})
    adapter.cov_error_eps = EPS_REL
    masks = compress_qk(adapter=adapter, cov=([cov_q.to(dev)], [cov_k.to(dev)]), keep_ratios=[KEEP], target_layers=[0])
    with caplog.at_level(logging.WARNING, logger="MoDeGPT"):
        caplog.clear()
        report = getattr(adapter, "report_attention_margins", None)
        rep = report() if report is not None else None
    return adapter, weights, masks, rep, [r.getMessage() for r in caplog.records]


def _check_fields(got, want):
    got, want = got.cpu(), want.cpu()
    for i in range(4):
        assert bool(((got[:, i] - want[:, i]).abs() <= ULPS * want[:, i].abs()).all()), (i, got[:, i], want[:, i])
    # [4] is a difference of two scores over the score: a few ulps OF THE SCORE, i.e. absolute
    assert bool(((got[:, 4] - want[:, 4]).abs() <= ULPS).all()), (got[:, 4], want[:, 4])
    assert torch.equal(got[:, 5:], want[:, 5:]), (got[:, 5:], want[:, 5:])


@pytest.mark.parametrize("mode,arch,n_heads,n_kv", MODES)
def test_qk_certified(ops, dev, caplog, mode, arch, n_heads, n_kv):
    """1. Neighbouring pair scores 1 % apart: every head certified, order too, no warning; margin as the oracle's eigh route gives it;
    all 8 numbers as the host restatement; mask as the reference's."""
    from modegpt_amd.compression.compress_qk import EIGH_ROUTE_EPS_ABS
    ridge_k, take = _ridge_k(mode), (RANK if mode == OPT else RANK // 2)
    cov_q, cov_k, _ = ladder_heads(n_heads, n_kv, HD, mode, torch.Generator().manual_seed(21 + mode), ridge_k)
    adapter, weights, masks, rep, warnings = _run_driver(arch, n_heads, n_kv, cov_q, cov_k, dev, caplog)
    m = rep["qk"][0]
    print(f"mode {mode}: margins {[h['margin'] for h in m['heads']]} half-widths {[h['score_halfwidth'] for h in m['heads']]}")
    assert m["certified"] and m["order_certified"] and not warnings and adapter.metrics["qk_selection"]["0"]["certified"] is True
    for h, head in enumerate(m["heads"]):
        assert head["certified"] and head["order_at_risk"] == 0 and head["units_at_risk"] == 0
        srt = torch.sort(_oracle_scores(mode, cov_q, cov_k, h, ridge_k), descending=True).values
        assert abs(head["margin"] - ((srt[take - 1] - srt[take]) / srt[take - 1]).item()) < 1e-9
    W = weights["q"].cpu(), weights["k"].cpu()
    ref, ref_mask = O.compress_qk_layer(W[0], W[1], cov_q, cov_k, n_heads, n_kv, HD, RANK, arch, ridge_k)
    mask, _, _ = ops.qk_select(cov_q.to(dev), cov_k.to(dev), RANK, mode, 1e-4, ridge_k)
    assert torch.equal(mask.cpu(), ref_mask) and torch.equal(adapter.store[(0, "qk")]["q_proj"].cpu(), ref["q_proj"])
    if arch != "opt":
        assert torch.equal(masks[0].cpu(), ref_mask)
    got = ops.qk_select_margin(cov_q.to(dev), cov_k.to(dev), RANK, mode, 1e-4, ridge_k, mask, EPS_REL, EIGH_ROUTE_EPS_ABS)
    _check_fields(got, qk_margin_host(cov_q, cov_k, RANK, mode, 1e-4, ridge_k, mask, EPS_REL, EIGH_ROUTE_EPS_ABS))


@pytest.mark.parametrize("mode,arch,n_heads,n_kv", MODES)
def test_qk_flagged(ops, dev, caplog, mode, arch, n_heads, n_kv):
    """2. The two units at the threshold of kv head 1 moved 2e-13 apart: that head alone is flagged, one warning names layer and
    head, the metrics say so, and the artefact is still written with the selection qk_select made."""
    from modegpt_amd.compression.compress_qk import EIGH_ROUTE_EPS_ABS
    ridge_k, take = _ridge_k(mode), (RANK if mode == OPT else RANK // 2)
    cov_q, cov_k, perms = ladder_heads(n_heads, n_kv, HD, mode, torch.Generator().manual_seed(21 + mode), ridge_k)
    a, b = perms[1][take - 1].item(), perms[1][take].item()
    for j in ((b,) if mode == OPT else (b, b + HD // 2)):       # scores 2e-13 apart (sqrt halves a relative step of the squared norm)
        cov_k[1, j, j] = (cov_k[1, a, a] + ridge_k) * (1 - (2e-13 if mode == ROPE_MHA else 4e-13)) - ridge_k
    adapter, weights, masks, rep, warnings = _run_driver(arch, n_heads, n_kv, cov_q, cov_k, dev, caplog)
    m = rep["qk"][0]
    print(f"mode {mode}: head 1 margin {m['heads'][1]['margin']:.3e} half-width {m['heads'][1]['score_halfwidth']:.3e} "
          f"units at risk {m['heads'][1]['units_at_risk']}; warning: {warnings}")
    assert not m["certified"] and m["weakest_head"] == 1 and not m["heads"][1]["certified"] and m["heads"][1]["units_at_risk"] >= 2
    assert 0 < m["heads"][1]["margin"] < 1e-12
    assert all(h["certified"] for i, h in enumerate(m["heads"]) if i != 1)
    assert len(warnings) == 1 and "Layer 0" in warnings[0] and "kv head 1" in warnings[0] and "NOT certified" in warnings[0]
    stored = adapter.metrics["qk_selection"]["0"]
    assert stored["certified"] is False and stored["heads"][1]["certified"] is False and stored["heads"][0]["certified"] is True
    mask, q_rows, k_rows = ops.qk_select(cov_q.to(dev), cov_k.to(dev), RANK, mode, 1e-4, ridge_k)
    art = adapter.store[(0, "qk")]
    assert torch.equal(art["q_proj"], weights["q"][q_rows]) and torch.equal(art["k_proj"], weights["k"][k_rows])
    assert art["q_proj"].shape[0] == n_heads * RANK
    got = ops.qk_select_margin(cov_q.to(dev), cov_k.to(dev), RANK, mode, 1e-4, ridge_k, mask, EPS_REL, EIGH_ROUTE_EPS_ABS)
    _check_fields(got, qk_margin_host(cov_q, cov_k, RANK, mode, 1e-4, ridge_k, mask, EPS_REL, EIGH_ROUTE_EPS_ABS))


def _random_heads(n_heads, n_kv, hd, gen):
    """sigma = X^T X / T of activations with per-column scales log-uniform over two decades (engine.make_activation_batch's law)."""
    def cov(n):
        X = torch.randn(n, 4 * hd, hd, generator=gen, dtype=F64)
        X = X * torch.exp(torch.empty(n, 1, hd, dtype=F64).uniform_(math.log(0.02), math.log(2.0), generator=gen))
        return X.transpose(1, 2) @ X / (4 * hd)
    return cov(n_heads), cov(n_kv)


def _identity_vs_eigh(ops, dev, mode, cov_q, cov_k, rank, ridge_k, what, eps_rel=0.0):
    """Wherever the certificate says certified, the oracle's pair set equals the engine's; where it also says the order is
    certified, the order too.  eps_rel = 0 (the default here): both sides read the SAME sigma, so the certificate is taken against
    the eigh route's rounding alone -- the sharpest form of the claim; every eps_rel > 0 certifies a subset of these heads."""
    from modegpt_amd.compression.compress_qk import EIGH_ROUTE_EPS_ABS
    take = rank if mode == OPT else rank // 2
    mask, _, _ = ops.qk_select(cov_q.to(dev), cov_k.to(dev), rank, mode, 1e-4, ridge_k)
    rows = ops.qk_select_margin(cov_q.to(dev), cov_k.to(dev), rank, mode, 1e-4, ridge_k, mask, eps_rel, EIGH_ROUTE_EPS_ABS).cpu()
    mask = mask.cpu()
    certified = ordered = same_set = 0
    for h in range(cov_k.shape[0]):
        want = _oracle_order(mode, cov_q, cov_k, h, ridge_k, take)
        equal_set = set(want.tolist()) == set(mask[h, :take].tolist())
        same_set += equal_set
        if rows[h, 7] == 1.0:
            certified += 1
            assert equal_set, (what, h, rows[h])
            if rows[h, 6] == 0.0:
                ordered += 1
                assert torch.equal(want, mask[h, :take]), (what, h, rows[h])
    print(f"{what}: {cov_k.shape[0]} heads, {certified} certified ({ordered} with their order), {same_set} with the oracle's set; "
          f"smallest margin {((rows[:, 0] - rows[:, 1]) / rows[:, 0]).min().item():.3e}, largest half-width {rows[:, 4].max().item():.3e}")
    return certified, rows, mask


def test_identity_against_the_eigh_route(ops, dev):
    """3. Goldens, the 1 % ladder, 201 seeded random heads; and pairs 1e-13 apart, which must NOT be certified (which side the
    oracle's eigh route lands on is printed, not asserted)."""
    from modegpt_amd.compression.compress_qk import qk_mode_and_ridges
    for name in CASES:
        c = Case(name)
        mode, ridge_q, ridge_k = qk_mode_and_ridges(c.arch, c.n_kv != c.n_h, c.ridges["ridge_qk"])
        _, _, mask = _identity_vs_eigh(ops, dev, mode, c.f64["sigma_q"], c.f64["sigma_k"], c.qk_rank, ridge_k, f"golden {name}")
        assert torch.equal(mask, c.qk_mask)
    for mode, arch, n_heads, n_kv in MODES:
        ridge_k = _ridge_k(mode)
        cov_q, cov_k, _ = ladder_heads(n_heads, n_kv, HD, mode, torch.Generator().manual_seed(31 + mode), ridge_k)
        certified, _, _ = _identity_vs_eigh(ops, dev, mode, cov_q, cov_k, RANK, ridge_k, f"ladder mode {mode}")
        assert certified == n_kv
        n = 67
        cov_q, cov_k = _random_heads(n * (2 if mode == ROPE_GROUPED else 1), n, HD, torch.Generator().manual_seed(41 + mode))
        certified, _, _ = _identity_vs_eigh(ops, dev, mode, cov_q, cov_k, RANK, ridge_k, f"random mode {mode}")
        # not vacuous: 32 (64) scores spread over decades have neighbouring gaps of the order 1e-2, the half-width against the eigh
        # route is eps_abs ||C||_inf / C_jj <= 1.8e-14 * 64 * 1e4 ~ 1e-8 -- all but a rare head must come out certified
        assert certified > n // 2
        # pairs 1e-13 apart at the threshold of every head
        cov_q, cov_k, perms = ladder_heads(n_heads, n_kv, HD, mode, torch.Generator().manual_seed(51 + mode), ridge_k)
        take = RANK if mode == OPT else RANK // 2
        for h in range(n_kv):
            a, b = perms[h][take - 1].item(), perms[h][take].item()
            for j in ((b,) if mode == OPT else (b, b + HD // 2)):
                cov_k[h, j, j] = (cov_k[h, a, a] + ridge_k) * (1 - (1e-13 if mode == ROPE_MHA else 2e-13)) - ridge_k
        _identity_vs_eigh(ops, dev, mode, cov_q, cov_k, RANK, ridge_k, f"1e-13 ties mode {mode}, against the eigh route alone")
        certified, rows, mask = _identity_vs_eigh(ops, dev, mode, cov_q, cov_k, RANK, ridge_k, f"1e-13 ties mode {mode}", eps_rel=EPS_REL)
        assert certified == 0 and bool((rows[:, 5] >= 2).all())
        for h in range(n_kv):
            a, b = perms[h][take - 1].item(), perms[h][take].item()
            want = set(_oracle_order(mode, cov_q, cov_k, h, ridge_k, take).tolist())
            got = set(mask[h, :take].tolist())
            print(f"  tie mode {mode} head {h}: the larger diagonal is unit {a}; identity keeps {'a' if a in got else 'b'}, "
                  f"eigh route keeps {'a' if a in want else 'b'}{' and b' if a in want and b in want else ''}")
            assert a in got and b not in got          # the identity route sees the exact diagonal: the larger one wins


@pytest.mark.parametrize("mode,arch,n_heads,n_kv", MODES)
def test_bound_is_sound_and_not_vacuous(ops, dev, mode, arch, n_heads, n_kv):
    """4. Every diagonal moved by (just under) eps_rel in the worst direction -- selected units down, unselected up: a certified
    head's selected set never changes; a near-tie inside the bound is flagged and does change."""
    eps_rel, ridge_k = 1e-6, _ridge_k(mode)
    take, half = (RANK if mode == OPT else RANK // 2), HD // 2
    n = 40
    g = 2 if mode == ROPE_GROUPED else 1
    cov_q, cov_k = _random_heads(n * g, n, HD, torch.Generator().manual_seed(61 + mode))
    lq, lk, perms = ladder_heads(2 * g, 2, HD, mode, torch.Generator().manual_seed(71 + mode), ridge_k)
    a, b = perms[1][take - 1].item(), perms[1][take].item()
    for j in ((b,) if mode == OPT else (b, b + half)):                      # scores 1e-7 apart: inside what eps_rel = 1e-6 can move
        lk[1, j, j] = (lk[1, a, a] + ridge_k) * (1 - (1e-7 if mode == ROPE_MHA else 2e-7)) - ridge_k
    cov_q, cov_k = torch.cat((cov_q, lq)), torch.cat((cov_k, lk))           # heads n (ladder, certified) and n + 1 (near-tie)
    mask, _, _ = ops.qk_select(cov_q.to(dev), cov_k.to(dev), RANK, mode, 1e-4, ridge_k)
    rows = ops.qk_select_margin(cov_q.to(dev), cov_k.to(dev), RANK, mode, 1e-4, ridge_k, mask, eps_rel, 0.0).cpu()
    mask = mask.cpu()
    pq, pk = cov_q.clone(), cov_k.clone()
    for h in range(n + 2):
        sel = torch.zeros(HD if mode == OPT else half, dtype=torch.bool)
        sel[mask[h, :take]] = True
        sign = torch.where(sel, -1.0, 1.0).to(F64)
        sign = sign if mode == OPT else torch.cat((sign, sign))
        for Cm in [pk[h]] + [pq[q] for q in range(h * g, (h + 1) * g)]:
            d = torch.diagonal(Cm)
            d += 0.999 * eps_rel * sign * d.abs()
    moved, _, _ = ops.qk_select(pq.to(dev), pk.to(dev), RANK, mode, 1e-4, ridge_k)
    moved = moved.cpu()
    changed = [set(moved[h, :take].tolist()) != set(mask[h, :take].tolist()) for h in range(n + 2)]
    print(f"mode {mode}: {int(rows[:, 7].sum())} of {n + 2} heads certified at eps_rel = {eps_rel:g}; {sum(changed)} selections changed "
          f"under the worst-direction perturbation")
    for h in range(n + 2):
        assert not (rows[h, 7] == 1.0 and changed[h]), (h, rows[h])
    assert rows[n, 7] == 1.0 and not changed[n]
    assert rows[n + 1, 7] == 0.0 and changed[n + 1]


def _vo_problem(n_heads, n_kv, hd, d, gen, tie=None, rank=RANK):
    """sigma_x = c I and W_v,h = diag(sv) Q_h with orthonormal rows Q_h: the Gram matrix is (c + rho) diag(sv^2) in closed form.
    sv: a 1 % ladder from 1 downwards (shuffled over the rows); tie: sigma_r+1 = sigma_r (1 - tie) in kv head 1."""
    c = 0.25
    Wv, svs = [], []
    for h in range(n_kv):
        Q, _ = torch.linalg.qr(torch.randn(d, hd, generator=gen, dtype=F64))
        sv = 1.01 ** (-torch.arange(hd, dtype=F64))
        if tie is not None and h == 1:
            sv[rank] = sv[rank - 1] * (1 - tie)
        sv = sv[torch.randperm(hd, generator=gen)]
        Wv.append(sv[:, None] * Q.T)
        svs.append(torch.sort(sv, descending=True).values)
    Wo = torch.randn(d, n_heads * hd, generator=gen, dtype=F64) * 0.02
    return c * torch.eye(d, dtype=F64), torch.cat(Wv), Wo, torch.stack(svs), c


def _run_vo(n_heads, n_kv, Cx, Wv, Wo, dev, caplog, adapter_cls=None):
    from modegpt_amd import engine
    from modegpt_amd.compression.compress_vo import compress_vo
    shape = _shape("llama", n_heads, n_kv, d=Cx.shape[0])
    adapter = (adapter_cls or engine.TensorAdapter)(shape, {0: {"v": Wv.to(dev), "o": Wo.to(dev)}})
    adapter.cov_error_eps = EPS_REL
    compress_vo(adapter=adapter, cov=[Cx.to(dev)], keep_ratios=[KEEP], target_layers=[0])
    adapter.check_chains()
    with caplog.at_level(logging.WARNING, logger="MoDeGPT"):
        caplog.clear()
        report = getattr(adapter, "report_attention_margins", None)
        rep = report() if report is not None else None
    return adapter, rep, [r.getMessage() for r in caplog.records]


def test_vo_spectrum(ops, dev, caplog):
    """5. Closed-form spectrum: lambda_r, lambda_r+1, gap, energy, lambda_1, lambda_hd; the Weyl bound against a torch restatement;
    separated.  Then sigma_r and sigma_r+1 of one head 1e-13 apart: not separated, warning, factors the bits of the plain call.
    MHA variant: the gap of the second spectrum, no bound."""
    from modegpt_amd import engine
    n_heads, n_kv, d, rho = 4, 2, 256, engine.RECIPE_RIDGES["ridge_vo"]
    # lambda: relative to lambda_1, the eigensolver's own tolerance in test_syevj (1e-13) times hd for the Gram product
    TOL = 1e-13 * HD
    for tie in (None, 1e-13):
        Cx, Wv, Wo, sv, c = _vo_problem(n_heads, n_kv, HD, d, torch.Generator().manual_seed(81), tie=tie)
        lam = (c + rho) * sv ** 2                                                                   # [n_kv, hd] descending
        adapter, rep, warnings = _run_vo(n_heads, n_kv, Cx, Wv, Wo, dev, caplog)
        m = rep["vo"][0]
        plain_v, plain_o = ops.vo_compress(Cx.to(dev), Wv.to(dev), Wo.to(dev), n_heads, n_kv, HD, RANK, rho)
        v, o, rows = ops.vo_compress(Cx.to(dev), Wv.to(dev), Wo.to(dev), n_heads, n_kv, HD, RANK, rho, want_spectrum=True,
                                     spectrum_eps=EPS_REL)
        art = adapter.store[(0, "vo")]
        assert torch.equal(v, plain_v) and torch.equal(o, plain_o)
        assert torch.equal(art["v_proj"], plain_v) and torch.equal(art["o_proj"], plain_o)
        rows = rows.cpu()
        bound = EPS_REL * ((Wv.abs() @ torch.sqrt(torch.diagonal(Cx))) ** 2).reshape(n_kv, HD).sum(dim=1)
        for h in range(n_kv):
            l1 = lam[h, 0].item()
            err = [abs(rows[h, 0] - lam[h, RANK - 1]).item() / l1, abs(rows[h, 1] - lam[h, RANK]).item() / l1,
                   abs(rows[h, 6] - lam[h, 0]).item() / l1, abs(rows[h, 7] - lam[h, -1]).item() / l1]
            gap = ((sv[h, RANK - 1] - sv[h, RANK]) / sv[h, RANK - 1]).item()
            energy = (lam[h, :RANK].sum() / lam[h].sum()).item()
            print(f"tie {tie} head {h}: lambda errors / lambda_1 {err}; gap {rows[h, 2].item():.6e} (closed form {gap:.6e}); energy "
                  f"{rows[h, 3].item():.12f} ({energy:.12f}); bound {rows[h, 4].item():.3e} ({bound[h].item():.3e}); separated {rows[h, 5].item()}")
            assert max(err) <= TOL
            # d(gap) <= (|d lambda_r| + |d lambda_r+1|) / (2 lambda_r); the energy is a ratio of sums of hd eigenvalues each within TOL lambda_1
            assert abs(rows[h, 2].item() - gap) <= TOL * l1 / lam[h, RANK - 1].item()
            assert abs(rows[h, 3].item() - energy) <= 2 * HD * TOL * l1 / lam[h].sum().item()
            assert abs(rows[h, 4].item() - bound[h].item()) <= 1e-12 * bound[h].item()
            want_sep = not (tie is not None and h == 1)
            assert rows[h, 5].item() == (1.0 if want_sep else 0.0)
            assert m["heads"][h]["separated"] is want_sep and abs(m["heads"][h]["gap"] - rows[h, 2].item()) == 0
        if tie is None:
            assert m["separated"] is True and not warnings and adapter.metrics["vo_spectrum"]["0"]["separated"] is True
        else:
            assert m["separated"] is False and adapter.metrics["vo_spectrum"]["0"]["separated"] is False
            assert len(warnings) == 1 and "[VO] Layer 0" in warnings[0] and "kv head 1" in warnings[0] and "NOT separated" in warnings[0]
    # the two-SVD MHA variant: sigma' = svdvals(diag(S) Vh W_o,h^T) (compress_vo.py:187-194)
    Cx, Wv, Wo, sv, c = _vo_problem(2, 2, HD, d, torch.Generator().manual_seed(82))
    adapter, rep, warnings = _run_vo(2, 2, Cx, Wv, Wo, dev, caplog)
    m = rep["vo"][0]
    _, _, rows = ops.vo_compress(Cx.to(dev), Wv.to(dev), Wo.to(dev), 2, 2, HD, RANK, rho, want_spectrum=True, spectrum_eps=EPS_REL)
    rows = rows.cpu()
    assert m["separated"] is None and not warnings and bool(torch.isnan(rows[:, 4:6]).all())
    for h in range(2):
        A = math.sqrt(c + rho) * Wv[h * HD:(h + 1) * HD].T
        _, S, Vh = torch.linalg.svd(A, full_matrices=False)
        lam2 = torch.linalg.svdvals(torch.diag(S) @ Vh @ Wo[:, h * HD:(h + 1) * HD].T) ** 2
        err = [abs(rows[h, 0] - lam2[RANK - 1]).item() / lam2[0].item(), abs(rows[h, 1] - lam2[RANK]).item() / lam2[0].item(),
               abs(rows[h, 6] - lam2[0]).item() / lam2[0].item(), abs(rows[h, 7] - lam2[-1]).item() / lam2[0].item()]
        gap = ((lam2[RANK - 1].sqrt() - lam2[RANK].sqrt()) / lam2[RANK - 1].sqrt()).item()
        print(f"MHA head {h}: lambda errors / lambda_1 {err}; gap {rows[h, 2].item():.6e} (svd {gap:.6e}); energy {rows[h, 3].item():.6f}")
        assert max(err) <= TOL and abs(rows[h, 2].item() - gap) <= TOL * lam2[0].item() / lam2[RANK - 1].item()
        assert m["heads"][h]["bound"] is None and m["heads"][h]["separated"] is None and m["heads"][h]["gap"] == rows[h, 2].item()


def test_nothing_moved(ops, dev, caplog):
    """6. qk_select / vo_compress outputs are the same bits with and without the certificate calls on every golden case, and the
    drivers run as before on an adapter without `attention_margin`."""
    from modegpt_amd import engine
    from modegpt_amd.compression.compress_qk import EIGH_ROUTE_EPS_ABS, qk_mode_and_ridges

    class Plain(engine.TensorAdapter):
        attention_margin = None                 # (what a duck-typed adapter written against the reference's ABC looks like)
        report_attention_margins = None

    for name in CASES:
        c = Case(name)
        mode, ridge_q, ridge_k = qk_mode_and_ridges(c.arch, c.n_kv != c.n_h, c.ridges["ridge_qk"])
        cq, ck = c.f64["sigma_q"].to(dev), c.f64["sigma_k"].to(dev)
        before = ops.qk_select(cq, ck, c.qk_rank, mode, ridge_q, ridge_k)
        ops.qk_select_margin(cq, ck, c.qk_rank, mode, ridge_q, ridge_k, before[0], EPS_REL, EIGH_ROUTE_EPS_ABS)
        after = ops.qk_select(cq, ck, c.qk_rank, mode, ridge_q, ridge_k)
        assert all(torch.equal(x, y) for x, y in zip(before, after)) and torch.equal(before[0].cpu(), c.qk_mask)
        args = (c.f64["sigma_x"].to(dev), c.W["v"].to(dev), c.W["o"].to(dev), c.n_h, c.n_kv, c.hd, c.vo_rank, c.ridges["ridge_vo"])
        plain = ops.vo_compress(*args, want_f64=True)
        with_spectrum = ops.vo_compress(*args, want_f64=True, want_spectrum=True, spectrum_eps=EPS_REL)
        assert len(plain) == 4 and len(with_spectrum) == 5 and tuple(with_spectrum[4].shape) == (c.n_kv, 8)
        assert all(torch.equal(x, y) for x, y in zip(plain, with_spectrum[:4]))
        rows = with_spectrum[4].cpu()
        print(f"golden {name}: VO spectrum rows {rows.tolist()}")
        if c.n_kv != c.n_h:          # bf16 weights (eight per load): the Weyl bound against the torch restatement
            want = EPS_REL * ((c.W["v"].double().abs() @ torch.sqrt(torch.diagonal(c.f64["sigma_x"]))) ** 2).reshape(c.n_kv, c.hd).sum(dim=1)
            assert bool(((rows[:, 4] - want).abs() <= 1e-12 * want).all()), (rows[:, 4], want)
        else:
            assert bool(torch.isnan(rows[:, 4:6]).all())
        assert bool((rows[:, 6] >= rows[:, 0]).all() and (rows[:, 0] >= rows[:, 1]).all() and (rows[:, 1] >= rows[:, 7]).all())
    mode, arch, n_heads, n_kv = MODES[0]
    cov_q, cov_k, _ = ladder_heads(n_heads, n_kv, HD, mode, torch.Generator().manual_seed(91), _ridge_k(mode))
    full = _run_driver(arch, n_heads, n_kv, cov_q, cov_k, dev, caplog)
    plain = _run_driver(arch, n_heads, n_kv, cov_q, cov_k, dev, caplog, adapter_cls=Plain)
    assert plain[3] is None and "_attention_margins" not in plain[0].__dict__ and "qk_selection" not in plain[0].metrics
    assert torch.equal(full[2][0], plain[2][0])
    assert all(torch.equal(full[0].store[(0, "qk")][k], plain[0].store[(0, "qk")][k]) for k in ("q_proj", "k_proj"))
    Cx, Wv, Wo, _, _ = _vo_problem(4, 2, HD, 256, torch.Generator().manual_seed(92))
    full, plain = _run_vo(4, 2, Cx, Wv, Wo, dev, caplog), _run_vo(4, 2, Cx, Wv, Wo, dev, caplog, adapter_cls=Plain)
    assert plain[1] is None and "vo_spectrum" not in plain[0].metrics
    assert all(torch.equal(full[0].store[(0, "vo")][k], plain[0].store[(0, "vo")][k]) for k in ("v_proj", "o_proj"))


def test_end_to_end_layers_carry_attention_certificates(dev, caplog):
    """7. Two layers of engine.SHAPES["tiny"] from activations to artefacts: every layer has its qk_selection and vo_spectrum
    entries; the margins are printed."""
    from modegpt_amd import engine
    shape = engine.SHAPES["tiny"]
    adapter = engine.TensorAdapter(shape, {i: engine.make_layer_weights(shape, 1234 + i, dev) for i in range(shape["n_layers"])})
    adapter.calib_tokens = 1024
    for layer in range(shape["n_layers"]):
        covs = engine.new_covs(shape, dev)
        for b in range(2):
            engine.accumulate(covs, engine.make_activation_batch(shape, 512, seed=50 + 10 * layer + b, device=dev, scale_seed=977 + layer), shape)
        engine.finalize(covs, 2)
        engine.compress_layer(adapter, layer, covs, 0.7)
    mlp = adapter.report_selection_margins()
    with caplog.at_level(logging.WARNING, logger="MoDeGPT"):
        rep = adapter.report_attention_margins()
    assert set(mlp) == {0, 1} and set(adapter.metrics["mlp_selection"]) == {"0", "1"}
    for layer in range(shape["n_layers"]):
        qk, vo = adapter.metrics["qk_selection"][str(layer)], adapter.metrics["vo_spectrum"][str(layer)]
        assert len(qk["heads"]) == shape["n_kv_heads"] and len(vo["heads"]) == shape["n_kv_heads"]
        assert qk is rep["qk"][layer] and vo is rep["vo"][layer]
        assert all(h["margin"] > 0 and h["score_halfwidth"] > 0 for h in qk["heads"]) and 0 < vo["gap"] < 1 and 0 < vo["energy_min"] <= 1
        assert vo["separated"] in (True, False)
        margins, widths = [h["margin"] for h in qk["heads"]], [h["score_halfwidth"] for h in qk["heads"]]
        gaps, bounds, energy = [h["gap"] for h in vo["heads"]], [h["bound"] for h in vo["heads"]], [h["energy"] for h in vo["heads"]]
        print(f"layer {layer}: QK margins {margins} half-widths {widths} certified {qk['certified']} order {qk['order_certified']}; "
              f"VO gaps {gaps} bounds {bounds} energy {energy} separated {vo['separated']}")
