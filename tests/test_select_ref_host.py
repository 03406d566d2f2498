"""The plain references of the index kernels (tests/select_ref.py) checked on the host: against the oracle where the oracle's order is
defined, against a brute-force rank count on the special values, against the hand-made certificate rows of tests/test_host.py, and
the two-step bf16 rounding against torch and against a single correct rounding.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import modegpt_oracle as O
from tests import select_ref as S

F64 = torch.float64
NAN, INF = float("nan"), float("inf")


def special_scores(n, seed):
    """-0.0, +0.0, +-inf, denormals, repeated values, and NaN over about a quarter of the entries."""
    rng = np.random.default_rng(seed)
    pool = np.array([-0.0, 0.0, INF, -INF, 5e-324, -5e-324, 2.0 ** -1040, 1.0, 1.0, -1.0, 2.5, 1e300, -1e300])
    s = pool[rng.integers(0, pool.size, n)]
    s[rng.random(n) < 0.25] = NAN
    return s


@pytest.mark.parametrize("n,k", [(1, 1), (5, 3), (160, 112), (1000, 1), (1000, 1000), (1025, 512)])
def test_smallest_sorted_is_the_oracle_without_ties(n, k):
    s = torch.rand(n, generator=torch.Generator().manual_seed(n + k), dtype=F64)
    assert s.unique().numel() == n
    assert np.array_equal(S.smallest_sorted(s.numpy(), k), O.mlp_select(s, k).numpy())


@pytest.mark.parametrize("n", [1, 2, 7, 64, 130])
def test_smallest_sorted_is_the_rank_count_on_special_values(n):
    s = special_scores(n, seed=n)
    for k in sorted({0, 1, n // 2, n - 1, n, int((~np.isnan(s)).sum()), min(n, int((~np.isnan(s)).sum()) + 1)}):
        got = S.smallest_sorted(s, k)
        assert got.dtype == np.int64 and got.size == k and np.array_equal(got, S.rank_count_select(s, k)), (n, k)


def test_smallest_sorted_order_in_words():
    s = np.array([3.0, 1.0, 2.0, 1.0, 1.0, 5.0, NAN, 0.5])
    assert S.smallest_sorted(s, 3).tolist() == [1, 3, 7]                        # ties: lower index first
    assert S.smallest_sorted(np.array([0.0, -0.0, 0.0, -0.0]), 2).tolist() == [0, 1]        # -0.0 == +0.0
    assert S.smallest_sorted(np.array([NAN, INF, NAN, -INF]), 3).tolist() == [0, 1, 3]      # NaN after +inf, lower NaN first
    assert S.smallest_sorted(np.full(9, 7.0), 4).tolist() == [0, 1, 2, 3]
    assert S.smallest_sorted(np.arange(5.0), 0).size == 0


def test_margin8_reproduces_the_hand_made_rows():
    """The two rows of test_selection_margin_report_certified_or_flagged, from scores that have them as their certificate."""
    eps = 1.1e-11
    for rel, at_risk, certified in ((1e-6, 0., 1.), (1e-13, 2., 0.)):
        want = [2.0, 2.0 * (1 + rel), 2.0 + eps * 40, 2.0 * (1 + rel) - eps * 60, 40., 60., at_risk, certified]
        #    selected: 0 (far below), 2 (s_k, the largest sens)   unselected: 1 (s_k+1, the largest sens), 3 (far above)
        s = np.array([1.0, 2.0 * (1 + rel), 2.0, 3.0])
        sens = np.array([5.0, 60.0, 40.0, 7.0])
        idx = S.smallest_sorted(s, 2)
        assert idx.tolist() == [0, 2]
        assert S.margin8(s, sens, idx, 4, 2, eps).tolist() == want


def test_margin8_edges():
    s = np.array([0.5, NAN, 0.25, 0.75, NAN])
    sens = np.array([1.0, 99.0, 2.0, 3.0, 98.0])
    none = S.margin8(s, sens, np.zeros(0, dtype=np.int64), 5, 0, 0.125)
    assert none.tolist() == [-INF, 0.25, -INF, 0.0, 0.0, 3.0, 0.0, 1.0]
    full = S.margin8(s, sens, np.arange(5), 5, 5, 0.125)
    assert full.tolist() == [0.75, INF, 1.125, INF, 3.0, 0.0, 0.0, 1.0]
    # NaN takes no part on either side; {0, 1, 2} selected: 0.5 + 0.125 < 0.75 - 0.375 fails
    got = S.margin8(s, sens, np.array([0, 1, 2]), 5, 3, 0.125)
    assert got.tolist() == [0.5, 0.75, 0.625, 0.375, 2.0, 3.0, 2.0, 0.0]
    # an ascending idx that is not the k smallest; eps = 0: only the score that IS the midpoint reaches it
    got = S.margin8(s, sens, np.array([3]), 5, 1, 0.0)
    assert got.tolist() == [0.75, 0.25, 0.75, 0.25, 3.0, 2.0, 1.0, 0.0]


@pytest.mark.parametrize("mode,n_heads,n_kv,arch", [(S.ROPE_GROUPED, 8, 2, "llama"), (S.ROPE_MHA, 3, 3, "llama"), (S.OPT, 3, 3, "opt")])
def test_qk_select_ref_is_the_oracle_on_a_ladder(mode, n_heads, n_kv, arch):
    """On scores 1 % apart the diagonal formulae pick what the oracle's eigh route picks, mask and order."""
    from tests.test_attn_certificate_host import ladder_heads
    hd, rank, ridge_k = 64, 44, (1e-2 if mode == S.ROPE_GROUPED else 1e-4)
    cov_q, cov_k, _ = ladder_heads(n_heads, n_kv, hd, mode, torch.Generator().manual_seed(3 + mode), ridge_k)
    W = torch.zeros(n_heads * hd, 8), torch.zeros(n_kv * hd, 8)
    _, want = O.compress_qk_layer(W[0], W[1], cov_q, cov_k, n_heads, n_kv, hd, rank, arch, ridge_k)
    mask, q_rows, k_rows = S.qk_select_ref(cov_q.numpy(), cov_k.numpy(), n_heads, n_kv, hd, 1e-4, ridge_k, rank, mode)
    assert np.array_equal(mask, want.numpy())
    g = n_heads // n_kv
    assert k_rows.tolist() == [h * hd + j for h in range(n_kv) for j in mask[h]]
    assert q_rows.tolist() == [q * hd + j for q in range(n_heads) for j in mask[q // g]]


def test_qk_select_ref_ties_clamp_and_nan():
    hd, n = 8, 1
    d = np.array([3.0, -5.0, 3.0, 7.0, 3.0, -9.0, 3.0, 7.0])                   # units (j, j + 4): scores 18, 0 (clamped), 18, 98
    cq, ck = np.diag(d)[None], np.diag(d)[None]
    mask, _, _ = S.qk_select_ref(cq, ck, n, n, hd, 0.0, 0.0, 8, S.ROPE_MHA)
    assert mask.tolist() == [[3, 0, 2, 1, 7, 4, 6, 5]]
    ck = ck.copy()
    ck[0, 5, 5] = NAN                                                           # unit 1 now scores NaN: first
    mask, _, _ = S.qk_select_ref(cq, ck, n, n, hd, 0.0, 0.0, 4, S.ROPE_MHA)
    assert mask.tolist() == [[1, 3, 5, 7]]
    mask, q_rows, k_rows = S.qk_select_ref(np.diag(d)[None], np.diag(d)[None], n, n, hd, 6.0, 6.0, 3, S.OPT)
    assert mask.tolist() == [[3, 7, 0]] and q_rows.tolist() == [3, 7, 0] and k_rows.tolist() == [3, 7, 0]


def test_two_step_rounding_is_torch_and_not_a_single_rounding():
    x = S.double_rounding_set()
    two = S.to_bf16_via_float(x)
    assert torch.equal(two.view(torch.int16), x.to(torch.bfloat16).view(torch.int16))
    one = S.to_bf16_single_rounding(x)
    differs = two.view(torch.int16) != one.view(torch.int16)
    assert int(differs.sum()) >= 2
    # the two bases named where the set is described: 1.0 and 1.5 * 2^-126 go down where the single rounding goes up
    for i, base in ((0, 1.0), (1, 1.5 * 2.0 ** -126)):
        assert bool(differs[i]) and two[i].double().item() == base and one[i].double().item() > base
    # elsewhere the single rounding is what the name says: the nearest bf16, checked against both neighbours
    y = torch.randn(4000, generator=torch.Generator().manual_seed(0), dtype=F64) * 2.0 ** torch.randint(-30, 30, (4000,)).double()
    r = S.to_bf16_single_rounding(y)
    below = ((r.view(torch.int16).int() - 1).to(torch.int16)).view(torch.bfloat16).double()
    above = ((r.view(torch.int16).int() + 1).to(torch.int16)).view(torch.bfloat16).double()
    err = (r.double() - y).abs()
    assert bool((err <= (below - y).abs()).all()) and bool((err <= (above - y).abs()).all())
    assert torch.equal(S.to_bf16_via_float(y).view(torch.int16), y.to(torch.bfloat16).view(torch.int16))
