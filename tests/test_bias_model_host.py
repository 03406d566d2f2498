"""CPU: the identities behind the carried projection biases (tests/bias_model.py) on random fp64 data, and the all-gather record
with and without biases."""
import numpy as np
import pytest
import torch

from tests import bias_model as B

LD = B.LD
SHAPES = [(4, 2, 8, 16), (4, 4, 8, 16), (6, 2, 12, 32)]      # (n_heads, n_kv, hd, d): GQA, MHA two-SVD, a group of three


def _attention_output(X, A, Wv, Wo, b_v, b_o, n_heads, n_kv, hd, facs=None):
    """Long double attention output of a layer whose softmax rows are A[h] (row-stochastic, [T, T]): concat_h(A_h v_g) W_o^T + b_o.
    facs: the truncated layer instead, v' = x (P_g W_v,g)^T + P_g b_v,g and W_o,h' = W_o,h Q_g."""
    g = n_heads // n_kv
    out = np.zeros((X.shape[0], Wo.shape[0]), dtype=LD)
    for h in range(n_heads):
        kv = h // g
        v = B.ld(X) @ B.ld(Wv[kv * hd:(kv + 1) * hd]).T + (0 if b_v is None else B.ld(b_v[kv * hd:(kv + 1) * hd]))
        Wh = B.ld(Wo[:, h * hd:(h + 1) * hd])
        if facs is not None:
            P, Q, _ = facs[kv]
            v, Wh = v @ B.ld(P).T, Wh @ B.ld(Q)
        out += B.ld(A[h]) @ v @ Wh.T
    return out + (0 if b_o is None else B.ld(b_o))


def _inputs(shape, rank, seed):
    n_heads, n_kv, hd, d = shape
    Wv, Wo, C, b_v, b_o = B.make_case(n_heads, n_kv, hd, d, rank, seed)
    rng = np.random.default_rng(seed + 1)
    T = 5
    X = rng.standard_normal((T, d))
    A = rng.uniform(size=(n_heads, T, T))
    A /= A.sum(-1, keepdims=True)
    return Wv, Wo, C, b_v, b_o, X, A


@pytest.mark.parametrize("shape", SHAPES)
def test_fold_is_exact_at_every_rank(shape):
    """o_bias = b_o + sum_h W_o,h b_v,kv(h) with a bias-free v_proj gives the layer's output, whatever the softmax rows are."""
    n_heads, n_kv, hd, d = shape
    Wv, Wo, C, b_v, b_o, X, A = _inputs(shape, hd, 3)
    want = _attention_output(X, A, Wv, Wo, b_v, b_o, n_heads, n_kv, hd)
    o_bias, absolute = B.fold(Wo, b_v, b_o, n_heads, n_kv, hd)
    got = _attention_output(X, A, Wv, Wo, None, o_bias, n_heads, n_kv, hd)
    assert float(np.abs(got - want).max()) <= 1e-17 * float(np.abs(want).max()) * d
    assert np.all(absolute >= np.abs(o_bias))
    # the same fold commutes with the truncation: it never meets P or Q
    for rank in (2, hd - 2):
        facs = B.factors(Wv, Wo, C, n_heads, n_kv, hd, rank)
        a = _attention_output(X, A, Wv, Wo, None, o_bias, n_heads, n_kv, hd, facs)
        b = _attention_output(X, A, Wv, Wo, None, None, n_heads, n_kv, hd, facs) + o_bias
        assert float(np.abs(a - b).max()) <= 1e-17 * float(np.abs(b).max()) * d


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("rank_of", [lambda hd: hd, lambda hd: hd - 2, lambda hd: 2])
def test_projected_bias_and_residual(shape, rank_of):
    """Without a bias on o_proj: v_bias_g = P_g b_v,g makes the truncated layer equal to the original layer with Pi_g inserted behind
    v_proj -- bias included -- and what is lost of the constant is rho = sum_h W_o,h (I - Pi_g) b_v,kv(h): zero at rank = hd, and in
    the kernel of P_g (orthogonal to the kept subspace for the grouped variant, whose Pi is an orthogonal projector)."""
    n_heads, n_kv, hd, d = shape
    rank = rank_of(hd)
    Wv, Wo, C, b_v, _, X, A = _inputs(shape, rank, 5)
    facs = B.factors(Wv, Wo, C, n_heads, n_kv, hd, rank)
    for P, Q, lam in facs:
        assert np.abs(P @ Q - np.eye(rank)).max() < 1e-12
        assert B.sigma_ratio(lam, rank) >= 2.0
    v_bias = B.projected_bias(facs, b_v, hd)
    g = n_heads // n_kv
    # the truncated layer with v_bias ...
    got = np.zeros((X.shape[0], d), dtype=LD)
    for h in range(n_heads):
        P, Q, _ = facs[h // g]
        v = B.ld(X) @ (B.ld(P) @ B.ld(Wv[(h // g) * hd:(h // g + 1) * hd])).T + v_bias[(h // g) * rank:(h // g + 1) * rank]
        got += B.ld(A[h]) @ v @ (B.ld(Wo[:, h * hd:(h + 1) * hd]) @ B.ld(Q)).T
    # ... is the truncated bias-free layer plus the constant W_o Pi b_v, and the original constant minus rho
    free = _attention_output(X, A, Wv, Wo, None, None, n_heads, n_kv, hd, facs)
    const, _ = B.fold(Wo, b_v, None, n_heads, n_kv, hd)
    rho, absolute = B.residual(Wo, facs, b_v, n_heads, n_kv, hd)
    scale = float(np.abs(got).max()) * d
    assert float(np.abs(got - (free + const - rho)).max()) <= 1e-14 * scale
    assert np.all(absolute >= np.abs(rho))
    if rank == hd:
        assert float(np.abs(rho).max()) <= 1e-12 * float(np.abs(const).max())
    else:
        assert float(np.abs(rho).max()) > 1e-3 * float(np.abs(const).max())     # (the inputs can see the truncation)
    kept = B.kept_part(facs, b_v, hd)
    for k, (P, Q, _) in enumerate(facs):
        u = B.ld(b_v[k * hd:(k + 1) * hd]) - kept[k * hd:(k + 1) * hd]
        assert float(np.abs(B.ld(P) @ u).max()) <= 1e-12 * float(np.abs(P).max()) * float(np.abs(b_v).max()) * hd
        if n_kv != n_heads:
            assert float(np.abs(B.ld(Q).T @ u).max()) <= 1e-12 * float(np.abs(Q).max()) * float(np.abs(b_v).max()) * hd


def test_bf16_round_is_torch_rounding():
    x = np.random.default_rng(0).standard_normal(4096) * np.exp(np.random.default_rng(1).uniform(-20, 20, 4096))
    want = torch.from_numpy(x).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(B.bf16_round(x), want)


def test_expand_bias_maps_query_heads_to_their_kv_head():
    b = np.arange(2 * 3, dtype=np.float64)
    assert B.expand_bias(b, 4, 2, 3).tolist() == [0, 1, 2, 0, 1, 2, 3, 4, 5, 3, 4, 5]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("which", ["none", "opt", "llama", "qwen2"])
def test_pack_unpack_round_trip_with_and_without_biases(which, dtype):
    """sharding.pack_layer / unpack_layer carry the biases an artefact has, bit for bit, beside the weights and the mask."""
    from modegpt_amd import sharding
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)      # noqa: E731
    t = {"up": rnd(5, 8), "down": rnd(8, 5), "q_proj": rnd(6, 8), "k_proj": rnd(2, 8), "v_proj": rnd(4, 8), "o_proj": rnd(8, 12)}
    if which != "opt":
        t["gate"] = rnd(5, 8)
    bias = lambda n: torch.randn(n, generator=g).to(dtype)                # noqa: E731
    if which == "opt":
        t.update(up_bias=bias(5), down_bias=bias(8), q_bias=bias(6), k_bias=bias(2), o_bias=bias(8))
    elif which == "llama":
        t.update(up_bias=bias(5), gate_bias=bias(5), down_bias=bias(8), q_bias=bias(6), k_bias=bias(2), o_bias=bias(8))
    elif which == "qwen2":
        t.update(q_bias=bias(7), k_bias=bias(3), v_bias=bias(5))          # (odd lengths: the words behind them stay in place)
    mask = None if which == "opt" else torch.randint(0, 9, (2, 3), generator=g)
    rec = sharding.pack_layer(11, t, mask)
    assert rec.dtype == torch.int16
    layer, out, m = sharding.unpack_layer(torch.cat([rec, torch.zeros(5, dtype=torch.int16)]))       # (padding up to a common stride)
    assert layer == 11 and set(out) == set(t)
    for k in t:
        assert out[k].dtype == t[k].dtype and out[k].shape == t[k].shape
        assert torch.equal(out[k].view(torch.uint8), t[k].contiguous().view(torch.uint8)), k
    assert (m is None) == (mask is None) and (mask is None or torch.equal(m, mask))


def test_pack_refuses_biases_of_mixed_dtypes():
    from modegpt_amd import sharding
    t = {"up": torch.zeros(2, 2, dtype=torch.bfloat16), "up_bias": torch.zeros(2, dtype=torch.bfloat16),
         "down_bias": torch.zeros(2, dtype=torch.float16)}
    with pytest.raises(ValueError):
        sharding.pack_layer(0, t, None)


def test_vo_bias_refuses_bad_arguments_without_touching_a_device():
    """Status codes, not aborts: every refusal below is decided before anything is enqueued (the pointers are never followed)."""
    import ctypes
    from modegpt_amd import _lib
    lib = _lib.load()
    host = (ctypes.c_double * 8)()
    p = ctypes.addressof(host)
    nbytes = lib.mdg_vo_compress_ws_bytes(64, 4, 2, 32)
    good = (("ws", p), ("ws_bytes", nbytes), ("Wo", p), ("ld_wo", 128), ("w_dtype", _lib.MDG_F64), ("d", 64), ("b_v", p), ("b_o", None),
            ("b_dtype", _lib.MDG_F64), ("n_heads", 4), ("n_kv", 2), ("hd", 32), ("rank", 8), ("o_bias", None), ("v_bias", p), ("resid", p),
            ("stream", None))
    for kw in (dict(ld_wo=127), dict(rank=33), dict(rank=0), dict(w_dtype=_lib.MDG_F32), dict(ws_bytes=nbytes - 8), dict(v_bias=None),
               dict(b_o=p), dict(n_kv=3), dict(b_dtype=9), dict(resid=None), dict(ws=None), dict(hd=130), dict(d=0)):
        assert lib.mdg_vo_bias(*[kw.get(k, v) for k, v in good]) == _lib.MDG_ERR_BAD_ARG, kw
        assert b"mdg_vo_bias" in lib.mdg_last_error()
    # a head so small that the scratch does not fit the workspace's T block
    tiny = dict(good, n_heads=1, n_kv=1, hd=2, d=2, ld_wo=2, rank=2, ws_bytes=lib.mdg_vo_compress_ws_bytes(2, 1, 1, 2))
    assert lib.mdg_vo_bias(*tiny.values()) == _lib.MDG_ERR_BAD_ARG and b"scratch" in lib.mdg_last_error()
