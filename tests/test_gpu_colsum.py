"""GPU: mdg_col_sum_accum (column sums of the sigma_mlp activation in fp64) through the raw C ABI.

Exact cases: the inputs are small integers (|k| <= 8) times a per-column power of two (2^-3 .. 2^3), representable in every dtype, so
every partial sum is an integer multiple of the column's power of two far below 2^53 of it: the fp64 sums are exact in ANY order and
the comparison is torch.equal against the long double model (tests/mean_model.py).  Token counts sit on both sides of the 128-token
chunk, widths on both sides of the 16-byte vector and of the 256-slot column block; a view offset by one element and a leading
dimension that is no multiple of the vector take the single-column slots.  `sum` and the workspace sit inside NaN-filled guards.
Generic Gaussian data is held entry-wise to tokens 2^-53 sum_t |x_t| (any order of `tokens` additions)."""
import numpy as np
import pytest
import torch

from tests import mean_model as M

pytestmark = pytest.mark.gpu
CHUNK = 128                       # ops.COL_SUM_CHUNK, asserted below
GUARD = 32
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f64": torch.float64}
VEC = {"bf16": 8, "f16": 8, "f32": 4, "f64": 2}


def _ints(tokens, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, size=(tokens, n)).astype(np.float64) * 2.0 ** rng.integers(-3, 4, size=n)


def _run(x_host, dt, relu=False, ld=None, offset=0, calls=1, start=None):
    """x_host [tokens, n] fp64 values -> device buffer of dtype dt with leading dimension ld, `offset` elements into an allocation;
    the padding columns hold NaN (never read).  Returns the sum as a host fp64 array after `calls` accumulating calls."""
    from modegpt_amd import _lib, ops
    assert ops.COL_SUM_CHUNK == CHUNK
    lib = _lib.load()
    dev = torch.device("cuda")
    tokens, n = x_host.shape
    ld = ld or n
    tdt = DTYPES[dt]
    flat = torch.full((offset + tokens * ld + 8,), float("nan"), dtype=tdt, device=dev)
    view = flat[offset:offset + tokens * ld].view(tokens, ld)
    view[:, :n] = torch.from_numpy(x_host).to(dev).to(tdt)
    assert view.data_ptr() == flat.data_ptr() + offset * flat.element_size()
    nbytes = lib.mdg_col_sum_ws_bytes(tokens, n)
    assert nbytes == 8 * n * ((tokens + CHUNK - 1) // CHUNK)
    sum_buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=dev)
    s = sum_buf[GUARD:GUARD + n]
    s.copy_(torch.zeros(n, dtype=torch.float64) if start is None else torch.from_numpy(start))
    ws_buf = torch.full((nbytes // 8 + 2 * GUARD,), float("nan"), dtype=torch.float64, device=dev)
    ws = ws_buf[GUARD:GUARD + nbytes // 8]
    st = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(calls):
        _lib.check(lib.mdg_col_sum_accum(view.data_ptr(), ops._DT[tdt], tokens, n, ld, int(relu), s.data_ptr(), ws.data_ptr(), nbytes,
                                         st), "mdg_col_sum_accum")
    torch.cuda.synchronize(dev)
    for buf, m in ((sum_buf, n), (ws_buf, nbytes // 8)):
        host = buf.cpu()
        assert bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[GUARD + m:]).all()), "a guard was written"
    return s.cpu().numpy().copy()


def _expect(x_host, relu=False, calls=1, start=None):
    ref = M.col_sums(x_host, relu=relu) * calls
    if start is not None:
        ref = ref + M.ld(start)
    out = ref.astype(np.float64)
    assert np.array_equal(out.astype(M.LD), ref)          # exact by construction
    return out


TOKENS = [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 37]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("tokens", TOKENS)
def test_token_counts_around_the_chunk(dt, tokens):
    x = _ints(tokens, 72, seed=tokens)
    for relu in (False, True):
        assert np.array_equal(_run(x, dt, relu=relu), _expect(x, relu=relu)), (dt, tokens, relu)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_widths_around_the_vector_and_the_column_block(dt):
    block = 256 * VEC[dt]                                  # columns of one 256-slot block on the vector path
    for n, ld in ((1, None), (7, None), (8, None), (9, None), (block - 1, None), (block + 1, None), (520, 528),
                  (block + 1, block + 8), (24, 27)):       # (ld 27: no multiple of any vector -> every column a scalar slot)
        x = _ints(CHUNK + 5, n, seed=n)
        for relu in (False, True):
            assert np.array_equal(_run(x, dt, relu=relu, ld=ld), _expect(x, relu=relu)), (dt, n, ld, relu)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_view_offset_by_one_element(dt):
    """The base is aligned to the element only: the columns in front of the first 16-byte boundary are single-column slots."""
    for n, ld in ((520, 528), (3, 8), (41, 48)):
        x = _ints(2 * CHUNK + 3, n, seed=7 + n)
        for off in (1, 3):
            assert np.array_equal(_run(x, dt, ld=ld, offset=off), _expect(x)), (dt, n, off)
            assert np.array_equal(_run(x, dt, relu=True, ld=ld, offset=off), _expect(x, relu=True)), (dt, n, off)


def test_two_calls_accumulate_on_what_sum_held():
    x = _ints(CHUNK + 9, 100, seed=5)
    start = np.arange(100, dtype=np.float64) - 50.0
    assert np.array_equal(_run(x, "bf16", calls=2, start=start), _expect(x, calls=2, start=start))


@pytest.mark.parametrize("relu", [False, True])
def test_nan_and_inf_stay_in_their_columns(relu):
    x = _ints(2 * CHUNK + 1, 75, seed=11)
    x[130, 9] = np.nan
    x[5, 41] = np.inf
    out = _run(x, "bf16", relu=relu, ld=80)
    assert np.isnan(out[9]) and out[41] == np.inf
    keep = np.ones(75, dtype=bool)
    keep[[9, 41]] = False
    assert np.array_equal(out[keep], _expect(x[:, keep], relu=relu))


def test_ops_front_end_takes_batched_activations_and_strided_views():
    from modegpt_amd import ops
    dev = torch.device("cuda")
    x = _ints(2 * 96, 136, seed=3)
    xb = torch.from_numpy(x).to(dev).to(torch.bfloat16).view(2, 96, 136)
    s = torch.zeros(136, dtype=torch.float64, device=dev)
    ops.col_sum_accum(s, xb)
    ops.col_sum_accum(s, xb[..., :136], relu=True)
    assert np.array_equal(s.cpu().numpy(), _expect(x) + _expect(x, relu=True))
    s2 = torch.zeros(64, dtype=torch.float64, device=dev)
    ops.col_sum_accum(s2, xb.view(192, 136)[:, 8:72])       # a column slice: ld 136, width 64
    assert np.array_equal(s2.cpu().numpy(), _expect(x[:, 8:72]))
    with pytest.raises(ValueError):
        ops.col_sum_accum(torch.zeros(5, dtype=torch.float64, device=dev), xb)
    with pytest.raises(RuntimeError):
        ops.col_sum_accum(torch.zeros(136, dtype=torch.float64), xb)


@pytest.mark.parametrize("dt", ["bf16", "f32", "f64"])
def test_generic_gaussian_data_within_the_rounding_bound(dt):
    rng = np.random.default_rng(17)
    tokens, n = 5 * CHUNK + 11, 200
    x = rng.standard_normal((tokens, n)) + 0.5
    x = torch.from_numpy(x).to(DTYPES[dt]).to(torch.float64).numpy()      # the values the device holds
    for relu in (False, True):
        out = _run(x, dt, relu=relu)
        ref = M.col_sums(x, relu=relu)
        mag = np.abs(M.ld(np.maximum(x, 0) if relu else x)).sum(axis=0)
        err = np.abs(M.ld(out) - ref)
        print(f"{dt} relu={relu}: max err / bound = {float((err / (tokens * 2.0 ** -53 * mag)).max()):.3e}")
        assert np.all(err <= tokens * M.LD(2.0 ** -53) * mag)


def test_runs_are_bit_identical():
    rng = np.random.default_rng(23)
    x = rng.standard_normal((4 * CHUNK + 3, 300))
    a = _run(x, "f64")
    b = _run(x, "f64")
    assert np.array_equal(a, b)
