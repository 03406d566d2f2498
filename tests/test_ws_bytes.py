"""Every workspace-size query returns what tests/golden/ws_bytes.json recorded (scripts/record_ws_bytes.py, from the commit before the
layouts were stated once): the size and the carve are one function now, so a size that moved is a block that moved.  Host only.

The sweep and what it leaves out (negative extents of the unguarded queries) are in tests/ws_bytes_cases.py.
"""
import json
import os

from modegpt_amd import _lib
from tests import ws_bytes_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_bytes.json")


def _golden():
    with open(GOLDEN) as f:
        return [(fn, tuple(args), want) for fn, args, want in json.load(f)]


def test_golden_is_the_sweep():
    assert [(fn, args) for fn, args, _ in _golden()] == cases.cases()


def test_sizes_are_the_recorded_ones():
    lib = _lib.load()
    rows = _golden()
    bad = [(fn, args, want, int(getattr(lib, fn)(*args))) for fn, args, want in rows if int(getattr(lib, fn)(*args)) != want]
    assert not bad, "%d of %d sizes differ, first: %s%s = recorded %d, now %d" % ((len(bad), len(rows)) + bad[0])
    # the guards are in the sweep: a refused argument gives 0
    fns = {fn for fn, _, _ in rows}
    guarded = {fn for fn, _, want in rows if want == 0}
    unguarded = {"mdg_potrf_inv_diag_elems", "mdg_chol_inverse_diag_ws_bytes", "mdg_ridge_scores_ws_bytes", "mdg_sqrt_psd_large_ws_bytes",
                 "mdg_sqrt_psd_small_ws_bytes", "mdg_vo_compress_ws_bytes", "mdg_nystrom_down_ws_bytes", "mdg_bi_ws_bytes"}
    assert fns - guarded <= unguarded, sorted(fns - guarded - unguarded)


def test_sqrt_psd_large_sweep_straddles_the_newton_crossover():
    """mdg_sqrt_psd_large's size is the larger of its two routes' layouts: n = 371 is the last n under np = 384 where the Jacobi layout is
    the larger, n = 372 the first where the Newton layout is."""
    lo, hi = cases.SQRT_LARGE_JACOBI_N, cases.SQRT_LARGE_NEWTON_N
    assert hi == lo + 1
    assert cases.sqrt_large_jacobi_bytes(lo) > cases.sqrt_large_newton_bytes(lo)
    assert cases.sqrt_large_jacobi_bytes(hi) < cases.sqrt_large_newton_bytes(hi)
    lib = _lib.load()
    assert lib.mdg_sqrt_psd_large_ws_bytes(lo) == cases.sqrt_large_jacobi_bytes(lo)
    assert lib.mdg_sqrt_psd_large_ws_bytes(hi) == cases.sqrt_large_newton_bytes(hi)
    got = {args[0]: want for fn, args, want in _golden() if fn == "mdg_sqrt_psd_large_ws_bytes"}
    assert got[lo] == cases.sqrt_large_jacobi_bytes(lo) and got[hi] == cases.sqrt_large_newton_bytes(hi)
