"""The sweep behind tests/golden/ws_bytes.json: every workspace-size query of the library with plain integer arguments (and
mdg_potrf_inv_diag_elems), at the sizes where a rounding of the layout bites.  scripts/record_ws_bytes.py records the numbers from a
built checkout, tests/test_ws_bytes.py holds the current library against them.  No device is needed: the queries are pure host calls.

Left out, because the recorded commit's function has no guard and would compute from a negative extent: every negative argument
of mdg_potrf_inv_diag_elems, mdg_chol_inverse_diag_ws_bytes, mdg_ridge_scores_ws_bytes, mdg_sqrt_psd_large_ws_bytes,
mdg_sqrt_psd_small_ws_bytes, mdg_vo_compress_ws_bytes and mdg_nystrom_down_ws_bytes, and for the last one also r > n (its n - r).
A zero extent is well defined there and is swept.  The queries that take an array of problems (mdg_cov_accum_multi_ws_bytes,
mdg_cov_accum_i8_multi_ws_bytes) are left out too: their layouts have their own tests.
"""

# n at and across multiples of 16 and 128, and the two MLP widths of the flagship workload
N = [1, 15, 16, 17, 127, 128, 129, 130, 300, 10035, 14336]

# mdg_sqrt_psd_large_ws_bytes is max(Jacobi, Newton).  With np = n rounded up to 128, the Jacobi layout is
# (4 np^2 + 2 (np / 128) 128^2 + 3 np + 64) * 8 + 2 (np / 64) * 4 + 256 bytes and the Newton layout (5 n^2 + 80 + n) * 8.  At np = 128
# and np = 256 Jacobi is the larger for every n; inside np = 384 Newton overtakes it between n = 371 and n = 372.
SQRT_LARGE_JACOBI_N, SQRT_LARGE_NEWTON_N = 371, 372


def sqrt_large_jacobi_bytes(n):
    np_ = (n + 127) // 128 * 128
    return (4 * np_ * np_ + 2 * (np_ // 128) * 128 * 128 + 3 * np_ + 64) * 8 + 2 * (np_ // 64) * 4 + 256


def sqrt_large_newton_bytes(n):
    return (5 * n * n + 80 + n) * 8


def cases():
    """[(function name, argument tuple)], in a fixed order."""
    out, seen = [], set()

    def add(fn, *args):
        row = (fn, tuple(int(a) for a in args))
        if row not in seen:                      # (rank = hd = 0 and the like name one call twice)
            seen.add(row)
            out.append(row)

    for n in [0] + N:
        add("mdg_potrf_inv_diag_elems", n)
        add("mdg_chol_inverse_diag_ws_bytes", n)
        add("mdg_ridge_scores_ws_bytes", n)
    for n in [-1, 0] + N:
        for nrhs in ((-1, 0, 1, 3, 4096) if n in (-1, 130) else (3, 4096)):
            add("mdg_potrs_lower_ws_bytes", n, nrhs)
    # r = 0, r = n, r odd, n - r a multiple of 16 and not
    add("mdg_nystrom_down_ws_bytes", 0, 0, 0)
    for n in N:
        ranks = sorted({0, 1, n, (n // 2) | 1, max(n - 16, 0), max(n - 7, 0), n * 7 // 10})
        for r in ranks:
            if r <= n:
                for d in ((1, 40, 4096) if n in (130, 10035, 14336) else (40,)):
                    add("mdg_nystrom_down_ws_bytes", n, r, d)
    for tokens in (-1, 0, 1, 127, 128, 129, 32768):
        for n in (-1, 0, 1, 150, 14336):
            add("mdg_col_sum_ws_bytes", tokens, n)
    for d in (-1, 0, 1, 40, 4096):
        add("mdg_nystrom_intercept_ws_bytes", d)
    for n in [-1, 0] + N:
        for d in ((0, 1, 40, 4096) if n in (-1, 130) else (40, 4096)):
            add("mdg_nystrom_rank_curve_ws_bytes", n, d)
            add("mdg_mlp_output_error_ws_bytes", n, d)
    # rounds of 1, below r, equal to r, above r; r = 0, odd, n; the guards
    for n, d in ((130, 3), (150, 40), (14336, 4096)):
        for r in sorted({0, 1, 2, 37, n * 7 // 10, n}):
            for rounds in sorted({1, 3, 5, max(r - 1, 1), max(r, 1), r + 1, r + 5}):
                if rounds <= 40 or rounds >= r - 1:
                    add("mdg_nystrom_greedy_ws_bytes", n, d, r, rounds)
    for args in ((0, 40, 0, 1), (150, 0, 37, 1), (150, 40, -1, 1), (150, 40, 151, 1), (150, 40, 37, 0), (-1, 40, 0, 1), (150, 40, 37, -2)):
        add("mdg_nystrom_greedy_ws_bytes", *args)
    # rank of 0 and hd; d across the 256-row chunks of the V/O curve
    for d in (48, 257, 4096):
        for n_heads, n_kv in ((4, 2), (2, 2), (32, 8)):
            for hd in (8, 128):
                add("mdg_vo_compress_ws_bytes", d, n_heads, n_kv, hd)
                add("mdg_vo_rank_curve_ws_bytes", d, n_heads, n_kv, hd)
                for rank in (0, 3, hd):
                    add("mdg_vo_output_error_ws_bytes", d, n_heads, n_kv, hd, rank)
                    add("mdg_vo_intercept_ws_bytes", d, n_kv, hd, rank)
    for d, n_heads, n_kv, hd in ((0, 4, 2, 8), (48, 0, 0, 8), (48, 4, 2, 0)):
        add("mdg_vo_compress_ws_bytes", d, n_heads, n_kv, hd)
    # the guards: d, the head layout (n_kv no divisor, hd odd or above 128), the rank outside 0 .. hd
    for d, n_heads, n_kv, hd, rank in ((-1, 4, 2, 8, 3), (0, 4, 2, 8, 3), (48, 4, 3, 8, 3), (48, 0, 0, 8, 3), (48, 4, -1, 8, 3), (48, 4, 2, 7, 3),
                                       (48, 4, 2, 0, 0), (48, 4, 2, 130, 3), (48, 4, 2, 8, -1), (48, 4, 2, 8, 9)):
        add("mdg_vo_rank_curve_ws_bytes", d, n_heads, n_kv, hd)
        add("mdg_vo_output_error_ws_bytes", d, n_heads, n_kv, hd, rank)
        add("mdg_vo_intercept_ws_bytes", d, n_kv, hd, rank)
    for n in (0, 1, 6, 64, 128):
        for batch in (0, 1, 3):
            add("mdg_sqrt_psd_small_ws_bytes", n, batch)
    for n in [0] + N + [256, 257, SQRT_LARGE_JACOBI_N, SQRT_LARGE_NEWTON_N, 384, 385, 4096]:
        add("mdg_sqrt_psd_large_ws_bytes", n)
    for fn in ("mdg_qk_pair_ws_bytes", "mdg_qk_causal_ws_bytes"):
        for B in (-1, 0, 1, 2):
            for n_heads in (0, 4):
                for hd in (0, 8, 128):
                    for want_raw in (0, 1):
                        add(fn, B, n_heads, hd, want_raw)
    for tokens, feat, batch in ((32768, 14336, 1), (32768, 128, 8), (1, 1, 1), (0, 128, 8), (129, 300, 3)):
        add("mdg_cov_accum_ws_bytes", tokens, feat, batch)
    for tokens, feat in ((32768, 14336), (1, 1), (0, 128), (129, 300)):
        add("mdg_cov_accum_i8_ws_bytes", tokens, feat)
    for tokens in (0, 1, 32768):
        add("mdg_bi_ws_bytes", tokens)
    for args in ((1, 1, 4, 8, 8), (2, 4, 32, 64, 16), (0, 1, 4, 8, 8)):
        add("mdg_attn_decode_ws_bytes", *args)
    return out
