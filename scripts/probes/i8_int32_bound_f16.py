"""Exact int32 headroom of the digit-plane classes for fp16 activations (csrc/cov_i8_split.hip, F16Elem) -- the fp16 twin of
i8_int32_bound.py.  An fp16 element is a signed 11-bit significand at some shift 0 .. 29 below its column's maximum (effective
exponents 1 .. 30), placed with the column maximum's significand below bit 46 (top shift 35): its six balanced base-256 digits
can fill THREE digits (11 bits straddle three bytes) plus a carry digit, where a bf16 element fills two.  Enumerates ALL digit
vectors the split pass can produce and, per class k, the largest |sum_{s+t=k} d_s(i) d_t(j)| over all pairs of elements ->
the number of tokens a class can accumulate before 2^31 - 1, for the three products (P = 3: the exact route's nine pairs of
planes 0 .. 2, classes 0 .. 4; P = 5, 6: the truncated products, pairs s + t < P).

Two figures.  per_token_bound(): an UPPER bound in a second -- the nonzero digits of an element fill a window of three planes; a
class sum of two elements is a coefficient of the product of their window polynomials, or (truncated products) a partial sum of
one, so sum_{u+v=m} |c_u| |c'_v| bounds it; the maximum is taken over the Pareto front of the |c| windows.  attained_per_token():
the exact class sums of every digit vector with ITSELF for the three products -- it reaches the bound (32768, the element
(-3, -128, -128, 0, 0, 0) in class 3), so the bound is the exact figure.  worst_per_token(P) is the brute-force enumeration over
all pairs (twenty minutes; not run by the tests).  Result: 32768 per token, the bf16 figure -- where two digits of an fp16
element are full, the third holds at most 3 bits and a carry -- so 2047 k-steps of 32 tokens between folds hold for fp16 too.

tests/test_i8_f16_host.py imports this file and checks FLUSH_STEPS_F16 of csrc/cov_i8.hpp against both figures.
"""
import numpy as np

NP_, TOP, SIG_MAX, SHIFT_MAX = 6, 35, 2047, 29


def balanced_digits(N):
    """Python int N -> its six balanced base-256 digits [d_0 .. d_5], d_1 .. d_5 in [-128, 127]."""
    d = [0] * NP_
    for s in range(NP_ - 1, 0, -1):
        b = ((N + 128) & 255) - 128
        d[s] = b
        N = (N - b) >> 8
    d[0] = N
    return d


def digit_vectors():
    vecs = set()
    for sh in range(0, SHIFT_MAX + 1):
        for sig in range(1, SIG_MAX + 1):
            d = balanced_digits(sig << (TOP - sh))          # (never rounded: sh <= 29 < 35)
            assert 0 <= d[0] <= 64, (sig, sh, d)
            vecs.add(tuple(d))
            vecs.add(tuple(balanced_digits(-(sig << (TOP - sh)))))   # (not the negated digits: -128 has no +128 partner)
    return np.array(sorted(vecs), dtype=np.int64)


def kept(P, s, t):
    return (s < 3 and t < 3) if P == 3 else (s + t < P)


def windows(V):
    """|digits| of every vector from its first nonzero plane on, three wide (asserts nothing lies beyond)."""
    A = np.abs(V)
    first = (A != 0).argmax(axis=1)
    W = np.zeros((len(V), 3), dtype=np.int64)
    for u in range(3):
        idx = first + u
        W[:, u] = np.where(idx < NP_, A[np.arange(len(V)), np.minimum(idx, NP_ - 1)], 0)
    assert (A.sum(1) == W.sum(1)).all(), "a digit outside the three-plane window"
    return W


def per_token_bound(V=None):
    V = digit_vectors() if V is None else V
    W = windows(V)
    best = np.full((130, 130), -1, dtype=np.int64)              # best[c0][c1] = largest c2; then the Pareto front of (c0, c1, c2)
    np.maximum.at(best, (W[:, 0], W[:, 1]), W[:, 2])
    dom = np.maximum.accumulate(np.maximum.accumulate(best[::-1, ::-1], axis=0), axis=1)[::-1, ::-1]
    up = np.full_like(dom, -1); up[:-1] = dom[1:]
    right = np.full_like(dom, -1); right[:, :-1] = dom[:, 1:]
    c0, c1 = np.nonzero((best >= 0) & (best > up) & (best > right))
    F = np.stack([c0, c1, best[c0, c1]], axis=1)
    worst = 0
    for m in range(5):
        tot = sum(np.outer(F[:, u], F[:, m - u]) for u in range(3) if 0 <= m - u < 3)
        worst = max(worst, int(tot.max()))
    return worst


def attained_per_token(V=None):
    """-> (largest |class sum| of a digit vector with itself over the three products, P, class, the vector)."""
    V = digit_vectors() if V is None else V
    out = (0, None, None, None)
    for P in (3, 5, 6):
        for k in range(2 * NP_ - 1):
            tot = np.zeros(len(V), dtype=np.int64)
            for s in range(NP_):
                t = k - s
                if 0 <= t < NP_ and kept(P, s, t):
                    tot += V[:, s] * V[:, t]
            i = int(np.abs(tot).argmax())
            if abs(int(tot[i])) > out[0]:
                out = (abs(int(tot[i])), P, k, tuple(int(x) for x in V[i]))
    return out


def worst_per_token(P, V=None):
    """Brute force: largest |class sum| one token can add, over all classes of the P-plane product and ALL pairs of elements."""
    V = digit_vectors() if V is None else V
    worst = (0, None, None, None)
    Vt = V.T.copy()
    for k in range(2 * NP_ - 1):
        W = np.zeros_like(V)                                # W[i][t] = d_{k-t}(i): class-k sum = W_i . V_j
        for t in range(NP_):
            if 0 <= k - t < NP_ and kept(P, k - t, t):
                W[:, t] = V[:, k - t]
        if not W.any():
            continue
        for lo in range(0, len(V), 2048):
            M = np.abs(W[lo:lo + 2048] @ Vt)
            m = int(M.max())
            if m > worst[0]:
                i, j = np.unravel_index(int(M.argmax()), M.shape)
                worst = (m, k, tuple(V[lo + i]), tuple(V[j]))
    return worst


if __name__ == "__main__":
    import sys
    V = digit_vectors()
    print(len(V), "distinct digit vectors; |d_0| max", np.abs(V[:, 0]).max(), "; nonzero digits per element max", (V != 0).sum(1).max())
    b, a = per_token_bound(V), attained_per_token(V)
    print(f"upper bound on |class sum| per token: {b}; attained by a vector with itself: {a[0]} (P={a[1]}, class {a[2]}, digits {a[3]})")
    print(f"a class holds {(2**31 - 1) // b} tokens = {(2**31 - 1) // b // 32} k-steps of 32 before int32 could overflow")
    if "--all-pairs" in sys.argv:
        for P in (3, 5, 6):
            w, k, x, y = worst_per_token(P, V)
            print(f"P={P}: all pairs: max |class sum| per token = {w} (class {k}, digits {x} x {y})")
