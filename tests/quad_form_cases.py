"""The calls whose raw bits tests/golden/quad_form_bits.npz holds (scripts/record_quad_form_bits.py writes it, tests/test_gpu_quad_form_bits.py
compares): mdg_mlp_output_error and mdg_vo_output_error on inputs made on the host from seeded generators alone -- the statistic from
tests.test_gpu_chol.matrix, the weights as tests/test_gpu_output_error.py builds them, a seeded permutation prefix as idx, seeded
replacement tensors -- so that the fixture depends on no device code but the two entry points it pins."""
import numpy as np
import torch

from tests.test_gpu_chol import matrix
from tests.test_gpu_output_error import weight

BF16, F64 = torch.bfloat16, torch.float64
KINDS = ["p3", "p6g3", "acts"]
# (n, d): one element, a ragged stage, one column past a tile edge, two row blocks, three and five tile columns
MLP_SHAPES = [(1, 1), (16, 70), (129, 1), (129, 257), (385, 70), (640, 257)]
# (hd, r, d, n_heads, n_kv): one tile column with a ragged stage; two tile columns and two row blocks; nothing subtracted
VO_SHAPES = [(16, 11, 70, 4, 2), (128, 88, 257, 2, 2), (6, 0, 257, 3, 1)]
WDTS = [BF16, torch.float32]               # (fp32 is widened exactly to fp64 by ops._as_weight)


def randn(seed, *shape, scale=0.05, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype) * scale


def mlp_inputs(n, d, r):
    """(idx [r], down bf16 [d, r], D fp64 [r, d]) -- `down` goes in as it is, D as D.T."""
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(31 * n + d))[:r]
    return idx, randn(17 * n + d, d, r).to(BF16), randn(19 * n + d, r, d, dtype=F64)


def mlp_cases():
    """(key, C, W, idx, down) on the host; rank 0 passes idx = down = None."""
    for i, (n, d) in enumerate(MLP_SHAPES):
        C = matrix(KINDS[i % 3], n)[0]
        for wdt in WDTS:
            W = weight(n, d, wdt)
            for r in sorted({0, n, int(0.7 * n)}):
                idx, down, D = mlp_inputs(n, d, r)
                for form, dn in (("bf16", down), ("f64T", D.T)):
                    key = "mlp-n%d-d%d-r%d-%s-%s" % (n, d, r, str(wdt)[6:], form)
                    yield key, C, W, (idx if r else None), (dn if r else None)
                    if (n, d, r, wdt) != (385, 70, int(0.7 * 385), BF16):
                        continue
                    perm = torch.randperm(r, generator=torch.Generator().manual_seed(3))
                    yield key + "-shuffled", C, W, idx[perm], dn[:, perm]
                    bad = idx.clone()
                    bad[5], bad[40] = n + 7, -2          # clamped to n - 1 and 0
                    bad[200] = bad[r - 1] = bad[17]      # one index at three positions
                    yield key + "-badidx", C, W, bad, dn


def vo_cases():
    """(key, C, W_v, W_o, n_heads, n_kv, hd, r, v_new, o_new, want_dnorm2) on the host."""
    for i, (hd, r, d, n_heads, n_kv) in enumerate(VO_SHAPES):
        C = matrix(KINDS[i % 3], d)[0]
        for wdt in WDTS:
            Wv, Wo = randn(41 * d + hd, n_kv * hd, d).to(wdt), randn(43 * d + hd, d, n_heads * hd).to(wdt)
            for fdt in (BF16, F64):
                vn = randn(47 * d + hd, n_kv * r, d).to(fdt) if r else None
                on = randn(53 * d + hd, d, n_heads * r).to(fdt) if r else None
                for want in (True, False):
                    key = "vo-hd%d-r%d-d%d-h%dkv%d-%s-%s-%s" % (hd, r, d, n_heads, n_kv, str(wdt)[6:], str(fdt)[6:],
                                                               "dnorm2" if want else "e")
                    yield key, C, Wv, Wo, n_heads, n_kv, hd, r, vn, on, want


def run(ops, dev):
    """{name: int64 numpy array}: the raw bits of e and unorm2 / dnorm2 of every case."""
    to = lambda t: None if t is None else t.to(dev)                    # noqa: E731
    raw = lambda t: t.cpu().contiguous().view(torch.int64).numpy().copy()      # noqa: E731
    out = {}
    for key, C, W, idx, down in mlp_cases():
        e, u2 = ops.mlp_output_error(to(C), to(W), to(idx), to(down), want_unorm2=True)
        out[key + "/e"], out[key + "/unorm2"] = raw(e), raw(u2)
    for key, C, Wv, Wo, n_heads, n_kv, hd, r, vn, on, want in vo_cases():
        res = ops.vo_output_error(to(C), to(Wv), to(Wo), n_heads, n_kv, hd, r, to(vn), to(on), want_dnorm2=want)
        e, dn = res if want else (res, None)
        out[key + "/e"] = raw(e)
        if want:
            out[key + "/dnorm2"] = raw(dn)
    return out


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}
