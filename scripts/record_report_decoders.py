"""Record tests/golden/report_decoders.json: inputs and returned dicts of the host-side report decoders (decode_margin,
decode_rank_curve, decode_output_error, decode_qk_margin, decode_qk_logit_error, decode_vo_spectrum, decode_vo_output_error) on
ordinary and degenerate inputs.  The decoders are taken from modegpt_amd.ops of PYTHONPATH if one is there (a checkout of the commit
whose behaviour is to be pinned), else of this tree.  tests/test_reports_host.py replays the file; non-finite numbers are written as
json's NaN / Infinity.

    PYTHONPATH=/path/to/parent python scripts/record_report_decoders.py [--out tests/golden/report_decoders.json]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)                      # (behind PYTHONPATH)

from modegpt_amd import ops  # noqa: E402

NAN, INF = float("nan"), float("inf")


def cases():
    rnd = random.Random(20260)
    pos = lambda k, lo=0.1, hi=2.0: [rnd.uniform(lo, hi) for _ in range(k)]          # noqa: E731
    rows = lambda r, k, lo=0.1, hi=2.0: [pos(k, lo, hi) for _ in range(r)]            # noqa: E731

    def falling(n, top=50.0, last=0.0):
        v = sorted((rnd.uniform(0.0, top) for _ in range(n - 1)), reverse=True)
        return [top] + v + [last]            # n + 1 numbers

    def poke(v, i, x):
        v = [list(r) if isinstance(r, list) else r for r in v]
        if isinstance(i, tuple):
            v[i[0]][i[1]] = x
        else:
            v[i] = x
        return v

    # ---- decode_margin
    m8 = [0.8, 1.1, 0.81, 1.09, 0.3, 0.4, 0.0, 1.0]
    yield "decode_margin", [m8, 1e-3], {}
    yield "decode_margin", [poke(m8, 7, 0.0)[:6] + [3.0, 0.0], 1e-2], {}
    yield "decode_margin", [poke(m8, 0, 0.0), 1e-3], {}
    yield "decode_margin", [poke(m8, 0, -INF), 1e-3], {}
    yield "decode_margin", [poke(m8, 1, INF), 0.0], {}
    yield "decode_margin", [poke(poke(m8, 4, 0.0), 5, 0.0), 1e-3], {}
    yield "decode_margin", [poke(m8, 0, NAN), 1e-3], {}

    # ---- decode_rank_curve
    c20 = falling(20)
    for rank in (0, 14, 20):
        yield "decode_rank_curve", [c20, rank], {}
    yield "decode_rank_curve", [falling(7, top=1.0, last=0.5), 3], {}                 # never under the smaller targets
    yield "decode_rank_curve", [[0.0] * 6, 2], {}                                     # zero energy
    yield "decode_rank_curve", [poke(c20, 0, NAN), 5], {}
    yield "decode_rank_curve", [poke(c20, 0, INF), 5], {}
    yield "decode_rank_curve", [poke(c20, 0, -1.0), 5], {}
    yield "decode_rank_curve", [poke(c20, 9, NAN), 9], {}                             # a NaN inside the curve
    yield "decode_rank_curve", [poke(c20, 9, NAN), 12], {}
    yield "decode_rank_curve", [poke(c20, 20, NAN), 12], {}
    yield "decode_rank_curve", [[3.0], 0], {}                                         # n = 0
    yield "decode_rank_curve", [c20, 21], {}
    yield "decode_rank_curve", [c20, -1], {}
    yield "decode_rank_curve", [[], 0], {}

    # ---- decode_output_error
    d = 9
    q, u2 = pos(d, 1.0, 3.0), pos(d, 0.5, 1.0)
    e = [x * rnd.uniform(1e-4, 0.2) for x in q]
    c9 = falling(12, top=30.0)
    yield "decode_output_error", [e, q, u2, 1e-6, 7], {}
    for rank in (0, 7, 12):
        yield "decode_output_error", [e, q, u2, 1e-6, rank], {"curve": c9}
    yield "decode_output_error", [e, [0.0] * d, u2, 1e-6, 7], {"curve": c9}           # zero energy
    yield "decode_output_error", [e, poke(q, 3, 0.0), u2, 1e-6, 7], {}                # one dead channel
    yield "decode_output_error", [poke(e, 2, NAN), q, u2, 1e-6, 7], {"curve": c9}
    yield "decode_output_error", [e, poke(q, 4, INF), u2, 1e-6, 7], {"curve": c9}
    yield "decode_output_error", [e, poke(q, 4, NAN), u2, 1e-6, 7], {}
    yield "decode_output_error", [e, q, poke(u2, 0, NAN), 1e-6, 7], {"curve": c9}
    yield "decode_output_error", [poke(e, 1, -1e-9), q, u2, 0.0, 7], {}               # rounding noise of the other sign
    yield "decode_output_error", [e, q, u2, 1e-6, 7], {"curve": poke(c9, 7, NAN)}
    yield "decode_output_error", [e, q, u2, 1e-6, 7], {"curve": poke(c9, 0, 0.0)}
    yield "decode_output_error", [e, q, u2, 1e-6, 7], {"curve": poke(c9, 0, INF)}
    yield "decode_output_error", [[], [], [], 1e-6, 0], {}
    yield "decode_output_error", [e, q[:-1], u2, 1e-6, 7], {}
    yield "decode_output_error", [e, q, u2, 1e-6, 13], {"curve": c9}

    # ---- decode_qk_margin
    k8 = [[1.4, 0.9, 1.38, 0.93, 0.01, 0.0, 0.0, 1.0], [1.2, 1.19, 1.15, 1.24, 0.05, 3.0, 2.0, 0.0],
          [2.0, 0.5, 1.9, 0.6, 0.02, 0.0, 1.0, 1.0]]
    yield "decode_qk_margin", [k8, 1e-6, 1e-9], {}
    yield "decode_qk_margin", [[k8[0], k8[2]], 1e-6, 0.0], {}
    yield "decode_qk_margin", [[poke(k8[0], 1, -INF), k8[2]], 1e-6, 1e-9], {}         # everything selected: infinite margin
    yield "decode_qk_margin", [[poke(k8[0], 0, INF)], 1e-6, 1e-9], {}                 # nothing selected
    yield "decode_qk_margin", [[poke(k8[1], 0, 0.0)], 1e-6, 1e-9], {}
    yield "decode_qk_margin", [[poke(k8[1], 0, -0.5), k8[0]], 1e-6, 1e-9], {}
    yield "decode_qk_margin", [[poke(k8[0], 0, NAN)], 1e-6, 1e-9], {}
    yield "decode_qk_margin", [[], 1e-6, 1e-9], {}                                    # an empty head list

    # ---- decode_qk_logit_error
    ns, n_kv, group = 8, 2, 2
    cv = [falling(ns, top=40.0) for _ in range(n_kv)]
    chh = [falling(ns, top=20.0) for _ in range(n_kv * group)]
    terms, scale = rows(n_kv, ns, 0.0, 5.0), pos(n_kv, 1e3, 1e4)
    gv = [[x * rnd.uniform(0.5, 1.0) for x in c] for c in cv]
    full = {"terms": terms, "scale": scale, "greedy_curve": gv}
    for rank in (0, 6, 16):
        yield "decode_qk_logit_error", [chh, cv, rank, 2], full
    yield "decode_qk_logit_error", [chh, cv, 6, 2], {}                                # missing optional arguments
    yield "decode_qk_logit_error", [chh, cv, 6, 2], {"terms": terms}
    yield "decode_qk_logit_error", [chh, cv, 6, 2], {"scale": scale}
    yield "decode_qk_logit_error", [chh, cv, 6, 2], {"greedy_curve": gv}
    yield "decode_qk_logit_error", [chh[:2], cv, 5, 1], full                          # OPT: single columns, MHA
    bumpy = poke(cv, (0, 4), cv[0][3] + 1.0)
    yield "decode_qk_logit_error", [chh, bumpy, 6, 2], full                           # a non-monotone curve
    yield "decode_qk_logit_error", [chh, poke(cv, (0, 4), cv[0][3] + 1e-13), 6, 2], full      # ... under the noise floor
    yield "decode_qk_logit_error", [chh, poke(cv, (0, 4), cv[0][3] + 1e-13), 6, 2], {"terms": terms}
    yield "decode_qk_logit_error", [chh, [[0.0] * (ns + 1), cv[1]], 6, 2], full       # zero energy in one head
    yield "decode_qk_logit_error", [chh, [[0.0] * (ns + 1)] * 2, 6, 2], full          # ... in the layer
    yield "decode_qk_logit_error", [chh, poke(cv, (1, 0), NAN), 6, 2], full
    yield "decode_qk_logit_error", [chh, poke(cv, (1, 0), INF), 6, 2], full
    yield "decode_qk_logit_error", [chh, poke(cv, (1, 5), NAN), 6, 2], full           # a NaN inside a curve
    yield "decode_qk_logit_error", [chh, poke(cv, (1, 3), NAN), 6, 2], full           # ... at the rank
    yield "decode_qk_logit_error", [poke(chh, (2, 0), 0.0), cv, 6, 2], full
    yield "decode_qk_logit_error", [poke(chh, (2, 3), NAN), cv, 6, 2], full
    yield "decode_qk_logit_error", [chh, cv, 6, 2], {**full, "terms": poke(terms, (0, 6), NAN)}
    yield "decode_qk_logit_error", [chh, cv, 6, 2], {**full, "scale": poke(scale, 1, NAN)}
    yield "decode_qk_logit_error", [chh, cv, 6, 2], {**full, "greedy_curve": poke(gv, (0, 3), INF)}
    yield "decode_qk_logit_error", [chh, cv, 6, 2], {**full, "greedy_curve": poke(gv, (0, 7), NAN)}
    yield "decode_qk_logit_error", [[], [], 0, 2], {}                                 # an empty head list
    yield "decode_qk_logit_error", [chh, cv, 5, 2], full
    yield "decode_qk_logit_error", [chh, cv, 18, 2], full
    yield "decode_qk_logit_error", [chh[:3], cv, 6, 2], full
    yield "decode_qk_logit_error", [chh, cv, 6, 2], {"scale": scale[:1]}

    # ---- decode_vo_spectrum
    s8 = [[2.0, 1.5, 0.25, 0.93, 0.01, 1.0, 9.0, 1e-3], [1.0, 0.99, 0.01, 0.8, 0.02, 0.0, 7.0, 1e-4]]
    yield "decode_vo_spectrum", [s8, 1e-7], {}
    yield "decode_vo_spectrum", [s8[:1], 0.0], {}
    mha = [poke(poke(r, 4, NAN), 5, NAN) for r in s8]                                  # MHA rows: NaN bound, NaN separated
    yield "decode_vo_spectrum", [mha, 1e-7], {}
    yield "decode_vo_spectrum", [[s8[0], mha[1]], 1e-7], {}
    yield "decode_vo_spectrum", [[poke(s8[0], 2, NAN), s8[1]], 1e-7], {}
    yield "decode_vo_spectrum", [[], 1e-7], {}

    # ---- decode_vo_output_error
    n_heads, n_kv, d, hd = 4, 2, 5, 6
    q = rows(n_heads, d, 1.0, 3.0)
    e = [[x * rnd.uniform(1e-5, 0.3) for x in r] for r in q]
    n2 = rows(n_heads, d, 0.1, 1.0)
    cu = [falling(hd, top=25.0) for _ in range(n_kv)]
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, n_kv], {}                     # missing optional arguments
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, n_kv], {"hd": hd}
    for rank in (0, 4, hd):
        yield "decode_vo_output_error", [e, q, n2, 1e-5, rank, n_kv], {"curve": cu}
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, n_kv], {"curve": cu, "hd": 99}
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, 4], {}                        # MHA
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, 1], {"curve": cu[:1]}
    zero = [[0.0] * d for _ in range(n_heads)]
    yield "decode_vo_output_error", [e, zero, n2, 1e-5, 4, n_kv], {"curve": cu}       # zero energy
    yield "decode_vo_output_error", [e, [q[0], q[1], zero[0], zero[1]], n2, 1e-5, 4, n_kv], {"curve": cu}
    yield "decode_vo_output_error", [e, poke(q, (1, 2), 0.0), n2, 1e-5, 4, n_kv], {}
    yield "decode_vo_output_error", [poke(e, (1, 2), NAN), q, n2, 1e-5, 4, n_kv], {"curve": cu}
    yield "decode_vo_output_error", [e, poke(q, (3, 0), INF), n2, 1e-5, 4, n_kv], {"curve": cu}
    yield "decode_vo_output_error", [e, poke(q, (3, 0), NAN), n2, 1e-5, 4, n_kv], {}
    yield "decode_vo_output_error", [e, q, poke(n2, (0, 0), NAN), 1e-5, 4, n_kv], {"curve": cu}
    yield "decode_vo_output_error", [poke(e, (0, 1), -1e-12), q, n2, 0.0, 4, n_kv], {"curve": cu}
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, n_kv], {"curve": poke(cu, (0, 3), NAN)}       # a NaN inside a curve
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, n_kv], {"curve": poke(cu, (1, 0), 0.0)}
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, n_kv], {"curve": poke(cu, (1, 0), INF)}
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, n_kv], {"curve": poke(cu, (0, 2), cu[0][1] + 1.0)}   # not monotone
    yield "decode_vo_output_error", [[], [], [], 1e-5, 0, 1], {}                      # an empty head list
    yield "decode_vo_output_error", [[], [], [], 1e-5, 0, 1], {"curve": [cu[0]]}
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, 3], {}
    yield "decode_vo_output_error", [e, q[:-1], n2, 1e-5, 4, n_kv], {}
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 7, n_kv], {"curve": cu}
    yield "decode_vo_output_error", [e, q, n2, 1e-5, 4, 0], {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "report_decoders.json"))
    a = ap.parse_args()
    out = []
    for fn, args, kwargs in cases():
        rec = {"fn": fn, "args": args, "kwargs": kwargs}
        try:
            rec["result"] = getattr(ops, fn)(*args, **kwargs)
        except Exception as err:           # noqa: BLE001  (the type is what the test pins)
            rec["raises"] = type(err).__name__
        out.append(rec)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("%d cases (%d raise) from %s -> %s (%d bytes)" % (len(out), sum("raises" in r for r in out), os.path.dirname(ops.__file__),
                                                            a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
