"""Record tests/golden/quad_form_bits.npz: the raw bits of mdg_mlp_output_error and mdg_vo_output_error on the cases of
tests/quad_form_cases.py, one GPU.  modegpt_amd is imported from PYTHONPATH if it is there (a built checkout of the commit whose bits
are to be pinned), else from this tree; the cases always come from this tree.

    PYTHONPATH=/path/to/built/parent python scripts/record_quad_form_bits.py [--out tests/golden/quad_form_bits.npz]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)                      # (behind PYTHONPATH)

from modegpt_amd import ops  # noqa: E402
from tests import quad_form_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "quad_form_bits.npz"))
    a = ap.parse_args()
    out = quad_form_cases.run(ops, torch.device("cuda:0"))
    torch.cuda.synchronize()
    np.savez_compressed(a.out, **out)
    print("%d arrays from %s -> %s (%d bytes)" % (len(out), os.path.dirname(ops.__file__), a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
