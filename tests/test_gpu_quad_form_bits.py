"""The raw bits of mdg_mlp_output_error and mdg_vo_output_error against tests/golden/quad_form_bits.npz, which
scripts/record_quad_form_bits.py recorded with the commit before the two kernels were folded into csrc/quad_form.hpp: every e, unorm2
and dnorm2 of tests/quad_form_cases.py (a single element, a ragged stage, one column past a tile edge, two row blocks, three and five
tile columns; ranks 0, n, 0.7 n; bf16 and fp32-widened weights; bf16 and fp64 replacement tensors; a shuffled, a repeated and an
out-of-range index; V/O with one and two tile columns, r = 0, dnorm2 on and off) must come out bit for bit.  The build contracts
floating-point expressions (-ffp-contract=fast), so a restructured epilogue shows here first."""
import os

import pytest
import torch

from tests import quad_form_cases as QF

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_form_bits.npz")


def test_bits_match_the_recording(dev):
    from modegpt_amd import ops
    want = QF.load(GOLDEN)
    got = QF.run(ops, dev)
    assert sorted(got) == sorted(want)
    assert sum(k.startswith("mlp-") for k in got) >= 2 * 72 and sum(k.startswith("vo-") for k in got) >= 36
    differ = [k for k in sorted(got) if not torch.equal(torch.from_numpy(got[k]), torch.from_numpy(want[k]))]
    print("QUAD FORM BITS: %d arrays, %d differ %s" % (len(got), len(differ), differ[:8]))
    assert not differ, "%d of %d arrays differ from the recording: %s" % (len(differ), len(got), differ[:8])
