"""CPU test (-m "not gpu"): the resources of the kernels of the adaptive plate (L2D_OP_MATTE_KEY_ADAPT, csrc/matte_key.hip), read
from the shipped code object's notes as tests/test_matte_key_resources.py reads them -- each present once, no scratch, no spills,
and the LDS size of L2D_OP_MATTE_KEY, whose tile form they are.  Nothing looks at the instruction stream."""
import os
import re

import pytest

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

LDS_BYTES = 13824      # 24 x 80 words of D + 24 x 64 words of row sums: the update rides along in registers
KERNELS = ("matte_key_adapt_init_kernel", "matte_key_adapt_state_kernel")


@pytest.mark.parametrize("name", KERNELS)
def test_matte_key_adapt_kernel_resources(kernels, name):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if name in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == LDS_BYTES


def test_the_header_and_the_design_state_the_size():
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    record = hdr[hdr.index(" * L2D_OP_MATTE_KEY_ADAPT  one launch"):]
    assert re.search(rf"{LDS_BYTES // 1000},{LDS_BYTES % 1000:03d} bytes of LDS", record[:record.index("*/")])
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z18"):]
    assert re.search(rf"{LDS_BYTES // 1000}[ ,]?{LDS_BYTES % 1000:03d} bytes", section), "DESIGN.md section 8.z18 states the LDS size"
