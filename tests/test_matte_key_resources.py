"""CPU test (-m "not gpu"): the resources of the kernels of the matte key (csrc/matte_key.hip), read from the shipped code object's
notes as tests/test_kernel_resources.py reads them -- each present once, no scratch, no spills, and the LDS size the source,
l2d.h and DESIGN.md section 8.z17 state.  Nothing looks at the instruction stream."""
import os
import re

import pytest

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

LDS_BYTES = 13824      # 24 x 80 words (D of a 16 x 64 tile, 4 rows of halo above and below, one 8-pixel group on either side)
#                        + 24 x 64 words (the row sums)
KERNELS = {"matte_key_color_kernel": LDS_BYTES, "matte_key_plate_kernel": LDS_BYTES, "frame_planar_bytes_kernel": 0}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_matte_key_kernel_resources(kernels, name):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if name in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == KERNELS[name]
    assert 4 * LDS_BYTES <= 160 * 1024                              # four work-groups of 128 lanes per CU, and more


def test_the_source_the_header_and_the_design_state_the_size():
    assert LDS_BYTES == (24 * 80 + 24 * 64) * 4
    src = open(os.path.join(ROOT, "live2diff_amd", "csrc", "matte_key.hip")).read()
    assert f"static_assert(MK_LDS_BYTES == {LDS_BYTES}," in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z17"):]
    assert re.search(rf"{LDS_BYTES // 1000}[ ,]?{LDS_BYTES % 1000:03d} bytes", section), "DESIGN.md section 8.z17 states the LDS size"
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    assert re.search(rf"{LDS_BYTES // 1000},{LDS_BYTES % 1000:03d} bytes of LDS", hdr)
