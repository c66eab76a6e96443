"""CPU test (-m "not gpu"): the resources of the three kernels of the mask ingest (csrc/mask_in.hip), read from the shipped code
object's notes as tests/test_kernel_resources.py reads them -- each present once, no scratch, no spills, and the LDS size the
source and DESIGN.md section 8.z16 state.  Nothing looks at the instruction stream."""
import os
import re

import pytest

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

LDS_BYTES = 20736      # 144 x 32 floats (the horizontal sums of the source rows under a tile) + 32 x 17 floats (the tile's x weights)
#                        + 32 words (its first taps)


@pytest.mark.parametrize("name", ["mask_ingest_u8_kernel", "mask_ingest_u16_kernel", "mask_ingest_f32_kernel"])
def test_mask_ingest_kernel_resources(kernels, name):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if name in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == LDS_BYTES
    assert 2 * LDS_BYTES <= 160 * 1024                              # two work-groups per CU, and more


def test_the_source_and_the_design_state_the_size():
    assert LDS_BYTES == (144 * 32 + 32 * 17 + 32) * 4
    src = open(os.path.join(ROOT, "live2diff_amd", "csrc", "mask_in.hip")).read()
    assert f"static_assert(MI_LDS_BYTES == {LDS_BYTES}," in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z16"):]
    assert re.search(rf"{LDS_BYTES // 1000}[ ,]?{LDS_BYTES % 1000:03d} bytes", section), "DESIGN.md section 8.z16 states the LDS size"
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    assert re.search(rf"{LDS_BYTES // 1000},{LDS_BYTES % 1000:03d} bytes of LDS", hdr)
