"""CPU test (-m "not gpu"): the resources of the two follow kernels (csrc/steady_follow.hip), read from the shipped code object's
notes as tests/test_kernel_resources.py reads them -- each present once, no scratch, no spills, and the LDS sizes DESIGN.md
section 8.z14 and the source's static_asserts state."""
import os
import re

import pytest

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

MOTION_LDS_BYTES = 14104    # 3 x 16 x 72 (now) + 3 x 32 x 88 + 8 (prev with the search margin) + 256 keys x 4 + 2 x 292 half-words (ranks)
FOLLOW_LDS_BYTES = 6656     # 32 x 80 bytes (d of the tile and its halo) + 32 x 64 half-words (row sums): the steady box kernel's


@pytest.mark.parametrize("name,lds", [("frame_motion_kernel", MOTION_LDS_BYTES), ("frame_steady_follow_kernel", FOLLOW_LDS_BYTES)])
def test_follow_kernel_resources(kernels, name, lds):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if name in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == lds
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z14"):]
    assert re.search(rf"{lds // 1000}[ ,]?{lds % 1000:03d} bytes", section), "DESIGN.md section 8.z14 states the LDS size"


def test_sizes_are_asserted_in_the_source():
    src = open(os.path.join(ROOT, "live2diff_amd", "csrc", "steady_follow.hip")).read()
    assert f"#define MF_LDS_BYTES {MOTION_LDS_BYTES}\n" in src and "static_assert(sizeof(mf_lds) == MF_LDS_BYTES," in src
    assert f"static_assert(FL_LDS_BYTES == {FOLLOW_LDS_BYTES}," in src
    assert 8 * MOTION_LDS_BYTES <= 160 * 1024                  # LDS leaves room for eight work-groups of either kernel per CU
