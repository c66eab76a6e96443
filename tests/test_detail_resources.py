"""CPU test (-m "not gpu"): the resources of the two kernels of the detail mode (csrc/detail.hip), read from the shipped code
object's notes as tests/test_kernel_resources.py reads them -- each present once, no scratch, no spills, and the LDS sizes
DESIGN.md section 8.z10 states; the gain kernel fits two work-groups per CU."""
import os
import re

import pytest

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

GAIN_LDS_BYTES = 79872      # 4 x 48 x 96 bytes (Y, P[3]) + 2 x 48 x 80 words (one set of row sums) + 2 x 32 x 80 words (S_I, S_II) + 32 x 80 words (A)
INJECT_LDS_BYTES = 53760    # 3 x 64 x 65 floats (the gains a tile's taps reach) + 32 x 32 x 3 bytes + 6 x 32 words


@pytest.mark.parametrize("name,lds", [("frame_detail_gain_kernel", GAIN_LDS_BYTES), ("frame_detail_kernel", INJECT_LDS_BYTES)])
def test_detail_kernel_resources(kernels, name, lds):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if name in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == lds
    assert 2 * lds <= 160 * 1024                                    # two work-groups per CU
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z10"):]
    assert re.search(rf"{lds // 1000}[ ,]?{lds % 1000:03d} bytes", section), f"DESIGN.md section 8.z10 states the LDS size of {name}"


def test_gain_kernel_stays_at_or_below_80_kb():
    assert GAIN_LDS_BYTES <= 80 * 1024
    src = open(os.path.join(ROOT, "live2diff_amd", "csrc", "detail.hip")).read()
    assert f"static_assert(DG_LDS_BYTES == {GAIN_LDS_BYTES}," in src and f"static_assert(DT_LDS_BYTES == {INJECT_LDS_BYTES}," in src
