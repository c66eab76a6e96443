"""CPU test (-m "not gpu"): the resources of the two kernels of the depth input (csrc/depth_in.hip), read from the shipped code
object's notes as tests/test_kernel_resources.py reads them -- each present once, no scratch, no spills, and the LDS sizes
DESIGN.md section 8.z12 states; the ingest kernel fits two work-groups per CU.  Nothing looks at the instruction stream."""
import os
import re

import pytest

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

INGEST_LDS_BYTES = 39216      # 2 x 144 x 32 floats (the horizontal num and den sums of the source rows under a tile) + 32 x 17 floats
#                               (the tile's x weights) + 32 words (its first taps) + 4 x 3 floats (the waves' min, max, any)
NORMALIZE_LDS_BYTES = 60      # 4 x 3 floats (the waves' min, max, any) + 3 floats (mn, mx - mn, the flat flag)


@pytest.mark.parametrize("name,lds", [("depth_ingest_kernel", INGEST_LDS_BYTES), ("depth_normalize_kernel", NORMALIZE_LDS_BYTES)])
def test_depth_in_kernel_resources(kernels, name, lds):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if name in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == lds
    assert 2 * lds <= 160 * 1024                                    # two work-groups per CU
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z12"):]
    want = rf"{lds // 1000}[ ,]?{lds % 1000:03d} bytes" if lds >= 1000 else rf"\b{lds} bytes"
    assert re.search(want, section), f"DESIGN.md section 8.z12 states the LDS size of {name}"


def test_ingest_kernel_stays_at_or_below_80_kb():
    assert INGEST_LDS_BYTES <= 80 * 1024
    src = open(os.path.join(ROOT, "live2diff_amd", "csrc", "depth_in.hip")).read()
    assert f"static_assert(DI_LDS_BYTES == {INGEST_LDS_BYTES}," in src and f"static_assert(DN_LDS_BYTES == {NORMALIZE_LDS_BYTES}," in src
