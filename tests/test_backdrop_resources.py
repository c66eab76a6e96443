"""CPU test (-m "not gpu"): the resources of the backdrop blur kernel (csrc/backdrop.hip), read from the shipped code object's
notes as tests/test_kernel_resources.py reads them -- present once, no scratch, no spills, and the LDS size DESIGN.md section
8.z13 states; it fits two work-groups per CU."""
import os
import re

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

BLUR_LDS_BYTES = 67584      # 4 x 64 x 120 bytes (P[3], W - 1) + 64 x 96 half-words (row sums of W) + 64 x 96 words (row sums of W P[c])


def test_backdrop_kernel_resources(kernels):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if "frame_backdrop_blur_kernel" in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == BLUR_LDS_BYTES
    assert 2 * BLUR_LDS_BYTES <= 160 * 1024                         # two work-groups per CU
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z13"):]
    assert re.search(rf"{BLUR_LDS_BYTES // 1000}[ ,]?{BLUR_LDS_BYTES % 1000:03d} bytes", section), "DESIGN.md section 8.z13 states the LDS size"


def test_blur_kernel_stays_at_or_below_80_kb():
    assert BLUR_LDS_BYTES <= 80 * 1024
    src = open(os.path.join(ROOT, "live2diff_amd", "csrc", "backdrop.hip")).read()
    assert f"static_assert(BD_LDS_BYTES == {BLUR_LDS_BYTES}," in src and "BD_LDS_BYTES <= 80 * 1024" in src
