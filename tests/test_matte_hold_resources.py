"""CPU test (-m "not gpu"): the resources of the matte hold's kernels (csrc/matte_hold.hip), read from the shipped code object's
notes as tests/test_kernel_resources.py reads them -- each variant present once, no scratch, no spills, and the LDS size DESIGN.md
section 8.z15 and the source's static_assert state."""
import os
import re

import pytest

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

HOLD_LDS_BYTES = 6656       # 32 x 80 bytes (d of the tile and its halo) + 32 x 64 half-words (row sums): the steady box kernel's
VARIANTS = ["frame_hold_depth_kernel", "frame_hold_plane_kernel", "frame_hold_depth_follow_kernel", "frame_hold_plane_follow_kernel"]


@pytest.mark.parametrize("name", VARIANTS)
def test_hold_kernel_resources(kernels, name):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if name in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == HOLD_LDS_BYTES
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z15"):]
    assert re.search(rf"{HOLD_LDS_BYTES // 1000}[ ,]?{HOLD_LDS_BYTES % 1000:03d} bytes", section), "DESIGN.md section 8.z15 states the LDS size"


def test_variants_and_size_are_stated_in_the_source(kernels):  # noqa: F811
    assert sorted(n for n in kernels if "frame_hold_" in n) == sorted(n for n in kernels if any(v in n for v in VARIANTS))
    assert sum("frame_hold_" in n for n in kernels) == len(VARIANTS)
    src = open(os.path.join(ROOT, "live2diff_amd", "csrc", "matte_hold.hip")).read()
    assert f"static_assert(MH_LDS_BYTES == {HOLD_LDS_BYTES}," in src and "static_assert(sizeof(dd) + sizeof(hh) == MH_LDS_BYTES," in src
    assert 8 * HOLD_LDS_BYTES <= 160 * 1024                   # LDS leaves room for eight work-groups per CU
    make = open(os.path.join(ROOT, "live2diff_amd", "csrc", "Makefile")).read()
    assert "matte_hold.o matte_hold.probes.o: CXXFLAGS += -ffp-contract=off" in make
    assert re.search(r"^steady\.o .*matte_hold\.o .*: steady_px\.h$", make, re.M)
