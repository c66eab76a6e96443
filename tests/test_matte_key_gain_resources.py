"""CPU test (-m "not gpu"): the resources of the kernels of the plate gain (L2D_OP_MATTE_KEY_GAIN_HIST, L2D_OP_MATTE_KEY_GAIN and
L2D_MATTE_KEY_GAIN on ops 59 / 61, csrc/matte_key.hip), read from the shipped code object's notes as
tests/test_matte_key_resources.py reads them -- each present once, no scratch, no spills, and the LDS sizes the header and
DESIGN.md section 8.z19 state.  The histogram op has two kernels, its compile-time PLATE and STATE variants.  Nothing looks at the
instruction stream."""
import os
import re

import pytest

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

HIST_LDS = 6144        # 3 x 512 counts
MEDIAN_LDS = 6144      # 3 x 512 running sums, scanned in place
KEY_LDS = 13824        # L2D_OP_MATTE_KEY's: the gain rides along in registers
KERNELS = {"matte_gain_hist_plate_kernel": HIST_LDS, "matte_gain_hist_state_kernel": HIST_LDS, "matte_gain_median_kernel": MEDIAN_LDS,
           "matte_gain_key_plate_kernel": KEY_LDS, "matte_gain_key_init_kernel": KEY_LDS, "matte_gain_key_state_kernel": KEY_LDS}
BEFORE = ("matte_key_color_kernel", "matte_key_plate_kernel", "matte_key_adapt_init_kernel", "matte_key_adapt_state_kernel",
          "frame_planar_bytes_kernel")


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_matte_key_gain_kernel_resources(kernels, name):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if name in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == KERNELS[name]


def test_no_new_name_holds_an_older_one(kernels):  # noqa: F811
    for old in BEFORE:
        assert not any(old in new for new in KERNELS), old
        assert len([n for n in kernels if old in n]) == 1, old


def test_the_header_and_the_design_state_the_sizes():
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z19"):]
    for head, size in ((" * L2D_OP_MATTE_KEY_GAIN_HIST  one launch", HIST_LDS), (" * L2D_OP_MATTE_KEY_GAIN  one launch", MEDIAN_LDS),
                       (" * L2D_MATTE_KEY_GAIN on L2D_OP_MATTE_KEY", KEY_LDS)):
        record = hdr[hdr.index(head):]
        record = record[:min(record.index("*/"), record.index("\n * L2D_", 4) if "\n * L2D_" in record[4:] else len(record))]
        assert re.search(rf"{size // 1000},{size % 1000:03d} bytes of LDS", record), head
        assert re.search(rf"{size // 1000}[ ,]?{size % 1000:03d} bytes", section), f"DESIGN.md section 8.z19 states {size}"
