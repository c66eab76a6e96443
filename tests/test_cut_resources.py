"""CPU test (-m "not gpu"): the resources of the kernels of the cut detector (L2D_OP_FRAME_CUT_SIG and L2D_OP_FRAME_CUT,
csrc/cut.hip), read from the shipped code object's notes as tests/test_matte_key_gain_resources.py reads them -- each present once,
no scratch, no spills, and the LDS sizes the header and DESIGN.md section 8.z21 state.  Each op has two kernels, its compile-time
INIT and compared variants.  Nothing looks at the instruction stream."""
import os
import re

import pytest

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

SIG_LDS = 272          # a partial as it is stored: 64 counts, the share of Dt, three zeros
CUT_LDS = 1056         # 4 x 64 partial sums of the bins and four 64-bit partial sums of Dt
KERNELS = {"frame_cut_sig_init_kernel": SIG_LDS, "frame_cut_sig_diff_kernel": SIG_LDS, "frame_cut_init_kernel": CUT_LDS,
           "frame_cut_decide_kernel": CUT_LDS}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_cut_kernel_resources(kernels, name):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if name in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == KERNELS[name]


def test_the_names_are_new(kernels):  # noqa: F811
    assert len([n for n in kernels if "frame_cut" in n]) == len(KERNELS)


def test_the_header_and_the_design_state_the_sizes():
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z21"):]
    for head, size in ((" * L2D_OP_FRAME_CUT_SIG  one launch", SIG_LDS), (" * L2D_OP_FRAME_CUT  one launch", CUT_LDS)):
        record = hdr[hdr.index(head):]
        record = record[:min(record.index("*/"), record.index("\n * L2D_", 4) if "\n * L2D_" in record[4:] else len(record))]
        text = f"{size // 1000},{size % 1000:03d}" if size >= 1000 else str(size)
        assert re.search(rf"\b{text} bytes of LDS", record), head
        assert re.search(rf"\b{size // 1000}[ ,]?{size % 1000:03d} bytes" if size >= 1000 else rf"\b{size} bytes", section), \
            f"DESIGN.md section 8.z21 states {size}"
