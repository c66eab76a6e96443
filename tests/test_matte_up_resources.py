"""CPU test (-m "not gpu"): the resources of L2D_OP_FRAME_MATTE_UP's kernel, read from the shipped code object's notes as
tests/test_kernel_resources.py reads them -- no scratch, no spills, and the LDS size DESIGN.md section 8.z7 states."""
import os
import re

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)

LDS_BYTES = 59136        # 2 x 80 x 80 floats (the patch, the horizontal pass) + 32 x 32 floats (M) + 32 x 32 x 3 bytes + 6 x 32 words


def test_matte_up_kernel_resources(kernels):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if "frame_matte_up_kernel" in n}
    assert len(mine) == 1, sorted(mine)
    (name, k), = mine.items()
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == LDS_BYTES
    assert 2 * LDS_BYTES <= 160 * 1024                              # two work-groups per CU
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 8.z7"):]
    assert re.search(r"59[ ,]?136 bytes", section), "DESIGN.md section 8.z7 states the kernel's LDS size"
