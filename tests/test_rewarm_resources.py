"""CPU test (-m "not gpu"): the resources of the sink commit's kernel (csrc/sink_commit.hip), read from the shipped code object's
notes as tests/test_kernel_resources.py reads them -- present once, no scratch, no spills, no LDS.  Nothing looks at the
instruction stream."""
import os

from test_kernel_resources import ROOT, kernels  # noqa: F401  (the module-scoped fixture)


def test_sink_commit_kernel_resources(kernels):  # noqa: F811
    mine = {n: k for n, k in kernels.items() if "sink_commit_kernel" in n}
    assert len(mine) == 1, sorted(mine)
    (full, k), = mine.items()
    print(full, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == 0                             # a copy: no LDS
    assert k["vgpr_count"] <= 64                                          # (4 x 16 bytes in flight per lane and their addresses)


def test_the_header_the_binding_and_the_makefile_name_the_op():
    from live2diff_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "l2d.h")).read()
    assert f"L2D_OP_SINK_COMMIT = {_lib.OP_SINK_COMMIT}," in hdr and _lib.OP_SINK_COMMIT == _lib.OP_MATTE_KEY_GAIN + 1      # the next free number
    assert _lib.ABI_VERSION == 6 and "#define L2D_ABI_VERSION 6" in hdr     # (an added op kind moves neither the ABI nor the pack manifest)
    mk = open(os.path.join(ROOT, "live2diff_amd", "csrc", "Makefile")).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS = ")).split()
    assert "sink_commit.hip" in srcs and "sink_commit" not in mk.replace("sink_commit.hip", "", 1)      # the common flags, no rule of its own
