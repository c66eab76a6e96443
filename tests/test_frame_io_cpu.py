"""CPU tests (-m "not gpu") of the frame I/O layer (live2diff_amd/frame_io.py, csrc/frame_io.hip): the geometry rule, the two
reference functions the GPU tests compare the kernels against -- pinned HERE to torch (`ingest_ref`) and to the reference's own
`image_utils.postprocess_image` (`egress_ref`, tests/golden/frame_io.npz) -- and the launchers' argument validation in dry-run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from live2diff_amd import frame_io as FIO

SIX = [((720, 1280), (512, 512)), ((1080, 1920), (512, 768)), ((480, 640), (512, 512)), ((512, 512), (512, 512)),
       ((360, 640), (576, 1024)), ((1280, 720), (512, 512))]
TEN = SIX + [((240, 320), (512, 512)), ((479, 641), (512, 512)), ((2160, 3840), (512, 512)), ((333, 517), (64, 96))]


@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_geometry_is_torchvision_resize_center_crop():
    want = [(512, 910, 0, 199), (512, 910, 0, 71), (512, 682, 0, 85), (512, 512, 0, 0), (576, 1024, 0, 0), (910, 512, 199, 0)]
    for ((Hs, Ws), (H, W)), w in zip(SIX, want):
        assert FIO.geometry(Hs, Ws, H, W) == w
    with pytest.raises(ValueError, match="crop window"):
        FIO.geometry(512, 512, 512, 768)


@pytest.mark.parametrize("src,dst", TEN)
def test_ingest_ref_matches_torch_antialiased_bilinear(src, dst):
    """bound 2e-4 = 2 x the 5.4e-5 measured between the float64 formula and torch on [0, 1] data (the x 2 of the [-1, 1] mapping),
    rounded up; torch's own two-pass fp32 path is the reference side of that number"""
    (Hs, Ws), (H, W) = src, dst
    g = torch.Generator().manual_seed(Hs * 10007 + Ws)
    u8 = torch.randint(0, 256, (1, Hs, Ws, 3), dtype=torch.uint8, generator=g)
    nh, nw, top, left = FIO.geometry(Hs, Ws, H, W)
    ref = F.interpolate(u8.permute(0, 3, 1, 2).float() / 255.0, (nh, nw), mode="bilinear", align_corners=False, antialias=True)
    ref = 2.0 * ref[:, :, top:top + H, left:left + W] - 1.0
    got = FIO.ingest_ref(u8, H, W)
    assert got.dtype == torch.float32 and got.shape == (1, 3, H, W)
    err = (got - ref).abs().max().item()
    print(f"{Hs}x{Ws} -> {H}x{W}: max-abs {err:.3e}")
    assert err <= 2e-4


def test_aa_weights_tap_counts_and_identity():
    xmin, w = FIO.aa_weights(512, 512)
    assert torch.equal(xmin, torch.arange(512)) and torch.equal(w[:, 0], torch.ones(512)) and float(w[:, 1:].abs().max()) == 0.0
    assert FIO.aa_weights(3840, 910)[1].shape[1] <= 10 and FIO.aa_weights(517, 99)[1].shape[1] <= 12
    for n_in, n_out in ((1280, 910), (320, 682), (3840, 910)):
        xmin, w = FIO.aa_weights(n_in, n_out)
        assert torch.allclose(w.sum(1), torch.ones(n_out), atol=1e-6) and int(xmin.min()) == 0
        assert int((xmin + (w > 0).sum(1)).max()) <= n_in


def test_egress_ref_equals_reference_postprocess_bytes(golden):
    g = golden("frame_io")
    x = torch.from_numpy(g["x"])
    assert x.dtype == torch.float16 and (x == 0).any() and (x == 1).any() and (x == -1).any()
    got = FIO.egress_ref(x).numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, g["pil"])
    sx = torch.from_numpy(g["sweep_x"])
    assert sx.numel() > 32000                                   # every finite fp16 in [-2, 2]
    su = FIO.egress_ref(sx.view(1, 1, -1, 1).repeat(1, 3, 1, 1)).numpy()[0, :, 0, :]
    assert np.array_equal(su, np.repeat(g["sweep_u8"][:, None], 3, 1))
    i0 = int(np.nonzero(g["sweep_x"] == 0)[0][0])
    assert g["sweep_u8"][i0] == 128                            # the tie 127.5 rounds to even


def test_op_codes_are_appended_and_abi_unchanged():
    from live2diff_amd import _lib
    assert _lib.OP_FRAME_INGEST == 34 and _lib.OP_FRAME_EGRESS == 35 and _lib.ABI_VERSION == 6
    assert _lib.lib.l2d_abi_version() == 6


@pytest.mark.parametrize("B", [1, 8])
def test_plans_validate_in_dry_run(dry_run, B):
    from live2diff_amd import ops
    for (Hs, Ws), (H, W) in SIX:
        nh, nw, top, left = FIO.geometry(Hs, Ws, H, W)
        src = torch.zeros(B, Hs, Ws, 3, dtype=torch.uint8)
        x = torch.zeros(B, 3, H, W, dtype=torch.float16)
        out = torch.zeros(B, H, W, 3, dtype=torch.uint8)
        ops.run(ops.frame_ingest(src, x, B=B, Hs=Hs, Ws=Ws, H=H, W=W, nh=nh, nw=nw, top=top, left=left))
        ops.run(ops.frame_egress(x, out, B=B, H=H, W=W))


def test_launchers_reject_what_the_kernels_cannot_do(dry_run):
    from live2diff_amd import ops
    from live2diff_amd._lib import L2DError
    src = torch.zeros(1, 64, 64, 3, dtype=torch.uint8)
    dst = torch.zeros(4096 * 3 + 64, dtype=torch.float16)
    ok = dict(B=1, Hs=64, Ws=64, H=64, W=64, nh=64, nw=64, top=0, left=0)
    ops.run(ops.frame_ingest(src, dst, **ok))

    def bad(match, d=dst, **kw):
        with pytest.raises(L2DError, match=match):
            ops.run(ops.frame_ingest(src, d, **{**ok, **kw}))

    bad("scale", Hs=4096, Ws=4096, nh=256, nw=256, H=256, W=256)            # 16 x: 33 taps
    bad("scale", Ws=580, nw=72, W=72)                                       # one axis is enough (8.06)
    bad("multiple of 8", W=60, nw=60)
    bad("16-byte aligned", d=dst[1:])
    bad("2\\^31", B=8, Hs=8192, Ws=16384, nh=8192, nw=16384)
    bad("crop window", top=1)
    bad("crop window", left=-1)
    bad("crop window", nw=56)
    with pytest.raises(L2DError, match="multiple of 16"):
        ops.run(ops.frame_egress(dst, torch.zeros(8 * 9 * 3, dtype=torch.uint8), B=1, H=9, W=8))
    with pytest.raises(L2DError, match="16-byte aligned"):
        ops.run(ops.frame_egress(dst[1:], torch.zeros(64 * 64 * 3, dtype=torch.uint8), B=1, H=64, W=64))


def test_frame_processor_routes_uint8_and_float(monkeypatch):
    """uint8 goes to the ingest (here a recording stand-in: no device), float tensors take `_ImageProcessor(assume_unit_range=True)`
    -- no `.min()` probe, so a non-negative [-1, 1]-looking frame is not what decides the mapping"""
    calls = []

    class IO:
        height, width = 8, 16

        def ingest(self, frame):
            calls.append(frame)
            return "ingested"

    fp = FIO.FrameProcessor(IO())
    assert fp.preprocess(np.zeros((4, 4, 3), np.uint8), 8, 16) == "ingested"
    assert fp.preprocess(torch.zeros(4, 4, 3, dtype=torch.uint8), 8, 16) == "ingested" and len(calls) == 2
    x = torch.rand(3, 8, 16)
    assert torch.equal(fp.preprocess(x, 8, 16), (2.0 * x - 1.0)[None])
    y = torch.rand(3, 8, 16) * 0.5 + 0.5                                    # bright: every value >= 0.5
    assert torch.equal(fp.preprocess(y, 8, 16), (2.0 * y - 1.0)[None])
    assert torch.equal(FIO._PassThrough.preprocess(x, 8, 16), x[None])
