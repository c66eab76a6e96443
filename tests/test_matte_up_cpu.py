"""CPU tests (-m "not gpu") of the matte at the output size: `resize.camera_box`, `matte.up_table` /
`matte_up_ref` / `composite_up_ref`, the launchers of L2D_OP_FRAME_MATTE_UP and of the pitched L2D_OP_FRAME_RESIZE in dry run, the
camera buffers of `MatteLine` with a stand-in for the tap, and `set_matte_source` on the wrapper with mock components."""
import numpy as np
import pytest
import torch

from live2diff_amd import matte as MT
from live2diff_amd import resize as R
from live2diff_amd.frame_io import egress_ref


@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


# ----------------------------------------------------------------------------- camera_box
BOXES = [((1080, 1920, 512, 512), (0, 420, 1080, 1080)), ((480, 640, 512, 512), (0, 80, 480, 480)),
         ((720, 1280, 512, 512), (0, 280, 720, 720)), ((1920, 1080, 512, 512), (420, 0, 1080, 1080)),
         ((96, 128, 64, 64), (0, 15, 96, 96)), ((1080, 1920, 384, 640), (0, 59, 1080, 1802))]


@pytest.mark.parametrize("args, want", BOXES)
def test_camera_box_table(args, want):
    assert R.camera_box(*args) == want


def test_camera_box_symmetry_and_containment():
    rng = np.random.default_rng(3)
    seen = 0
    for _ in range(300):
        Hs, Ws = (int(v) for v in rng.integers(48, 2200, 2))
        H, W = (int(v) * 8 for v in rng.integers(4, 96, 2))
        try:
            y0, x0, bh, bw = R.camera_box(Hs, Ws, H, W)
        except ValueError:                       # (a crop window outside the resized image: `frame_io.geometry` refuses it)
            with pytest.raises(ValueError):
                R.camera_box(Ws, Hs, W, H)
            continue
        seen += 1
        assert 1 <= bh <= Hs and 1 <= bw <= Ws and 0 <= y0 <= Hs - bh and 0 <= x0 <= Ws - bw
        assert R.camera_box(Ws, Hs, W, H) == (x0, y0, bw, bh)                # portrait <-> landscape
    assert seen > 50


# ----------------------------------------------------------------------------- up_table, matte_up_ref
def depth_planes(B, H, W, seed=0):
    rng = np.random.default_rng(seed)
    d = (rng.standard_normal((B, H, W)) * 0.6).clip(-1, 1).astype(np.float16)
    d[:, 0, :4] = np.array([-0.4, 0.4, -1.0, 1.0], np.float16)
    if H >= 24 and W >= 32:                      # flat regions wider than the widest box: the matte reaches exactly 1 and 0
        d[:, 1:13, :16], d[:, -12:, -16:] = 1.0, -1.0
    return d


def test_up_table_is_half_pixel_bilinear():
    i0, i1, f = MT.up_table(16, 16)
    assert np.array_equal(i0, np.arange(16)) and np.array_equal(i1, np.minimum(np.arange(16) + 1, 15)) and not f.any()
    i0, i1, f = MT.up_table(4, 8)
    assert i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and i1.tolist() == [0, 1, 1, 2, 2, 3, 3, 3]
    assert f.tolist() == [0.75, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25] and f.dtype == np.float32 and i0.dtype == np.int32
    i0, i1, f = MT.up_table(8, 4)
    assert i0.tolist() == [0, 2, 4, 6] and i1.tolist() == [1, 3, 5, 7] and f.tolist() == [0.5] * 4
    w = MT.table_words(4, 8)
    assert w.dtype == np.int32 and w.shape == (3, 8) and np.array_equal(w[2].view(np.float32), f if len(f) == 8 else MT.up_table(4, 8)[2])


def test_matte_up_ref_identity_constants_and_range():
    d = depth_planes(2, 24, 40)
    for r in (0, 3, 8):
        m = MT.matte_ref(d, 0.3, 0.7, r)
        assert np.array_equal(MT.matte_up_ref(m, 24, 40).view(np.int32), m.view(np.int32))          # bit for bit
    for v in (0.0, 1.0):
        c = np.full((1, 24, 40), v, np.float32)
        assert np.all(MT.matte_up_ref(c, 50, 99) == np.float32(v)) and np.all(MT.matte_up_ref(c, 12, 20) == np.float32(v))
    rng = np.random.default_rng(11)
    for case in range(60):
        H, W = int(rng.integers(8, 48)), int(rng.integers(8, 48))
        Ho = int(rng.integers(-(-H // 2), 8 * H + 1))
        Wo = int(rng.integers(-(-W // 2), 8 * W + 1))
        lo = float(rng.uniform(0, 1))
        hi = float(rng.uniform(lo, 1)) if case % 5 else lo
        m = MT.matte_ref(depth_planes(1, H, W, seed=case), lo, hi, int(rng.integers(0, 9)), "near" if case % 2 else "far")
        M = MT.matte_up_ref(m, Ho, Wo)
        assert M.shape == (1, Ho, Wo) and M.dtype == np.float32 and M.min() >= 0.0 and M.max() <= 1.0, (case, H, W, Ho, Wo)


def test_matte_up_ref_is_close_to_torch_bilinear():
    """a sanity check, not the definition: torch orders its operations differently"""
    import torch.nn.functional as F
    m = MT.matte_ref(depth_planes(2, 24, 40), 0.3, 0.7, 2)
    for Ho, Wo in ((50, 99), (12, 20), (24, 64), (192, 320)):
        t = F.interpolate(torch.from_numpy(m)[None], size=(Ho, Wo), mode="bilinear", align_corners=False)[0].numpy()
        assert np.abs(MT.matte_up_ref(m, Ho, Wo) - t).max() < 2e-6


# ----------------------------------------------------------------------------- composite_up_ref
def test_composite_up_ref_endpoints():
    rng = np.random.default_rng(5)
    d = depth_planes(2, 24, 40)
    S, C = (rng.integers(0, 256, (2, 50, 99, 3), dtype=np.uint8) for _ in range(2))
    assert np.array_equal(MT.composite_up_ref(S, C, d, 0, 0), S) and np.array_equal(MT.composite_up_ref(S, C, d, 0, 0, keep="far"), C)
    for r in (0, 4):
        M = MT.matte_up_ref(MT.matte_ref(d, 0.3, 0.7, r), 50, 99)
        o = MT.composite_up_ref(S, C, d, 0.3, 0.7, r)
        assert (M == 1).any() and (M == 0).any() and len(np.unique(M)) > 16
        assert np.array_equal(o[M == 1], S[M == 1]) and np.array_equal(o[M == 0], C[M == 0])
        show = MT.composite_up_ref(S, C, d, 0.3, 0.7, r, show=True)
        assert np.array_equal(show[..., 0], np.rint(M * np.float32(255)).astype(np.uint8)) and np.array_equal(show[..., 0], show[..., 2])
    with pytest.raises(ValueError):
        MT.composite_up_ref(S, C[:, :49], d, 0.3, 0.7)
    with pytest.raises(ValueError):
        MT.composite_up_ref(S.astype(np.float32), C, d, 0.3, 0.7)


def test_composite_up_ref_at_the_streams_size_is_composite_ref_within_one():
    """at Ho, Wo == H, W with C = egress_ref(source) and S = egress_ref(styled): M is the matte itself, and the two differ only
    in where they round -- 255 (v_c + m (v_s - v_c)) once, against the two frames rounded to bytes first: two half-unit roundings,
    at most 1 in any byte"""
    g = torch.Generator().manual_seed(9)
    styled, source = ((torch.randn(2, 3, 24, 40, generator=g) * 0.7).half() for _ in range(2))
    d = depth_planes(2, 24, 40)
    worst = 0
    for r, keep in ((0, "near"), (3, "far"), (8, "near")):
        a = MT.composite_ref(styled, source, d, 0.3, 0.7, r, keep)
        b = MT.composite_up_ref(egress_ref(styled).numpy(), egress_ref(source).numpy(), d, 0.3, 0.7, r, keep)
        worst = max(worst, int(np.abs(a.astype(int) - b.astype(int)).max()))
    print("largest difference:", worst)
    assert worst <= 1


# ----------------------------------------------------------------------------- the launchers (dry run)
def test_matte_up_launcher_checks(dry_run):
    import os

    from live2diff_amd import _lib, ops
    assert _lib.OP_FRAME_MATTE_UP == 47
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_FRAME_MATTE_UP = 47," in hdr
    B, H, W = 2, 24, 40

    def mk(Ho=60, Wo=33, r=2, H=H, W=W, tx=None, ty=None, lo=0.3, hi=0.7, **kw):
        s, c, o = (torch.zeros(B, Ho, Wo, 3, dtype=torch.uint8) for _ in range(3))
        d = torch.zeros(B, H, W, dtype=torch.float16)
        lo32, inv32, hard = MT.matte_params(lo, hi)
        tx = torch.from_numpy(MT.table_words(W, Wo)) if tx is None else tx
        ty = torch.from_numpy(MT.table_words(H, Ho)) if ty is None else ty
        return ops.frame_matte_up(s, c, d, o, tx, ty, B=B, H=H, W=W, Ho=Ho, Wo=Wo, lo32=lo32, inv32=inv32, hard=hard, r=r, **kw)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    op, _ = mk(far=True, show=True)
    assert [op.i[j] for j in range(7)] == [B, H, W, 60, 33, 2, 6] and op.kind == 47 and op.l[0] == H * W
    for kw in (dict(), dict(Ho=H, Wo=W), dict(Ho=12, Wo=20, r=8), dict(Ho=8 * H, Wo=8 * W, r=0), dict(lo=0.5, hi=0.5)):
        ops.run(mk(**kw))
    # sizes outside check_size
    bad("between half and 8 times", mk(Ho=9 * H))
    bad("between half and 8 times", mk(Wo=19))
    bad("between half and 8 times", mk(Ho=4100, H=1024))
    for r in (-1, 9):
        bad("feather radius", mk(r=r))
    for k in range(6):
        op, keep = mk()
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
    for k in (4, 5):
        op, keep = mk()
        op.p[k] = op.p[k] + 2
        bad(f"table pointer {k} is not 4-byte aligned", (op, keep))
    for k in (0, 1, 3):                                              # (the three frames may start at any byte)
        op, keep = mk()
        op.p[k] = op.p[k] + 1
        ops.run((op, keep))
    op, keep = mk()
    op.i[6] = 8
    bad("unknown flag bits", (op, keep))
    op, keep = mk()
    op.l[0] = H * W - 1
    bad("depth plane stride", (op, keep))
    op, keep = mk()
    op.f[1] = 0.0
    bad("0 exactly when the hard flag is set", (op, keep))
    # the binding's own checks
    with pytest.raises(ValueError, match="contiguous int32 table of 3 x 33"):
        mk(tx=torch.zeros(3 * 34, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous int32 table"):
        mk(ty=torch.zeros(3 * 60, dtype=torch.int64))
    with pytest.raises(AssertionError):
        ops.frame_matte_up(torch.zeros(B, 60, 33, 3, dtype=torch.uint8), torch.zeros(B, 60, 32, 3, dtype=torch.uint8),
                           torch.zeros(B, H, W, dtype=torch.float16), torch.zeros(B, 60, 33, 3, dtype=torch.uint8),
                           torch.from_numpy(MT.table_words(W, 33)), torch.from_numpy(MT.table_words(H, 60)), B=B, H=H, W=W, Ho=60,
                           Wo=33, lo32=0.0, inv32=1.0, hard=False)


def test_pitched_resize_launcher_checks(dry_run):
    from live2diff_amd import _lib, ops
    Hs, Ws = 40, 72
    y0, x0, bh, bw = 3, 5, 33, 61
    frame = torch.zeros(1, Hs, Ws, 3, dtype=torch.uint8)

    def tables(Ho, Wo, bw=bw, bh=bh):
        return torch.from_numpy(R.axis_table(bw, Wo, "lanczos")), torch.from_numpy(R.axis_table(bh, Ho, "lanczos"))

    def mk(pitch=Ws, B=1, src=None, Ho=50, Wo=99, bh=bh, bw=bw):
        src = frame.reshape(-1)[(y0 * Ws + x0) * 3:] if src is None else src
        return ops.frame_resize(src, torch.zeros(B, Ho, Wo, 3, dtype=torch.uint8), *tables(Ho, Wo, bw, bh), B=B, H=bh, W=bw, Ho=Ho, Wo=Wo,
                                src_pitch=pitch)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    op, _ = mk()
    assert op.i[8] == Ws and [op.i[j] for j in (0, 1, 2, 5)] == [1, bh, bw, 1]
    ops.run(mk())
    ops.run(mk(pitch=bw, src=torch.zeros(bh * bw * 3, dtype=torch.uint8)))
    for pitch in (None, 0):                                          # today's record: the integer stays 0
        op, _ = mk(pitch=pitch, src=torch.zeros(1, bh, bw, 3, dtype=torch.uint8))
        assert op.i[8] == 0
        ops.run((op, _))
    bad("row pitch", mk(pitch=bw - 1, src=torch.zeros(bh * bw * 3, dtype=torch.uint8)))
    bad("row pitch", mk(pitch=Ws, B=2, src=torch.zeros(2 * Hs * Ws * 3, dtype=torch.uint8)))
    op, keep = mk(src=torch.zeros(Hs * Ws * 3, dtype=torch.uint8))
    op.i[5] = 0                                                      # an fp16 source
    bad("row pitch", (op, keep))
    # the size assertion follows (H - 1) pitch + W: a window that touches the bottom right corner fits, one row more does not
    tail = frame.reshape(-1)[((Hs - bh) * Ws + (Ws - bw)) * 3:]
    ops.run(mk(src=tail))
    with pytest.raises(AssertionError):
        mk(src=tail, bh=bh + 1)
    with pytest.raises(AssertionError):
        mk(src=frame.reshape(-1)[((Hs - bh) * Ws + (Ws - bw) + 1) * 3:])


def test_camera_tap_builds_plans_and_refuses_a_geometry(dry_run):
    tap = R.CameraTap(64, 64, 80, 112, "lanczos", device="cpu")
    frames = [torch.zeros(1, 96, 128, 3, dtype=torch.uint8) for _ in range(2)]
    tap(frames[0])
    assert tap.box == (0, 15, 96, 96) and tap.pending is not None and tuple(tap.pending.data.shape) == (80, 112, 3)
    assert tap.pending.key == (80, 112, "lanczos") and tap.allocated == 1
    first = tap.pending
    tap(frames[1])                                                   # nobody claimed the buffer: the next ingest overwrites it
    assert tap.pending is first and tap.allocated == 1 and not tap.free
    for _ in range(3):
        for f in frames:
            tap(f)
    assert tap.allocated == 1 and 1 <= len(tap._plans) <= tap.MAX_PLANS
    tap.prepare(48, 64)                                              # another camera: new tables, the buffers stay
    assert tap.box == R.camera_box(48, 64, 64, 64) and tap.pending is first
    with pytest.raises(ValueError, match="output size"):
        R.CameraTap(64, 64, 80, 112, device="cpu").prepare(1080, 1920)       # a 1080-pixel window to 80 lines: below 1/2
    other = R.CameraBuffer(torch.zeros(8, 8, 3, dtype=torch.uint8), (8, 8, "lanczos"))
    tap.give_back(other)
    assert not tap.free                                              # a buffer of another output size is not pooled


# ----------------------------------------------------------------------------- MatteLine and the camera buffers
class FakeTap:
    """what `MatteLine.camera_source` needs: `pending` and `give_back`; `ingest()` plays the tap's call inside `HipFrameIO.ingest`"""

    def __init__(self):
        self.pending, self.free, self.allocated, self.n = None, [], 0, 0

    def ingest(self):
        if self.pending is not None:
            self.free.append(self.pending)
        if self.free:
            buf = self.free.pop()
        else:
            buf, self.allocated = {}, self.allocated + 1
        buf["frame"] = self.n
        self.n += 1
        self.pending = buf
        return buf

    def give_back(self, buf):
        self.free.append(buf)


def line_and_tap(n, H=4, W=8):
    line, tap = MT.MatteLine(n, H, W), FakeTap()
    line.camera_source = tap
    return line, tap, torch.zeros(1, 3, H, W, dtype=torch.float16), torch.zeros(1, 3, H, W, dtype=torch.float16)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_matte_line_moves_camera_buffers(n):
    line, tap, x, dn = line_and_tap(n)
    line.prime(x, dn)                                                # (no frame was ingested: the warm-up position has no buffer)
    assert all(s.camera is None for s in line.slots)
    allocated = []
    for t in range(12):
        buf = tap.ingest()
        line(x, dn)
        assert tap.pending is None                                   # ownership moved, nothing was copied
        slot = line.take()
        want = t - (n - 1)
        assert (slot.camera is None) if want < 0 else (slot.camera["frame"] == want), (t, slot.camera)
        assert line.last is slot
        allocated.append(tap.allocated)
    assert allocated[-1] == allocated[n + 2] <= len(line.slots) + 1  # the pool stops growing: one per slot, one pending
    assert len(line.slots) <= n + 1


def test_matte_line_dropped_frame_last_prime_and_push_depth():
    n = 2
    line, tap, x, dn = line_and_tap(n)
    tap.ingest()                                                     # the last warm-up frame came through the tap
    line.prime(x, dn)
    primed = line.slots[line._hist[0]].camera
    assert primed == {"frame": 0} and tap.pending is None
    tap.ingest(); line(x, dn)                                        # frame 1
    assert line.take().camera is primed                              # the warm-up position keeps its buffer
    # a dropped frame: ingested, never tapped; its buffer goes to the next frame and no slot shifts
    dropped = tap.ingest()
    assert line.last.camera is primed and tap.pending is dropped
    tap.ingest(); line(x, dn)                                        # frame 3 reuses the dropped frame's buffer
    slot = line.take()
    assert slot.camera["frame"] == 1 and line.last is slot
    newest = line.slots[line._hist[-1]].camera
    assert newest is dropped and newest["frame"] == 3
    # `last` keeps its buffer while later frames are stored
    keep = line.last.camera
    for _ in range(4):
        tap.ingest(); line(x, dn)
    assert line.last.camera is keep and keep["frame"] == 1
    # push depth 2: two frames tapped before the first is taken; the pool settles
    line, tap, x, dn = line_and_tap(n)
    line.prime(x, dn)
    tap.ingest(); line(x, dn)
    tap.ingest(); line(x, dn)
    counts = []
    for t in range(10):
        tap.ingest(); line(x, dn)
        slot = line.take()
        assert (slot.camera is None) if t < n - 1 else slot.camera["frame"] == t - (n - 1)
        counts.append(tap.allocated)
    assert counts[-1] == counts[4] <= len(line.slots) + 1            # a slot holds one buffer at the most; one is pending
    # a frame that was not ingested on the device leaves the slot without a buffer; without a source nothing is taken
    line(x, dn)
    assert line.slots[line._hist[-1]].camera is None
    line.camera_source = None
    tap.ingest(); line(x, dn)
    assert line.slots[line._hist[-1]].camera is None and tap.pending is not None
    line.drop_cameras()
    assert all(s.camera is None for s in line.slots)


# ----------------------------------------------------------------------------- the wrapper on the mock components
def test_wrapper_matte_source_arguments_and_state(monkeypatch):
    import pipeline_mocks as M
    from test_resize_cpu import build, call, noise_frame, out_size
    w = build(monkeypatch)
    assert w.matte_source == "stream"
    for bad in ("Camera", "host", None, 1, ""):
        with pytest.raises(ValueError, match="'stream' or 'camera'"):
            w.set_matte_source(bad)
    assert w.matte_source == "stream"
    with pytest.raises(ValueError, match="'stream' or 'camera'"):
        build(monkeypatch, matte_source="source")
    w = build(monkeypatch, matte_source="camera", output_size=out_size())
    assert w.matte_source == "camera" and w._camera is None                  # no device: nothing is installed
    w.set_matte(0.3, 0.7, feather=2)
    assert w.matte == dict(lo=0.3, hi=0.7, keep="near", feather=2, show=False)
    assert w.output_size == dict(height=out_size()[0], width=out_size()[1], resample="lanczos")
    assert w._camera is None and w._matte_line.camera_source is None
    w.set_matte_source("stream")
    w.set_matte_source("camera")
    w.clear_matte()
    w.clear_output_size()
    assert w.matte_source == "camera" and w._camera is None and w._matte_up is None and w._matte_line is None
    torch.manual_seed(123)
    w.prepare(M.frames(8, seed=7), "a prompt")
    assert call(w, noise_frame(0)).shape == (M.H, M.W, 3)


def test_wrapper_float_frames_take_the_stream_route(monkeypatch):
    """the host route, float frames: "camera" changes no byte, for every served output type"""
    from test_resize_cpu import call, noise_frame, pair

    def setup(source):
        def f(w):
            w.set_matte(0.3, 0.7, feather=2)
            w.set_matte_source(source)
        return f

    a, _ = pair(monkeypatch, setup("camera"))
    b, _ = pair(monkeypatch, setup("stream"))
    assert (a.matte_source, b.matte_source) == ("camera", "stream")
    for i, ot in enumerate(("u8", "pil", "jpeg", "u8")):
        a.output_type = b.output_type = ot
        if i == 3:
            a.set_matte_source("stream"), b.set_matte_source("camera")       # (and changed between two frames)
        x, y = call(a, noise_frame(i)), call(b, noise_frame(i))
        assert (np.array_equal(np.asarray(x), np.asarray(y)) if ot != "jpeg" else x == y), ot


def test_wrapper_installs_and_removes_the_tap():
    """`_sync_camera` alone, on a stand-in with a device route: installed while all three are set, rebuilt for a new size, gone
    -- buffers included -- when any of them goes"""
    from types import SimpleNamespace

    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    w = Wrapper.__new__(Wrapper)
    w.output_type, w.height, w.width, w.batch_size = "u8", 64, 64, 2
    w.io = SimpleNamespace(device=torch.device("cpu"), camera_tap=None)
    w.stream = SimpleNamespace(device="cpu", matte_tap=None)
    w.set_matte_source("camera")
    w.set_output_size(80, 112)
    assert w._camera is None and w.io.camera_tap is None
    w.set_matte(0.3, 0.7)
    tap = w._camera
    assert tap is not None and w.io.camera_tap is tap and w._matte_line.camera_source is tap and tap.key == (80, 112, "lanczos")
    w.set_matte(0.2, 0.8, feather=3)
    assert w._camera is tap                                          # the matte's settings do not rebuild it
    w._matte_line.slots.append(SimpleNamespace(camera=R.CameraBuffer(torch.zeros(80, 112, 3, dtype=torch.uint8), tap.key)))
    assert w._camera_slot(w._matte_line.slots[0], torch.zeros(1)) is False   # (a host tensor takes the stream route)
    w.set_output_size(96, 96, "bicubic")
    assert w._camera is not tap and w._camera.key == (96, 96, "bicubic") and w.io.camera_tap is w._camera
    assert w._matte_line.slots[0].camera is None                     # buffers of the old size are dropped
    line = w._matte_line
    for off, on in ((w.clear_output_size, lambda: w.set_output_size(96, 96)), (lambda: w.set_matte_source("stream"),
                                                                               lambda: w.set_matte_source("camera"))):
        line.slots[0].camera = R.CameraBuffer(torch.zeros(96, 96, 3, dtype=torch.uint8), w._camera.key)
        off()
        assert w._camera is None and w.io.camera_tap is None and line.camera_source is None and line.slots[0].camera is None
        assert w._matte_up is None
        on()
        assert w._camera is not None and w.io.camera_tap is w._camera
    w.clear_matte()
    assert w._camera is None and w.io.camera_tap is None and w._matte_line is None and w.stream.matte_tap is None
