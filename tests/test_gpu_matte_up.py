"""-m gpu: the matte at the output size.  L2D_OP_FRAME_MATTE_UP (csrc/matte.hip) against
`matte.composite_up_ref` and the pitched L2D_OP_FRAME_RESIZE against `resize.resize_ref` of the window, on every byte and behind
guard bytes; and `set_matte_source("camera")` on the wrapper with small native components against a twin wrapper's plain bytes."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64

# the geometries of tests/test_gpu_resize.py, for the reasons listed there: smaller than a tile with one axis skipped; the 8x
# limit; a batch with non-integer ratios, rows of 297 bytes and no axis a whole number of tiles; the 1/2 limit (the widest
# patch: 64 + 2 r columns); one axis down and one nearly unchanged
GEOMETRIES = [((1, 16, 16), (17, 16)), ((1, 16, 16), (128, 128)), ((3, 40, 72), (100, 99)), ((1, 24, 136), (12, 68)),
              ((2, 64, 96), (33, 95))]
RAMPS = {"soft": (0.3, 0.7), "hard": (0.5, 0.5)}
# (geometry, feather, keep, ramp, show): every feather on every geometry; far, the hard step and `show` each on geometries with
# partial tiles (all but the second).  Feather 8 on the 16-pixel image: the halo leaves the image on both sides.
CASES = [(g, r, "near", "soft", False) for g in range(5) for r in (0, 3, 8)] + [
    (0, 3, "far", "soft", False), (2, 8, "far", "soft", False), (3, 3, "far", "soft", False), (4, 8, "far", "hard", False),
    (2, 3, "near", "hard", False), (2, 0, "near", "hard", False), (2, 3, "near", "soft", True), (4, 0, "far", "soft", True)]


@functools.lru_cache(maxsize=None)
def depth(B, H, W, r):
    """depth N(0, 0.6) clipped, with the values of tests/test_gpu_matte.py planted in the middle rows -- lo_d and hi_d of both
    ramps (-0.4, 0.4, 0 as fp16), their fp16 neighbours, -1, +1, subnormals -- and two flat blocks, -1 in the top right corner
    and +1 in the bottom left one, of r + 2 pixels: every tap of the corner outputs then sees a window of one value, so M
    reaches exactly 0 and exactly 1 there (not at 16 pixels with r = 8: see `exact_ends`)"""
    g = torch.Generator().manual_seed(100 * H + W)
    d = (torch.randn(B, H, W, generator=g) * 0.6).clamp(-1, 1).half()
    dplant = torch.tensor([-0.4, 0.4, 0.0, -1.0, 1.0, -0.39990234375, 0.400146484375, 6e-8, -6e-8], dtype=torch.float16)
    k = min(r + 2, H // 2 - 1, W // 2 - 1)
    for b in range(B):
        d[b, H // 2, 2:2 + len(dplant)] = dplant
        d[b, H // 2 - 1, -len(dplant):] = dplant
        d[b, :k, W - k:] = -1.0
        d[b, H - k:, :k] = 1.0
    return d


def exact_ends(H, W, r):
    """can M be exactly 0 somewhere and exactly 1 elsewhere?  Every (2r+1)^2 window of an image no larger than 2r + 1 holds the
    image's centre, so at 16 x 16 with r = 8 no two windows are disjoint and one value cannot be 0 in one and 1 in another"""
    return min(H, W) >= 2 * (r + 2)


@functools.lru_cache(maxsize=None)
def frames8(B, Ho, Wo):
    """styled and camera bytes: noise, with runs of 0 and 255 in both and against each other (S - C = +-255)"""
    rng = np.random.default_rng(1000 * Ho + Wo)
    S, C = (rng.integers(0, 256, (B, Ho, Wo, 3), dtype=np.uint8) for _ in range(2))
    S[:, :, :Wo // 4], C[:, :, :Wo // 4] = 255, 0
    S[:, : Ho // 4, Wo // 2:], C[:, : Ho // 4, Wo // 2:] = 0, 255
    return S, C


@functools.lru_cache(maxsize=None)
def reference(g, r, keep, ramp, show):
    from live2diff_amd import matte as MT
    (B, H, W), (Ho, Wo) = GEOMETRIES[g]
    S, C = frames8(B, Ho, Wo)
    d = depth(B, H, W, r)
    lo, hi = RAMPS[ramp]
    M = MT.matte_up_ref(MT.matte_ref(d, lo, hi, r, keep), Ho, Wo)
    return MT.composite_up_ref(S, C, d, lo, hi, r, keep, show), M


def launch(g, r, keep, ramp, show, fill=7, off=0):
    """the op into a destination with GUARD bytes on either side (and `off` more in front), all pre-filled: (frame, the rest)"""
    from live2diff_amd import ops
    from live2diff_amd.matte import matte_params, table_words
    (B, H, W), (Ho, Wo) = GEOMETRIES[g]
    S, C = (torch.from_numpy(a).to(DEV) for a in frames8(B, Ho, Wo))
    lo32, inv32, hard = matte_params(*RAMPS[ramp])
    n = B * Ho * Wo * 3
    buf = torch.full((GUARD + off + n + GUARD,), fill, dtype=torch.uint8, device=DEV)
    tx, ty = (torch.from_numpy(table_words(i, o)).to(DEV) for i, o in ((W, Wo), (H, Ho)))
    ops.run(ops.frame_matte_up(S, C, depth(B, H, W, r).to(DEV), buf[GUARD + off:GUARD + off + n], tx, ty, B=B, H=H, W=W, Ho=Ho, Wo=Wo,
                               lo32=lo32, inv32=inv32, hard=hard, far=keep == "far", show=show, r=r))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    return got[GUARD + off:GUARD + off + n].reshape(B, Ho, Wo, 3), np.concatenate([got[:GUARD + off], got[GUARD + off + n:]])


def report(tag, got, want):
    n = int((got != want).sum())
    print(f"{tag}: {n} of {want.size} bytes differ" + (f", max |diff| {int(np.abs(got.astype(int) - want.astype(int)).max())}" if n else ""))
    return n


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"g{c[0]}-r{c[1]}-{c[2]}-{c[3]}" + ("-show" if c[4] else ""))
def test_kernel_equals_composite_up_ref(case):
    g, r, keep, ramp, show = case
    (B, H, W), _ = GEOMETRIES[g]
    want, M = reference(*case)
    assert len(np.unique(M)) > 16
    if exact_ends(H, W, r):
        assert (M == 0).any() and (M == 1).any()
    got, guard = launch(*case)
    assert report(f"{GEOMETRIES[g]} r {r} {keep} {ramp} show {show}", got, want) == 0
    assert np.all(guard == 7)


def test_chosen_inputs_reach_both_ends():
    """(no launch) the case list covers what it claims, and the cases without exact ends are the ones `exact_ends` explains"""
    without = [c for c in CASES if not exact_ends(*GEOMETRIES[c[0]][0][1:], c[1])]
    assert sorted(without) == [(0, 8, "near", "soft", False), (1, 8, "near", "soft", False)]
    assert {c[1] for c in CASES if c[0] == 0} == {0, 3, 8}
    for setting in (lambda c: c[2] == "far", lambda c: c[3] == "hard", lambda c: c[4]):
        assert any(setting(c) and c[0] != 1 for c in CASES)


def test_kernel_repeatable_and_unaligned_destination():
    """two launches into differently filled outputs agree; a destination that starts at an odd address keeps the bytes around it"""
    case = (2, 3, "near", "soft", False)
    want, _ = reference(*case)
    a, _ = launch(*case, fill=0)
    b, _ = launch(*case, fill=0xFF)
    assert np.array_equal(a, b) and np.array_equal(a, want)
    for off in (1, 2, 3):
        got, guard = launch(*case, off=off)
        assert np.array_equal(got, want), off
        assert np.all(guard == 7), off


# ----------------------------------------------------------------------------- the pitched resize
# (frame, box (y0, x0, bh, bw), output): an odd origin inside a larger frame; a window that touches the right and the bottom
# edge (the last byte read is the frame's last); a down-scale out of the corner at the top right
WINDOWS = [((40, 72), (3, 5, 33, 61), (50, 99)), ((40, 72), (7, 11, 33, 61), (33, 70)), ((24, 136), (0, 67, 24, 69), (12, 35))]


@pytest.mark.parametrize("resample", ["lanczos", "bicubic", "bilinear"])
@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "x".join(map(str, w[1])))
def test_pitched_resize_equals_resize_ref_of_the_window(window, resample):
    from test_gpu_resize import data8

    from live2diff_amd import ops
    from live2diff_amd.resize import axis_table, resize_ref
    (Hs, Ws), (y0, x0, bh, bw), (Ho, Wo) = window
    assert y0 + bh <= Hs and x0 + bw <= Ws
    frame = data8(1, Hs, Ws)
    want = resize_ref(frame[0, y0:y0 + bh, x0:x0 + bw], Ho, Wo, resample)
    dev = torch.from_numpy(frame).to(DEV)
    n = Ho * Wo * 3
    buf = torch.full((n + GUARD,), 7, dtype=torch.uint8, device=DEV)
    tx, ty = (torch.from_numpy(axis_table(i, o, resample)).to(DEV) for i, o in ((bw, Wo), (bh, Ho)))
    ops.run(ops.frame_resize(dev.reshape(-1)[(y0 * Ws + x0) * 3:], buf[:n], tx, ty, B=1, H=bh, W=bw, Ho=Ho, Wo=Wo, src_pitch=Ws))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert report(f"{window} {resample}", got[:n].reshape(Ho, Wo, 3), want) == 0
    assert np.all(got[n:] == 7)


# ----------------------------------------------------------------------------- the wrapper on the device
FRAME_OPS = ("OP_FRAME_INGEST", "OP_FRAME_EGRESS", "OP_FRAME_MATTE", "OP_FRAME_MOMENTS", "OP_COLOR_LOCK", "OP_FRAME_RESIZE",
             "OP_FRAME_MATTE_UP", "OP_JPEG_DCT", "OP_JPEG_HUFF", "OP_JPEG_PACK")
INGEST, OUTPUT = ("OP_FRAME_INGEST", "OP_FRAME_RESIZE"), ("OP_FRAME_RESIZE", "OP_FRAME_MATTE_UP")
LOCK, JPEG = ("OP_FRAME_MOMENTS", "OP_COLOR_LOCK"), ("OP_JPEG_DCT", "OP_JPEG_HUFF", "OP_JPEG_PACK")


def test_wrapper_matte_source_camera_on_device(monkeypatch):
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd import _lib, jpeg
    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.matte import composite_ref, composite_up_ref
    from live2diff_amd.resize import camera_box, resize_ref
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    N = 2
    Ho, Wo = 80, 112
    MATTE = dict(lo=0.3, hi=0.7, keep="near", feather=2, show=False)
    parts = Parts(ucfg, ccfg, H, W, N)
    warm = u8_frames(8, 96, 128, seed=1)
    frames = u8_frames(N + 4, 96, 128, seed=2)
    y0, x0, bh, bw = camera_box(96, 128, H, W)
    assert (y0, x0, bh, bw) == (0, 15, 96, 96)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    kinds = {v: k for k, v in vars(_lib).items() if k.startswith("OP_")}
    ran, run = [], _lib.OpList.run

    def recording(self, *a, **k):
        ran.extend(kinds[op.kind] for op in self._ops if kinds[op.kind] in FRAME_OPS)
        return run(self, *a, **k)

    monkeypatch.setattr(_lib.OpList, "run", recording)

    def wrapper(camera=False, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, **kw, **more)
        if camera:
            w.set_matte(MATTE["lo"], MATTE["hi"], feather=MATTE["feather"])
            w.set_output_size(Ho, Wo)
            w.set_matte_source("camera")
        w.prepare(warm, PROMPT)
        return w

    def window(f, size=(Ho, Wo)):
        return resize_ref(np.ascontiguousarray(f[y0:y0 + bh, x0:x0 + bw]), *size, "lanczos")

    def want_camera(w, plain, f):
        return composite_up_ref(resize_ref(plain, Ho, Wo, "lanczos"), window(f), w._matte_line.last.depth[None], **MATTE)[0]

    def want_stream(w):
        slot = w._matte_line.last
        return resize_ref(composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **MATTE)[0], Ho, Wo, "lanczos")

    def same(ot, got, want, tag):
        if ot == "u8":
            assert got.dtype == np.uint8 and got.shape == want.shape and report(f"{tag} u8", got, want) == 0
        elif ot == "pil":
            assert got.size == want.shape[1::-1] and report(f"{tag} pil", np.array(got), want) == 0
        else:
            assert isinstance(got, bytes) and got == jpeg.encode_ref(want, 75), (tag, ot)

    twin, w = wrapper(), wrapper(camera=True)
    assert w.matte_source == "camera" and w.io.camera_tap is w._camera and w.matte == MATTE
    assert w.output_size == dict(height=Ho, width=Wo, resample="lanczos")

    def step(x, f):
        """one frame through `x`: (its output, the frame launches it made)"""
        del ran[:]
        got = x(f)
        return got, tuple(ran)

    # __call__: output t is paired with frame t - (N - 1); the first one with the last warm-up frame, which came in a batch and
    # carries no camera buffer -- the stream route
    for t, ot in enumerate(("u8", "u8", "pil", "jpeg")):
        w.output_type = ot
        (got, seen), plain = step(w, frames[t]), twin(frames[t])
        if t == 0:
            same(ot, got, want_stream(w), "call 0, the warm-up position")
            assert seen == INGEST + ("OP_FRAME_MATTE", "OP_FRAME_RESIZE"), seen
            continue
        want = want_camera(w, plain, frames[t - 1])
        assert 0 < np.count_nonzero(want != resize_ref(plain, Ho, Wo, "lanczos"))       # (the matte does something)
        same(ot, got, want, f"call {t}")
        assert seen == INGEST + OUTPUT + (JPEG if ot == "jpeg" else ()), seen
    w.output_type = "u8"
    pool = w._camera.allocated
    assert pool <= len(w._matte_line.slots) + 1

    # a colour lock "ema" on both
    for x in (w, twin):
        x.set_color_lock("ema", 0.8, 0.3)
    for t in (4, 5):
        (got, seen), plain = step(w, frames[t]), twin(frames[t])
        same("u8", got, want_camera(w, plain, frames[t - 1]), f"lock, call {t}")
        assert seen == INGEST + LOCK + OUTPUT, seen
    for x in (w, twin):
        x.clear_color_lock()
    assert w._camera.allocated == pool                               # nothing is allocated in steady state

    # a float frame in the same stream: it has no camera frame, its output takes the stream route; the next one is back
    flt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3))
    w(frames[0]), twin(frames[0])
    w(flt), twin(flt)                                                # (this output is still frame 0's)
    (got, seen), plain = step(w, frames[2]), twin(frames[2])         # the float frame's output
    assert w._matte_line.last.camera is None
    same("u8", got, want_stream(w), "the float frame's output")
    assert seen == INGEST + ("OP_FRAME_MATTE", "OP_FRAME_RESIZE"), seen
    got, plain = w(frames[3]), twin(frames[3])
    same("u8", got, want_camera(w, plain, frames[2]), "behind the float frame")

    # the headline: everything kept, at the window's own size -- the camera's bytes, unchanged, N - 1 frames late
    def box(f):
        return f[y0:y0 + bh, x0:x0 + bw]

    w.set_matte(0, 0, keep="far")
    w.set_output_size(bh, bw)
    assert all(s.camera is None for s in w._matte_line.slots)        # the buffers of the old size are gone
    w(frames[0])
    for t in range(1, 4):
        got = w(frames[t])
        assert got.shape == (bh, bw, 3) and report(f"all far at {bh} x {bw}, call {t}", got, box(frames[t - 1])) == 0

    # clear_*: nothing of the feature stays
    w.clear_output_size()
    assert w._camera is None and w.io.camera_tap is None and w._matte_up is None and all(s.camera is None for s in w._matte_line.slots)
    assert step(w, frames[0])[1] == ("OP_FRAME_INGEST", "OP_FRAME_MATTE")

    # push / pop with one frame in flight: the tap's pointer move runs beside the side stream, the launches on this one
    wp, tp = wrapper(camera=True, frame_pipelining=True), wrapper(frame_pipelining=True)
    out, plain, depths = [], [], []
    for x, o in ((wp, out), (tp, plain)):
        x.push(frames[0])
        for i in range(5):
            if i + 1 < 5:
                x.push(frames[i + 1])
            o.append(x.pop())
            if x is wp:
                depths.append(wp._matte_line.last.depth.clone())
    torch.cuda.synchronize()
    for i in range(1, 5):
        want = composite_up_ref(resize_ref(plain[i], Ho, Wo, "lanczos"), window(frames[i - 1]), depths[i][None], **MATTE)[0]
        assert report(f"push / pop {i}", out[i], want) == 0
    assert wp._camera.allocated <= len(wp._matte_line.slots) + 1
    # ... and the bytes of `__call__`: all far at the window's size the output does not depend on the stream at all
    wp.set_matte(0, 0, keep="far")
    wp.set_output_size(bh, bw)
    wp.push(frames[0])
    got = []
    for t in range(1, 5):
        if t < 4:
            wp.push(frames[t])
        got.append(wp.pop())                                         # the output of frame t - 1, paired with frame t - 2
    torch.cuda.synchronize()
    for t in range(2, 5):
        assert report(f"push / pop, all far, frame {t - 1}", got[t - 1], box(frames[t - 2])) == 0


def test_wrapper_refuses_an_unserved_camera_geometry():
    """a window the output size does not serve raises from the frame that first meets it, before that frame launches anything"""
    from live2diff_amd import _lib
    from live2diff_amd.frame_io import HipFrameIO
    from live2diff_amd.resize import CameraTap
    io = HipFrameIO(64, 64, device=DEV)
    io.camera_tap = CameraTap(64, 64, 80, 112, device=DEV)
    ran, run = [], _lib.OpList.run
    try:
        _lib.OpList.run = lambda self, *a, **k: (ran.append(len(self._ops)), run(self, *a, **k))[1]
        with pytest.raises(ValueError, match="output size: height=80 is outside 384 / 2"):
            io.ingest(np.zeros((384, 512, 3), np.uint8))
        assert not ran
        io.ingest(np.zeros((96, 128, 3), np.uint8))
        assert ran == [1, 1] and io.camera_tap.pending is not None
    finally:
        _lib.OpList.run = run
