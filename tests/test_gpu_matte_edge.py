"""-m gpu: L2D_OP_FRAME_MATTE_EDGE (csrc/matte_edge.hip) against `matte.edge_ref` on every bit of its fp32 plane, the plane
variants of L2D_OP_FRAME_MATTE and L2D_OP_FRAME_MATTE_UP against `composite_ref` / `composite_up_ref` on every byte, and
`set_matte_edge` on the wrapper with small native components against the host oracle fed with the same frames: `__call__`, push /
pop, a frame the near-duplicate filter repeats, `matte_source="camera"`, and the setting switched on and off mid-stream."""
import functools

import numpy as np
import pytest
import torch

from test_matte_edge_cpu import frame_of_bytes, planted

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # floats (or bytes) in front of and behind an output, pre-filled and checked

# (40, 136): three tiles across and down, the last ones partial; (8, 16): smaller than the window -- both sides clamp at once
SHAPES = [(40, 136), (8, 16)]
RADII, EPS = (1, 4, 8), (1.0, 10.0)
INPUTS = ("planted", "random", "saturated", "constant", "hard")


@functools.lru_cache(maxsize=None)
def case(name, H, W):
    """(source fp16 [3,H,W], depth fp16 [H,W], lo, hi, keep)"""
    rng = np.random.default_rng(1000 * H + W + len(name))
    noise = lambda: np.clip(rng.normal(0.0, 0.6, (H, W)), -1, 1).astype(np.float16)
    if name == "planted":
        # the case of tests/test_matte_edge_cpu.py: with lo, hi = 0.25, 0.75 the ramp runs over d in [-0.5, 0.5], and
        # d = -0.5 + (column - 38) / 16 (exact in fp16) makes t = (column - 38) / 16
        m0, src = planted(H, W)
        d = np.clip(-0.5 + (np.arange(W) - 38) / 16.0, -1, 1).astype(np.float16)
        return src, np.ascontiguousarray(np.broadcast_to(d, (H, W))), 0.25, 0.75, "near"
    if name == "random":
        src = frame_of_bytes(rng.integers(0, 256, (3, H, W), dtype=np.uint8))
        return src, noise(), 0.3, 0.7, "far"
    if name == "saturated":
        # bytes 0 and 255 in blocks of a few pixels, channel by channel, written as values at and beyond +-1
        b = rng.integers(0, 2, (3, (H + 2) // 3, (W + 4) // 5)).repeat(3, 1).repeat(5, 2)[:, :H, :W]
        lo_v, hi_v = rng.choice([-1.0, -2.0, -1.5], (3, H, W)), rng.choice([1.0, 1.5, 6.0], (3, H, W))
        return np.where(b == 1, hi_v, lo_v).astype(np.float16), noise(), 0.3, 0.7, "near"
    if name == "constant":
        return frame_of_bytes(np.full((H, W), 93, np.uint8)), noise(), 0.2, 0.9, "near"
    if name == "hard":
        src = frame_of_bytes(rng.integers(0, 256, (3, H, W), dtype=np.uint8))
        return src, noise(), 0.5, 0.5, "far"
    raise KeyError(name)


def edge_launch(src, depth, lo, hi, keep, r, eps, fill=float("nan")):
    """op 49 into a plane with GUARD floats on either side, all pre-filled: (the plane's words, the guards' words)"""
    from live2diff_amd import ops
    from live2diff_amd.matte import edge_E, matte_params
    H, W = depth.shape
    lo32, inv32, hard = matte_params(lo, hi)
    buf = torch.full((GUARD + H * W + GUARD,), fill, dtype=torch.float32, device=DEV)
    ops.run(ops.frame_matte_edge(torch.from_numpy(src).to(DEV), torch.from_numpy(depth).to(DEV), buf[GUARD:GUARD + H * W], H=H, W=W, r=r,
                                 E=edge_E(r, eps), lo32=lo32, inv32=inv32, hard=hard, far=keep == "far"))
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    return got[GUARD:GUARD + H * W].reshape(H, W), np.concatenate([got[:GUARD], got[GUARD + H * W:]])


def report(tag, got, want):
    n = int((got != want).sum())
    print(f"{tag}: {n} of {want.size} differ")
    return n


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plane_equals_edge_ref(shape, name):
    from live2diff_amd import matte as MT
    H, W = shape
    src, depth, lo, hi, keep = case(name, H, W)
    m0 = MT.matte_ref(depth, lo, hi, 0, keep)[0]
    if name == "planted":
        assert np.array_equal(np.rint(m0 * np.float32(255)), np.rint(planted(H, W)[0] * np.float32(255)))
    if name == "hard":
        assert set(np.unique(m0)) == {0.0, 1.0}
    nan = np.float32("nan").view(np.uint32)
    for r in RADII:
        for eps in EPS:
            want = MT.edge_ref(m0, src, r, eps)
            got, guard = edge_launch(src, depth, lo, hi, keep, r, eps)
            assert report(f"{shape} {name} r {r} eps {eps}: fp32 words", got, want.view(np.uint32)) == 0
            assert np.all(guard == nan)
    if (H, W) == SHAPES[0] and name != "constant":
        assert len(np.unique(want)) > 16                                   # (the last one: the plane is no constant)


def test_plane_is_repeatable_and_constant_mattes_are_exact():
    """two launches into differently filled planes agree; an all-near matte is 1.0 and an all-far one 0.0 everywhere"""
    H, W = SHAPES[0]
    src, depth, lo, hi, keep = case("random", H, W)
    a, _ = edge_launch(src, depth, lo, hi, keep, 4, 10.0, fill=0.0)
    b, _ = edge_launch(src, depth, lo, hi, keep, 4, 10.0, fill=7.0)
    assert np.array_equal(a, b)
    one = np.float32(1.0).view(np.uint32)
    assert np.all(edge_launch(src, depth, 0, 0, "near", 8, 1.0)[0] == one) and np.all(edge_launch(src, depth, 0, 0, "far", 8, 1.0)[0] == 0)


def styled_frame(H, W):
    g = torch.Generator().manual_seed(7 * H + W)
    x = (torch.randn(1, 3, H, W, generator=g) * 0.7).half()
    x.view(-1)[:6] = torch.tensor([-1.0, 1.0, 0.0, 1.5, -2.0, 6e-8], dtype=torch.float16)
    return x


@pytest.mark.parametrize("feather,show", [(0, False), (3, False), (0, True), (3, True)])
def test_composite_reads_the_plane(feather, show):
    """op 49, then op 43 with L2D_MATTE_PLANE, against `composite_ref(..., edge=...)`: the point kernel and the box kernel"""
    from live2diff_amd import matte as MT
    from live2diff_amd import ops
    H, W = SHAPES[0]
    edge = dict(radius=4, eps=10.0)
    for name in ("random", "planted"):
        src, depth, lo, hi, keep = case(name, H, W)
        styled = styled_frame(H, W)
        want = MT.composite_ref(styled, torch.from_numpy(src)[None], torch.from_numpy(depth)[None], lo, hi, feather, keep, show, edge=edge)[0]
        lo32, inv32, hard = MT.matte_params(lo, hi)
        s16, d16 = torch.from_numpy(src).to(DEV), torch.from_numpy(depth).to(DEV)
        plane = torch.full((H, W), float("nan"), dtype=torch.float32, device=DEV)
        buf = torch.full((GUARD + H * W * 3 + GUARD,), 7, dtype=torch.uint8, device=DEV)
        ops.run(ops.frame_matte_edge(s16, d16, plane, H=H, W=W, r=4, E=MT.edge_E(4, 10.0), lo32=lo32, inv32=inv32, hard=hard, far=keep == "far"))
        ops.run(ops.frame_matte(styled.to(DEV), s16, None, buf[GUARD:GUARD + H * W * 3], B=1, H=H, W=W, r=feather, show=show, plane=plane))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert report(f"{name} feather {feather} show {show}: bytes", got[GUARD:-GUARD].reshape(H, W, 3), want) == 0
        assert np.all(got[:GUARD] == 7) and np.all(got[-GUARD:] == 7)
        if not show:
            plain = MT.composite_ref(styled, torch.from_numpy(src)[None], torch.from_numpy(depth)[None], lo, hi, feather, keep)[0]
            assert np.count_nonzero(plain != want) > 0                     # (the refinement does something)


@pytest.mark.parametrize("feather,show", [(0, False), (3, False), (2, True)])
def test_composite_up_reads_the_plane(feather, show):
    """op 49, then op 47 with L2D_MATTE_PLANE at 40 x 136 -> 60 x 204, against `composite_up_ref(..., edge=..., source=...)`"""
    from live2diff_amd import matte as MT
    from live2diff_amd import ops
    (H, W), (Ho, Wo) = SHAPES[0], (60, 204)
    edge = dict(radius=8, eps=1.0)
    src, depth, lo, hi, keep = case("random", H, W)
    rng = np.random.default_rng(5)
    S, C = (rng.integers(0, 256, (1, Ho, Wo, 3), dtype=np.uint8) for _ in range(2))
    S[:, :, :Wo // 4], C[:, :, :Wo // 4] = 255, 0
    want = MT.composite_up_ref(S, C, torch.from_numpy(depth)[None], lo, hi, feather, keep, show, edge=edge, source=torch.from_numpy(src)[None])[0]
    lo32, inv32, hard = MT.matte_params(lo, hi)
    plane = torch.full((H, W), float("nan"), dtype=torch.float32, device=DEV)
    n = Ho * Wo * 3
    buf = torch.full((GUARD + n + GUARD,), 7, dtype=torch.uint8, device=DEV)
    tx, ty = (torch.from_numpy(MT.table_words(i, o)).to(DEV) for i, o in ((W, Wo), (H, Ho)))
    ops.run(ops.frame_matte_edge(torch.from_numpy(src).to(DEV), torch.from_numpy(depth).to(DEV), plane, H=H, W=W, r=8, E=MT.edge_E(8, 1.0),
                                 lo32=lo32, inv32=inv32, hard=hard, far=keep == "far"))
    ops.run(ops.frame_matte_up(torch.from_numpy(S).to(DEV), torch.from_numpy(C).to(DEV), None, buf[GUARD:GUARD + n], tx, ty, B=1, H=H, W=W,
                               Ho=Ho, Wo=Wo, r=feather, show=show, plane=plane))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert report(f"up, feather {feather} show {show}: bytes", got[GUARD:-GUARD].reshape(Ho, Wo, 3), want) == 0
    assert np.all(got[:GUARD] == 7) and np.all(got[-GUARD:] == 7)
    plain = MT.composite_up_ref(S, C, torch.from_numpy(depth)[None], lo, hi, feather, keep, show)[0]
    assert np.count_nonzero(plain != want) > 0


# ----------------------------------------------------------------------------- the wrapper on the device
MATTE = dict(lo=0.3, hi=0.7, keep="near", feather=2, show=False)
EDGE = dict(radius=4, eps=10.0)


def _setup():
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    N = 2
    parts = Parts(ucfg, ccfg, H, W, N)
    warm = u8_frames(8, 96, 128, seed=1)
    frames = u8_frames(N + 4, 96, 128, seed=2)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(matte=True, edge=None, size=None, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, matte_edge=edge, **kw, **more)
        if matte:
            w.set_matte(MATTE["lo"], MATTE["hi"], keep=MATTE["keep"], feather=MATTE["feather"])
        if size is not None:
            w.set_output_size(*size)
            w.set_matte_source("camera")
        w.prepare(warm, PROMPT)
        return w

    return wrapper, frames, N


def _want(w, edge, styled=None, slot=None):
    from live2diff_amd.matte import composite_ref
    slot = w._matte_line.last if slot is None else slot
    styled = w.stream.prev_image_result if styled is None else styled
    return composite_ref(styled, slot.source[None], slot.depth[None], **w.matte, edge=edge)[0]


def test_wrapper_matte_edge_on_device():
    from test_matte_cpu import DropFilter

    from live2diff_amd import jpeg
    wrapper, frames, N = _setup()
    w, twin = wrapper(edge=EDGE), wrapper()
    assert w.matte_edge == EDGE and twin.matte_edge is None and w.matte == MATTE == twin.matte

    # __call__, N = 2: the host oracle fed with the stream's output tensor and the delay line's slot
    for t in range(3):
        got, plain = w(frames[t]), twin(frames[t])
        assert got.dtype == np.uint8 and report(f"call {t}: bytes", got, _want(w, EDGE)) == 0
        assert report(f"call {t}, the twin without the setting: bytes", plain, _want(twin, None)) == 0
        assert np.count_nonzero(got != plain) > 0
    # the matte itself
    w.set_matte(MATTE["lo"], MATTE["hi"], feather=0, show=True)
    shown = w(frames[3])
    twin(frames[3])
    assert report("show: bytes", shown, _want(w, EDGE)) == 0 and np.array_equal(shown[..., 0], shown[..., 2])
    w.set_matte(MATTE["lo"], MATTE["hi"], keep=MATTE["keep"], feather=MATTE["feather"])
    # off mid-stream: the bytes of the route without the setting, and nothing of it is left
    w.clear_matte_edge()
    assert w.matte_edge is None and w._matte_dev.edge is None
    for t in (4, 5):
        assert np.array_equal(w(frames[t]), twin(frames[t])), t
    # on again with other settings, as a JPEG file
    w.set_matte_edge(8, 1.0)
    w.output_type = "jpeg"
    got = w(frames[0])
    twin(frames[0])
    assert isinstance(got, bytes) and got == jpeg.encode_ref(_want(w, dict(radius=8, eps=1.0)), w.jpeg_quality)
    w.output_type = "u8"
    # a frame the near-duplicate filter repeats: `line.last` refined again, the same bytes
    w.stream.similar_filter, w.stream.similar_image_filter = DropFilter({1}), True
    w.stream.inference_time_ema = 0.0            # (a dropped frame waits that long)
    first = w(frames[1])
    tapped = w._matte_line.tapped
    again = w(frames[2])
    assert w._matte_line.tapped == tapped and np.array_equal(first, again)
    assert report("repeated frame: bytes", again, _want(w, dict(radius=8, eps=1.0))) == 0
    w.stream.similar_image_filter = False

    # push / pop with one frame in flight
    wp = wrapper(edge=EDGE, frame_pipelining=True)
    styled, pop = [], wp.stream.pop

    def keeping():
        x = pop()
        styled.append(x.clone())
        return x

    wp.stream.pop = keeping
    out, slots = [], []
    wp.push(frames[0])
    for i in range(4):
        if i + 1 < 4:
            wp.push(frames[i + 1])
        out.append(wp.pop())
        last = wp._matte_line.last
        slots.append((last.source.clone(), last.depth.clone()))
    torch.cuda.synchronize()
    from live2diff_amd.matte import composite_ref
    for i, got in enumerate(out):
        want = composite_ref(styled[i], slots[i][0][None], slots[i][1][None], **MATTE, edge=EDGE)[0]
        assert report(f"push / pop {i}: bytes", got, want) == 0
    assert len({o.tobytes() for o in out}) == len(out)


def test_wrapper_matte_edge_camera_on_device():
    from live2diff_amd.matte import composite_up_ref
    from live2diff_amd.resize import camera_box, resize_ref
    wrapper, frames, N = _setup()
    Ho, Wo = 80, 112
    y0, x0, bh, bw = camera_box(96, 128, 64, 64)
    wc, plain = wrapper(edge=EDGE, size=(Ho, Wo)), wrapper(matte=False)
    assert wc.matte_source == "camera" and wc.matte_edge == EDGE

    def want(f, styled_u8, edge):
        slot = wc._matte_line.last
        cam = resize_ref(np.ascontiguousarray(f[y0:y0 + bh, x0:x0 + bw]), Ho, Wo, "lanczos")
        return composite_up_ref(resize_ref(styled_u8, Ho, Wo, "lanczos"), cam, slot.depth[None], **MATTE, edge=edge,
                                source=slot.source[None] if edge is not None else None)[0]

    wc(frames[0]), plain(frames[0])              # (the warm-up position carries no camera frame: the stream route)
    for t in (1, 2):
        got, p = wc(frames[t]), plain(frames[t])
        assert got.shape == (Ho, Wo, 3) and report(f"camera, call {t}: bytes", got, want(frames[t - 1], p, EDGE)) == 0
        assert np.count_nonzero(got != want(frames[t - 1], p, None)) > 0
    # off mid-stream: the route without the setting
    wc.clear_matte_edge()
    got, p = wc(frames[3]), plain(frames[3])
    assert wc._matte_up.edge is None and report("camera, the setting off: bytes", got, want(frames[2], p, None)) == 0
    wc.set_matte_edge(2, 3.0)
    got, p = wc(frames[4]), plain(frames[4])
    assert report("camera, on again: bytes", got, want(frames[3], p, dict(radius=2, eps=3.0))) == 0
