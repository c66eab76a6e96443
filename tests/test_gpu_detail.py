"""-m gpu: L2D_OP_FRAME_DETAIL_GAIN (csrc/detail.hip) against `detail.gains_ref` on every int32 word, L2D_OP_FRAME_DETAIL against
`detail.inject_ref` on every byte -- both between pre-filled guard bands that are checked afterwards --, and `set_detail` on the
wrapper with small native components against `detail.detail_ref` fed with the same frames: `__call__`, push / pop, a frame the
near-duplicate filter repeats, a "stream" matte, a "camera" matte, a JPEG file, the mode switched on and off mid-stream, and a
float-tensor frame."""
import functools

import numpy as np
import pytest
import torch

from test_detail_cpu import frame_of_bytes, planted

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # words (or bytes) in front of and behind an output, pre-filled and checked

# (40, 136): three tiles across and down, the last ones partial; (8, 16): smaller than the window -- both sides clamp at once
SHAPES = [(40, 136), (8, 16)]
RADII, EPS = (1, 4, 8), (1.0, 10.0)
INPUTS = ("random", "planted", "saturated", "constant")


def report(tag, got, want):
    n = int((got != want).sum())
    print(f"{tag}: {n} of {want.size} differ")
    return n


@functools.lru_cache(maxsize=None)
def case(name, H, W):
    """(the frame the resize reads, fp16 [3,H,W]; its source frame, fp16 [3,H,W])"""
    rng = np.random.default_rng(1000 * H + W + len(name))
    rand = lambda: frame_of_bytes(rng.integers(0, 256, (3, H, W), dtype=np.uint8))
    if name == "random":
        return rand(), rand()
    if name == "planted":
        c = planted(48, 144)
        return (np.ascontiguousarray(c["styled"].numpy()[:, :H, :W]), np.ascontiguousarray(c["source"].numpy()[:, :H, :W]))
    if name == "saturated":
        # bytes 0 and 255 in blocks of a few pixels, channel by channel, written as values at and beyond +-1
        def sat():
            b = rng.integers(0, 2, (3, (H + 2) // 3, (W + 4) // 5)).repeat(3, 1).repeat(5, 2)[:, :H, :W]
            lo_v, hi_v = rng.choice([-1.0, -2.0, -1.5], (3, H, W)), rng.choice([1.0, 1.5, 6.0], (3, H, W))
            return np.where(b == 1, hi_v, lo_v).astype(np.float16)
        return sat(), sat()
    if name == "constant":
        return frame_of_bytes(np.full((3, H, W), 201, np.uint8)), frame_of_bytes(np.full((3, H, W), 93, np.uint8))
    raise KeyError(name)


def gain_launch(frame, source, r, eps, fill=0x55555555):
    """op 50 into planes with GUARD words on either side, all pre-filled: (the planes' words, the guards' words)"""
    from live2diff_amd import ops
    from live2diff_amd.matte import edge_E
    H, W = source.shape[1:]
    n = 3 * H * W
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.int32, device=DEV)
    ops.run(ops.frame_detail_gain(torch.from_numpy(np.ascontiguousarray(frame)).to(DEV), torch.from_numpy(source).to(DEV),
                                  buf[GUARD:GUARD + n].view(3, H, W), H=H, W=W, r=r, E=edge_E(r, eps)))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    return got[GUARD:GUARD + n].reshape(3, H, W), np.concatenate([got[:GUARD], got[GUARD + n:]])


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gains_equal_gains_ref(shape, name):
    from live2diff_amd import detail as D
    H, W = shape
    frame, source = case(name, H, W)
    as_bytes = D.frame_bytes(frame)                                          # the L2D_DETAIL_U8 form of the same frame
    for r in RADII:
        for eps in EPS:
            want = D.gains_ref(frame, source, r, eps)
            for form, f in (("fp16", frame), ("u8", as_bytes)):
                got, guard = gain_launch(f, source, r, eps)
                assert report(f"{shape} {name} {form} r {r} eps {eps}: int32 words", got, want) == 0
                assert np.all(guard == 0x55555555)
    if name == "constant":
        assert not want.any()
    elif shape == SHAPES[0]:
        assert len(np.unique(want)) > 16                                     # (the last one: the planes are no constant)


def test_gains_are_repeatable():
    H, W = SHAPES[0]
    frame, source = case("random", H, W)
    a, _ = gain_launch(frame, source, 4, 1.0, fill=0)
    b, _ = gain_launch(frame, source, 4, 1.0, fill=-7)
    assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- the injection
# 40 x 136 -> 60 x 204; the identity tables; a downscale with an odd width and byte ends; ratio 8
GEOMETRIES = [((40, 136), (60, 204)), ((40, 136), (40, 136)), ((8, 16), (5, 9)), ((8, 16), (64, 128))]


@functools.lru_cache(maxsize=None)
def inject_case(H, W, Ho, Wo):
    """(S, C, L uint8 [Ho,Wo,3]; G int32 [3,H,W] at the bound of the gains, r = 8: |G| <= 261120 * 289)"""
    from live2diff_amd.detail import MAX_GAIN
    rng = np.random.default_rng(H * 7 + Wo)
    S, C, L = (rng.integers(0, 256, (Ho, Wo, 3), dtype=np.uint8) for _ in range(3))
    S[:, :Wo // 4], S[:, Wo // 4:Wo // 2] = 255, 0                          # (where the clamp to 0..255 acts)
    bound = MAX_GAIN * 289
    G = rng.integers(-bound, bound + 1, (3, H, W)).astype(np.int32)
    G[:, 0, :4], G[:, -1, -4:] = bound, -bound
    G[:, H // 2] //= 4096                                                    # (gains near 1 as well: the limit does not always act)
    return S, C, L, G


def inject_launch(S, C, L, G, Ho, Wo, strength, limit, show, fill=7, r=8):
    from live2diff_amd import detail as D
    from live2diff_amd import matte as MT
    from live2diff_amd import ops
    H, W = G.shape[1:]
    n = Ho * Wo * 3
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.uint8, device=DEV)
    tx, ty = (torch.from_numpy(MT.table_words(i, o)).to(DEV) for i, o in ((W, Wo), (H, Ho)))
    dev = lambda a: torch.from_numpy(a).to(DEV)
    ops.run(ops.frame_detail(dev(S), dev(C), dev(L), dev(G), tx, ty, buf[GUARD:GUARD + n].view(Ho, Wo, 3), H=H, W=W, Ho=Ho, Wo=Wo,
                             k=D.gain_scale(r, strength), limit=np.float32(limit), show=show))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == fill) and np.all(got[-GUARD:] == fill)
    return got[GUARD:-GUARD].reshape(Ho, Wo, 3)


@pytest.mark.parametrize("show", [False, True])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_inject_equals_inject_ref(geometry, show):
    from live2diff_amd import detail as D
    (H, W), (Ho, Wo) = geometry
    S, C, L, G = inject_case(H, W, Ho, Wo)
    for limit in (8.0, 64.0):
        for strength in (1.0, 1.0 / 4096):                                   # (the second: injected terms below the limit)
            want = D.inject_ref(S, C, L, G, H, W, 8, strength, limit, show)
            got = inject_launch(S, C, L, G, Ho, Wo, strength, limit, show)
            assert report(f"{geometry} show {show} limit {limit} strength {strength:g}: bytes", got, want) == 0
            flat = np.full_like(S, 128) if show else S
            assert np.abs(got.astype(int) - flat.astype(int)).max() <= limit and np.count_nonzero(got != flat) > 0


def test_inject_is_repeatable_and_the_identities_hold():
    (H, W), (Ho, Wo) = GEOMETRIES[0]
    S, C, L, G = inject_case(H, W, Ho, Wo)
    a = inject_launch(S, C, L, G, Ho, Wo, 1.0, 64.0, False, fill=0)
    b = inject_launch(S, C, L, G, Ho, Wo, 1.0, 64.0, False, fill=255)
    assert np.array_equal(a, b) and not np.array_equal(a, S)
    assert np.array_equal(inject_launch(S, C, C, G, Ho, Wo, 4.0, 255.0, False), S)                    # C == L
    assert np.array_equal(inject_launch(S, C, L, G, Ho, Wo, 0.0, 255.0, False), S)                    # strength == 0
    assert np.array_equal(inject_launch(S, C, L, np.zeros_like(G), Ho, Wo, 4.0, 255.0, False), S)     # G == 0
    assert np.all(inject_launch(S, C, C, G, Ho, Wo, 4.0, 255.0, True) == 128)


# ----------------------------------------------------------------------------- the wrapper on the device
MATTE = dict(lo=0.3, hi=0.7, keep="near", feather=2, show=False)
DETAIL = dict(radius=2, eps=2.0, strength=1.0, limit=64.0, show=False)
SIZE = (80, 112)


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
    frames = u8_frames(12, 96, 128, seed=2)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(detail=None, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, output_size=SIZE, detail=detail, **kw, **more)
        w.prepare(warm, PROMPT)
        return w

    return wrapper, frames, N


def _camera(frame):
    """the camera frame of a 96 x 128 uint8 frame at the output size: `CameraTap`'s resample of the ingest's window"""
    from live2diff_amd.resize import camera_box, resize_ref
    y0, x0, bh, bw = camera_box(96, 128, 64, 64)
    return resize_ref(np.ascontiguousarray(np.asarray(frame)[y0:y0 + bh, x0:x0 + bw]), *SIZE, "lanczos")


def _want(w, frame, settings, styled=None, slot=None):
    """`detail_ref` fed with the stream's output tensor, the delay line's slot and the camera frame of `frame`; under a matte
    the composite goes in front ("stream") or behind ("camera")"""
    from live2diff_amd import detail as D
    from live2diff_amd.matte import composite_ref, composite_up_ref
    slot = w._matte_line.last if slot is None else slot
    styled = w.stream.prev_image_result if styled is None else styled
    cam = _camera(frame)
    P = styled[0]
    if w.matte is not None and w.matte_source == "stream":
        P = composite_ref(styled, slot[0][None], slot[1][None], **w.matte)[0]
    out = D.detail_ref(P, slot[0], cam, *SIZE, "lanczos", **settings)
    if w.matte is not None and w.matte_source == "camera":
        out = composite_up_ref(out, cam, slot[1][None], **w.matte)[0]
    return out


def _slot(w):
    last = w._matte_line.last
    return last.source, last.depth


def test_wrapper_detail_on_device():
    from test_matte_cpu import DropFilter

    from live2diff_amd import jpeg
    wrapper, frames, N = _setup()
    w, twin = wrapper(detail=DETAIL), wrapper()
    assert w.detail == DETAIL and twin.detail is None and w.output_size == twin.output_size
    assert w._camera is not None and twin._camera is None and twin._matte_line is None

    # __call__, N = 2: the output of call t belongs to frame t - 1.  The warm-up position carries no camera frame: the plain route.
    assert np.array_equal(w(frames[0]), twin(frames[0]))
    for t in (1, 2):
        got, plain = w(frames[t]), twin(frames[t])
        assert got.dtype == np.uint8 and got.shape == SIZE + (3,)
        assert report(f"call {t}: bytes", got, _want(w, frames[t - 1], DETAIL, slot=_slot(w))) == 0
        assert np.count_nonzero(got != plain) > 0
    # the injected term itself, and other settings
    other = dict(radius=8, eps=1.0, strength=2.5, limit=20.0, show=True)
    w.set_detail(**other)
    shown = w(frames[3])
    twin(frames[3])
    assert report("show: bytes", shown, _want(w, frames[2], other, slot=_slot(w))) == 0
    # off mid-stream: the bytes of a wrapper that never had the mode, and nothing of it is left
    w.clear_detail()
    assert w.detail is None and w._detail_dev is None and w._camera is None and w.io.camera_tap is None and w._matte_line is None
    for t in (4, 5):
        assert np.array_equal(w(frames[t]), twin(frames[t])), t
    # on again: the line starts with the next frame, whose output comes one call later
    w.set_detail(**DETAIL)
    assert np.array_equal(w(frames[6]), twin(frames[6]))
    got = w(frames[7])
    twin(frames[7])
    assert report("on again: bytes", got, _want(w, frames[6], DETAIL, slot=_slot(w))) == 0
    # a float-tensor frame has no camera frame: its output passes as without the mode, the one before it does not
    f = torch.from_numpy(np.asarray(frames[8])[16:80, 32:96].copy()).permute(2, 0, 1).float() / 255.0
    got = w(f)
    twin(f)
    assert report("the frame before the float frame: bytes", got, _want(w, frames[7], DETAIL, slot=_slot(w))) == 0
    assert np.array_equal(w(frames[9]), twin(frames[9]))
    # as a JPEG file
    w.output_type = twin.output_type = "jpeg"
    got = w(frames[10])
    twin(frames[10])
    assert isinstance(got, bytes) and got == jpeg.encode_ref(_want(w, frames[9], DETAIL, slot=_slot(w)), w.jpeg_quality)
    w.output_type = twin.output_type = "u8"
    # a frame the near-duplicate filter repeats: `line.last` computed again, the same bytes
    w.stream.similar_filter, w.stream.similar_image_filter = DropFilter({1}), True
    w.stream.inference_time_ema = 0.0            # (a dropped frame waits that long)
    first = w(frames[11])
    tapped = w._matte_line.tapped
    again = w(frames[0])
    assert w._matte_line.tapped == tapped and np.array_equal(first, again)
    assert report("repeated frame: bytes", again, _want(w, frames[10], DETAIL, slot=_slot(w))) == 0
    w.stream.similar_image_filter = False
    # the camera pool allocates nothing in steady state (the repeated frame grew the ring by the slot `last` held on to)
    w(frames[1])
    allocated = w._camera.allocated
    for t in (2, 3, 4, 5):
        w(frames[t])
    assert w._camera.allocated == allocated and allocated <= len(w._matte_line.slots) + 1      # (a buffer per slot, one pending)


def test_wrapper_detail_with_mattes_on_device():
    wrapper, frames, N = _setup()
    w = wrapper(detail=DETAIL)
    plain = wrapper()
    plain.set_matte(MATTE["lo"], MATTE["hi"], keep=MATTE["keep"], feather=MATTE["feather"])
    w.set_matte(MATTE["lo"], MATTE["hi"], keep=MATTE["keep"], feather=MATTE["feather"])
    assert w.matte_source == "stream"
    w(frames[0]), plain(frames[0])
    # a "stream" matte sits in front of the resize: the gains are fitted on the composite's bytes
    for t in (1, 2):
        got, p = w(frames[t]), plain(frames[t])
        assert report(f"stream matte, call {t}: bytes", got, _want(w, frames[t - 1], DETAIL, slot=_slot(w))) == 0
        assert np.count_nonzero(got != p) > 0
    # a "camera" matte: only the styled frame is sharpened, in front of the composite at the output size
    w.set_matte_source("camera")
    plain.set_matte_source("camera")
    for t in (3, 4):
        got, p = w(frames[t]), plain(frames[t])
        assert report(f"camera matte, call {t}: bytes", got, _want(w, frames[t - 1], DETAIL, slot=_slot(w))) == 0
        if t == 4:                               # (call 3 of `plain` pairs a frame from before its tap: the stream route)
            assert np.count_nonzero(got != p) > 0
    # the mode off: the "camera" matte keeps the tap and its bytes
    w.clear_detail()
    assert w._camera is not None and w._detail_dev is None
    assert np.array_equal(w(frames[5]), plain(frames[5]))


def test_wrapper_detail_push_pop_on_device():
    from live2diff_amd import detail as D
    wrapper, frames, N = _setup()
    wp = wrapper(detail=DETAIL, frame_pipelining=True)
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
        slots.append((last.source.clone(), last.depth.clone(), last.camera))
    torch.cuda.synchronize()
    assert slots[0][2] is None                   # (the warm-up position: no camera frame, the plain route)
    for i in range(1, 4):
        want = _want(wp, frames[i - 1], DETAIL, styled=styled[i], slot=slots[i])
        assert report(f"push / pop {i}: bytes", out[i], want) == 0
        assert np.count_nonzero(out[i] != D.resize_ref(D.frame_bytes(styled[i][0]), *SIZE, "lanczos")) > 0
    assert len({o.tobytes() for o in out}) == len(out)
