"""GPU tests of the backdrop (csrc/backdrop.hip, live2diff_amd/backdrop.py): op 54 against
`frame_of(blur_ref(...))` word for word, the composites with every backdrop kind against the host oracles byte for byte, and
the wrapper on the device on the stream route and on the camera route."""
import functools

import numpy as np
import pytest
import torch

from test_backdrop_cpu import frame16

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # halves in front of and behind the output frame, pre-filled and checked
# 24 x 40: narrower than the halo of 24 on both sides at once; 48 x 72: partial tiles; 72 x 136: an interior tile with a full halo
SHAPES = [(24, 40), (48, 72), (72, 136)]
SETTINGS = [(1, 1), (8, 1), (3, 2), (8, 3)]
INPUTS = ("saturated", "subject", "step", "step_far", "hard")


@functools.lru_cache(maxsize=None)
def case(name, H, W):
    """(source fp16 [3,H,W], depth fp16 [H,W], lo, hi, keep)"""
    rng = np.random.default_rng(1000 * H + W)
    random = lambda: frame16(rng.integers(0, 256, (3, H, W), dtype=np.uint8))                # noqa: E731
    if name == "saturated":                      # the largest numerators: all-255 bytes, M == 0, W == 256
        return frame16(np.full((3, H, W), 255, np.uint8)), np.full((H, W), -1.0, np.float16), 0.3, 0.7, "near"
    if name == "subject":                        # M == 255 everywhere: W == 1
        return random(), np.full((H, W), 1.0, np.float16), 0.3, 0.7, "near"
    yy, xx = np.mgrid[0:H, 0:W]
    step = np.where(xx + yy // 2 > W // 2 + 3, 0.8, -0.6) + rng.normal(0, 0.25, (H, W))      # a diagonal step through every tile border
    depth = np.clip(step, -1, 1).astype(np.float16)
    if name == "step":
        return random(), depth, 0.3, 0.7, "near"
    if name == "step_far":
        return random(), depth, 0.2, 0.9, "far"
    if name == "hard":
        return random(), depth, 0.5, 0.5, "near"
    raise KeyError(name)


def blur_launch(src, depth, lo, hi, keep, r, passes, fill=float("nan")):
    """op 54 into a frame with GUARD halves on either side, all pre-filled: (the frame's words, the guards' words)"""
    from live2diff_amd import ops
    from live2diff_amd.matte import matte_params
    H, W = depth.shape
    lo32, inv32, hard = matte_params(lo, hi)
    n = 3 * H * W
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float16, device=DEV)
    ops.run(ops.frame_backdrop_blur(torch.from_numpy(src).to(DEV), torch.from_numpy(depth).to(DEV), buf[GUARD:GUARD + n].view(3, H, W), H=H, W=W,
                                    r=r, passes=passes, lo32=lo32, inv32=inv32, hard=hard, far=keep == "far"))
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint16)
    return got[GUARD:GUARD + n].reshape(3, H, W), np.concatenate([got[:GUARD], got[GUARD + n:]])


def report(tag, got, want):
    n = int((got != want).sum())
    print(f"{tag}: {n} of {want.size} differ")
    return n


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_equals_blur_ref(shape, name):
    from live2diff_amd import backdrop as BD
    H, W = shape
    src, depth, lo, hi, keep = case(name, H, W)
    W0 = BD.weight_ref(depth, lo, hi, keep)
    if name == "saturated":
        assert np.all(W0 == 256)
    elif name == "subject":
        assert np.all(W0 == 1)
    elif name == "hard":
        assert set(np.unique(W0)) == {1, 256}
    else:
        assert len(np.unique(W0)) > 16
    nan = np.float16("nan").view(np.uint16)
    for r, passes in SETTINGS:
        want = BD.frame_of(BD.blur_ref(src, depth, lo, hi, keep, r, passes))
        got, guard = blur_launch(src, depth, lo, hi, keep, r, passes)
        assert report(f"{shape} {name} r {r} passes {passes}: fp16 words", got, want.view(np.uint16)) == 0
        assert np.all(guard == nan)
    if name == "saturated":
        assert np.all(want == 1.0)
    elif name != "subject":
        assert len(np.unique(want)) > 16                                   # (the last one: the frame is no constant)


def test_frame_is_repeatable():
    """two launches into differently filled frames agree bit for bit"""
    H, W = SHAPES[2]
    src, depth, lo, hi, keep = case("step", H, W)
    a, _ = blur_launch(src, depth, lo, hi, keep, 6, 3, fill=0.0)
    b, _ = blur_launch(src, depth, lo, hi, keep, 6, 3, fill=7.0)
    assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- the composites
def styled_frame(H, W):
    g = torch.Generator().manual_seed(7 * H + W)
    x = (torch.randn(1, 3, H, W, generator=g) * 0.7).half()
    x.view(-1)[:6] = torch.tensor([-1.0, 1.0, 0.0, 1.5, -2.0, 6e-8], dtype=torch.float16)
    return x


ROOM = np.random.default_rng(21).integers(0, 256, (90, 200, 3), dtype=np.uint8)
KINDS = {"blur": dict(to="blur", radius=4, passes=2, color=None), "color": dict(to="color", radius=6, passes=3, color=(0, 177, 64)),
         "image": dict(to="image", radius=6, passes=3, color=None)}


def _slot(src, depth):
    from live2diff_amd.matte import _Slot
    H, W = depth.shape
    slot = _Slot(H, W, DEV)
    slot.source.copy_(torch.from_numpy(src))
    slot.depth.copy_(torch.from_numpy(depth))
    return slot


@pytest.mark.parametrize("feather", [0, 2])
@pytest.mark.parametrize("edge", [None, dict(radius=3, eps=4.0)], ids=["plain", "edge"])
def test_composite_with_every_backdrop(edge, feather):
    """`HipMatte.composite(backdrop=HipBackdrop.stream(...))` against `composite_ref(backdrop=stream_ref(...))`"""
    from live2diff_amd import backdrop as BD
    from live2diff_amd import matte as MT
    H, W = SHAPES[1]
    src, depth, lo, hi, keep = case("step", H, W)
    matte = dict(lo=lo, hi=hi, keep=keep, feather=feather, show=False)
    styled, slot = styled_frame(H, W), _slot(src, depth)
    hm, hb = MT.HipMatte(H, W, device=DEV), BD.HipBackdrop(H, W, device=DEV)
    plain = MT.composite_ref(styled, torch.from_numpy(src)[None], torch.from_numpy(depth)[None], **matte, edge=edge)[0]
    for kind, setting in KINDS.items():
        image = ROOM if kind == "image" else None
        kept = BD.stream_ref(setting, image, src, depth, matte)
        want = MT.composite_ref(styled, torch.from_numpy(src)[None], torch.from_numpy(depth)[None], **matte, edge=edge, backdrop=kept[None])[0]
        for again in range(2):                                             # (the second time from the prepared buffers)
            got = hm.composite(styled[0].to(DEV), slot, matte, edge=edge, backdrop=hb.stream(slot, matte, setting, image)).copy()
            assert report(f"{kind}, feather {feather}, edge {edge}: bytes", got, want) == 0
        assert np.count_nonzero(want != plain) > 0
    assert np.array_equal(hm.composite(styled[0].to(DEV), slot, matte, edge=edge), plain)     # without the keyword: as before


@pytest.mark.parametrize("feather", [0, 2])
@pytest.mark.parametrize("edge", [None, dict(radius=3, eps=4.0)], ids=["plain", "edge"])
def test_composite_up_with_every_backdrop(edge, feather):
    """`HipMatteUp.composite(backdrop=HipBackdrop.output(...))` at 48 x 72 -> 72 x 104 against `composite_up_ref(backdrop=output_ref(...))`"""
    from live2diff_amd import backdrop as BD
    from live2diff_amd import matte as MT
    (H, W), (Ho, Wo) = SHAPES[1], (72, 104)
    src, depth, lo, hi, keep = case("step", H, W)
    matte = dict(lo=lo, hi=hi, keep=keep, feather=feather, show=False)
    slot = _slot(src, depth)
    S = np.random.default_rng(5).integers(0, 256, (Ho, Wo, 3), dtype=np.uint8)
    S_dev = torch.from_numpy(S).to(DEV)
    mu, hb = MT.HipMatteUp(H, W, Ho, Wo, device=DEV), BD.HipBackdrop(H, W, device=DEV)
    source = torch.from_numpy(src)[None] if edge is not None else None
    for kind, setting in KINDS.items():
        image = ROOM if kind == "image" else None
        kept = BD.output_ref(setting, image, src, depth, matte, Ho, Wo, "bicubic")
        want = MT.composite_up_ref(S, None, torch.from_numpy(depth)[None], **matte, edge=edge, source=source, backdrop=kept)[0]
        for again in range(2):
            got = mu.composite(S_dev, slot, matte, edge=edge, backdrop=hb.output(slot, matte, setting, Ho, Wo, image, "bicubic")).copy()
            assert report(f"up, {kind}, feather {feather}, edge {edge}: bytes", got, want) == 0
    # a device tensor of the target size is used in place
    video = torch.from_numpy(np.ascontiguousarray(ROOM[:Ho, :Wo])).to(DEV)
    tensor, records = hb.output(slot, matte, KINDS["image"], Ho, Wo, video)
    assert tensor is video and not records
    got = mu.composite(S_dev, slot, matte, edge=edge, backdrop=(tensor, records))
    assert np.array_equal(got, MT.composite_up_ref(S, None, torch.from_numpy(depth)[None], **matte, edge=edge, source=source,
                                                   backdrop=ROOM[:Ho, :Wo])[0])
    with pytest.raises(ValueError, match="used in place"):
        hb.output(slot, matte, KINDS["image"], Ho, Wo, video[:-1])


# ----------------------------------------------------------------------------- the wrapper on the device
MATTE = dict(lo=0.3, hi=0.7, keep="near", feather=2, show=False)


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

    def wrapper(matte=True, size=None, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, **kw, **more)
        if matte:
            w.set_matte(MATTE["lo"], MATTE["hi"], keep=MATTE["keep"], feather=MATTE["feather"])
        if size is not None:
            w.set_output_size(*size)
            w.set_matte_source("camera")
        w.prepare(warm, PROMPT)
        return w

    return wrapper, frames, N


def test_wrapper_backdrop_on_device():
    """the stream route: every kind against the host oracles, switched mid-stream; cleared, the parent's bytes"""
    from live2diff_amd import backdrop as BD
    from live2diff_amd.matte import composite_ref
    wrapper, frames, N = _setup()
    w, twin = wrapper(backdrop=dict(to="blur", radius=3, passes=2)), wrapper()
    assert w.backdrop == dict(to="blur", radius=3, passes=2, color=None) and twin.backdrop is None

    def want(image=None):
        slot = w._matte_line.last
        kept = BD.stream_ref(w.backdrop, image, slot.source, slot.depth, w.matte)
        return composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **w.matte, edge=w.matte_edge, backdrop=kept[None])[0]

    got, plain = w(frames[0]), twin(frames[0])
    assert got.dtype == np.uint8 and report("blur: bytes", got, want()) == 0 and np.count_nonzero(got != plain) > 0
    w.set_backdrop((0, 177, 64))
    got, plain = w(frames[1]), twin(frames[1])
    assert report("colour: bytes", got, want()) == 0 and np.count_nonzero(got != plain) > 0
    w.set_backdrop(ROOM)
    w.set_matte_edge(3, 4.0)
    twin.set_matte_edge(3, 4.0)
    got, plain = w(frames[2]), twin(frames[2])
    assert report("image, with the edge refinement: bytes", got, want(ROOM)) == 0 and np.count_nonzero(got != plain) > 0
    w.set_backdrop("blur")
    got, plain = w(frames[3]), twin(frames[3])
    assert report("blur, with the edge refinement: bytes", got, want()) == 0 and np.count_nonzero(got != plain) > 0
    w.clear_backdrop()
    assert w.backdrop is None and w._backdrop_dev is None
    assert np.array_equal(w(frames[4]), twin(frames[4]))


def test_wrapper_backdrop_camera_on_device():
    """an output size with the "camera" matte: the first output takes the stream route and is resampled, the later ones the
    composite at the output size with the backdrop in the camera's place"""
    from live2diff_amd import backdrop as BD
    from live2diff_amd.matte import composite_ref, composite_up_ref
    from live2diff_amd.resize import resize_ref
    wrapper, frames, N = _setup()
    Ho, Wo = 80, 112
    wc, twin, plain = wrapper(size=(Ho, Wo), backdrop=dict(to="blur", radius=4)), wrapper(size=(Ho, Wo)), wrapper(matte=False)
    setting = wc.backdrop

    def want(styled_u8, image=None):
        slot = wc._matte_line.last
        kept = BD.output_ref(setting, image, slot.source, slot.depth, MATTE, Ho, Wo, "lanczos")
        return composite_up_ref(resize_ref(styled_u8, Ho, Wo, "lanczos"), None, slot.depth[None], **MATTE, backdrop=kept)[0]

    got = wc(frames[0])                          # (the warm-up position carries no camera frame: the stream route)
    twin(frames[0]), plain(frames[0])
    slot = wc._matte_line.last
    kept = BD.stream_ref(setting, None, slot.source, slot.depth, MATTE, "lanczos")
    first = composite_ref(wc.stream.prev_image_result, slot.source[None], slot.depth[None], **MATTE, backdrop=kept[None])[0]
    assert got.shape == (Ho, Wo, 3) and report("stream route under an output size: bytes", got, resize_ref(first, Ho, Wo, "lanczos")) == 0
    got, t, p = wc(frames[1]), twin(frames[1]), plain(frames[1])
    assert report("camera route, blur: bytes", got, want(p)) == 0 and np.count_nonzero(got != t) > 0
    wc.set_backdrop(ROOM)
    setting = wc.backdrop
    got, t, p = wc(frames[2]), twin(frames[2]), plain(frames[2])
    assert report("camera route, image: bytes", got, want(p, ROOM)) == 0 and np.count_nonzero(got != t) > 0
    wc.set_backdrop((255, 0, 255))
    setting = wc.backdrop
    got, t, p = wc(frames[3]), twin(frames[3]), plain(frames[3])
    assert report("camera route, colour: bytes", got, want(p)) == 0 and np.count_nonzero(got != t) > 0
    wc.clear_backdrop()
    assert np.array_equal(wc(frames[4]), twin(frames[4]))


def test_device_tensors_at_the_streams_size():
    """a device uint8 [H,W,3] tensor on the stream route: converted on the device on every frame, word for word `frame_of` of
    its bytes, and it follows the tensor's content; a device fp16 [3,H,W] frame is used in place"""
    from live2diff_amd import backdrop as BD
    from live2diff_amd import matte as MT
    H, W = SHAPES[1]
    src, depth, lo, hi, keep = case("step", H, W)
    matte = dict(lo=lo, hi=hi, keep=keep, feather=2, show=False)
    styled, slot = styled_frame(H, W), _slot(src, depth)
    hm, hb = MT.HipMatte(H, W, device=DEV), BD.HipBackdrop(H, W, device=DEV)
    every = np.arange(H * W * 3, dtype=np.int64).reshape(H, W, 3) % 256      # every byte value, in every channel
    video = torch.from_numpy(every.astype(np.uint8)).to(DEV)
    setting = BD.check_settings(video)
    for turn in range(2):
        kept, records = hb.stream(slot, matte, setting, video)
        px = video.cpu().numpy()
        want16 = BD.frame_of(np.ascontiguousarray(px.transpose(2, 0, 1)))
        assert not records and kept.dtype == torch.float16 and kept.is_contiguous() and tuple(kept.shape) == (3, H, W)
        assert report(f"device uint8 tensor, turn {turn}: fp16 words", kept.cpu().numpy().view(np.uint16), want16.view(np.uint16)) == 0
        got = hm.composite(styled[0].to(DEV), slot, matte, backdrop=(kept, records)).copy()
        want = MT.composite_ref(styled, torch.from_numpy(src)[None], torch.from_numpy(depth)[None], **matte, backdrop=want16[None])[0]
        assert report(f"device uint8 tensor, turn {turn}: bytes", got, want) == 0
        video.copy_(torch.flip(video, dims=(0,)))                            # the next frame of the video: no host copy, no cache
    frame = torch.from_numpy(want16).to(DEV)
    kept, records = hb.stream(slot, matte, setting, frame)
    assert kept is frame and not records
    with pytest.raises(ValueError, match="used in place"):
        hb.stream(slot, matte, setting, video[:-1])
