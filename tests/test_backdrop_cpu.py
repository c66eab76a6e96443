"""CPU tests (-m "not gpu") of the backdrop (live2diff_amd/backdrop.py): the oracle's own properties, the
`backdrop=` keyword of the composite oracles, the launcher's refusals in dry-run mode, and the wrapper on the host route."""
import os

import numpy as np
import pytest
import torch

from live2diff_amd import backdrop as BD
from live2diff_amd import matte as MT
from live2diff_amd.frame_io import egress_ref
from live2diff_amd.resize import resize_ref
from live2diff_amd.steady import source_bytes


def frame16(b) -> np.ndarray:
    """an fp16 [3,H,W] frame whose egress bytes are the planar bytes `b`"""
    f = BD.frame_of(np.ascontiguousarray(b, dtype=np.uint8))
    assert np.array_equal(source_bytes(f), b)
    return f


def depth_of(M) -> np.ndarray:
    """an fp16 depth plane that a hard matte at 0.5 turns into M = 255 where `M` is set and 0 elsewhere"""
    return np.where(np.asarray(M) > 0, 1.0, -1.0).astype(np.float16)


HARD = dict(lo=0.5, hi=0.5)


# ----------------------------------------------------------------------------- the arithmetic
def test_frame_of_round_trips_every_byte():
    b = np.arange(256, dtype=np.uint8)
    f = BD.frame_of(np.broadcast_to(b, (3, 1, 256)).copy())
    assert f.dtype == np.float16 and f.shape == (3, 1, 256)
    assert np.array_equal(egress_ref(torch.from_numpy(f)[None])[0].numpy()[0, :, 0], b)
    want = (b.astype(np.float32) * np.float32(2.0 / 255.0) - np.float32(1.0)).astype(np.float16)
    assert np.array_equal(f[0, 0].view(np.uint16), want.view(np.uint16)) and f[0, 0, 0] == -1.0 and f[0, 0, 255] == 1.0
    with pytest.raises(ValueError, match="uint8"):
        BD.frame_of(np.zeros(4, np.float32))


@pytest.mark.parametrize("r,passes", [(1, 1), (8, 3), (3, 2)])
def test_a_constant_image_is_a_fixed_point(r, passes):
    rng = np.random.default_rng(r)
    W0 = 256 - rng.integers(0, 256, (20, 24))
    for value in (0, 1, 127, 255):
        P = np.full((3, 20, 24), value)
        assert np.array_equal(BD.blur_weighted(P, W0, r, passes), P)


def _box_mean(P: np.ndarray, r: int) -> np.ndarray:
    """(2r+1)^2 box mean of an integer plane, edge replicated, by cumulative sums, rounded half up"""
    H, W = P.shape
    p = np.pad(P.astype(np.int64), r, mode="edge")
    c = np.zeros((H + 2 * r + 1, W + 2 * r + 1), np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    k = 2 * r + 1
    s = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
    n = k * k
    return (2 * s + n) // (2 * n)


@pytest.mark.parametrize("r,passes", [(1, 1), (2, 3), (8, 2)])
def test_without_a_subject_it_is_the_iterated_box_mean(r, passes):
    rng = np.random.default_rng(10 + r)
    P = rng.integers(0, 256, (3, 21, 32))
    got = BD.blur_weighted(P, np.full((21, 32), 256), r, passes)
    want = P
    for _ in range(passes):
        want = np.stack([_box_mean(want[c], r) for c in range(3)])
    assert np.array_equal(got, want)
    # and through blur_ref: a depth plane the matte maps to M == 0 everywhere
    src = frame16(P.astype(np.uint8))
    assert np.array_equal(BD.blur_ref(src, np.full((21, 32), -1.0, np.float16), 0.25, 0.75, "near", r, passes), want)
    assert np.array_equal(BD.blur_ref(src, np.full((21, 32), 1.0, np.float16), 0.25, 0.75, "far", r, passes), want)


def test_bounds_hold_on_the_largest_numerators():
    P = np.full((3, 40, 40), 255)
    assert np.array_equal(BD.blur_weighted(P, np.full((40, 40), 256), 8, 3), P)      # (the asserts inside are the test)
    assert np.array_equal(BD.blur_weighted(P, np.full((40, 40), 1), 8, 3), P)
    n = 17 * 17
    assert 2 * n * 256 * 255 + 256 * n < 1 << 26


def test_the_subject_stays_out_of_the_room():
    rng = np.random.default_rng(0)
    P = rng.integers(0, 100, (3, 64, 96))
    background = P.copy()
    P[:, 16:48, 30:60] = 255
    M = np.zeros((64, 96), np.int64)
    M[16:48, 30:60] = 255
    ring = np.zeros((64, 96), bool)
    ring[12:52, 26:64] = True
    ring[16:48, 30:60] = False
    truth = background[:, ring].mean()
    weighted = BD.blur_weighted(P, 256 - M, 8, 3)[:, ring].mean()
    plain = BD.blur_weighted(P, np.full((64, 96), 256), 8, 3)[:, ring].mean()
    print(f"ring mean: truth {truth:.2f}, weighted {weighted:.2f}, plain {plain:.2f}")
    assert abs(weighted - truth) <= 2.0
    assert plain >= truth + 30.0
    # the same through blur_ref and a hard matte
    got = BD.blur_ref(frame16(P.astype(np.uint8)), depth_of(M), **HARD, keep="near", radius=8, passes=3)
    assert np.array_equal(got, BD.blur_weighted(P, 256 - M, 8, 3))


def test_weight_is_the_raw_ramp():
    rng = np.random.default_rng(3)
    d = (rng.random((12, 16)) * 2 - 1).astype(np.float16)
    for keep in ("near", "far"):
        W0 = BD.weight_ref(d, 0.3, 0.7, keep)
        M = np.rint(MT.matte_ref(d, 0.3, 0.7, 0, keep)[0] * np.float32(255)).astype(np.int64)
        assert np.array_equal(W0, 256 - M) and W0.min() >= 1 and W0.max() <= 256


# ----------------------------------------------------------------------------- image, colour, settings
def test_crop_box_and_image_ref():
    assert BD.crop_box(100, 200, 50, 50) == (0, 50, 100, 100)
    assert BD.crop_box(200, 100, 50, 50) == (50, 0, 100, 100)
    assert BD.crop_box(90, 160, 64, 96) == (0, 12, 90, 135)          # 90 * 96 // 64
    assert BD.crop_box(160, 90, 64, 96) == (50, 0, 60, 90)           # 90 * 64 // 96
    assert BD.crop_box(64, 96, 64, 96) == (0, 0, 64, 96)
    assert BD.crop_box(1, 1000, 512, 8) == (0, 499, 1, 1)
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (90, 160, 3), dtype=np.uint8)
    for resample in ("lanczos", "bilinear"):
        got = BD.image_ref(img, 64, 96, resample)
        assert got.dtype == np.uint8 and got.shape == (64, 96, 3)
        assert np.array_equal(got, resize_ref(np.ascontiguousarray(img[:, 12:147]), 64, 96, resample))
    same = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    assert np.array_equal(BD.image_ref(same, 64, 96), same)
    from PIL import Image
    assert np.array_equal(BD.image_ref(Image.fromarray(img), 64, 96), BD.image_ref(img, 64, 96))
    with pytest.raises(ValueError, match="uint8"):
        BD.image_ref(np.zeros((4, 4, 3), np.float32), 8, 8)


def test_image_ref_reads_a_path(tmp_path):
    from PIL import Image
    img = np.random.default_rng(5).integers(0, 256, (40, 72, 3), dtype=np.uint8)
    path = tmp_path / "room.png"
    Image.fromarray(img).save(path)
    assert np.array_equal(BD.image_ref(str(path), 24, 40), BD.image_ref(img, 24, 40))
    assert BD.check_settings(str(path))["to"] == "image"


def test_color_ref():
    c = BD.color_ref((0, 177, 64), 5, 8)
    assert c.shape == (5, 8, 3) and c.dtype == np.uint8 and np.all(c == np.array([0, 177, 64], np.uint8))
    with pytest.raises(ValueError):
        BD.color_ref((0, 256, 0), 5, 8)


def test_check_settings():
    assert BD.check_settings() == dict(to="blur", radius=6, passes=3, color=None)
    assert BD.check_settings((1, 2, 3), 8, 1) == dict(to="color", radius=8, passes=1, color=(1, 2, 3))
    assert BD.check_settings([np.uint8(9), 0, 255])["color"] == (9, 0, 255)
    assert BD.check_settings(np.zeros((4, 4, 3), np.uint8))["to"] == "image"
    assert BD.check_settings(torch.zeros(4, 4, 3, dtype=torch.uint8))["to"] == "image"
    for bad in (0, 9, -1, 2.5, True, "6"):
        with pytest.raises(ValueError, match="radius"):
            BD.check_settings("blur", bad)
    for bad in (0, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="passes"):
            BD.check_settings("blur", 6, bad)
    for bad in ((1, 2), (1, 2, 256), (-1, 0, 0), (1.0, 2, 3), (True, 0, 0)):
        with pytest.raises(ValueError, match="colour"):
            BD.check_settings(bad)
    for bad in ("blurr", "/no/such/file.png", None, 7, np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32),
                torch.zeros(4, 4, 3)):
        with pytest.raises(ValueError, match="backdrop"):
            BD.check_settings(bad)


# ----------------------------------------------------------------------------- the composite oracles
def _scene(H=24, W=40, seed=6):
    rng = np.random.default_rng(seed)
    styled, source, back = (frame16(rng.integers(0, 256, (3, H, W), dtype=np.uint8)) for _ in range(3))
    depth = (rng.random((H, W)) * 2 - 1).astype(np.float16)
    return styled, source, back, depth


def test_composite_ref_takes_the_kept_part_from_the_backdrop():
    styled, source, back, depth = _scene()
    hwc = lambda f: source_bytes(f).transpose(1, 2, 0)                                       # noqa: E731
    near, far = np.full_like(depth, 1.0), np.full_like(depth, -1.0)
    for feather in (0, 2):
        assert np.array_equal(MT.composite_ref(styled[None], source[None], near[None], 0.3, 0.7, feather, backdrop=back[None])[0], hwc(styled))
        assert np.array_equal(MT.composite_ref(styled[None], source[None], far[None], 0.3, 0.7, feather, backdrop=back[None])[0], hwc(back))
    # without the keyword nothing changes, and the backdrop equal to the source is the same call
    plain = MT.composite_ref(styled[None], source[None], depth[None], 0.3, 0.7, 2)
    assert np.array_equal(MT.composite_ref(styled[None], source[None], depth[None], 0.3, 0.7, 2, backdrop=None), plain)
    assert np.array_equal(MT.composite_ref(styled[None], source[None], depth[None], 0.3, 0.7, 2, backdrop=source[None]), plain)
    # `show` reads neither
    assert np.array_equal(MT.composite_ref(styled[None], source[None], depth[None], 0.3, 0.7, 2, show=True, backdrop=back[None]),
                          MT.composite_ref(styled[None], source[None], depth[None], 0.3, 0.7, 2, show=True))
    # with edge=: the matte by edge_ref of the REAL source, over the backdrop
    edge = dict(radius=3, eps=4.0)
    got = MT.composite_ref(styled[None], source[None], depth[None], 0.3, 0.7, 1, "far", edge=edge, backdrop=back[None])
    m = MT.matte_ref(depth, 0.3, 0.7, 1, "far", edge=edge, source=source[None])[..., None]
    vs, vc = MT._unit(styled), MT._unit(back)
    assert np.array_equal(got, np.rint((vc + m * (vs - vc)) * np.float32(255)).astype(np.uint8))
    assert not np.array_equal(got, MT.composite_ref(styled[None], back[None], depth[None], 0.3, 0.7, 1, "far", edge=edge))


def test_composite_up_ref_takes_the_kept_part_from_the_backdrop():
    styled, source, back, depth = _scene()
    Ho, Wo = 36, 60
    rng = np.random.default_rng(8)
    S, C, B = (rng.integers(0, 256, (Ho, Wo, 3), dtype=np.uint8) for _ in range(3))
    near, far = np.full_like(depth, 1.0), np.full_like(depth, -1.0)
    for feather in (0, 2):
        assert np.array_equal(MT.composite_up_ref(S, C, near[None], 0.3, 0.7, feather, backdrop=B)[0], S)
        assert np.array_equal(MT.composite_up_ref(S, C, far[None], 0.3, 0.7, feather, backdrop=B)[0], B)
        assert np.array_equal(MT.composite_up_ref(S, None, far[None], 0.3, 0.7, feather, backdrop=B)[0], B)
    plain = MT.composite_up_ref(S, C, depth[None], 0.3, 0.7, 2)
    assert np.array_equal(MT.composite_up_ref(S, C, depth[None], 0.3, 0.7, 2, backdrop=None), plain)
    assert np.array_equal(MT.composite_up_ref(S, None, depth[None], 0.3, 0.7, 2, backdrop=C), plain)
    edge = dict(radius=2, eps=3.0)
    got = MT.composite_up_ref(S, C, depth[None], 0.3, 0.7, 1, edge=edge, source=source[None], backdrop=B)
    assert np.array_equal(got, MT.composite_up_ref(S, B, depth[None], 0.3, 0.7, 1, edge=edge, source=source[None]))


# ----------------------------------------------------------------------------- the launcher (dry-run)
@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_launcher_checks(dry_run):
    from live2diff_amd import _lib, ops
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert _lib.OP_FRAME_BACKDROP_BLUR == 54 and "L2D_OP_FRAME_BACKDROP_BLUR = 54," in hdr
    assert f"#define L2D_BACKDROP_MAX_R {ops.BACKDROP_MAX_R}\n" in hdr and f"#define L2D_BACKDROP_MAX_PASSES {ops.BACKDROP_MAX_PASSES}\n" in hdr
    assert _lib.ABI_VERSION == 6
    H, W = 24, 40

    def mk(H=H, W=W, **kw):
        args = dict(H=H, W=W, r=4, passes=2, lo32=-0.4, inv32=1.25, hard=False)
        args.update(kw)
        return ops.frame_backdrop_blur(torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(H, W, dtype=torch.float16),
                                       torch.zeros(3, H, W, dtype=torch.float16), **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    op, keep = mk(far=True)
    assert op.kind == 54 and [op.i[j] for j in range(5)] == [H, W, 4, 2, ops.MATTE_FAR] and op.p[3] is None
    ops.run((op, keep))
    ops.run(mk(r=8, passes=3, lo32=0.0, inv32=0.0, hard=True))
    ops.run(mk(H=8, W=16, r=8, passes=3))                                # an image smaller than the halo
    for r in (0, 9, -1, 1.5, True):
        with pytest.raises(ValueError, match="use an integer from 1 to 8"):
            mk(r=r)
    for n in (0, 4, 1.5, True):
        with pytest.raises(ValueError, match="use an integer from 1 to 3"):
            mk(passes=n)
    with pytest.raises(ValueError, match="contiguous fp16"):
        ops.frame_backdrop_blur(torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(H, W), torch.zeros(3, H, W, dtype=torch.float16),
                                H=H, W=W, r=1, passes=1, lo32=0.0, inv32=1.0, hard=False)
    with pytest.raises(ValueError, match="contiguous fp16"):
        ops.frame_backdrop_blur(torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(H, W, dtype=torch.float16), torch.zeros(3, H, W),
                                H=H, W=W, r=1, passes=1, lo32=0.0, inv32=1.0, hard=False)
    bad("multiple of 8", mk(W=36))
    bad("hard flag", mk(inv32=0.0))
    bad("hard flag", mk(hard=True))
    bad(r"lo = .* must lie in", mk(lo32=1.5))
    bad("be finite", mk(inv32=float("inf")))
    for field, value, match in ((2, 0, "radius 0, need 1..8"), (2, 9, "radius 9"), (3, 0, "0 passes, need 1..3"), (3, 4, "4 passes"),
                                (4, 4, "unknown flag bits"), (4, 16, "unknown flag bits"), (0, 0, "non-positive size")):
        op, keep = mk()
        op.i[field] = value
        bad(match, (op, keep))
    for k in range(3):
        op, keep = mk()
        op.p[k] = op.p[k] + 4
        bad(f"pointer {k} is not 16-byte aligned", (op, keep))
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
    op, keep = mk()
    op.p[2] = op.p[0]
    bad("the output overlaps pointer 0", (op, keep))
    op, keep = mk()
    op.i[0], op.i[1] = 32768, 32768                                      # 3 H W >= 2^31 is refused on the sizes alone
    bad("below 2\\^31", (op, keep))


# ----------------------------------------------------------------------------- the wrapper on the mock components (host route)
MATTE = dict(lo=0.3, hi=0.7, keep="far", feather=2, show=False)


def _want(w, setting, image=None, edge=None):
    slot = w._matte_line.last
    kept = BD.stream_ref(setting, image, slot.source, slot.depth, w.matte)
    return MT.composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **w.matte, edge=edge, backdrop=kept[None])[0]


def test_wrapper_host_route(monkeypatch):
    import pipeline_mocks as M
    from test_matte_cpu import build
    warm, frames = M.frames(8, seed=7), M.frames(8, seed=8)
    room = np.random.default_rng(11).integers(0, 256, (M.H + 9, M.W * 2, 3), dtype=np.uint8)

    def run():
        torch.manual_seed(123)
        w = build(monkeypatch, 2)
        w.set_matte(MATTE["lo"], MATTE["hi"], keep=MATTE["keep"], feather=MATTE["feather"])
        w.prepare(warm, "a prompt")
        return w

    def call(w, f):
        torch.manual_seed(77)                    # (the host path draws its re-noising from the global generator)
        return w(f)

    w, twin = run(), run()
    assert w.backdrop is None
    # set, then cleared, before any frame: byte-identical to a run that never set it
    w.set_backdrop("blur")
    w.clear_backdrop()
    assert w.backdrop is None and w._backdrop_dev is None
    assert np.array_equal(call(w, frames[0]), call(twin, frames[0]))
    # every kind equals the oracle, switched mid-stream
    w.set_backdrop("blur", radius=3, passes=2)
    assert w.backdrop == dict(to="blur", radius=3, passes=2, color=None)
    got, plain = call(w, frames[1]), call(twin, frames[1])
    assert got.dtype == np.uint8 and np.array_equal(got, _want(w, w.backdrop)) and not np.array_equal(got, plain)
    w.set_backdrop((0, 177, 64))
    assert w.backdrop == dict(to="color", radius=6, passes=3, color=(0, 177, 64))
    got, plain = call(w, frames[2]), call(twin, frames[2])
    assert np.array_equal(got, _want(w, w.backdrop)) and not np.array_equal(got, plain)
    w.set_backdrop(room)
    assert w.backdrop == dict(to="image", radius=6, passes=3, color=None)
    got, plain = call(w, frames[3]), call(twin, frames[3])
    assert np.array_equal(got, _want(w, w.backdrop, room)) and not np.array_equal(got, plain)
    # with the edge refinement: the guide stays the real source
    w.set_matte_edge(3, 4.0)
    twin.set_matte_edge(3, 4.0)
    w.set_backdrop()
    got, plain = call(w, frames[4]), call(twin, frames[4])
    assert np.array_equal(got, _want(w, w.backdrop, edge=w.matte_edge)) and not np.array_equal(got, plain)
    w.clear_matte_edge()
    twin.clear_matte_edge()
    # `show` is unaffected
    w.set_matte(0.3, 0.7, keep="far", feather=2, show=True)
    twin.set_matte(0.3, 0.7, keep="far", feather=2, show=True)
    assert np.array_equal(call(w, frames[5]), call(twin, frames[5]))
    w.set_matte(**{k: v for k, v in MATTE.items() if k != "show"})
    twin.set_matte(**{k: v for k, v in MATTE.items() if k != "show"})
    # cleared: the parent's bytes again
    w.clear_backdrop()
    assert np.array_equal(call(w, frames[6]), call(twin, frames[6]))
    # the setting acts only while a matte is set
    w.set_backdrop("blur")
    w.clear_matte()
    twin.clear_matte()
    assert w.backdrop["to"] == "blur"
    assert np.array_equal(call(w, frames[7]), call(twin, frames[7]))
    for bad in (dict(radius=0), dict(passes=4), dict(to="fog"), dict(to=(1, 2)), dict(to="color"), dict(to="blur", color=(1, 2, 3)),
                dict(to="image")):
        with pytest.raises(ValueError, match="backdrop"):
            w.set_backdrop(**bad)
    assert w.backdrop == dict(to="blur", radius=6, passes=3, color=None)


def test_wrapper_keyword_property_and_repeated_frame(monkeypatch):
    """`backdrop=` at construction is `set_backdrop`; the property round-trips; a frame the near-duplicate filter drops repeats
    the same bytes"""
    import pipeline_mocks as M

    import live2diff_amd.pipeline_stream_animation_depth as P
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    from test_matte_cpu import DropFilter, RampDepth
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: None)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)

    def make(**more):
        pipe = M.MockPipe()
        pipe.unet, pipe.vae, pipe.depth_model = M.MockStreamUNet(), M.MockVAE(), RampDepth()
        pipe.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
        pipe.similar_filter = DropFilter({1})
        w = Wrapper.from_components(pipe, output_type="u8", dtype=torch.float32, device="cpu", seed=2, num_inference_steps=50,
                                    t_index_list=[10, 20], width=M.W, height=M.H, enable_similar_image_filter=True, **more)
        s = w.stream
        s.scheduler = M.MockScheduler()
        s.timesteps = s.scheduler.timesteps
        s.image_processor = M.MockImageProcessor()
        s.unet_warmup = M.MockWarmupUNet()
        return w

    for bad in (4, "blur", [1, 2, 3]):
        with pytest.raises(ValueError, match="backdrop="):
            make(backdrop=bad)
    with pytest.raises(ValueError, match="backdrop"):
        make(backdrop=dict(radius=0))
    assert make().backdrop is None
    w = make(backdrop=dict(to=(1, 2, 3)))
    assert w.backdrop == dict(to="color", radius=6, passes=3, color=(1, 2, 3)) and w.matte is None
    w2 = make(backdrop=w.backdrop)                                        # the property is a keyword again
    assert w2.backdrop == w.backdrop
    torch.manual_seed(123)
    w = make(backdrop=dict(radius=2, passes=1))
    assert w.backdrop == dict(to="blur", radius=2, passes=1, color=None)
    w.set_backdrop(**w.backdrop)
    assert w.backdrop == dict(to="blur", radius=2, passes=1, color=None)
    w.set_matte(0.2, 0.8, feather=1)
    w.prepare(M.frames(8, seed=7), "a prompt")
    w.stream.inference_time_ema = 0.0            # (a dropped frame waits that long)
    out = [w(f) for f in M.frames(3, seed=9)]
    assert np.array_equal(out[1], out[0]) and w._matte_line.tapped == 2
    assert np.array_equal(out[2], _want(w, w.backdrop))


def test_an_image_is_decoded_when_it_is_set(monkeypatch, tmp_path):
    """a path or a PIL image becomes a uint8 array inside `set_backdrop`: a file that is no image raises ValueError there, the
    setting before it stays, and frames go on; `BackdropBox.apply` of the MJPEG server counts it as failed"""
    import sys

    import pipeline_mocks as M
    from PIL import Image
    from test_matte_cpu import build
    junk = tmp_path / "notes.txt"
    junk.write_text("an existing file that is no image\n")
    cut = tmp_path / "cut.png"
    room_px = np.random.default_rng(12).integers(0, 256, (M.H + 5, M.W + 20, 3), dtype=np.uint8)
    Image.fromarray(room_px).save(tmp_path / "room.png")
    cut.write_bytes((tmp_path / "room.png").read_bytes()[:40])               # a damaged file
    with pytest.raises(ValueError, match="cannot be read as an image"):
        BD.load_image(str(junk))
    assert np.array_equal(BD.load_image(str(tmp_path / "room.png")), room_px)

    torch.manual_seed(123)
    w = build(monkeypatch, 2)
    w.set_matte(MATTE["lo"], MATTE["hi"], keep=MATTE["keep"], feather=MATTE["feather"])
    w.prepare(M.frames(8, seed=7), "a prompt")
    frames = M.frames(3, seed=8)
    w.set_backdrop((9, 8, 7))
    for bad in (str(junk), junk, str(cut)):
        with pytest.raises(ValueError, match="cannot be read as an image"):
            w.set_backdrop(bad)
    assert w.backdrop == dict(to="color", radius=6, passes=3, color=(9, 8, 7))
    assert np.array_equal(w(frames[0]), _want(w, w.backdrop))                # the stream goes on under the setting before
    w.set_backdrop(str(tmp_path / "room.png"))
    (tmp_path / "room.png").unlink()                                         # (decoded already: the file is not read again)
    assert isinstance(w._backdrop_image, np.ndarray) and np.array_equal(w(frames[1]), _want(w, w.backdrop, room_px))
    w.set_backdrop(Image.fromarray(room_px))
    assert isinstance(w._backdrop_image, np.ndarray) and np.array_equal(w(frames[2]), _want(w, w.backdrop, room_px))

    # the server's box on this wrapper: a request that carries such a path never reaches it, and one the wrapper refuses counts
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    with pytest.raises(ValueError, match="cannot be read as an image"):
        S.parse_backdrop_arg(str(junk))
    box = S.BackdropBox(w.backdrop)
    box.put(dict(to=str(junk)))                                              # (as a caller that skipped the parser would)
    box.apply(w)
    assert box.failed == 1 and box.current == w.backdrop and w.backdrop["to"] == "image"
    box.put(dict(to="blur", radius=2))
    box.apply(w)
    assert box.failed == 1 and box.current == w.backdrop == dict(to="blur", radius=2, passes=3, color=None)
    box.put(None)
    box.apply(w)
    assert box.current is None and w.backdrop is None


def test_a_tensor_is_checked_when_it_is_set(monkeypatch):
    import pipeline_mocks as M
    from test_matte_cpu import build
    H, W = M.H, M.W
    BD.check_tensor(torch.zeros(3, H, W, dtype=torch.float16), H, W, on_device=False)
    BD.check_tensor(torch.zeros(H, W, 3, dtype=torch.uint8), H, W, on_device=False)
    BD.check_tensor(torch.zeros(2 * H, 3 * W, 3, dtype=torch.uint8), H, W, (2 * H, 3 * W), on_device=False)
    for t, size in ((torch.zeros(3, H, W + 8, dtype=torch.float16), None), (torch.zeros(2 * H, 3 * W, 3, dtype=torch.uint8), None),
                    (torch.zeros(2 * H, 3 * W, 3, dtype=torch.uint8), (2 * H, 2 * W)), (torch.zeros(3, H, W), None),
                    (torch.zeros(3, W, H, dtype=torch.float16).permute(0, 2, 1), None)):
        with pytest.raises(ValueError, match="used in place"):
            BD.check_tensor(t, H, W, size, on_device=False)
    with pytest.raises(ValueError, match="stream's device"):
        BD.check_tensor(torch.zeros(3, H, W, dtype=torch.float16), H, W)
    w = build(monkeypatch, 2)
    with pytest.raises(ValueError, match="used in place"):
        w.set_backdrop(torch.zeros(3, H + 1, W, dtype=torch.float16))
    assert w.backdrop is None
    w.set_backdrop(torch.zeros(3, H, W, dtype=torch.float16))               # the host route takes an fp16 frame on the host
    assert torch.is_tensor(w._backdrop_image)
    w.set_backdrop(torch.zeros(5, 7, 3, dtype=torch.uint8))                 # a uint8 tensor on the host is an image like an array
    assert isinstance(w._backdrop_image, np.ndarray) and w._backdrop_image.shape == (5, 7, 3)
