"""Output size on the CPU: `resize.resize_ref` pinned to Pillow's `Image.resize` on every byte, the accumulator bound and tap count
of every table over the served ratios, the size rules, the wrapper's host route on the mock components, and the launcher's argument
checks in dry run.  The kernel itself: tests/test_gpu_resize.py."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from live2diff_amd import resize as R
from live2diff_amd.frame_io import egress_ref

PIL_FILTERS = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
# (H, W) -> (Ho, Wo): up-scales; one axis unchanged or changed by one pixel; down-scales and mixed
GEOMETRIES = [((16, 24), (40, 56)), ((64, 64), (128, 128)), ((32, 48), (77, 100)), ((64, 64), (192, 256)), ((16, 16), (128, 128)),
              ((40, 72), (100, 99)), ((48, 64), (48, 160)), ((16, 16), (17, 16)), ((24, 136), (24, 137)), ((64, 96), (32, 48)),
              ((64, 96), (33, 95)), ((40, 72), (20, 36)), ((40, 72), (57, 36)), ((512, 512), (1080, 1080))]


@functools.lru_cache(maxsize=None)
def image(kind, H, W):
    if kind == "smooth":
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        planes = [255 * x / max(W - 1, 1), 255 * y / max(H - 1, 1), 127.5 + 127.5 * np.sin(x / 7.0) * np.cos(y / 5.0)]
        return np.stack(planes, -1).round().astype(np.uint8)
    a = np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    a[::3, ::5] = 0
    a[1::4, 2::3] = 255
    return a


# ----------------------------------------------------------------------------- the oracle is Pillow
@pytest.mark.parametrize("resample", list(PIL_FILTERS))
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "x".join(map(str, g[0])) + "-" + "x".join(map(str, g[1])))
def test_resize_ref_equals_pillow(geometry, resample):
    (H, W), (Ho, Wo) = geometry
    for kind in ("noise", "smooth"):
        a = image(kind, H, W)
        want = np.asarray(Image.fromarray(a).resize((Wo, Ho), PIL_FILTERS[resample]))
        got = R.resize_ref(a, Ho, Wo, resample)
        assert got.dtype == np.uint8 and got.shape == (Ho, Wo, 3)
        assert np.array_equal(got, want), (kind, int((got != want).sum()))


def test_resize_ref_batch_and_tensor():
    a = np.stack([image("noise", 40, 72), image("smooth", 40, 72)])
    got = R.resize_ref(torch.from_numpy(a), 57, 36, "bicubic")
    assert got.shape == (2, 57, 36, 3)
    for b in range(2):
        assert np.array_equal(got[b], R.resize_ref(a[b], 57, 36, "bicubic"))
    with pytest.raises(ValueError):
        R.resize_ref(a.astype(np.float32), 57, 36)
    with pytest.raises(ValueError):
        R.resize_ref(a[..., :2], 57, 36)


# ----------------------------------------------------------------------------- tables
def test_accumulator_bound_taps_and_tile_span():
    """Over ratios from 1/2 to 8, ends included: every row keeps 255 sum |k| + 2^21 below 2^31 (asserted by the builder, and again
    here), KS <= 13, and an output tile of `ops.RESIZE_TILE` pixels reads at most 2 T + 13 source pixels -- the kernel's LDS patch"""
    from live2diff_amd import ops
    T = ops.RESIZE_TILE
    worst_sum, worst_ks, worst_span = 0, 0, 0
    for n_in in (16, 17, 24, 40, 63, 64, 136, 512):
        outs = {-(-n_in // 2), n_in // 2 + 1, n_in - 1, n_in + 1, (3 * n_in) // 4, (21 * n_in) // 10, 3 * n_in, 5 * n_in + 3, 8 * n_in}
        for n_out in sorted(o for o in outs if 2 * o >= n_in and o <= min(8 * n_in, R.MAX_SIZE)):
            for resample in R.FILTERS:
                xmin, count, k = R.coefficients(n_in, n_out, resample)
                assert xmin.dtype == count.dtype == k.dtype == np.int32 and k.shape == (n_out, k.shape[1])
                worst_ks = max(worst_ks, k.shape[1])
                sums = np.abs(k.astype(np.int64)).sum(1)
                worst_sum = max(worst_sum, int(sums.max()))
                assert np.all(255 * sums + (1 << 21) < 1 << 31)
                assert np.all(xmin >= 0) and np.all(count >= 1) and np.all(xmin + count <= n_in) and np.all(count <= k.shape[1])
                assert np.all(np.diff(xmin) >= 0) and np.all(np.diff(xmin + count) >= 0)       # a tile's span is first .. last
                for xx in range(n_out):
                    assert not k[xx, count[xx]:].any()
                    assert abs(int(k[xx].sum()) - (1 << 22)) <= k.shape[1]                     # the weights sum to 1
                for o in range(0, n_out, T):
                    last = min(o + T, n_out) - 1
                    worst_span = max(worst_span, int(xmin[last] + count[last] - xmin[o]))
    print(f"largest sum |k| = {worst_sum / (1 << 22):.4f} x 2^22, KS = {worst_ks}, tile span = {worst_span}")
    assert worst_ks == 13 == R.MAX_KS == ops.RESIZE_MAX_KS
    assert worst_span <= 2 * T + ops.RESIZE_MAX_KS
    assert R.coefficients(136, 68, "lanczos")[2].shape[1] == 13 and R.coefficients(16, 128, "lanczos")[2].shape[1] == 7


def test_identity_axis():
    a = image("noise", 24, 136)
    assert np.array_equal(R.resize_ref(a, 24, 136), a)
    wide = R.resize_ref(a, 24, 137, "lanczos")                       # only the horizontal pass ran: rows stay independent
    assert np.array_equal(wide[5:6], R.resize_ref(a[5:6], 1, 137, "lanczos"))
    # the identity table the kernel gets for such an axis returns its input
    t = R.axis_table(24, 24, "lanczos")
    xmin, count, k = t[:24], t[24:48], t[48:].reshape(24, 1)
    assert np.array_equal(R.resize_pass(a, 0, (xmin, count, k)), a)
    t = R.axis_table(16, 40, "bicubic")
    xmin, count, k = R.coefficients(16, 40, "bicubic")
    assert np.array_equal(t, np.concatenate([xmin, count, k.reshape(-1)]))


# ----------------------------------------------------------------------------- the size rules
def test_check_size_and_filter():
    assert R.check_size(512, 512, 1080, 1920) == (1080, 1920)
    assert R.check_size(64, 64, 32, 512) == (32, 512)
    for ho, wo, match in ((31, 64, "height=31 is outside 64 / 2"), (64, 513, "width=513 is outside"), (0, 64, "outside 1..4096"),
                          (64, 0, "outside 1..4096"), (64.0, 64, "use an integer"), (True, 64, "use an integer")):
        with pytest.raises(ValueError, match=match):
            R.check_size(64, 64, ho, wo)
    with pytest.raises(ValueError, match="outside 1..4096"):
        R.check_size(1024, 1024, 4097, 1024)
    with pytest.raises(ValueError, match="below 2\\^31"):
        R.check_size(1024, 1024, 4096, 4096, batch=43)
    with pytest.raises(ValueError, match="'lanczos', 'bicubic', 'bilinear'"):
        R.check_filter("nearest")
    with pytest.raises(ValueError):
        R.coefficients(16, 32, "box")
    R.check_jpeg_size(1088, 1920)
    with pytest.raises(ValueError, match="multiple of 16"):
        R.check_jpeg_size(1080, 1920)
    with pytest.raises(ValueError, match="above 1920"):
        R.check_jpeg_size(1088, 1936)


# ----------------------------------------------------------------------------- the launcher (dry run)
@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_launcher_checks(dry_run):
    import os

    from live2diff_amd import _lib, ops
    assert (_lib.OP_FRAME_RESIZE, _lib.ABI_VERSION) == (46, 6)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_FRAME_RESIZE = 46," in hdr
    assert f"#define L2D_RESIZE_MAX_KS {ops.RESIZE_MAX_KS} " in hdr and f"#define L2D_RESIZE_MAX_SIZE {ops.RESIZE_MAX_SIZE}\n" in hdr
    B, H, W = 2, 24, 40

    def table(n_in, n_out, ks=None):
        if ks is None:
            return torch.from_numpy(R.axis_table(n_in, n_out, "lanczos"))
        return torch.zeros(n_out * (2 + ks), dtype=torch.int32)

    def mk(Ho=60, Wo=33, u8=False, tx=None, ty=None, H=H, W=W):
        src = torch.zeros(B, H, W, 3, dtype=torch.uint8) if u8 else torch.zeros(B, 3, H, W, dtype=torch.float16)
        dst = torch.zeros(B, Ho, Wo, 3, dtype=torch.uint8)
        return ops.frame_resize(src, dst, table(W, Wo) if tx is None else tx, table(H, Ho) if ty is None else ty, B=B, H=H, W=W, Ho=Ho, Wo=Wo)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    op, _ = mk()
    assert [op.i[j] for j in range(8)] == [B, H, W, 60, 33, 0, 9, 7] and op.kind == 46
    ops.run(mk())
    ops.run(mk(u8=True))
    ops.run(mk(Ho=H, Wo=W))                                          # both axes identity: KS 1
    ops.run(mk(Ho=12, Wo=20))                                        # the 1/2 limit: KS 13
    ops.run(mk(Ho=8 * H, Wo=8 * W))
    bad("KS = 14", mk(tx=table(W, 33, ks=14)))
    bad("KS = .*, 14", mk(ty=table(H, 60, ks=14)))
    bad("between half and 8 times", mk(Ho=9 * H, ty=table(H, 9 * H, ks=7)))
    bad("between half and 8 times", mk(Wo=19, tx=table(W, 19, ks=13)))
    bad("between half and 8 times", mk(Ho=4100, H=1024, ty=table(1024, 4100, ks=7)))
    op, keep = mk()
    op.p[2] = op.p[2] + 2
    bad("table pointer 2 is null or not 4-byte aligned", (op, keep))
    op, keep = mk()
    op.p[3] = None
    bad("table pointer 3 is null", (op, keep))
    op, keep = mk()
    op.p[0] = op.p[0] + 2
    bad("fp16 source is not 4-byte aligned", (op, keep))
    op, keep = mk(u8=True)
    op.p[0] = op.p[0] + 1                                            # (a uint8 source may start anywhere)
    ops.run((op, keep))
    op, keep = mk()
    op.p[1] = None
    bad("invalid arguments", (op, keep))
    # the binding's own checks
    with pytest.raises(ValueError, match="contiguous int32 table"):
        mk(tx=torch.zeros(33 * 9, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous int32 table"):
        mk(tx=torch.zeros(33 * 9 + 1, dtype=torch.int32))
    with pytest.raises(AssertionError):
        ops.frame_resize(torch.zeros(B, 3, H, W), torch.zeros(B, 60, 33, 3, dtype=torch.uint8), table(W, 33), table(H, 60), B=B, H=H,
                         W=W, Ho=60, Wo=33)
    with pytest.raises(AssertionError):
        ops.frame_resize(torch.zeros(B, 3, H, W, dtype=torch.float16), torch.zeros(B, 59, 33, 3, dtype=torch.uint8), table(W, 33),
                         table(H, 60), B=B, H=H, W=W, Ho=60, Wo=33)


def test_hip_resize_builds_and_keeps_its_plans(dry_run):
    rs = R.HipResize(24, 40, 60, 33, "bicubic", device="cpu")
    assert (rs.ks_x, rs.ks_y, rs.host) == (7, 5, None) and tuple(rs.dev.shape) == (1, 60, 33, 3)
    x, u = torch.zeros(3, 24, 40, dtype=torch.float16), torch.zeros(24, 40, 3, dtype=torch.uint8)
    assert rs.resize(x, to_host=False) is not None and rs.resize(u, to_host=False).shape == (60, 33, 3)
    assert not rs._plans                                             # a source seen once keeps nothing alive
    rs.resize(x, to_host=False), rs.resize(u, to_host=False)
    plans = dict(rs._plans)                                          # seen again: a static buffer, its plan is kept
    rs.resize(x, to_host=False), rs.resize(u, to_host=False)
    assert len(plans) == 2 and all(rs._plans[k] is v for k, v in plans.items())
    for _ in range(6):
        rs.resize(torch.zeros(3, 24, 40, dtype=torch.float16), to_host=False)
    assert len(rs._plans) <= rs.MAX_PLANS
    with pytest.raises(ValueError, match="expected fp16"):
        rs.resize(torch.zeros(3, 24, 41, dtype=torch.float16))
    with pytest.raises(ValueError):
        R.HipResize(24, 40, 11, 33)


# ----------------------------------------------------------------------------- the wrapper on the mock components
class RampDepth:
    """a depth detector whose map does not depend on the frame (tests/test_matte_cpu.py)"""
    dtype = torch.float32

    def __call__(self, x):
        return torch.linspace(1.0, 5.0, 384 * 384).view(1, 384, 384).repeat(x.shape[0], 1, 1) + 0.0 * x[:, 0]


def picture_vae():
    """the mock VAE, with a decoder whose picture has detail (the mock's own is one flat colour per frame: nothing to resample)"""
    import pipeline_mocks as M
    import torch.nn.functional as F
    detail = torch.rand(1, 3, M.H, M.W, generator=torch.Generator().manual_seed(5)) * 1.6 - 0.8

    class PictureVAE(M.MockVAE):
        def decode(self, z, return_dict=False):
            return (0.5 * torch.tanh(F.interpolate(z[:, :3] * 0.02 + z[:, 3:4] * 0.004, scale_factor=8)) + detail,)

    return PictureVAE()


def build(monkeypatch, n_steps=2, output_type="u8", **more):
    import pipeline_mocks as M

    import live2diff_amd.pipeline_stream_animation_depth as P
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: None)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)
    pipe = M.MockPipe()
    pipe.unet, pipe.vae, pipe.depth_model = M.MockStreamUNet(), picture_vae(), RampDepth()
    pipe.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
    drop = more.pop("drop", None)
    if drop is not None:
        pipe.similar_filter = DropFilter(drop)
        more["enable_similar_image_filter"] = True
    w = Wrapper.from_components(pipe, output_type=output_type, dtype=torch.float32, device="cpu", seed=2, num_inference_steps=50,
                                t_index_list=[10, 20, 30][:n_steps], width=M.W, height=M.H, **more)
    s = w.stream
    s.scheduler = M.MockScheduler()
    s.timesteps = s.scheduler.timesteps
    s.image_processor = M.MockImageProcessor()
    s.unet_warmup = M.MockWarmupUNet()
    return w


class DropFilter:
    """the near-duplicate filter's interface; drops the calls whose number is in `drop` (tests/test_matte_cpu.py)"""

    def __init__(self, drop):
        self.drop, self.calls = set(drop), 0

    def set_threshold(self, t):
        pass

    def set_max_skip_frame(self, n):
        pass

    def __call__(self, x):
        self.calls += 1
        return None if self.calls - 1 in self.drop else x


def noise_frame(i):
    import pipeline_mocks as M
    return torch.rand(3, M.H, M.W, generator=torch.Generator().manual_seed(100 + i))


def out_size():
    import pipeline_mocks as M
    assert M.H % 16 == 0 and M.W % 16 == 0
    return 2 * M.H + 16, M.W + 16                                    # (multiples of 16: "jpeg" is served)


def pair(monkeypatch, setup=None, **more):
    """(resized wrapper, its unresized twin), prepared alike; `setup(w)` runs on both before `prepare`"""
    import pipeline_mocks as M
    made = []
    for sized in (True, False):
        torch.manual_seed(123)
        w = build(monkeypatch, **more)
        if setup is not None:
            setup(w)
        if sized:
            w.set_output_size(*out_size(), resample="bicubic")
        warm = w.prepare(M.frames(8, seed=7), "a prompt")
        made.append((w, warm))
    (w, warm), (twin, twin_warm) = made
    assert torch.equal(warm, twin_warm) and tuple(warm.shape[1:3]) == (M.H, M.W)          # `prepare`'s frames are not resized
    return w, twin


def call(w, f):
    torch.manual_seed(77)                        # (the host path draws its re-noising from the global generator)
    return w(f)


def check_types(w, twin, frames):
    from live2diff_amd.jpeg import encode_ref
    Ho, Wo = out_size()
    for i, ot in enumerate(("u8", "pil", "jpeg")):
        w.output_type = ot
        twin.output_type = "u8"
        got, plain = call(w, frames[i]), call(twin, frames[i])
        want = R.resize_ref(plain, Ho, Wo, "bicubic")
        assert want.shape == (Ho, Wo, 3) and len(np.unique(want)) > 16
        if ot == "u8":
            assert got.dtype == np.uint8 and np.array_equal(got, want)
        elif ot == "pil":
            assert got.size == (Wo, Ho) and np.array_equal(np.array(got), want)
        else:
            assert isinstance(got, bytes) and got == encode_ref(want, w.jpeg_quality)
    w.output_type = twin.output_type = "u8"


def test_wrapper_host_route_every_output_type(monkeypatch):
    import pipeline_mocks as M
    frames = [noise_frame(i) for i in range(5)]
    w, twin = pair(monkeypatch)
    Ho, Wo = out_size()
    assert w.output_size == dict(height=Ho, width=Wo, resample="bicubic") and twin.output_size is None
    check_types(w, twin, frames)
    # a change of size and filter applies from the next output
    w.set_output_size(M.H // 2, M.W * 3, "lanczos")
    assert np.array_equal(call(w, frames[3]), R.resize_ref(call(twin, frames[3]), M.H // 2, M.W * 3, "lanczos"))
    # cleared: the twin's bytes
    w.clear_output_size()
    assert w.output_size is None and w._size_dev is None and w._size_jpeg is None
    assert np.array_equal(call(w, frames[4]), call(twin, frames[4]))


def test_wrapper_host_route_under_matte_and_colour_lock(monkeypatch):
    import pipeline_mocks as M

    def setup(w):
        w.set_matte(0.3, 0.7, feather=2)
        w.set_color_lock("ema", 0.8, 0.3)

    frames = [noise_frame(i) for i in range(4)]
    w, twin = pair(monkeypatch, setup)
    check_types(w, twin, frames)
    plain = call(twin, frames[3])
    assert not np.array_equal(plain, egress_ref(twin.stream.prev_image_result)[0].numpy())       # (the matte and the lock do something)
    assert np.array_equal(call(w, frames[3]), R.resize_ref(plain, *out_size(), "bicubic"))
    w.clear_output_size()
    assert w.matte is not None and w.color_lock is not None
    assert np.array_equal(call(w, frames[0]), call(twin, frames[0]))


def test_wrapper_dropped_frame_repeats_the_resized_frame(monkeypatch):
    import pipeline_mocks as M
    torch.manual_seed(123)
    w = build(monkeypatch, drop={1, 2}, output_size=out_size())
    w.prepare(M.frames(8, seed=7), "a prompt")
    got = [call(w, noise_frame(i)) for i in range(4)]
    assert all(o.shape == (*out_size(), 3) for o in got)
    assert np.array_equal(got[1], got[0]) and np.array_equal(got[2], got[0]) and not np.array_equal(got[3], got[0])


def test_wrapper_constructor_keyword_and_validation(monkeypatch):
    import pipeline_mocks as M
    w = build(monkeypatch, output_size=(M.H * 2, M.W), output_resample="bilinear")
    assert w.output_size == dict(height=M.H * 2, width=M.W, resample="bilinear")
    with pytest.raises(ValueError, match="use \\(height, width\\)"):
        build(monkeypatch, output_size=64)
    with pytest.raises(ValueError, match="'lanczos', 'bicubic', 'bilinear'"):
        build(monkeypatch, output_size=(M.H, M.W), output_resample="nearest")
    w = build(monkeypatch)
    for args in ((M.H // 2 - 1, M.W), (M.H, 8 * M.W + 1), (0, M.W), (M.H, 4097), (M.H, M.W, "box"), (float(M.H), M.W)):
        with pytest.raises(ValueError):
            w.set_output_size(*args)
    assert w.output_size is None
    # an unserved output type: when the size is set, and at the frame
    for ot in ("pt", "np", "latent"):
        w.output_type = ot
        with pytest.raises(ValueError, match="set_output_size: .*'u8'.*'pil'.*'jpeg'"):
            w.set_output_size(M.H, 2 * M.W)
        with pytest.raises(ValueError, match="is not resampled"):
            build(monkeypatch, output_type=ot, output_size=(M.H, 2 * M.W))
    w.output_type = "u8"
    w.set_output_size(M.H, 2 * M.W)
    torch.manual_seed(123)
    w.prepare(M.frames(8, seed=7), "a prompt")
    w.output_type = "pt"
    with pytest.raises(ValueError, match="an output size is set and output_type='pt'.*clear_output_size"):
        w(noise_frame(0))
    # the encoder's rules, when the size is set
    w.output_type = "jpeg"
    for size, match in (((M.H + 8, M.W), "multiple of 16"), ((M.H, M.W + 24), "multiple of 16")):
        with pytest.raises(ValueError, match=match):
            w.set_output_size(*size)
    assert w.output_size == dict(height=M.H, width=2 * M.W, resample="lanczos")        # a refused call changes nothing


def test_wrapper_jpeg_width_limit(monkeypatch):
    """wider than the encoder's 1920 columns: refused when the size is set (a stand-in of the wrapper: no stream is needed)"""
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    w = Wrapper.__new__(Wrapper)
    w.output_type, w.height, w.width = "jpeg", 512, 512
    with pytest.raises(ValueError, match="above 1920"):
        w.set_output_size(1088, 1936)
    with pytest.raises(ValueError, match="multiple of 16"):
        w.set_output_size(1080, 1920)
    w.set_output_size(1088, 1920)
    assert w.output_size == dict(height=1088, width=1920, resample="lanczos")
