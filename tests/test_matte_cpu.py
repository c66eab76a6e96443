"""CPU tests (-m "not gpu") of live2diff_amd/matte.py: the identities of `composite_ref` (an all-near matte is `egress_ref` of the
styled frame, an all-far one that of the source, whatever the feather radius), an independent float64 restatement, the launcher's
argument checks (dry-run), and `set_matte` / `clear_matte` on the wrapper built from the mock components of tests/pipeline_mocks.py:
which source frame an output is composited with, for 1, 2 and 3 denoising steps, with and without the near-duplicate filter."""
import numpy as np
import pytest
import torch

from live2diff_amd import matte as MT
from live2diff_amd.frame_io import egress_ref

SHAPES = [(1, 16, 16), (2, 40, 72), (1, 64, 64)]
RADII = [0, 1, 4, 8]


def data(B, H, W, seed=0):
    """frames N(0, 0.7) in fp16 with planted extremes, depth N(0, 0.6) clipped to [-1, 1]"""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    styled = (torch.randn(B, 3, H, W, generator=g) * 0.7).half()
    source = (torch.randn(B, 3, H, W, generator=g) * 0.7).half()
    depth = (torch.randn(B, H, W, generator=g) * 0.6).clamp(-1, 1).half()
    for t in (styled, source):
        t.view(-1)[:8] = torch.tensor([-1.0, 1.0, 0.0, 1.5, -2.0, 6e-8, -6e-8, 3e-5], dtype=torch.float16)
    depth.view(-1)[:4] = torch.tensor([-1.0, 1.0, 0.0, -0.4], dtype=torch.float16)
    return styled, source, depth


# ----------------------------------------------------------------------------- the arithmetic
def test_matte_params():
    lo32, inv32, hard = MT.matte_params(0.3, 0.7)
    assert lo32.dtype == np.float32 and inv32.dtype == np.float32 and hard is False
    assert lo32 == np.float32(2 * 0.3 - 1) and inv32 == np.float32(1.0 / ((2 * 0.7 - 1) - (2 * 0.3 - 1)))
    lo32, inv32, hard = MT.matte_params(0.5, 0.5)
    assert (lo32, inv32, hard) == (np.float32(0.0), np.float32(0.0), True)
    assert MT.matte_params(0, 1) == (np.float32(-1.0), np.float32(0.5), False)
    assert MT.matte_params(0.0, 1e-40)[2] is True                   # 2 hi - 1 rounds to -1 in doubles: a step
    for bad in ((0.6, 0.4), (-0.1, 0.5), (0.2, 1.5)):
        with pytest.raises(ValueError):
            MT.matte_params(*bad)


@pytest.mark.parametrize("shape", SHAPES)
def test_identities(shape):
    styled, source, depth = data(*shape)
    near, far = egress_ref(styled).numpy(), egress_ref(source).numpy()
    for r in (0, 1, 8):
        assert np.array_equal(MT.composite_ref(styled, source, depth, 0, 0, feather=r), near), r
        assert np.array_equal(MT.composite_ref(styled, source, depth, 0, 0, feather=r, keep="far"), far), r
    for keep in ("near", "far"):
        show = MT.composite_ref(styled, source, depth, 0.5, 0.5, keep=keep, show=True)
        assert set(np.unique(show)) == {0, 255} and np.array_equal(show[..., 0], show[..., 1]) and np.array_equal(show[..., 0], show[..., 2])
    m = MT.matte_ref(depth, 0.5, 0.5)
    assert m.dtype == np.float32 and np.array_equal(m, (depth.numpy().astype(np.float32) >= 0).astype(np.float32))
    assert np.array_equal(MT.matte_ref(depth, 0.5, 0.5, keep="far"), 1 - m)
    soft = MT.matte_ref(depth, 0.3, 0.7, feather=4)
    assert soft.min() >= 0 and soft.max() <= 1 and 0 < soft.mean() < 1


def _ref64(styled, source, depth, lo, hi, r, keep, show=False):
    """an independent restatement: the same fp16 v_s / v_c, everything behind them in float64, the box filter as one 2-D mean"""
    lo_d, hi_d = 2.0 * lo - 1.0, 2.0 * hi - 1.0
    d = depth.double().numpy()
    t = (d >= np.float32(lo_d)).astype(np.float64) if hi_d <= lo_d else np.clip((d - lo_d) / (hi_d - lo_d), 0, 1)
    m = t * t * (3 - 2 * t)
    if keep == "far":
        m = 1 - m
    if r:
        B, H, W = m.shape
        p = np.pad(m, ((0, 0), (r, r), (r, r)), mode="edge")
        m = sum(p[:, dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)) / (2 * r + 1) ** 2
    m = m[..., None]
    if show:
        return np.repeat(m, 3, -1) * 255
    vs = (styled * 0.5 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).double().numpy()
    vc = (source * 0.5 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).double().numpy()
    return (vc + m * (vs - vc)) * 255


@pytest.mark.parametrize("shape", SHAPES)
def test_float64_restatement(shape):
    """at most 1 level everywhere, and at no more than 1 % of the bytes (a cap against a systematically shifted oracle, not a
    measurement: the shares seen are a few 1e-4)"""
    styled, source, depth = data(*shape, seed=3)
    for lo, hi in ((0.3, 0.7), (0.5, 0.5)):
        for r in RADII:
            for keep in ("near", "far"):
                got = MT.composite_ref(styled, source, depth, lo, hi, feather=r, keep=keep).astype(np.int64)
                diff = np.abs(got - np.rint(_ref64(styled, source, depth, lo, hi, r, keep)).astype(np.int64))
                share = float((diff != 0).mean())
                print(f"{shape} lo, hi {lo}, {hi} r {r} {keep}: max {diff.max()} share {share:.2e}")
                assert diff.max() <= 1 and share <= 0.01, (shape, lo, hi, r, keep)
    show = MT.composite_ref(styled, source, depth, 0.3, 0.7, feather=4, show=True).astype(np.int64)
    assert np.abs(show - np.rint(_ref64(styled, source, depth, 0.3, 0.7, 4, "near", show=True)).astype(np.int64)).max() <= 1


def test_setting_errors():
    for bad in (dict(lo=0.6, hi=0.4), dict(lo=-0.1, hi=0.5), dict(lo=0.1, hi=1.01), dict(lo="a", hi=1), dict(lo=0.1, hi=0.9, feather=9),
                dict(lo=0.1, hi=0.9, feather=-1), dict(lo=0.1, hi=0.9, feather=1.5), dict(lo=0.1, hi=0.9, feather=True),
                dict(lo=0.1, hi=0.9, keep="middle")):
        with pytest.raises(ValueError):
            MT.check_settings(**bad)
    assert MT.check_settings(0.25, 0.75, keep="far", feather=3, show=1) == dict(lo=0.25, hi=0.75, keep="far", feather=3, show=True)


# ----------------------------------------------------------------------------- the launcher (dry-run)
@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_launcher_checks(dry_run):
    from live2diff_amd import _lib, ops
    assert _lib.OP_FRAME_MATTE == 43 and ops.MATTE_MAX_R == MT.MAX_FEATHER == 8
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_FRAME_MATTE = 43," in hdr and f"#define L2D_MATTE_MAX_R {ops.MATTE_MAX_R}" in hdr
    assert all(f"#define L2D_MATTE_{n} {v}" in hdr for n, v in (("HARD", ops.MATTE_HARD), ("FAR", ops.MATTE_FAR), ("SHOW", ops.MATTE_SHOW)))
    B, H, W = 2, 24, 40

    def mk(H=H, W=W, B=B, **kw):
        s, c = torch.zeros(B, 3, H, W, dtype=torch.float16), torch.zeros(B, 3, H, W, dtype=torch.float16)
        d, o = torch.zeros(B, 3, H, W, dtype=torch.float16), torch.zeros(B, H, W, 3, dtype=torch.uint8)
        args = dict(B=B, H=H, W=W, lo32=-0.4, inv32=1.25, hard=False, r=2)
        args.update(kw)
        return ops.frame_matte(s, c, d, o, **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    ops.run(mk())
    ops.run(mk(depth_stride=3 * H * W, r=8, far=True, show=True))
    ops.run(mk(lo32=0.0, inv32=0.0, hard=True, r=0))
    bad("feather radius 9", mk(r=9))
    bad("feather radius -1", mk(r=-1))
    bad("multiple of 8", mk(W=36))
    bad("multiple of 16", mk(H=3, W=8))
    bad("depth plane stride", mk(depth_stride=H * W + 4))
    bad("hard flag", mk(inv32=0.0))
    bad("hard flag", mk(hard=True))
    bad(r"lo = .* must lie in", mk(lo32=1.5))
    bad("inv", mk(inv32=float("nan")))
    op, keep = mk()
    op.i[4] = 8
    bad("unknown flag bits", (op, keep))
    op, keep = mk()
    op.p[2] = op.p[2] + 2
    bad("pointer 2 is not 16-byte aligned", (op, keep))
    op, keep = mk()
    op.p[1] = None
    bad("invalid arguments", (op, keep))


# ----------------------------------------------------------------------------- the delay line
def test_matte_line_slots_and_growth():
    H = W = 8
    line = MT.MatteLine(3, H, W)

    def frame(v):
        return torch.full((1, 3, H, W), float(v)), torch.full((1, 3, H, W), float(v) / 100)

    def val(slot):
        assert float(slot.depth[0, 0]) == pytest.approx(float(slot.source[0, 0, 0]) / 100, abs=1e-3)
        return float(slot.source[0, 0, 0])

    # mid-stream start: the positions it does not have use the oldest entry
    seen = []
    for k in range(6):
        line(*frame(k))
        seen.append(val(line.take()))
    assert seen == [0, 0, 0, 1, 2, 3] and len(line.slots) == 4 and val(line.last) == 3       # N - 1 behind, the last one, the next
    # primed: the N - 1 positions behind the first frame hold the last warm-up frame
    line.prime(torch.cat([frame(70)[0], frame(71)[0]]), torch.cat([frame(70)[1], frame(71)[1]]))
    assert (line.tapped, line.taken) == (0, 0)
    with pytest.raises(RuntimeError):
        line.take()
    seen = []
    for k in range(5):
        line(*frame(k))
        seen.append(val(line.take()))
    assert seen == [71, 71, 0, 1, 2] and len(line.slots) <= 4
    # up to three tapped frames wait for their output: N + 3 slots, and no growth in steady state
    line.prime(*frame(9))
    line(*frame(0))
    line(*frame(1))
    seen = []
    for k in range(2, 12):
        line(*frame(k))
        seen.append(val(line.take()))
    assert seen == [9, 9, 0, 1, 2, 3, 4, 5, 6, 7] and len(line.slots) == 6
    # one step: no delay
    one = MT.MatteLine(1, H, W)
    one.prime(*frame(50))
    for k in range(4):
        one(*frame(k))
        assert val(one.take()) == k
    assert len(one.slots) <= 2


# ----------------------------------------------------------------------------- the wrapper on the mock components
class RampDepth:
    """a depth detector whose map does not depend on the frame (constant-colour frames would give a constant map, and min-max
    normalisation 0 / 0)"""
    dtype = torch.float32

    def __call__(self, x):
        return torch.linspace(1.0, 5.0, 384 * 384).view(1, 384, 384).repeat(x.shape[0], 1, 1) + 0.0 * x[:, 0]


class DropFilter:
    """the near-duplicate filter's interface; drops the calls whose number is in `drop`"""

    def __init__(self, drop):
        self.drop, self.calls = set(drop), 0

    def set_threshold(self, t):
        pass

    def set_max_skip_frame(self, n):
        pass

    def __call__(self, x):
        self.calls += 1
        return None if self.calls - 1 in self.drop else x


def build(monkeypatch, n_steps, output_type="u8", drop=None):
    import pipeline_mocks as M

    import live2diff_amd.pipeline_stream_animation_depth as P
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    monkeypatch.setattr(torch.cuda, "Event", M.NoCudaEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: None)
    monkeypatch.setattr(P, "retrieve_latents", M.retrieve_latents)
    pipe = M.MockPipe()
    pipe.unet, pipe.vae, pipe.depth_model = M.MockStreamUNet(), M.MockVAE(), RampDepth()
    pipe.prepare_cache = lambda height, width, denoising_steps_num: M.make_caches(denoising_steps_num)
    if drop is not None:
        pipe.similar_filter = DropFilter(drop)
    w = Wrapper.from_components(pipe, output_type=output_type, dtype=torch.float32, device="cpu", seed=2, num_inference_steps=50,
                                t_index_list=[10, 20, 30][:n_steps], width=M.W, height=M.H, enable_similar_image_filter=drop is not None)
    s = w.stream
    s.scheduler = M.MockScheduler()
    s.timesteps = s.scheduler.timesteps
    s.image_processor = M.MockImageProcessor()
    s.unet_warmup = M.MockWarmupUNet()
    return w


def colour(i):
    import pipeline_mocks as M
    c = torch.tensor([(37 * i + 11) % 256, (91 * i + 60) % 256, (53 * i + 200) % 256], dtype=torch.float32) / 255.0
    return c.view(3, 1, 1).expand(3, M.H, M.W).contiguous()


def src_bytes(frame):
    """what the source frame looks like on its way out: the preprocessed frame (2 x - 1) through the egress arithmetic"""
    return egress_ref(2.0 * frame - 1.0)[0].numpy()


@pytest.mark.parametrize("n_steps", [1, 2, 3])
def test_wrapper_far_matte_returns_the_delayed_source_frame(monkeypatch, n_steps):
    import pipeline_mocks as M
    warm = M.frames(8, seed=7)
    frames = [colour(i) for i in range(6)]

    def run(matte):
        torch.manual_seed(123)
        w = build(monkeypatch, n_steps)
        assert w.matte is None
        if matte:
            w.set_matte(0, 0, keep="far", feather=2)                      # before prepare: the line is primed with the last warm-up frame
            assert w.matte == dict(lo=0.0, hi=0.0, keep="far", feather=2, show=False)
        w.prepare(warm, "a prompt")
        return w, [w(f) for f in frames[:4]]

    w, got = run(True)
    for t, o in enumerate(got):
        want = src_bytes(frames[t - (n_steps - 1)] if t >= n_steps - 1 else warm[-1])
        assert o.dtype == np.uint8 and o.shape == (M.H, M.W, 3) and np.array_equal(o, want), (n_steps, t)
    twin, plain = run(False)
    assert not any(np.array_equal(a, b) for a, b in zip(got, plain))
    # an all-near matte is today's output, and so is no matte
    def call(wr, f):
        torch.manual_seed(77)                    # (the host path draws its re-noising from the global generator)
        return wr(f)

    w.set_matte(0, 0)
    assert np.array_equal(call(w, frames[4]), call(twin, frames[4]))
    w.clear_matte()
    assert w.matte is None and w.stream.matte_tap is None
    assert np.array_equal(call(w, frames[5]), call(twin, frames[5]))
    # turned on mid-stream: the line starts with the next frame; positions it does not have use the oldest entry it has
    w.set_matte(0, 0, keep="far")
    more = [colour(i) for i in range(10, 14)]
    for t, f in enumerate(more):
        assert np.array_equal(w(f), src_bytes(more[max(t - (n_steps - 1), 0)])), (n_steps, t)
    # the matte itself, and a soft one against the oracle
    w.set_matte(0.3, 0.7, feather=3, show=True)
    shown = w(colour(20))
    assert np.array_equal(shown, MT.composite_ref(w.stream.prev_image_result, w._matte_line.last.source[None], w._matte_line.last.depth[None],
                                                  0.3, 0.7, feather=3, show=True)[0])
    assert len(np.unique(shown)) > 2 and np.array_equal(shown[..., 0], shown[..., 2])
    w.output_type = "pil"
    w.set_matte(0.3, 0.7, feather=3)
    pil = w(colour(21))
    want = MT.composite_ref(w.stream.prev_image_result, w._matte_line.last.source[None], w._matte_line.last.depth[None], 0.3, 0.7, feather=3)[0]
    assert pil.size == (M.W, M.H) and np.array_equal(np.array(pil), want)
    assert len(w._matte_line.slots) <= n_steps + 1


def test_wrapper_dropped_frame_repeats_and_does_not_shift(monkeypatch):
    import pipeline_mocks as M
    n_steps = 2
    warm = M.frames(8, seed=7)
    frames = [colour(i) for i in range(7)]
    torch.manual_seed(123)
    w = build(monkeypatch, n_steps, drop={2, 3, 5})
    w.set_matte(0, 0, keep="far")
    w.prepare(warm, "a prompt")
    got = [w(f) for f in frames]
    accepted = [0, 1, 4, 6]                                                  # calls 2, 3 and 5 are dropped
    shown = {0: None, 1: 0, 2: 0, 3: 0, 4: 1, 5: 1, 6: 4}                    # call -> the frame whose bytes leave
    for t, o in enumerate(got):
        want = src_bytes(warm[-1] if shown[t] is None else frames[shown[t]])
        assert np.array_equal(o, want), t
    assert w._matte_line.tapped == len(accepted) == w._matte_line.taken


def test_wrapper_jpeg_route_on_the_host(monkeypatch):
    import pipeline_mocks as M
    from live2diff_amd.jpeg import encode_ref
    torch.manual_seed(123)
    w = build(monkeypatch, 2, output_type="jpeg")
    w.set_matte(0, 0, keep="far")
    w.prepare(M.frames(8, seed=7), "a prompt")
    w(colour(1))
    assert w(colour(2)) == encode_ref(src_bytes(colour(1)), w.jpeg_quality)


def test_wrapper_argument_errors(monkeypatch):
    w = build(monkeypatch, 2)
    for args, kw in (((0.6, 0.4), {}), ((-0.1, 0.5), {}), ((0.1, 1.5), {}), ((0.1, 0.9), dict(feather=9)), ((0.1, 0.9), dict(feather=2.0)),
                     ((0.1, 0.9), dict(feather=-1)), ((0.1, 0.9), dict(keep="both"))):
        with pytest.raises(ValueError):
            w.set_matte(*args, **kw)
    assert w.matte is None and w.stream.matte_tap is None
    for ot in ("pt", "np", "latent"):
        w.output_type = ot
        with pytest.raises(ValueError, match="'u8'.*'pil'.*'jpeg'"):
            w.set_matte(0.3, 0.7)
    w.output_type = "u8"
    w.set_matte(0.3, 0.7)
    assert w.matte["feather"] == 0 and w.stream.matte_tap is w._matte_line
