"""CPU tests (-m "not gpu") of live2diff_amd/steady.py: the identities of `steady_ref`, `weight_ref` against a direct int64
double loop, the coverage of the shared test sequences (every branch of the weight on every frame), `check_settings`, the
launcher's argument checks (dry-run), and `set_steady` / `clear_steady` on the wrapper built from the mock components of
tests/pipeline_mocks.py: every served output type, the order lock -> steady -> matte, dropped frames, `prepare`, and the delay
line steady shares with the matte and the colour lock.  The sequence generator is shared with tests/test_gpu_steady.py."""
import functools

import numpy as np
import pytest
import torch

from live2diff_amd import steady as SD
from live2diff_amd.frame_io import egress_ref
from test_matte_cpu import build, colour

K = 5                                            # frames per sequence; the first one is the init frame
LO, HI, STRENGTH = 2, 10, 0.8
COVER_SHAPES = [(40, 72), (48, 136), (64, 64)]
RADII = [0, 1, 3, 8]


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- the shared sequences
@functools.lru_cache(maxsize=None)
def sequence(H, W):
    """(sources, styled): K fp16 [3,H,W] frames each, read-only.  A source is a fixed random byte image plus +-1 level of noise
    per frame everywhere (still), a band of fresh random content W // 4 wide that starts at x0 = (5 k) % (W // 2) (moving), and
    on the right quarter a ramp of 0..14 levels added on odd frames only (the ramp of the weight), mapped to fp16 [-1, 1].
    A styled frame is 0.6 N(0, 1): values beyond +-1 included."""
    rng = np.random.default_rng(H * 1009 + W)
    base = rng.integers(0, 256, (3, H, W)).astype(np.int64)
    q = W // 4
    ramp = np.rint(np.linspace(0, 14, q)).astype(np.int64)
    sources, styled = [], []
    for k in range(K):
        b = base + rng.integers(-1, 2, (3, H, W))
        x0 = (5 * k) % (W // 2)
        b[:, :, x0:x0 + q] = rng.integers(0, 256, (3, H, q))
        if k % 2:
            b[:, :, W - q:] += ramp
        x = (np.clip(b, 0, 255) / 127.5 - 1.0).astype(np.float16)
        s = (0.6 * rng.standard_normal((3, H, W))).astype(np.float16)
        for a in (x, s):
            a.setflags(write=False)
        sources.append(x)
        styled.append(s)
    return tuple(sources), tuple(styled)


@functools.lru_cache(maxsize=None)
def oracle(H, W, radius, lo=LO, hi=HI, strength=STRENGTH, show=False):
    """`steady_ref` over the sequence, frame 0 as the init frame: ([fp16 [1,3,H,W] outputs], [(out, bytes) states]), read-only"""
    sources, styled = sequence(H, W)
    outs, states, state = [], [], None
    for k in range(K):
        o, state = SD.steady_ref(styled[k], sources[k], state, lo=lo, hi=hi, strength=strength, radius=radius, show=show, init=k == 0)
        for a in (o, *state):
            a.setflags(write=False)
        outs.append(o)
        states.append(state)
    return outs, states


def weight_direct(b, bp, lo, hi, r):
    """the weight by a double loop over the pixels, the sums in Python integers"""
    lo32, inv32, hard = SD.steady_params(lo, hi)
    _, H, W = b.shape
    d = np.abs(b.astype(np.int64) - bp.astype(np.int64)).max(0)
    w = np.empty((H, W), dtype=np.float32)
    for y in range(H):
        for x in range(W):
            D = 0
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    D += int(d[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)])
            dbar = np.float32(D) / np.float32((2 * r + 1) ** 2)
            if hard:
                t = np.float32(1.0) if dbar >= lo32 else np.float32(0.0)
            else:
                t = min(max((dbar - lo32) * inv32, np.float32(0.0)), np.float32(1.0))
            w[y, x] = (t * t) * (np.float32(3.0) - np.float32(2.0) * t)
    return w


# ----------------------------------------------------------------------------- steady_ref
def test_steady_ref_identities():
    H, W = 24, 40
    sources, styled = sequence(H, W)
    S0, S1 = styled[0], styled[1]
    kw = dict(lo=LO, hi=HI, strength=STRENGTH, radius=3)
    # init: the styled bits, and the state is (styled, the source's bytes)
    o, (p, b) = SD.steady_ref(S0, sources[0], None, init=True, **kw)
    assert o.shape == (1, 3, H, W) and o.dtype == np.float16 and same(o[0], S0) and same(p, S0)
    assert b.dtype == np.uint8 and b.shape == (3, H, W)
    assert np.array_equal(b.transpose(1, 2, 0), egress_ref(torch.from_numpy(np.array(sources[0])))[0].numpy())
    assert same(SD.source_bytes(torch.from_numpy(np.array(sources[0]))[None]), b)
    state = (p, b)
    # strength 0: the styled bits, whatever moved
    o, new = SD.steady_ref(S1, sources[1], state, **dict(kw, strength=0.0))
    assert same(o[0], S1) and same(new[0], S1)
    # identical consecutive sources, strength 1: P's values (a == 0: P + 0 (S - P))
    o, new = SD.steady_ref(S1, sources[0], state, **dict(kw, strength=1.0))
    assert np.array_equal(o[0], S0) and same(new[1], b)
    # lo = hi = 0: a step at 0, everything counts as moving
    o, _ = SD.steady_ref(S1, sources[0], state, **dict(kw, lo=0, hi=0, strength=1.0))
    assert same(o[0], S1)
    assert SD.steady_params(0, 0) == (np.float32(0), np.float32(0), True) and SD.steady_params(2, 10)[2] is False
    assert SD.steady_params(2, 10)[1] == np.float32(0.125)
    # a hard cut: every source pixel changed by >= hi in some channel -> the frame passes, bit for bit
    cut = np.array(sources[0])
    cut = np.where(cut > 0, cut - np.float16(0.5), cut + np.float16(0.5)).astype(np.float16)
    bc = SD.source_bytes(cut)
    assert np.all(np.abs(bc.astype(int) - b.astype(int)).max(0) >= HI)
    for r in (0, 3, 8):
        o, new = SD.steady_ref(S1, cut, state, **dict(kw, radius=r, strength=1.0))
        assert same(o[0], S1) and same(new[1], bc)
    # show: fp16(2 w - 1) in all three channels; the state's frame is the normal blend
    o, new = SD.steady_ref(S1, sources[1], state, show=True, **kw)
    w = SD.weight_ref(SD.source_bytes(sources[1]), b, lo=LO, hi=HI, radius=3)
    pic = (np.float32(2.0) * w - np.float32(1.0)).astype(np.float16)
    assert all(same(o[0, c], pic) for c in range(3))
    plain, new2 = SD.steady_ref(S1, sources[1], state, **kw)
    assert same(new[0], plain[0]) and same(new[0], new2[0]) and same(new[1], new2[1])
    # between S and P, and S's own bits where the weight is 1
    lo_, hi_ = np.minimum(S1, S0), np.maximum(S1, S0)
    assert np.all(plain[0] >= lo_) and np.all(plain[0] <= hi_)
    assert same(plain[0][:, w == 1], S1[:, w == 1]) and (w == 1).any() and (w == 0).any()
    still = plain[0][:, w == 0].astype(np.float32)
    want = S0[:, w == 0].astype(np.float32) + (np.float32(1.0) - np.float32(STRENGTH)) * (S1[:, w == 0].astype(np.float32) - S0[:, w == 0].astype(np.float32))
    assert same(still.astype(np.float16), want.astype(np.float16))
    # -0.0 and +0.0 keep their signs where the frame passes
    z = np.zeros((3, H, W), dtype=np.float16)
    z[0] = -z[0]
    o, _ = SD.steady_ref(z, cut, state, **kw)
    assert same(o[0], z)
    with pytest.raises(ValueError):
        SD.steady_ref(S1[:, :8], sources[1], state, **kw)
    with pytest.raises(ValueError):
        SD.steady_ref(S1, sources[1], state, **dict(kw, strength=1.5))
    with pytest.raises(ValueError):
        SD.steady_ref(S1, sources[1], state, **dict(kw, radius=9))


@pytest.mark.parametrize("shape,r", [((8, 8), 8), ((24, 40), 3)])
def test_weight_ref_against_direct_int64(shape, r):
    H, W = shape
    sources, _ = sequence(H, W)
    b0, b1 = SD.source_bytes(sources[0]), SD.source_bytes(sources[1])
    for lo, hi in ((LO, HI), (4, 4), (0, 255)):
        got = SD.weight_ref(b1, b0, lo=lo, hi=hi, radius=r)
        assert got.dtype == np.float32 and same(got, weight_direct(b1, b0, lo, hi, r)), (lo, hi)
    assert same(SD.weight_ref(b1, b0, lo=LO, hi=HI, radius=0), weight_direct(b1, b0, LO, HI, 0))
    d = np.abs(b1.astype(np.int64) - b0.astype(np.int64)).max(0)
    assert int(SD.window_sum(d, r).max()) <= 255 * (2 * r + 1) ** 2 < 1 << 24          # float32(D) is exact


@pytest.mark.parametrize("shape", COVER_SHAPES)
def test_sequences_cover_every_branch(shape):
    """on every non-init frame, each of w == 0, w == 1 and 0 < w < 1 holds at least a tenth of the pixels"""
    H, W = shape
    sources, _ = sequence(H, W)
    by = [SD.source_bytes(s) for s in sources]
    low = [1.0, 1.0, 1.0]
    for r in RADII:
        for k in range(1, K):
            w = SD.weight_ref(by[k], by[k - 1], lo=LO, hi=HI, radius=r)
            shares = [float((w == 0).mean()), float((w == 1).mean()), float(((w > 0) & (w < 1)).mean())]
            low = [min(a, b) for a, b in zip(low, shares)]
            assert min(shares) >= 0.10, (shape, r, k, shares)
    print(f"{shape}: smallest shares of still / moving / ramp: {low}")


def test_check_settings():
    assert SD.check_settings() == dict(lo=2.0, hi=10.0, strength=0.8, radius=2, show=False)
    assert SD.check_settings(0, 255, 1, np.int64(8), 1) == dict(lo=0.0, hi=255.0, strength=1.0, radius=8, show=True)
    assert SD.MAX_RADIUS == 8 and SD.SERVED_OUTPUT_TYPES == ("pil", "pt", "np", "u8", "jpeg")
    for args, match in (((-1, 10), r"lo=-1.*\[0, 255\]"), ((2, 256), "hi=256"), ((True, 10), "lo=True"), (("2", 10), "lo='2'"),
                        ((11, 10), "lo=11 is above hi=10"), ((2, 10, 1.5), r"strength=1.5.*\[0, 1\]"), ((2, 10, -0.1), "strength"),
                        ((2, 10, True), "strength"), ((2, 10, 0.8, 9), "radius=9.*0 to 8"), ((2, 10, 0.8, -1), "radius"),
                        ((2, 10, 0.8, 2.0), "radius"), ((2, 10, 0.8, True), "radius")):
        with pytest.raises(ValueError, match=match):
            SD.check_settings(*args)


# ----------------------------------------------------------------------------- the launcher
@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_launcher_checks(dry_run):
    import os

    from live2diff_amd import _lib, ops
    assert (_lib.OP_FRAME_STEADY, _lib.ABI_VERSION) == (48, 6)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_FRAME_STEADY = 48," in hdr
    assert all(f"#define L2D_STEADY_{n} {v}" in hdr for n, v in (
        ("HARD", ops.STEADY_HARD), ("SHOW", ops.STEADY_SHOW), ("INIT", ops.STEADY_INIT), ("MAX_R", ops.STEADY_MAX_R)))
    assert (ops.STEADY_HARD, ops.STEADY_SHOW, ops.STEADY_INIT, ops.STEADY_MAX_R) == (1, 2, 4, 8)
    H, W = 24, 40

    def frame(H=H, W=W, dtype=torch.float16):
        return torch.zeros(3, H, W, dtype=dtype)

    def plane(H=H, W=W, dtype=torch.uint8):
        return torch.zeros(3, H, W, dtype=dtype)

    def mk(H=H, W=W, **kw):
        args = dict(styled=frame(H, W), source=frame(H, W), prev_out=frame(H, W), prev_bytes=plane(H, W), out=frame(H, W),
                    next_bytes=plane(H, W), H=H, W=W, lo32=2.0, inv32=0.125, s32=0.8, r=2)
        args.update(kw)
        first = [args.pop(k) for k in ("styled", "source", "prev_out", "prev_bytes", "out", "next_bytes")]
        return ops.frame_steady(*first, **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    # the record
    tensors = [frame(), frame(), frame(), plane(), frame(), plane(), frame()]
    op, keep = ops.frame_steady(*tensors[:6], H=H, W=W, lo32=np.float32(2), inv32=np.float32(0.125), s32=np.float32(0.8), r=3,
                                hard=True, show=True, picture=tensors[6])
    assert op.kind == 48 and [op.p[j] for j in range(7)] == [t.data_ptr() for t in tensors] and op.p[7] is None
    assert [op.i[j] for j in range(5)] == [H, W, 3, ops.STEADY_HARD | ops.STEADY_SHOW, 0]
    assert [op.f[j] for j in range(4)] == [2.0, 0.125, float(np.float32(0.8)), 0.0] and all(a is b for a, b in zip(keep, tensors))
    ops.run((op, keep))
    op, keep = mk(init=True, prev_out=None, prev_bytes=None)
    assert op.p[2] is None and op.p[3] is None and op.i[3] == ops.STEADY_INIT
    ops.run((op, keep))
    for kw in (dict(), dict(r=0), dict(r=8), dict(hard=True, inv32=0.0), dict(init=True), dict(H=1, W=8), dict(H=512, W=512),
               dict(s32=0.0), dict(s32=1.0), dict(lo32=0.0, inv32=0.0), dict(lo32=255.0, inv32=3.0e38)):
        ops.run(mk(**kw))
    # the builder: dtype, shape, the picture
    for call in (lambda: mk(styled=frame(dtype=torch.float32)), lambda: mk(source=frame(H, W + 8)), lambda: mk(out=frame(H + 1, W)),
                 lambda: mk(prev_out=frame(dtype=torch.bfloat16)), lambda: mk(prev_bytes=plane(dtype=torch.int8)),
                 lambda: mk(next_bytes=torch.zeros(H, W, 3, dtype=torch.uint8)), lambda: mk(prev_out=None), lambda: mk(prev_bytes=None),
                 lambda: mk(show=True), lambda: mk(picture=frame()), lambda: mk(show=True, picture=frame(H, 2 * W)),
                 lambda: mk(r=9), lambda: mk(r=-1), lambda: mk(r=1.5), lambda: mk(init=True, next_bytes=None)):
        with pytest.raises((ValueError, AttributeError)):
            call()
    # the launcher
    bad("multiple of 8", mk(H=24, W=36))
    bad("below 2\\^31", _big(ops, frame(), plane()))
    op, keep = mk()
    op.i[2] = 9
    bad("radius 9, need 0..8", (op, keep))
    op, keep = mk()
    op.i[2] = -1
    bad("radius -1", (op, keep))
    op, keep = mk()
    op.i[3] = 8
    bad("unknown flag bits", (op, keep))
    op, keep = mk()
    op.i[0] = 0
    bad("non-positive size", (op, keep))
    for k in range(6):
        op, keep = mk()
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
        if k in (2, 3):                                  # ... but not with the init flag
            op, keep = mk(init=True)
            op.p[k] = None
            ops.run((op, keep))
    op, keep = mk(show=True, picture=frame())
    op.p[6] = None
    bad("pointer 6 is null", (op, keep))
    op, keep = mk()
    op.p[0] = op.p[0] + 8
    bad("pointer 0 is not aligned", (op, keep))
    op, keep = mk()
    op.p[5] = op.p[5] + 4
    bad("pointer 5 is not aligned", (op, keep))
    x, y = frame(), plane()
    bad("output frame 4 overlaps input frame 2", mk(prev_out=x, out=x))
    bad("output frame 4 overlaps input frame 0", mk(styled=x, out=x))
    bad("output frame 4 overlaps input frame 1", mk(source=x, out=x))
    bad("next_bytes overlaps prev_bytes", mk(prev_bytes=y, next_bytes=y))
    bad("output frame 6 overlaps input frame 0", mk(styled=x, show=True, picture=x))
    bad("picture overlaps the output frame", mk(out=x, show=True, picture=x))
    two = torch.zeros(2, 3, H, W, dtype=torch.float16)
    ops.run(mk(prev_out=two[0], out=two[1]))
    for kw in (dict(lo32=-1.0), dict(lo32=float("nan")), dict(lo32=float("inf")), dict(inv32=-0.5), dict(inv32=float("inf")),
               dict(inv32=float("nan"))):
        bad("must be finite and not negative", mk(**kw))
    for s in (-0.1, 1.5, float("nan"), float("inf")):
        bad("strength = .* must lie in \\[0, 1\\]", mk(s32=s))


def _big(ops, x, y):
    """a record whose sizes say 3 H W = 2^31 (dry run: the tensors are never touched)"""
    op, keep = ops.frame_steady(x, x.clone(), x.clone(), y, x.clone(), y.clone(), H=24, W=40, lo32=2.0, inv32=0.125, s32=0.8, r=2)
    op.i[0], op.i[1] = 1 << 15, 21848                    # 3 * 32768 * 21848 = 2^31 + 98304; W % 8 == 0
    return op, keep


# ----------------------------------------------------------------------------- the wrapper on the mock components
def pre(frame):
    """the mock image processor's frame, as the delay line keeps it"""
    return (2.0 * frame - 1.0).to(torch.float16)


def frames_of(k, seed):
    import pipeline_mocks as M
    return list(M.frames(k, seed=seed))


def moving(frames):
    """camera-like frames for the mocks: the first one plus a little noise, a band of the frame's own content"""
    out = []
    g = torch.Generator().manual_seed(5)
    for k, f in enumerate(frames):
        x = (frames[0] + torch.randint(-1, 2, f.shape, generator=g) / 255.0).clamp(0, 1)
        x[:, :, 8 * k:8 * k + 16] = f[:, :, 8 * k:8 * k + 16]
        out.append(x)
    return out


SET = dict(lo=2.0, hi=10.0, strength=0.8, radius=2, show=False)


@pytest.mark.parametrize("output_type", ["u8", "pil", "jpeg", "pt", "np"])
def test_wrapper_serves_every_output_type(monkeypatch, output_type):
    import pipeline_mocks as M
    from live2diff_amd.jpeg import encode_ref
    warm, frames = M.frames(8, seed=7), moving(frames_of(4, seed=8))
    torch.manual_seed(123)
    w = build(monkeypatch, 2, output_type=output_type)
    assert w.steady is None
    w.set_steady()
    assert w.steady == SET and w.stream.matte_tap is w._matte_line is not None
    w.prepare(warm, "a prompt")
    state, changed = None, 0
    for t, f in enumerate(frames):
        got = w(f)
        source = pre(frames[t - 1] if t else warm[-1])
        out, state = SD.steady_ref(w.stream.prev_image_result, source, state, init=t == 0, **SET)
        changed += not np.array_equal(out[0], w.stream.prev_image_result[0].to(torch.float16).numpy())
        assert same(w._steady_state[0], state[0]) and same(w._steady_state[1], state[1])
        lt = torch.from_numpy(out)
        u8 = egress_ref(lt)[0].numpy()
        if output_type == "u8":
            assert got.dtype == np.uint8 and np.array_equal(got, u8)
        elif output_type == "pil":
            assert got.size == (M.W, M.H) and np.array_equal(np.array(got), u8)
        elif output_type == "jpeg":
            assert got == encode_ref(u8, w.jpeg_quality)
        elif output_type == "pt":
            assert torch.equal(got, (lt / 2 + 0.5).clamp(0, 1)[0])
        else:
            assert np.array_equal(got, (lt / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float().numpy()[0])
    # steady does something on every frame but the init frame and the one behind it, whose source follows the unrelated last
    # warm-up frame: a hard cut, which passes by itself
    assert changed == len(frames) - 2


def test_wrapper_latent_raises_and_keywords(monkeypatch):
    import pipeline_mocks as M
    w = build(monkeypatch, 2, output_type="latent")
    with pytest.raises(ValueError, match="set_steady.*'pil'.*'u8'.*'jpeg'"):
        w.set_steady()
    assert w.steady is None and w._matte_line is None
    w.output_type = "u8"
    w.set_steady(3, 12, strength=0.5, radius=0, show=True)
    assert w.steady == dict(lo=3.0, hi=12.0, strength=0.5, radius=0, show=True)
    w.output_type = "latent"                                         # changed behind its back: the frame says so
    w.prepare(M.frames(8, seed=7), "a prompt")
    with pytest.raises(ValueError, match="clear_steady"):
        w(colour(1))
    for args, kw in (((11, 10), {}), ((2, 300), {}), ((), dict(strength=2.0)), ((), dict(radius=9)), ((), dict(radius=1.5))):
        with pytest.raises(ValueError, match="steady: "):
            w.set_steady(*args, **kw)
    # the constructor keyword
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    import inspect
    assert inspect.signature(Wrapper.__init__).parameters["steady"].default is None
    real = Wrapper.from_components
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, steady=dict(lo=1, hi=5, radius=1), **kw)))
    w = build(monkeypatch, 2)
    assert w.steady == dict(lo=1.0, hi=5.0, strength=0.8, radius=1, show=False) and w._matte_line is not None
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, steady=(2, 10), **kw)))
    with pytest.raises(ValueError, match="steady="):
        build(monkeypatch, 2)


def test_wrapper_steady_runs_behind_the_lock_and_before_the_matte(monkeypatch):
    import pipeline_mocks as M
    from live2diff_amd import color_lock as CL
    from live2diff_amd.matte import composite_ref
    warm, frames = M.frames(8, seed=7), moving(frames_of(5, seed=9))
    torch.manual_seed(123)
    w = build(monkeypatch, 2)
    w.set_matte(0.3, 0.7, feather=2)
    w.set_color_lock("source")
    w.set_steady()
    w.prepare(warm, "a prompt")
    state = None
    for t, f in enumerate(frames[:4]):
        got = w(f)
        slot = w._matte_line.last
        assert torch.equal(slot.source, pre(frames[t - 1] if t else warm[-1]).float())          # one line, one take per output
        locked, _ = CL.lock_ref(w.stream.prev_image_result, None, mode="source", source=slot.source)
        out, state = SD.steady_ref(locked, slot.source, state, init=t == 0, **SET)
        want = composite_ref(torch.from_numpy(out), slot.source[None], slot.depth[None], 0.3, 0.7, feather=2)[0]
        assert np.array_equal(got, want)
        if t > 1:                                                     # (frame 1 follows the unrelated warm-up frame: it passes)
            plain = composite_ref(torch.from_numpy(locked), slot.source[None], slot.depth[None], 0.3, 0.7, feather=2)[0]
            assert not np.array_equal(got, plain)
    assert w._matte_line.tapped == w._matte_line.taken == 4
    # m == 0 everywhere: the real picture, untouched by steady
    w.set_matte(0, 0, keep="far")
    assert np.array_equal(w(frames[4]), egress_ref(pre(frames[3]))[0].numpy())


def test_wrapper_dropped_frame_reuses_the_steady_frame(monkeypatch):
    import pipeline_mocks as M
    frames = moving(frames_of(7, seed=10))
    torch.manual_seed(123)
    w = build(monkeypatch, 2, drop={2, 3, 5})
    w.set_steady()
    w.prepare(M.frames(8, seed=7), "a prompt")
    got, states, last = [], [], []
    for f in frames:
        got.append(w(f))
        states.append(w._steady_state)
        last.append(w._steady_last)
    for t in (2, 3, 5):
        assert np.array_equal(got[t], got[t - 1]) and last[t] is last[t - 1] and states[t] is states[t - 1], t
    for t in (1, 4, 6):
        assert not np.array_equal(got[t], got[t - 1]) and states[t] is not states[t - 1], t
    assert w._matte_line.tapped == w._matte_line.taken == 4


def test_wrapper_prepare_and_set_steady_restart(monkeypatch):
    import pipeline_mocks as M
    warm, frames = M.frames(8, seed=7), moving(frames_of(4, seed=11))
    torch.manual_seed(123)
    w = build(monkeypatch, 2)
    w.set_steady()
    w.prepare(warm, "a prompt")
    for f in frames[:3]:
        w(f)
    assert not w._steady_init and not same(w._steady_state[0], w.stream.prev_image_result[0].to(torch.float16).numpy())
    w.prepare(warm, "a prompt")
    assert w._steady_init and w._steady_state is None and w._steady_last is None and w.steady == SET
    got = w(frames[3])
    assert np.array_equal(got, egress_ref(w.stream.prev_image_result)[0].numpy())               # the first frame passes
    assert same(w._steady_state[0], w.stream.prev_image_result[0].to(torch.float16).numpy())
    w(frames[0])
    w.set_steady()
    got = w(frames[1])
    assert np.array_equal(got, egress_ref(w.stream.prev_image_result)[0].numpy())


def test_wrapper_line_is_shared_and_released(monkeypatch):
    w = build(monkeypatch, 2)
    tap = lambda: w.stream.matte_tap
    w.set_steady()
    line = w._matte_line
    assert line is not None and line is tap()
    w.set_matte(0.3, 0.7)
    w.set_color_lock("source")
    assert w._matte_line is line is tap()
    w.clear_matte()
    assert w._matte_line is line is tap()                                 # steady and the lock keep it
    w.clear_color_lock()
    assert w._matte_line is line is tap()                                 # steady keeps it
    w.set_color_lock("ema")                                               # (a mode that needs no line lets go of nothing)
    assert w._matte_line is line is tap()
    w.clear_steady()
    assert w.steady is None and w._matte_line is None and tap() is None
    # the others first
    w.set_color_lock("source")
    line = w._matte_line
    w.set_steady()
    assert w._matte_line is line
    w.clear_steady()
    assert w._matte_line is line is tap()                                 # the lock keeps it
    w.set_matte(0.3, 0.7)
    w.set_steady()
    w.clear_color_lock()
    w.clear_steady()
    assert w._matte_line is line is tap()                                 # the matte keeps it
    w.clear_matte()
    assert w._matte_line is None and tap() is None


def test_wrapper_without_steady_is_the_twin(monkeypatch):
    import pipeline_mocks as M
    warm, frames = M.frames(8, seed=7), moving(frames_of(6, seed=13))

    def run(steady):
        torch.manual_seed(123)
        w = build(monkeypatch, 2)
        if steady:
            w.set_steady()
        w.prepare(warm, "a prompt")
        out = [w(f) for f in frames[:4]]
        if steady:
            w.clear_steady()
        torch.manual_seed(77)                    # (the host path draws its re-noising from the global generator)
        return w, out + [w(f) for f in frames[4:]]

    (w, got), (twin, plain) = run(True), run(False)
    # the init frame passes, and so does the one behind it: its source follows the unrelated last warm-up frame, a hard cut
    assert all(np.array_equal(a, b) for a, b in zip(got[:2], plain[:2]))
    assert not any(np.array_equal(a, b) for a, b in zip(got[2:4], plain[2:4]))
    assert all(np.array_equal(a, b) for a, b in zip(got[4:], plain[4:]))
    assert w._steady is None and w._steady_dev is None and w._steady_state is None and w._steady_last is None
    assert w._matte_line is None and w.stream.matte_tap is None
    # mid-stream (N = 2): the line starts with the next frame, whose output belongs to a frame the line has not seen -- it passes,
    # the sequence has not started and the state holds nothing of the foreign slot
    w.set_steady()
    got = w(frames[0])
    assert np.array_equal(got, egress_ref(w.stream.prev_image_result)[0].numpy())
    assert not w._matte_line.last_own and w._steady_init and w._steady_state is None and w._steady_last is None
    # the first output with its own slot is the init frame: it passes, and the state is that frame and its own source's bytes
    got = w(frames[1])
    assert np.array_equal(got, egress_ref(w.stream.prev_image_result)[0].numpy())
    assert w._matte_line.last_own and not w._steady_init
    assert same(w._steady_state[0], w.stream.prev_image_result[0].to(torch.float16).numpy())
    assert same(w._steady_state[1], SD.source_bytes(pre(frames[0])))
    # ... and the one after it is the first that differs
    got = w(frames[2])
    assert not np.array_equal(got, egress_ref(w.stream.prev_image_result)[0].numpy())
    assert same(w._steady_state[1], SD.source_bytes(pre(frames[1])))


@pytest.mark.parametrize("n_steps", [1, 2, 3])
@pytest.mark.parametrize("kind", ["unrelated", "moving"])
def test_wrapper_mid_stream_start_never_holds_a_foreign_source(monkeypatch, n_steps, kind):
    """`set_steady()` with its defaults after two plain frames.  The first N - 1 outputs behind it belong to frames that entered
    before the delay line existed: `take()` hands out the oldest entry it has, another frame's, and steady must not start on
    it.  On unrelated frames (everything moves between any two) every output equals the unsteadied bytes -- the largest byte
    difference is 0 on calls 3 .. 7 for N = 1, 2 and 3; a sequence started on the foreign slot measured zero motion on the
    first own slot and held it to the output before (on these frames 30 levels on call 4 at N = 2; 26 and 30 on calls 4 and 5 at
    N = 3).  On moving-camera frames the first
    output with its own slot passes as the init frame and the one after it is the first that differs."""
    import pipeline_mocks as M
    frames = frames_of(7, seed=21)
    if kind == "moving":
        frames = moving(frames)
    torch.manual_seed(123)
    w = build(monkeypatch, n_steps)
    w.prepare(M.frames(8, seed=7), "a prompt")
    for f in frames[:2]:
        w(f)
    w.set_steady()
    own, diffs = [], []
    for t, f in enumerate(frames[2:]):
        got = w(f)
        plain = egress_ref(w.stream.prev_image_result)[0].numpy()
        own.append(w._matte_line.last_own)
        diffs.append(int(np.abs(got.astype(int) - plain.astype(int)).max()))
        if own[-1]:                              # the state is the output's own source, always
            assert same(w._steady_state[1], SD.source_bytes(pre(frames[2 + t - (n_steps - 1)])))
        else:
            assert w._steady_init and w._steady_state is None and w._steady_last is None
    print(f"N = {n_steps}, {kind}: last_own {own}, largest byte difference to the unsteadied frame {diffs}")
    assert own == [False] * (n_steps - 1) + [True] * (5 - (n_steps - 1))
    if kind == "unrelated":
        assert diffs == [0] * 5
    else:
        assert diffs[:n_steps] == [0] * n_steps and all(d > 0 for d in diffs[n_steps:])
