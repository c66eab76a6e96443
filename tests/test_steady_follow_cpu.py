"""CPU tests (-m "not gpu") of follow (live2diff_amd/steady.py): `motion_ref` recovers a pan exactly, its
tie rules and its bias, `follow_ref` against `steady_ref` on a still source and against it under a pan (what the feature is for),
odd shapes, `check_follow`, the builders and launchers of ops 55 and 56 (dry-run), and `set_steady_follow` on the wrapper built
from the mock components of tests/pipeline_mocks.py.  The sequence generator is shared with tests/test_gpu_steady_follow.py."""
import functools
import os

import numpy as np
import pytest
import torch

from live2diff_amd import steady as SD
from test_matte_cpu import build
from test_steady_cpu import SET, frames_of, pre, same

K = 5                                            # frames per sequence; the first one is the init frame
LO, HI, STRENGTH = 2, 10, 0.8
PAD = 40                                         # the canvas around a frame: room for 8 frames of a pan by up to 5 pixels


# ----------------------------------------------------------------------------- frames
def texture(rng, H, W):
    """uint8 [3, H + 2 PAD, W + 2 PAD]: random bytes box-smoothed 3 x 3 (structure a block can be matched by)"""
    a = rng.integers(0, 256, (3, H + 2 * PAD, W + 2 * PAD)).astype(np.int64)
    p = np.pad(a, ((0, 0), (1, 1), (1, 1)), mode="edge")
    s = sum(p[:, i:i + a.shape[1], j:j + a.shape[2]] for i in range(3) for j in range(3))
    return ((2 * s + 9) // 18).astype(np.uint8)


def view(canvas, H, W, oy, ox):
    """the [3,H,W] frame of a camera whose corner stands at (PAD + oy, PAD + ox) of the canvas"""
    return canvas[:, PAD + oy:PAD + oy + H, PAD + ox:PAD + ox + W]


def to16(b):
    return (np.clip(b, 0, 255) / 127.5 - 1.0).astype(np.float16)


def interior(H, W, R):
    """the blocks whose window plus search range lies inside the image"""
    return [(i, j) for i in range(-(-H // 8)) for j in range(-(-W // 8))
            if 8 * i - 4 - R >= 0 and 8 * i + 11 + R <= H - 1 and 8 * j - 4 - R >= 0 and 8 * j + 11 + R <= W - 1]


@functools.lru_cache(maxsize=None)
def sequence(H, W):
    """(sources, styled): K fp16 [3,H,W] frames each, read-only.  Frame 1 is frame 0 panned by (3, -2) plus +-1 level of noise;
    frame 2 is frame 1 again plus noise (a still stretch) with, on the right quarter, a ramp of 0..14 levels (the ramp of the
    weight); frame 3 is unrelated (a hard cut); frame 4 is frame 3 panned by (-1, 1) with a band of fresh content W // 4 wide.
    A styled frame is 0.6 N(0, 1): values beyond +-1 included."""
    rng = np.random.default_rng(H * 1013 + W)
    one, two = texture(rng, H, W), texture(rng, H, W)
    q = max(W // 4, 1)
    ramp = np.rint(np.linspace(0, 14, q)).astype(np.int64)
    noise = lambda: rng.integers(-1, 2, (3, H, W))
    b = [view(one, H, W, 0, 0).astype(np.int64), view(one, H, W, -3, 2) + noise(), view(one, H, W, -3, 2) + noise(),
         view(two, H, W, 0, 0).astype(np.int64), view(two, H, W, 1, -1) + noise()]
    b[2][:, :, W - q:] += ramp
    b[4][:, :, q:2 * q] = rng.integers(0, 256, (3, H, q))
    sources, styled = [], []
    for k in range(K):
        x, s = to16(b[k]), (0.6 * rng.standard_normal((3, H, W))).astype(np.float16)
        for a in (x, s):
            a.setflags(write=False)
        sources.append(x)
        styled.append(s)
    return tuple(sources), tuple(styled)


@functools.lru_cache(maxsize=None)
def oracle(H, W, search, bias, radius, lo=LO, hi=HI, strength=STRENGTH, show=False):
    """`follow_ref` over the sequence, frame 0 as the init frame: ([fp16 [1,3,H,W] outputs], [(out, bytes) states], [fields])"""
    sources, styled = sequence(H, W)
    outs, states, fields, state = [], [], [], None
    for k in range(K):
        o, state, f = SD.follow_ref(styled[k], sources[k], state, search=search, bias=bias, lo=lo, hi=hi, strength=strength,
                                    radius=radius, show=show, init=k == 0)
        for a in (o, f, *state):
            a.setflags(write=False)
        outs.append(o)
        states.append(state)
        fields.append(f)
    return outs, states, fields


def motion_direct(b, bp, R, bias):
    """the field by loops over blocks, candidates and pixels, in Python integers"""
    _, H, W = b.shape
    cl = lambda v, n: min(max(v, 0), n - 1)
    cands = SD.follow_candidates(R)
    out = np.zeros((-(-H // 8), -(-W // 8), 2), dtype=np.int8)
    b, bp = b.astype(int), bp.astype(int)
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            best = None
            for rank, (dy, dx) in enumerate(cands):
                ys, xs = range(8 * i - 4, 8 * i + 12), range(8 * j - 4, 8 * j + 12)
                now = b[:, [cl(y, H) for y in ys]][:, :, [cl(x, W) for x in xs]]
                was = bp[:, [cl(y + dy, H) for y in ys]][:, :, [cl(x + dx, W) for x in xs]]
                key = (int(np.abs(now - was).sum()) + bias * (abs(dy) + abs(dx))) * 512 + rank
                if best is None or key < best[0]:
                    best = (key, dy, dx)
            out[i, j] = best[1:]
    return out


# ----------------------------------------------------------------------------- motion_ref
def test_candidates_and_constants():
    assert (SD.FOLLOW_BLOCK, SD.FOLLOW_APRON, SD.FOLLOW_MAX_SEARCH, SD.FOLLOW_MAX_BIAS) == (8, 4, 8, 4096)
    for R in (1, 4, 8):
        c = SD.follow_candidates(R)
        assert len(c) == (2 * R + 1) ** 2 == len(set(c)) and c[0] == (0, 0) and len(c) - 1 <= 288
        assert c == sorted(c, key=lambda v: (abs(v[0]) + abs(v[1]), v[0], v[1]))
    assert SD.follow_candidates(1)[:5] == [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0)]
    assert (768 * 255 + 4096 * 16) * 512 + 288 < 1 << 27


@pytest.mark.parametrize("shape,R,bias", [((8, 8), 8, 0), ((20, 40), 2, 256), ((24, 16), 3, 7)])
def test_motion_ref_against_direct_loops(shape, R, bias):
    H, W = shape
    sources, _ = sequence(H, W)
    for k in (1, 4):
        b, bp = SD.source_bytes(sources[k]), SD.source_bytes(sources[k - 1])
        got = SD.motion_ref(b, bp, R, bias)
        assert got.dtype == np.int8 and np.array_equal(got, motion_direct(b, bp, R, bias)), k


@pytest.mark.parametrize("v,R", [((3, -2), 4), ((0, 1), 1), ((-8, 8), 8)])
def test_vector_recovery_under_a_pan(v, R):
    """the content moves by `v` per frame: every block whose window plus search range lies inside the image looks back by -v"""
    H, W = 64, 96
    canvas = texture(np.random.default_rng(3), H, W)
    prev, now = view(canvas, H, W, 0, 0), view(canvas, H, W, -v[0], -v[1])          # now[y, x] == prev[y - v0, x - v1]
    field = SD.motion_ref(np.ascontiguousarray(now), np.ascontiguousarray(prev), R, 256)
    assert field.shape == (8, 12, 2)
    inner = interior(H, W, R)
    assert len(inner) >= 8
    for i, j in inner:
        assert tuple(field[i, j]) == (-v[0], -v[1]), (i, j, field[i, j])


def test_tie_rules():
    flat = np.full((3, 24, 40), 77, dtype=np.uint8)
    assert not SD.motion_ref(flat, flat, 8, 0).any() and not SD.motion_ref(flat, flat + 1, 8, 0).any()
    H, W = 48, 96
    pat = np.ascontiguousarray(np.broadcast_to(np.tile(np.array([10, 80, 200, 120], dtype=np.uint8), W // 4), (3, H, W)))
    assert not SD.motion_ref(pat, pat, 8, 0).any()                               # period 4: (0, +-4), (0, +-8) cost 0 too
    field = SD.motion_ref(pat, np.roll(pat, 2, axis=2), 8, 0)                    # (0, -2) and (0, 2) both match: the smaller dx
    inner = interior(H, W, 8)
    assert len(inner) >= 8 and all(tuple(field[i, j]) == (0, -2) for i, j in inner)


def test_bias_keeps_noise_from_making_vectors():
    rng = np.random.default_rng(1)
    a, b = (np.clip(np.rint(128 + rng.normal(0, 2, (3, 64, 96))), 0, 255).astype(np.uint8) for _ in range(2))
    assert not SD.motion_ref(a, b, 8, 256).any()
    moved = np.abs(SD.motion_ref(a, b, 8, 0).astype(int)).sum(-1) > 0
    print(f"bias 0: {moved.mean():.2f} of the blocks have a vector")
    assert moved.mean() > 0.5


# ----------------------------------------------------------------------------- follow_ref
def test_still_source_is_steady_ref():
    H, W = 40, 72
    rng = np.random.default_rng(5)
    src = to16(view(texture(rng, H, W), H, W, 0, 0))
    styled = [(0.6 * rng.standard_normal((3, H, W))).astype(np.float16) for _ in range(4)]
    for r in (0, 2, 8):
        kw = dict(lo=LO, hi=HI, strength=STRENGTH, radius=r)
        f_state = s_state = None
        for k in range(4):
            fo, f_state, field = SD.follow_ref(styled[k], src, f_state, search=8, bias=256, init=k == 0, **kw)
            so, s_state = SD.steady_ref(styled[k], src, s_state, init=k == 0, **kw)
            assert not field.any() and same(fo, so) and same(f_state[0], s_state[0]) and same(f_state[1], s_state[1])
            assert k == 0 or not same(fo[0], styled[k])
    # an all-zero field is the identity of the warp
    assert same(SD.warp_ref(styled[0], np.zeros((5, 9, 2), dtype=np.int8)), styled[0])


def test_follow_holds_under_a_pan_where_steady_does_not():
    """a pan by (3, -2) per frame over 8 frames; the styled frame is an affine function of the source plus N(0, 0.05).  Away
    from the border the noise that is left at frame 7 is at most half of plain steady's (which holds nothing there): the EMA
    bound for strength 0.8 is sqrt(0.2 / 1.8) = 0.33, and seven frames of transient leave about 0.4"""
    H, W, v, n = 64, 96, (3, -2), 8
    rng = np.random.default_rng(11)
    canvas = texture(rng, H, W)
    kw = dict(lo=LO, hi=HI, strength=STRENGTH, radius=2)
    f_state = s_state = None
    for k in range(n):
        b = view(canvas, H, W, -k * v[0], -k * v[1])
        src = to16(b)
        clean = 0.8 * src.astype(np.float32) + 0.05
        styled = (clean + rng.normal(0, 0.05, clean.shape)).astype(np.float16)
        fo, f_state, field = SD.follow_ref(styled, src, f_state, search=4, bias=256, init=k == 0, **kw)
        so, s_state = SD.steady_ref(styled, src, s_state, init=k == 0, **kw)
        if k:
            assert all(tuple(field[i, j]) == (-v[0], -v[1]) for i, j in interior(H, W, 4))
    m = 24                                     # 7 frames x 3 pixels of travel, and a block that leans on the border matches nothing
    noise = lambda o: float((o[0].astype(np.float32) - clean)[:, m:H - m, m:W - m].std())
    nf, ns = noise(fo), noise(so)
    print(f"noise std away from the border at frame {n - 1}: follow {nf:.4f}, steady {ns:.4f}, ratio {nf / ns:.3f}")
    assert ns > 0.045 and nf <= 0.5 * ns


@pytest.mark.parametrize("shape,R", [((8, 8), 8), ((20, 40), 4), ((40, 72), 4)])
def test_shapes_show_and_init(shape, R):
    H, W = shape
    sources, styled = sequence(H, W)
    outs, states, fields = oracle(H, W, R, 256, 2)
    shown, shown_states, _ = oracle(H, W, R, 256, 2, show=True)
    Hb, Wb = -(-H // 8), W // 8
    for k in range(K):
        assert fields[k].shape == (Hb, Wb, 2) and fields[k].dtype == np.int8 and np.abs(fields[k]).max() <= R
        assert outs[k].shape == (1, 3, H, W) and outs[k].dtype == np.float16 and states[k][1].dtype == np.uint8
        assert same(shown_states[k][0], states[k][0]) and same(shown_states[k][1], states[k][1])
        assert same(states[k][1], SD.source_bytes(sources[k]))                   # the bytes where they are, not displaced
    # show: fp16(2 w - 1) of the weight along the vectors, in all three channels
    b, (P, bp) = SD.source_bytes(sources[1]), states[0]
    w = SD.weight_ref(b, SD.warp_ref(bp, fields[1]), lo=LO, hi=HI, radius=2)
    pic = (np.float32(2.0) * w - np.float32(1.0)).astype(np.float16)
    assert all(same(shown[1][0, c], pic) for c in range(3))
    # init ignores the state, and searches nothing
    o, new, f = SD.follow_ref(styled[1], sources[1], None, search=R, bias=256, lo=LO, hi=HI, strength=STRENGTH, radius=2, init=True)
    o2, new2, _ = SD.follow_ref(styled[1], sources[1], states[3], search=R, bias=256, lo=LO, hi=HI, strength=STRENGTH, radius=2, init=True)
    assert same(o[0], styled[1]) and same(o, o2) and same(new[0], new2[0]) and same(new[1], new2[1]) and not f.any()
    if shape == (40, 72):                                                         # the pan of frame 1 is found where it can be
        assert all(tuple(fields[1][i, j]) == (-3, 2) for i, j in interior(H, W, R)) and len(interior(H, W, R)) >= 8
        assert not fields[2][:, :Wb - Wb // 4 - 1].any() and fields[4].any()


def test_check_follow():
    assert SD.check_follow() == dict(search=4, bias=256)
    assert SD.check_follow(np.int64(8), np.int32(0)) == dict(search=8, bias=0) and SD.check_follow(1, 4096) == dict(search=1, bias=4096)
    for args, match in (((0,), "search=0.*1 to 8"), ((9,), "search=9"), ((True,), "search=True"), ((4.0,), "search=4.0"), (("4",), "search='4'"),
                        ((4, -1), "bias=-1.*0 to 4096"), ((4, 4097), "bias=4097"), ((4, True), "bias=True"), ((4, 256.0), "bias=256.0")):
        with pytest.raises(ValueError, match=match):
            SD.check_follow(*args)
    with pytest.raises(ValueError):
        SD.motion_ref(np.zeros((3, 8, 8), np.uint8), np.zeros((3, 8, 16), np.uint8), 4, 256)
    with pytest.raises(ValueError):
        SD.warp_ref(np.zeros((3, 8, 8), np.uint8), np.zeros((1, 1, 2), np.int16))


# ----------------------------------------------------------------------------- the builders and the launchers
@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_launcher_checks(dry_run):
    from live2diff_amd import _lib, ops
    assert (_lib.OP_FRAME_MOTION, _lib.OP_FRAME_STEADY_FOLLOW) == (55, 56)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_FRAME_MOTION = 55," in hdr and "L2D_OP_FRAME_STEADY_FOLLOW = 56," in hdr
    assert all(f"#define L2D_FOLLOW_{n} {v}" in hdr for n, v in (
        ("BLOCK", ops.FOLLOW_BLOCK), ("APRON", ops.FOLLOW_APRON), ("MAX_SEARCH", ops.FOLLOW_MAX_SEARCH), ("MAX_BIAS", ops.FOLLOW_MAX_BIAS)))
    H, W = 20, 40

    def frame(H=H, W=W, dtype=torch.float16):
        return torch.zeros(3, H, W, dtype=dtype)

    def plane(H=H, W=W, dtype=torch.uint8):
        return torch.zeros(3, H, W, dtype=dtype)

    def fld(H=H, W=W, dtype=torch.int8):
        return torch.zeros((H + 7) // 8, W // 8, 2, dtype=dtype)

    def motion(H=H, W=W, **kw):
        args = dict(source=frame(H, W), prev_bytes=plane(H, W), field=fld(H, W), H=H, W=W, search=4, bias=256)
        args.update(kw)
        return ops.frame_motion(*[args.pop(k) for k in ("source", "prev_bytes", "field")], **args)

    def follow(H=H, W=W, **kw):
        args = dict(styled=frame(H, W), source=frame(H, W), prev_out=frame(H, W), prev_bytes=plane(H, W), out=frame(H, W),
                    next_bytes=plane(H, W), field=fld(H, W), H=H, W=W, lo32=2.0, inv32=0.125, s32=0.8, r=2)
        args.update(kw)
        return ops.frame_steady_follow(*[args.pop(k) for k in ("styled", "source", "prev_out", "prev_bytes", "out", "next_bytes", "field")], **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    # the records
    t = [frame(), plane(), fld()]
    op, keep = ops.frame_motion(*t, H=H, W=W, search=8, bias=4096)
    assert op.kind == 55 and [op.p[j] for j in range(4)] == [x.data_ptr() for x in t] + [None]
    assert [op.i[j] for j in range(5)] == [H, W, 8, 4096, 0] and all(a is b for a, b in zip(keep, t))
    ops.run((op, keep))
    t = [frame(), frame(), frame(), plane(), frame(), plane(), frame(), fld()]
    op, keep = ops.frame_steady_follow(*t[:6], t[7], H=H, W=W, lo32=np.float32(2), inv32=np.float32(0.125), s32=np.float32(0.8), r=3,
                                       hard=True, show=True, picture=t[6])
    assert op.kind == 56 and [op.p[j] for j in range(9)] == [x.data_ptr() for x in t] + [None]
    assert [op.i[j] for j in range(5)] == [H, W, 3, ops.STEADY_HARD | ops.STEADY_SHOW, 0]
    assert [op.f[j] for j in range(4)] == [2.0, 0.125, float(np.float32(0.8)), 0.0]
    ops.run((op, keep))
    for kw in (dict(), dict(search=1, bias=0), dict(H=1, W=8), dict(H=8, W=8, search=8), dict(H=512, W=512)):
        ops.run(motion(**kw))
    for kw in (dict(), dict(r=0), dict(r=8), dict(hard=True, inv32=0.0), dict(H=1, W=8), dict(H=512, W=512), dict(s32=0.0), dict(s32=1.0)):
        ops.run(follow(**kw))
    # the builders
    for call in (lambda: motion(source=frame(dtype=torch.float32)), lambda: motion(prev_bytes=plane(dtype=torch.int8)),
                 lambda: motion(field=fld(dtype=torch.uint8)), lambda: motion(field=torch.zeros(2, 5, 2, dtype=torch.int8)),
                 lambda: motion(search=0), lambda: motion(search=9), lambda: motion(search=1.5), lambda: motion(search=True),
                 lambda: motion(bias=-1), lambda: motion(bias=4097), lambda: motion(bias=True),
                 lambda: follow(styled=frame(dtype=torch.float32)), lambda: follow(prev_out=frame(H, W + 8)),
                 lambda: follow(next_bytes=torch.zeros(H, W, 3, dtype=torch.uint8)), lambda: follow(field=fld(H + 8, W)),
                 lambda: follow(prev_out=None), lambda: follow(show=True), lambda: follow(picture=frame()), lambda: follow(r=9),
                 lambda: follow(r=-1), lambda: follow(init=True)):
        with pytest.raises((ValueError, AttributeError, TypeError)):
            call()
    # the launcher of op 55
    for k, v, match in ((2, 0, "search 0, need 1..8"), (2, 9, "search 9"), (3, -1, "bias -1, need 0..4096"), (3, 4097, "bias 4097"),
                        (0, 0, "non-positive size"), (1, 36, "multiple of 8")):
        op, keep = motion()
        op.i[k] = v
        bad(match, (op, keep))
    for k in range(3):
        op, keep = motion()
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
    for k, off in ((0, 8), (1, 4)):
        op, keep = motion()
        op.p[k] = op.p[k] + off
        bad("not aligned", (op, keep))
    op, keep = motion()
    op.p[2] = op.p[2] + 1                                # the field takes any alignment
    ops.run((op, keep))
    raw = torch.zeros(3 * H * W, dtype=torch.uint8)
    over = raw[8:8 + 30].view(torch.int8).view(3, 5, 2)
    bad("field overlaps an input", motion(prev_bytes=raw.view(3, H, W), field=over))
    halves = torch.zeros(3 * H * W, dtype=torch.float16)
    over16 = halves[8:8 + 15].view(torch.int8).view(3, 5, 2)
    bad("field overlaps an input", motion(source=halves.view(3, H, W), field=over16))
    # the launcher of op 56
    for k, v, match in ((2, 9, "radius 9, need 0..8"), (2, -1, "radius -1"), (3, 4, "unknown flag bits"), (3, 8, "unknown flag bits"),
                        (0, 0, "non-positive size"), (1, 36, "multiple of 8")):
        op, keep = follow()
        op.i[k] = v
        bad(match, (op, keep))
    for k in (0, 1, 2, 3, 4, 5, 7):
        op, keep = follow()
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
    op, keep = follow(show=True, picture=frame())
    op.p[6] = None
    bad("pointer 6 is null", (op, keep))
    for k, off in ((0, 8), (2, 8), (3, 4), (5, 4)):
        op, keep = follow()
        op.p[k] = op.p[k] + off
        bad(f"pointer {k} is not aligned", (op, keep))
    x, y = frame(), plane()
    bad("output frame 4 overlaps input frame 2", follow(prev_out=x, out=x))
    bad("output frame 4 overlaps input frame 0", follow(styled=x, out=x))
    bad("output frame 4 overlaps input frame 1", follow(source=x, out=x))
    bad("next_bytes overlaps prev_bytes", follow(prev_bytes=y, next_bytes=y))
    bad("output frame 6 overlaps input frame 0", follow(styled=x, show=True, picture=x))
    bad("picture overlaps the output frame", follow(out=x, show=True, picture=x))
    bad("field overlaps an output", follow(out=halves.view(3, H, W), field=over16))
    bad("field overlaps an output", follow(next_bytes=raw.view(3, H, W), field=over))
    bad("field overlaps an output", follow(show=True, picture=halves.view(3, H, W), field=over16))
    ops.run(follow(prev_bytes=raw.view(3, H, W), field=over))                     # ... an input may share memory with it
    for kw in (dict(lo32=-1.0), dict(lo32=float("nan")), dict(inv32=-0.5), dict(inv32=float("inf"))):
        bad("must be finite and not negative", follow(**kw))
    for s in (-0.1, 1.5, float("nan")):
        bad("strength = .* must lie in \\[0, 1\\]", follow(s32=s))


# ----------------------------------------------------------------------------- the wrapper on the mock components
FOLLOW = dict(search=4, bias=256)


def panned(frames, v=(2, -1)):
    """camera-like frames for the mocks: one picture the camera pans over by `v` per frame (np.roll: the seam moves too), a little
    noise on every frame"""
    g = torch.Generator().manual_seed(5)
    base = torch.nn.functional.avg_pool2d(frames[0][None], 3, stride=1, padding=1)[0]
    return [(torch.roll(base, (k * v[0], k * v[1]), dims=(1, 2)) + torch.randint(-1, 2, base.shape, generator=g) / 255.0).clamp(0, 1)
            for k in range(len(frames))]


def test_wrapper_follow_on_the_host_route(monkeypatch):
    import pipeline_mocks as M
    from live2diff_amd.frame_io import egress_ref
    warm, frames = M.frames(8, seed=7), panned(frames_of(6, seed=8))
    torch.manual_seed(123)
    w = build(monkeypatch, 2)
    assert w.steady is None and w.steady_follow is None
    w.set_steady()
    w.set_steady_follow()
    assert w.steady == SET and w.steady_follow == FOLLOW                         # steady keeps its five keys
    w.prepare(warm, "a prompt")
    f_state = before = None
    followed = 0
    for t, f in enumerate(frames[:4]):
        got = w(f)
        source = pre(frames[t - 1] if t else warm[-1])
        out, f_state, field = SD.follow_ref(w.stream.prev_image_result, source, before, init=t == 0, **FOLLOW, **SET)
        plain, _ = SD.steady_ref(w.stream.prev_image_result, source, before, init=t == 0, **SET)
        before = f_state
        assert same(w._steady_state[0], f_state[0]) and same(w._steady_state[1], f_state[1])
        assert np.array_equal(got, egress_ref(torch.from_numpy(out))[0].numpy()), t
        followed += bool(field.any()) and not same(out, plain)
    assert followed == 2                         # frames 2 and 3: frame 0 is the init frame, frame 1 follows the unrelated warm-up frame
    # cleared: steady_ref's bits again, from the same state -- the sequence is not restarted
    w.clear_steady_follow()
    assert w.steady_follow is None and w.steady == SET and not w._steady_init
    got = w(frames[4])
    out, f_state = SD.steady_ref(w.stream.prev_image_result, pre(frames[3]), f_state, **SET)
    assert np.array_equal(got, egress_ref(torch.from_numpy(out))[0].numpy())
    # set again with other values: applies from the next output, the state goes on
    w.set_steady_follow(8, bias=0)
    assert w.steady_follow == dict(search=8, bias=0) and not w._steady_init
    got = w(frames[5])
    out, f_state, _ = SD.follow_ref(w.stream.prev_image_result, pre(frames[4]), f_state, search=8, bias=0, **SET)
    assert np.array_equal(got, egress_ref(torch.from_numpy(out))[0].numpy())
    # prepare restarts the sequence; the setting stays
    w.prepare(warm, "a prompt")
    assert w._steady_init and w._steady_state is None and w.steady_follow == dict(search=8, bias=0)
    got = w(frames[0])
    assert np.array_equal(got, egress_ref(w.stream.prev_image_result)[0].numpy())


def test_wrapper_follow_without_steady_changes_nothing(monkeypatch):
    import pipeline_mocks as M
    warm, frames = M.frames(8, seed=7), panned(frames_of(3, seed=9))

    def run(follow):
        torch.manual_seed(123)
        w = build(monkeypatch, 2)
        if follow:
            w.set_steady_follow(4, 128)
        w.prepare(warm, "a prompt")
        return w, [w(f) for f in frames]

    (w, got), (_, plain) = run(True), run(False)
    assert w.steady is None and w.steady_follow == dict(search=4, bias=128) and w._matte_line is None and w._steady_state is None
    assert all(np.array_equal(a, b) for a, b in zip(got, plain))
    for args, kw in (((0,), {}), ((9,), {}), ((4.0,), {}), ((4,), dict(bias=5000)), ((4,), dict(bias=1.0))):
        with pytest.raises(ValueError, match="steady follow: "):
            w.set_steady_follow(*args, **kw)
    assert w.steady_follow == dict(search=4, bias=128)
    # the constructor keyword
    import inspect

    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    assert inspect.signature(Wrapper.__init__).parameters["steady_follow"].default is None
    real = Wrapper.from_components
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, steady=dict(), steady_follow=dict(search=2), **kw)))
    w = build(monkeypatch, 2)
    assert w.steady == SET and w.steady_follow == dict(search=2, bias=256)
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, steady_follow=(4, 256), **kw)))
    with pytest.raises(ValueError, match="steady_follow="):
        build(monkeypatch, 2)


def test_wrapper_dropped_frame_repeats_under_follow(monkeypatch):
    import pipeline_mocks as M
    frames = panned(frames_of(5, seed=10))
    torch.manual_seed(123)
    w = build(monkeypatch, 2, drop={2})
    w.set_steady()
    w.set_steady_follow()
    w.prepare(M.frames(8, seed=7), "a prompt")
    got, states = [], []
    for f in frames:
        got.append(w(f))
        states.append(w._steady_state)
    assert np.array_equal(got[2], got[1]) and states[2] is states[1]
    assert not np.array_equal(got[3], got[2]) and states[3] is not states[2]
