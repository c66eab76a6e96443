"""CPU tests (-m "not gpu") of the matte hold (live2diff_amd/matte.py `hold_ref`): `hold_ref` against a
restatement in Python scalars, the init frame, the noise reduction on a still source against its closed form, the identities
(`w == 1`, a hard cut, exact 0 and 1), the interval, follow on a still source and under a pan, `plane=` on the three oracles,
`check_hold`, the builder and the launcher of op 57 (dry-run), and `set_matte_hold` on the wrapper built from the mock components
of tests/pipeline_mocks.py.  The sequence generators are shared with tests/test_gpu_matte_hold.py."""
import functools
import os

import numpy as np
import pytest
import torch

from live2diff_amd import matte as MT
from live2diff_amd import steady as SD
from live2diff_amd.frame_io import egress_ref
from test_matte_cpu import build
from test_steady_cpu import bits, frames_of, pre, same
from test_steady_follow_cpu import K, motion_direct, panned, sequence, texture, to16, view

HOLD = dict(lo=2.0, hi=10.0, strength=0.8, radius=2, search=0, bias=256)
MATTE = (0.3, 0.7)
EDGE = dict(radius=2, eps=4.0)
FORMS = ("near", "far", "hard", "plane")         # the depth ramp three ways, and op 49's plane


# ----------------------------------------------------------------------------- frames
@functools.lru_cache(maxsize=None)
def depths(H, W):
    """K fp16 [H,W] depth planes, read-only: the luma of the sequence's source frames (so the matte's edges move with the
    picture) on a horizontal gradient that saturates the ramp at both ends, plus N(0, 0.03) per frame"""
    rng = np.random.default_rng(H * 7 + W)
    sources, _ = sequence(H, W)
    out = []
    for k in range(K):
        y = MT.guide_ref(sources[k]).astype(np.float64) / 127.5 - 1.0
        d = np.clip(y + np.linspace(-0.7, 0.7, W)[None] + 0.03 * rng.standard_normal((H, W)), -1, 1).astype(np.float16)
        d.setflags(write=False)
        out.append(d)
    return tuple(out)


def matte_in(depth, source, form):
    """m0 of one frame, fp32 [H,W]: the matte in front of the feather in one of FORMS"""
    if form == "hard":
        return MT.matte_ref(depth, 0.5, 0.5, 0, "near")[0]
    m = MT.matte_ref(depth, *MATTE, 0, "far" if form in ("far", "plane") else "near")[0]
    return MT.edge_ref(m, source, **EDGE) if form == "plane" else m


@functools.lru_cache(maxsize=None)
def oracle(H, W, form, radius, search, bias=256, lo=2.0, hi=10.0, strength=0.8):
    """`hold_ref` over the sequence, frame 0 as the init frame: ([m0], [h], [(plane, bytes) states], [fields])"""
    sources, _ = sequence(H, W)
    ms, hs, states, fields, state = [], [], [], [], None
    for k in range(K):
        m0 = matte_in(depths(H, W)[k], sources[k], form)
        h, state, f = MT.hold_ref(m0, sources[k], state, lo=lo, hi=hi, strength=strength, radius=radius, search=search, bias=bias,
                                  init=k == 0)
        for a in (m0, h, f, *state):
            a.setflags(write=False)
        ms.append(m0)
        hs.append(h)
        states.append(state)
        fields.append(f)
    return ms, hs, states, fields


def hold_direct(m0, b, state, lo, hi, s, r, search, bias):
    """one frame of `hold_ref` by loops over pixels in Python and numpy scalars, the field by `motion_direct`"""
    P, bp = state
    _, H, W = b.shape
    cl = lambda v, n: min(max(v, 0), n - 1)
    f32 = np.float32
    field = motion_direct(b, bp, search, bias) if search else np.zeros((-(-H // 8), -(-W // 8), 2), dtype=np.int8)
    lo32, inv32, hard = SD.steady_params(lo, hi)
    n = f32((2 * r + 1) ** 2)
    out = np.empty((H, W), dtype=np.float32)
    bi, bpi = b.astype(int), bp.astype(int)
    for y in range(H):
        for x in range(W):
            D = 0
            for wy in range(y - r, y + r + 1):
                for wx in range(x - r, x + r + 1):
                    cy, cx = cl(wy, H), cl(wx, W)
                    dy, dx = (int(v) for v in field[cy // 8, cx // 8])
                    D += max(abs(bi[c, cy, cx] - bpi[c, cl(cy + dy, H), cl(cx + dx, W)]) for c in range(3))
            dbar = f32(D) / n
            t = (f32(1) if dbar >= lo32 else f32(0)) if hard else min(max((dbar - lo32) * inv32, f32(0)), f32(1))
            w = (t * t) * (f32(3) - f32(2) * t)
            a = f32(1) - f32(s) * (f32(1) - w)
            dy, dx = (int(v) for v in field[y // 8, x // 8])
            p, m = P[cl(y + dy, H), cl(x + dx, W)], m0[y, x]
            h = p + a * (m - p)
            h = min(max(h, min(m, p)), max(m, p))
            out[y, x] = m if a == f32(1) else h
            assert all(isinstance(v, np.float32) for v in (dbar, t, w, a, h))
    return out, field


# ----------------------------------------------------------------------------- hold_ref
@pytest.mark.parametrize("search", [0, 4])
@pytest.mark.parametrize("radius", [0, 2])
@pytest.mark.parametrize("shape", [(8, 8), (20, 40)])
def test_hold_ref_against_python_scalars(shape, radius, search):
    H, W = shape
    sources, _ = sequence(H, W)
    ms, hs, states, fields = oracle(H, W, "near", radius, search)
    moved = 0
    for k in range(1, K):
        want, field = hold_direct(ms[k], SD.source_bytes(sources[k]), states[k - 1], 2.0, 10.0, 0.8, radius, search, 256)
        assert same(hs[k], want) and np.array_equal(fields[k], field), k
        moved += not same(hs[k], ms[k])
    assert moved >= 1                            # (the hold acts: on the still stretch at least)


def test_init_frame_and_state():
    H, W = 20, 40
    sources, _ = sequence(H, W)
    m0 = matte_in(depths(H, W)[0], sources[0], "near")
    for state in (None, (np.full((H, W), np.nan, np.float32), np.zeros((3, H, W), np.uint8))):
        h, new, field = MT.hold_ref(m0, sources[0], state, init=True, search=4)
        assert same(h, m0) and same(new[0], m0) and np.array_equal(new[1], SD.source_bytes(sources[0]))
        assert field.dtype == np.int8 and field.shape == (3, 5, 2) and not field.any()
        assert h is not m0 and new[0] is not h
    for k in range(1, K):                        # the state's bytes are the frame's own, where they are
        ms, hs, states, _ = oracle(H, W, "far", 2, 4)
        assert np.array_equal(states[k][1], SD.source_bytes(sources[k])) and same(states[k][0], hs[k])
    with pytest.raises(ValueError):
        MT.hold_ref(m0[None], sources[0], None, init=True)
    with pytest.raises(ValueError):
        MT.hold_ref(m0[:, :8], sources[0], None, init=True)
    with pytest.raises(ValueError):
        MT.hold_ref(m0, sources[0], (m0.astype(np.float64), SD.source_bytes(sources[0])))


@pytest.mark.parametrize("strength", [0.8, 0.5])
def test_noise_reduction_on_a_still_source(strength):
    """a still source, a noisy depth: the deviation of h from the matte of the noiseless depth, relative to that of m0, follows the
    closed form of an EMA with gain a = 1 - strength started at the first frame: sqrt(a^2 (1 - q^k) / (1 - q) + q^k), q = (1 - a)^2,
    within 5 % (derived, not tuned: 0.587 / 0.388 / 0.343 at strength 0.8)"""
    H, W, N = 64, 96, 12
    rng = np.random.default_rng(11)
    source = to16(view(texture(rng, H, W), H, W, 0, 0))
    clean = np.broadcast_to(np.linspace(-0.2, 0.2, W), (H, W))
    ref = MT.matte_ref(clean.astype(np.float16), *MATTE)[0]
    state, got = None, {}
    for k in range(N):
        m0 = MT.matte_ref((clean + 0.02 * rng.standard_normal((H, W))).astype(np.float16), *MATTE)[0]
        h, state, _ = MT.hold_ref(m0, source, state, strength=strength, init=k == 0)
        rms = lambda v: float(np.sqrt(np.mean((v.astype(np.float64) - ref) ** 2)))
        got[k] = rms(h) / rms(m0)
    a = 1.0 - strength
    q = (1.0 - a) ** 2
    for k in (3, 7, 11):
        want = np.sqrt(a * a * (1 - q ** k) / (1 - q) + q ** k)
        print(f"strength {strength} frame {k}: measured {got[k]:.4f}, closed form {want:.4f}")
        assert abs(got[k] / want - 1.0) <= 0.05, (k, got[k], want)


def test_moving_pixels_and_a_hard_cut_pass_the_new_matte():
    H, W = 40, 72
    sources, _ = sequence(H, W)
    for form in ("near", "plane"):
        ms, hs, states, _ = oracle(H, W, form, 2, 0)
        assert same(hs[3], ms[3])                                                # frame 3 is unrelated to frame 2: everything moved
        for k in (1, 2, 4):
            w = SD.weight_ref(SD.source_bytes(sources[k]), states[k - 1][1], lo=2.0, hi=10.0, radius=2)
            assert np.array_equal(bits(hs[k])[w == 1], bits(ms[k])[w == 1]) and (w == 1).any()
        w = SD.weight_ref(SD.source_bytes(sources[2]), states[1][1], lo=2.0, hi=10.0, radius=2)
        assert (w == 0).any() and not np.array_equal(hs[2][w == 0], ms[2][w == 0])  # the still stretch is held


def test_exact_ends_and_the_composite_there():
    from test_matte_cpu import data
    H, W = 24, 40
    styled, source, _ = data(1, H, W, seed=3)
    sources, _ = sequence(H, W)
    for v, want in ((1.0, egress_ref(torch.from_numpy(np.asarray(styled)))), (0.0, egress_ref(torch.from_numpy(np.asarray(source))))):
        m0 = np.full((H, W), v, dtype=np.float32)
        state = (m0.copy(), SD.source_bytes(sources[1]))
        h, _, _ = MT.hold_ref(m0, sources[2], state, radius=2)                    # (frames 1 and 2: the weight takes every value)
        assert same(h, m0)
        for r in (0, 3):
            assert np.array_equal(MT.composite_ref(styled, source, None, *MATTE, feather=r, plane=h[None]), want.numpy())


def test_interval_and_the_clamp():
    """h lies in [min(m0, P), max(m0, P)] for every weight, while the unclamped fp32 blend P + a (m0 - P) does not: the inputs hold
    values where it leaves the interval (computed here: fl(P + fl(m0 - P)) misses m0 by an ulp where m0 is much smaller than P).
    On these inputs all of them sit where a == 1, which takes m0's own bits anyway; where a < 1 the clamp changes no bit here."""
    H, W = 64, 512
    rng = np.random.default_rng(5)
    sources, _ = sequence(H, W)
    m0, P = (rng.uniform(0, 1, (H, W)).astype(np.float32) for _ in range(2))
    P[:, ::3] = np.exp(rng.uniform(np.log(1e-6), 0, (H, (W + 2) // 3))).astype(np.float32)
    outside = 0
    for strength in (0.8, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24):
        bp = SD.source_bytes(sources[1])
        h, _, _ = MT.hold_ref(m0, sources[2], (P, bp), strength=strength, radius=0)
        assert np.all(h >= np.minimum(m0, P)) and np.all(h <= np.maximum(m0, P)) and h.min() >= 0 and h.max() <= 1
        w = SD.weight_ref(SD.source_bytes(sources[2]), bp, lo=2.0, hi=10.0, radius=0)
        a = np.float32(1) - np.float32(strength) * (np.float32(1) - w)
        raw = P + a * (m0 - P)
        outside += int(((raw < np.minimum(m0, P)) | (raw > np.maximum(m0, P))).sum())
        assert same(np.where(a == 1, m0, raw), h) and 0 < (a < 1).sum() and (a == 1).any()
    print(f"unclamped blends outside [min, max]: {outside} of {4 * H * W}")
    assert outside >= 1


def test_follow_on_a_still_source_and_under_a_pan():
    H, W = 64, 96
    rng = np.random.default_rng(9)
    canvas = texture(rng, H, W)
    still = to16(view(canvas, H, W, 0, 0))
    m = [rng.uniform(0, 1, (H, W)).astype(np.float32) for _ in range(3)]
    a = b = None
    for k in range(3):
        ha, a, fa = MT.hold_ref(m[k], still, a, search=8, init=k == 0)
        hb, b, _ = MT.hold_ref(m[k], still, b, search=0, init=k == 0)
        assert same(ha, hb) and same(a[0], b[0]) and not fa.any()
    # a pan by (3, -2): the matte's edge is painted on the canvas and moves with the picture
    edge = (np.arange(canvas.shape[2])[None] > canvas.shape[2] // 2).astype(np.float32) * np.ones((canvas.shape[1], 1), np.float32)
    prev, now = to16(view(canvas, H, W, 0, 0)), to16(view(canvas, H, W, -3, 2))
    mp, mn = view(edge[None], H, W, 0, 0)[0].copy(), view(edge[None], H, W, -3, 2)[0].copy()
    mn_noisy = np.clip(mn + 0.1 * rng.standard_normal((H, W)).astype(np.float32), 0, 1).astype(np.float32)
    _, st, _ = MT.hold_ref(mp, prev, None, init=True)
    h, _, field = MT.hold_ref(mn_noisy, now, st, search=4)
    inner = (slice(16, H - 16), slice(16, W - 16))
    assert (field[2:-2, 2:-2] == np.array([-3, 2])).all()
    P = SD.warp_ref(mp[None], field)[0]
    assert np.array_equal(P[inner], mn[inner])                                   # the previous plane lands on this frame's edge
    alpha = np.float32(1) - np.float32(0.8)
    want = P + alpha * (mn_noisy - P)
    assert same(h[inner], np.minimum(np.maximum(want, np.minimum(mn_noisy, P)), np.maximum(mn_noisy, P))[inner])
    plain, _, _ = MT.hold_ref(mn_noisy, now, st, search=0)
    assert same(plain[inner], mn_noisy[inner])                                   # the same coordinates: everything moved, nothing is held


def test_plane_keyword_on_the_three_oracles():
    from test_matte_cpu import data
    from test_matte_edge_cpu import _composite_before, _composite_up_before, _matte_before
    B, H, W = 2, 24, 40
    styled, source, depth = data(B, H, W, seed=5)
    rng = np.random.default_rng(1)
    S, C = (rng.integers(0, 256, (B, 36, 56, 3), dtype=np.uint8) for _ in range(2))
    for lo, hi in ((0.3, 0.7), (0.5, 0.5)):
        for keep in ("near", "far"):
            ramp = MT.matte_ref(depth, lo, hi, 0, keep)
            refined = MT.matte_ref(depth, lo, hi, 0, keep, edge=EDGE, source=source)
            for r in (0, 3):
                assert same(MT.matte_ref(depth, lo, hi, r, keep), _matte_before(depth, lo, hi, r, keep))
                assert same(MT.matte_ref(None, lo, hi, r, keep, plane=ramp), MT.matte_ref(depth, lo, hi, r, keep))
                assert same(MT.matte_ref(None, lo, hi, r, keep, plane=torch.from_numpy(refined)),
                            MT.matte_ref(depth, lo, hi, r, keep, edge=EDGE, source=source))
                for show in (False, True):
                    plain = MT.composite_ref(styled, source, depth, lo, hi, r, keep, show)
                    assert np.array_equal(plain, _composite_before(styled, source, depth, lo, hi, r, keep, show))
                    assert np.array_equal(MT.composite_ref(styled, source, None, lo, hi, r, keep, show, plane=ramp), plain)
                    assert np.array_equal(MT.composite_ref(styled, source, depth, lo, hi, r, keep, show, plane=refined),
                                          MT.composite_ref(styled, source, depth, lo, hi, r, keep, show, edge=EDGE))
                    up = MT.composite_up_ref(S, C, depth, lo, hi, r, keep, show)
                    assert np.array_equal(up, _composite_up_before(S, C, depth, lo, hi, r, keep, show))
                    assert np.array_equal(MT.composite_up_ref(S, C, None, lo, hi, r, keep, show, plane=ramp), up)
                    assert np.array_equal(MT.composite_up_ref(S, C, None, lo, hi, r, keep, show, plane=refined),
                                          MT.composite_up_ref(S, C, depth, lo, hi, r, keep, show, edge=EDGE, source=source))
    with pytest.raises(ValueError, match="plane"):
        MT.matte_ref(None, 0.3, 0.7, plane=np.zeros((H, W), np.float64))


def test_check_hold():
    assert MT.check_hold() == HOLD
    assert MT.check_hold(0, 255, 1, np.int64(8), np.int64(8), 4096) == dict(lo=0.0, hi=255.0, strength=1.0, radius=8, search=8, bias=4096)
    for bad in (dict(lo=-1), dict(hi=256), dict(lo=5, hi=4), dict(lo="2"), dict(strength=1.5), dict(strength=-0.1), dict(strength=True),
                dict(radius=9), dict(radius=-1), dict(radius=2.0), dict(search=-1), dict(search=9), dict(search=1.0), dict(search=True),
                dict(bias=-1), dict(bias=4097), dict(bias=1.5), dict(bias=False)):
        with pytest.raises(ValueError, match="matte hold"):
            MT.check_hold(**bad)
    with pytest.raises(ValueError, match="matte hold"):
        MT.hold_ref(np.zeros((8, 8), np.float32), np.zeros((3, 8, 8), np.float16), None, search=9, init=True)


# ----------------------------------------------------------------------------- the builder and the launcher
@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_launcher_checks(dry_run):
    from live2diff_amd import _lib, ops
    assert _lib.OP_FRAME_MATTE_HOLD == 57
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_FRAME_MATTE_HOLD = 57," in hdr
    assert all(f"#define L2D_MATTE_HOLD_{n} {v} " in hdr for n, v in (
        ("HARD", ops.MATTE_HOLD_HARD), ("INIT", ops.MATTE_HOLD_INIT), ("PLANE", ops.MATTE_HOLD_PLANE), ("FOLLOW", ops.MATTE_HOLD_FOLLOW),
        ("RAMP_HARD", ops.MATTE_HOLD_RAMP_HARD), ("RAMP_FAR", ops.MATTE_HOLD_RAMP_FAR)))
    H, W = 20, 40
    frame = lambda H=H, W=W, dtype=torch.float16: torch.zeros(3, H, W, dtype=dtype)
    dplane = lambda H=H, W=W, dtype=torch.float16: torch.zeros(H, W, dtype=dtype)
    fplane = lambda H=H, W=W, dtype=torch.float32: torch.zeros(H, W, dtype=dtype)
    bplane = lambda H=H, W=W, dtype=torch.uint8: torch.zeros(3, H, W, dtype=dtype)
    fld = lambda H=H, W=W, dtype=torch.int8: torch.zeros((H + 7) // 8, W // 8, 2, dtype=dtype)
    names = ("source", "depth", "prev_plane", "prev_bytes", "out_plane", "next_bytes")

    def hold(H=H, W=W, **kw):
        args = dict(source=frame(H, W), depth=dplane(H, W), prev_plane=fplane(H, W), prev_bytes=bplane(H, W), out_plane=fplane(H, W),
                    next_bytes=bplane(H, W), H=H, W=W, lo32=2.0, inv32=0.125, s32=0.8, r=2, ramp_lo32=-0.4, ramp_inv32=1.25)
        args.update(kw)
        if args.get("plane") is not None:
            args["depth"] = None
        return ops.frame_matte_hold(*[args.pop(k) for k in names], **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    # the record
    t = [frame(), dplane(), fplane(), bplane(), fplane(), bplane(), fld()]
    op, keep = ops.frame_matte_hold(*t[:6], H=H, W=W, lo32=np.float32(2), inv32=np.float32(0.125), s32=np.float32(0.8), r=3, hard=True,
                                    ramp_lo32=np.float32(-0.4), ramp_inv32=np.float32(1.25), far=True, field=t[6])
    assert op.kind == 57 and [op.p[j] for j in range(8)] == [x.data_ptr() for x in t] + [None]
    assert [op.i[j] for j in range(4)] == [H, W, 3, ops.MATTE_HOLD_HARD | ops.MATTE_HOLD_FOLLOW | ops.MATTE_HOLD_RAMP_FAR]
    assert [np.int32(op.i[j]).view(np.float32) for j in (4, 5)] == [np.float32(-0.4), np.float32(1.25)] and op.i[6] == 0
    assert [op.f[j] for j in range(4)] == [2.0, 0.125, float(np.float32(0.8)), 0.0] and all(a is b for a, b in zip(keep, t))
    ops.run((op, keep))
    op, _ = hold(plane=fplane(), init=True)
    assert op.i[3] == ops.MATTE_HOLD_INIT | ops.MATTE_HOLD_PLANE and op.i[4] == op.i[5] == 0
    for kw in (dict(), dict(r=0), dict(r=8), dict(hard=True, inv32=0.0), dict(H=1, W=8), dict(H=512, W=512), dict(s32=0.0), dict(s32=1.0),
               dict(plane=fplane()), dict(field=fld()), dict(plane=fplane(), field=fld()), dict(ramp_hard=True, ramp_inv32=0.0, far=True),
               dict(init=True, prev_plane=None, prev_bytes=None), dict(init=True, prev_plane=None, prev_bytes=None, plane=fplane()),
               dict(init=True, field=fld())):
        ops.run(hold(**kw))
    # the builder
    for call in (lambda: hold(source=frame(dtype=torch.float32)), lambda: hold(depth=dplane(dtype=torch.float32)), lambda: hold(depth=None),
                 lambda: hold(depth=dplane(H, W + 8)), lambda: hold(plane=fplane(dtype=torch.float16)), lambda: hold(plane=fplane(), far=True),
                 lambda: hold(plane=fplane(), ramp_hard=True), lambda: hold(prev_plane=None), lambda: hold(prev_bytes=None),
                 lambda: hold(prev_plane=fplane(H + 1, W)), lambda: hold(out_plane=dplane()), lambda: hold(out_plane=None),
                 lambda: hold(next_bytes=torch.zeros(H, W, 3, dtype=torch.uint8)), lambda: hold(field=fld(H + 8, W)),
                 lambda: hold(field=fld(dtype=torch.uint8)), lambda: hold(r=9), lambda: hold(r=-1), lambda: hold(r=1.5), lambda: hold(r=True)):
        with pytest.raises((ValueError, AttributeError, TypeError)):
            call()
    with pytest.raises(ValueError, match="plane= goes with depth=None"):
        ops.frame_matte_hold(frame(), dplane(), fplane(), bplane(), fplane(), bplane(), H=H, W=W, lo32=2.0, inv32=0.125, s32=0.8, plane=fplane())
    # the launcher: ranges and flags
    for k, v, match in ((2, 9, "radius 9, need 0..8"), (2, -1, "radius -1"), (3, 2, "unknown flag bits"), (3, 8, "unknown flag bits"),
                        (3, 256, "unknown flag bits"), (0, 0, "non-positive size"), (1, 36, "multiple of 8")):
        op, keep = hold()
        op.i[k] = v
        bad(match, (op, keep))
    op, keep = hold()
    op.i[0], op.i[1] = 1 << 15, 21848                    # 3 * 32768 * 21848 = 2^31 + 98304; W % 8 == 0
    bad("must stay below 2\\^31", (op, keep))
    op, keep = hold(plane=fplane())
    op.i[3] |= ops.MATTE_HOLD_RAMP_FAR
    bad("ramp's flags do not go with a plane", (op, keep))
    # null pointers: 2 and 3 only with INIT, 6 with INIT or without FOLLOW
    for k in range(6):
        op, keep = hold()
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
    op, keep = hold(field=fld())
    op.p[6] = None
    bad("pointer 6 is null", (op, keep))
    for k in (0, 1, 4, 5):
        op, keep = hold(init=True)
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
    op, keep = hold(init=True, field=fld())
    op.p[2] = op.p[3] = op.p[6] = None
    ops.run((op, keep))
    # alignment: planes and frames 16 bytes, byte planes 8, the field any
    for k, off in ((0, 8), (1, 8), (2, 8), (3, 4), (4, 8), (5, 4)):
        op, keep = hold()
        op.p[k] = op.p[k] + off
        bad(f"pointer {k} is not aligned", (op, keep))
    op, keep = hold(plane=fplane())
    op.p[1] = op.p[1] + 4
    bad("pointer 1 is not aligned", (op, keep))
    op, keep = hold(field=fld())
    op.p[6] = op.p[6] + 1                                # the field at an odd address
    ops.run((op, keep))
    # overlaps: each output against every input and the other output; the field against the outputs
    floats, raw = torch.zeros(3 * H * W, dtype=torch.float32), torch.zeros(4 * H * W, dtype=torch.uint8)
    f_as = lambda n, dt: floats.view(torch.uint8)[:n * H * W * torch.empty(0, dtype=dt).element_size()].view(dt)
    bad("output 4 overlaps input 0", hold(source=f_as(3, torch.float16).view(3, H, W), out_plane=floats[:H * W].view(H, W)))
    bad("output 4 overlaps input 1", hold(depth=f_as(1, torch.float16).view(H, W), out_plane=floats[:H * W].view(H, W)))
    x = fplane()
    bad("output 4 overlaps input 1", hold(plane=x, out_plane=x))
    bad("output 4 overlaps input 2", hold(prev_plane=x, out_plane=x))
    bad("output 4 overlaps input 3", hold(prev_bytes=f_as(3, torch.uint8).view(3, H, W), out_plane=floats[:H * W].view(H, W)))
    six = torch.zeros(6 * H * W, dtype=torch.uint8)
    bad("output 5 overlaps input 0", hold(source=six.view(torch.float16).view(3, H, W), next_bytes=six[:3 * H * W].view(3, H, W)))
    bad("output 5 overlaps input 1", hold(depth=raw[:2 * H * W].view(torch.float16).view(H, W), next_bytes=raw[:3 * H * W].view(3, H, W)))
    bad("output 5 overlaps input 2", hold(prev_plane=raw[:4 * H * W].view(torch.float32).view(H, W), next_bytes=raw[:3 * H * W].view(3, H, W)))
    y = bplane()
    bad("output 5 overlaps input 3", hold(prev_bytes=y, next_bytes=y))
    bad("out plane overlaps next_bytes", hold(out_plane=raw[:4 * H * W].view(torch.float32).view(H, W), next_bytes=raw[:3 * H * W].view(3, H, W)))
    over = raw[8:8 + 30].view(torch.int8).view(3, 5, 2)
    bad("field overlaps an output", hold(next_bytes=raw[:3 * H * W].view(3, H, W), field=over))
    bad("field overlaps an output", hold(out_plane=raw[:4 * H * W].view(torch.float32).view(H, W), field=over))
    ops.run(hold(prev_bytes=raw[:3 * H * W].view(3, H, W), field=over))          # ... an input may share memory with it
    # the floats
    for kw in (dict(lo32=-1.0), dict(lo32=float("nan")), dict(inv32=-0.5), dict(inv32=float("inf"))):
        bad("must be finite and not negative", hold(**kw))
    for s in (-0.1, 1.5, float("nan")):
        bad("strength = .* must lie in \\[0, 1\\]", hold(s32=s))
    for kw in (dict(ramp_lo32=-1.5), dict(ramp_lo32=float("nan")), dict(ramp_inv32=-1.0), dict(ramp_inv32=float("inf")),
               dict(ramp_inv32=0.0), dict(ramp_hard=True)):
        bad("must lie in \\[-1, 1\\]", hold(**kw))
    ops.run(hold(plane=fplane(), ramp_lo32=-5.0))                                # (a plane: the ramp is not read)


# ----------------------------------------------------------------------------- the wrapper on the mock components (host route)
WMATTE = dict(lo=0.3, hi=0.7, keep="far", feather=2, show=False)


def call(w, f):
    torch.manual_seed(77)                        # (the host path draws its re-noising from the global generator)
    return w(f)


class NoisyDepth:
    """a depth detector whose map is a ramp plus fresh noise at every call: the matte of a still scene crawls"""
    dtype = torch.float32

    def __init__(self):
        self.g = torch.Generator().manual_seed(31)

    def __call__(self, x):
        ramp = torch.linspace(1.0, 5.0, 384 * 384).view(1, 384, 384).repeat(x.shape[0], 1, 1)
        return ramp + 0.3 * torch.randn(ramp.shape, generator=self.g) + 0.0 * x[:, 0]


def made(monkeypatch, hold=True, edge=None, drop=None, matte=True):
    import pipeline_mocks as M
    torch.manual_seed(123)
    w = build(monkeypatch, 2, drop=drop)
    assert w.stream.depth_detector is not None
    w.stream.depth_detector = NoisyDepth()
    if hold:
        w.set_matte_hold()                       # before the matte
    if matte:
        w.set_matte(WMATTE["lo"], WMATTE["hi"], keep=WMATTE["keep"], feather=WMATTE["feather"])
    if edge:
        w.set_matte_edge(**edge)
    w.prepare(M.frames(8, seed=7), "a prompt")
    return w


class ByHand:
    """`hold_ref` and `composite_ref(plane=)` composed by hand beside a wrapper"""

    def __init__(self):
        self.state = None

    def step(self, w, init=False, backdrop=None, **hold):
        slot = w._matte_line.last
        m = w.matte
        m0 = MT.matte_ref(slot.depth[None], m["lo"], m["hi"], 0, m["keep"], edge=w.matte_edge,
                          source=slot.source[None] if w.matte_edge else None)[0]
        self.h, self.state, _ = MT.hold_ref(m0, slot.source, self.state, init=init or self.state is None, **(hold or w.matte_hold))
        more = {} if backdrop is None else dict(backdrop=backdrop)
        return MT.composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **m, plane=self.h[None], **more)[0]


@pytest.mark.parametrize("edge", [None, dict(radius=3, eps=4.0)])
def test_wrapper_host_route(monkeypatch, edge):
    frames = moving_frames(7)
    w, twin, hand = made(monkeypatch, edge=edge), made(monkeypatch, hold=False, edge=edge), ByHand()
    assert w.matte_hold == HOLD and twin.matte_hold is None and w.matte == WMATTE
    differs = 0
    for t in range(3):
        got, plain = call(w, frames[t]), call(twin, frames[t])
        assert got.dtype == np.uint8 and np.array_equal(got, hand.step(w)), t
        assert same(w._hold_state[0], hand.state[0]) and np.array_equal(w._hold_state[1], hand.state[1])
        differs += not np.array_equal(got, plain)
        assert t or np.array_equal(got, plain)                                   # the init frame is the matte's own
    assert differs >= 1
    # changed settings mid-stream restart nothing; `show` shows the held matte
    w.set_matte_hold(1.0, 20.0, strength=0.5, radius=1, search=4, bias=0)
    assert w.matte_hold == dict(lo=1.0, hi=20.0, strength=0.5, radius=1, search=4, bias=0) and not w._hold_init
    assert np.array_equal(call(w, frames[3]), hand.step(w))
    # set_matte (a `keep` flip, `show`) restarts the hold: the next frame is the new matte's own
    w.set_matte(0.3, 0.7, keep="near", feather=0, show=True)
    assert w._hold_init
    shown = call(w, frames[4])
    assert np.array_equal(shown, hand.step(w, init=True)) and same(hand.h, hand.state[0])
    slot = w._matte_line.last
    m0 = MT.matte_ref(slot.depth[None], 0.3, 0.7, 0, "near", edge=w.matte_edge, source=slot.source[None] if edge else None)[0]
    assert np.array_equal(shown[..., 0], np.rint(m0 * np.float32(255)).astype(np.uint8))
    shown = call(w, frames[5])
    assert np.array_equal(shown, hand.step(w)) and np.array_equal(shown[..., 0], np.rint(hand.h * np.float32(255)).astype(np.uint8))
    # set_matte_edge / clear_matte_edge restart it too
    w.set_matte_edge(2, 8.0) if edge is None else w.clear_matte_edge()
    assert w._hold_init
    assert np.array_equal(call(w, frames[6]), hand.step(w, init=True))
    for bad in (dict(lo=-1.0), dict(lo=9.0, hi=3.0), dict(strength=2.0), dict(radius=9), dict(search=9), dict(bias=-1), dict(search=1.5)):
        with pytest.raises(ValueError, match="matte hold"):
            w.set_matte_hold(**bad)


def moving_frames(k):
    from test_steady_cpu import moving
    return moving(frames_of(k, seed=8))


def test_wrapper_with_a_backdrop(monkeypatch):
    from live2diff_amd.backdrop import stream_ref
    frames = moving_frames(3)
    w, hand = made(monkeypatch), ByHand()
    w.set_backdrop("blur", radius=2, passes=1)
    for t in range(3):
        got = call(w, frames[t])
        slot = w._matte_line.last
        bd = stream_ref(w.backdrop, None, slot.source, slot.depth, w.matte)[None]      # (the blur weighs by the raw matte)
        assert np.array_equal(got, hand.step(w, backdrop=bd)), t


def test_wrapper_prepare_clear_and_set_mid_stream(monkeypatch):
    import pipeline_mocks as M
    frames = moving_frames(7)
    w, twin, hand = made(monkeypatch), made(monkeypatch, hold=False), ByHand()
    for t in range(2):
        assert np.array_equal(call(w, frames[t]), hand.step(w))
        call(twin, frames[t])
    # cleared: the matte of each frame alone again, and the state is dropped
    w.clear_matte_hold()
    assert w.matte_hold is None and w._hold_state is None and w._hold_init
    assert np.array_equal(call(w, frames[2]), call(twin, frames[2]))
    # set again mid-stream: an init frame, then held
    w.set_matte_hold(strength=0.6)
    hand = ByHand()
    for t in (3, 4):
        got, plain = call(w, frames[t]), call(twin, frames[t])
        assert np.array_equal(got, hand.step(w)), t
    assert not np.array_equal(got, plain)
    # prepare restarts the sequence; the setting stays
    for x in (w, twin):
        torch.manual_seed(5)
        x.prepare(M.frames(8, seed=7), "a prompt")
    assert w._hold_init and w._hold_state is None and w.matte_hold["strength"] == 0.6
    assert np.array_equal(call(w, frames[5]), call(twin, frames[5]))
    # clear_matte drops the state; the hold's setting stays and acts again with the next matte
    w.clear_matte()
    twin.clear_matte()
    assert w._hold_state is None and w._hold_init and w.matte_hold is not None and w.stream.matte_tap is None
    assert np.array_equal(call(w, frames[6]), call(twin, frames[6]))


def test_wrapper_hold_without_a_matte_changes_nothing(monkeypatch):
    frames = moving_frames(3)
    w, twin = made(monkeypatch, matte=False), made(monkeypatch, hold=False, matte=False)
    assert w.matte is None and w.matte_hold == HOLD and w._matte_line is None
    for f in frames:
        assert np.array_equal(call(w, f), call(twin, f))
    assert w._hold_state is None and w._hold_dev is None


def test_wrapper_dropped_frame_repeats_and_moves_no_state(monkeypatch):
    frames = moving_frames(5)
    w = made(monkeypatch, drop={2})
    w.stream.inference_time_ema = 0.0            # (a dropped frame waits that long)
    got, states = [], []
    for f in frames:
        got.append(call(w, f))
        states.append(w._hold_state)
    assert np.array_equal(got[2], got[1]) and states[2] is states[1] and w._matte_line.tapped == 4
    assert not np.array_equal(got[3], got[2]) and states[3] is not states[2]


def test_constructor_keyword(monkeypatch):
    import inspect

    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    assert inspect.signature(Wrapper.__init__).parameters["matte_hold"].default is None
    real = Wrapper.from_components
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, matte_hold=dict(search=2), **kw)))
    w = build(monkeypatch, 2)
    assert w.matte_hold == dict(HOLD, search=2) and w.matte is None
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, matte_hold=(2, 10), **kw)))
    with pytest.raises(ValueError, match="matte_hold="):
        build(monkeypatch, 2)
    monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, matte_hold=dict(radius=9), **kw)))
    with pytest.raises(ValueError, match="matte hold"):
        build(monkeypatch, 2)
