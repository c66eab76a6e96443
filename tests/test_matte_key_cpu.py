"""CPU tests (-m "not gpu") of the matte key (live2diff_amd/matte_key.py): the exact properties of
`key_ref`, planted boundaries of the thresholds, the integer bounds at the extreme byte triples, "and" / "or" against
`mask_io.front_ref`, the refusals, the builders and the launchers of ops 59 and 60 (dry-run), and `set_matte_key` on the wrapper
built from the mock components of tests/pipeline_mocks.py -- the N - 1 delay, a captured plate, the exclusion with masks.  There
is no tolerance anywhere."""
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

from live2diff_amd import mask_io as MI
from live2diff_amd import matte as MT
from live2diff_amd import matte_key as MK
from live2diff_amd.backdrop import frame_of
from live2diff_amd.frame_io import egress_ref
from live2diff_amd.steady import source_bytes
from test_matte_cpu import build, src_bytes

H, W = 40, 72
GREEN = (0, 177, 64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def frame16(seed, h=H, w=W):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(3, h, w, generator=g) * 2.2 - 1.1).to(torch.float16)


def depth16(seed, h=H, w=W):
    rng = np.random.default_rng(seed)
    return np.clip(np.linspace(-1.0, 1.0, w)[None] + 0.2 * rng.standard_normal((h, w)), -1, 1).astype(np.float16)


def of_bytes(b):
    """an fp16 [3,H,W] frame whose egress bytes are the planar uint8 `b`"""
    f = frame_of(np.asarray(b, dtype=np.uint8))
    assert np.array_equal(source_bytes(f), b)
    return f


# ----------------------------------------------------------------------------- the oracle
def test_a_frame_equal_to_its_plate_gives_zero():
    src = frame16(1)
    plate = source_bytes(src)
    for radius, luma in ((0, 0.0), (1, 0.25), (4, 1.0)):
        assert not MK.key_ref(src, plate, lo=1, hi=2, luma=luma, radius=radius).any()
        assert not MK.key_ref(src, plate, lo=3, hi=3, luma=luma, radius=radius).any()          # (hard)
    assert (MK.key_ref(src, plate, lo=0, hi=0) == 255).all()                                   # lo = 0, hard: 0 >= 0 everywhere


def test_invert_colour_as_plate_and_radius_zero():
    src = frame16(2)
    b = source_bytes(src)
    for kw in (dict(lo=130, hi=200), dict(lo=140, hi=190, luma=0.25, radius=2), dict(lo=175, hi=175, luma=1.0, radius=4)):
        P = MK.key_ref(src, GREEN, **kw)
        assert P.dtype == np.uint8 and P.shape == (H, W) and (P == 0).any() and (P == 255).any()
        assert np.array_equal(MK.key_ref(src, GREEN, invert=True, **kw), 255 - P)
        plate = np.ascontiguousarray(np.broadcast_to(np.array(GREEN, np.uint8)[:, None, None], b.shape))
        assert np.array_equal(MK.key_ref(src, plate, **kw), P)
    # radius 0: the per-pixel formula, written out again
    lo, hi, luma = 100.0, 260.0, 0.25
    d = b.astype(np.int64) - np.array(GREEN, np.int64)[:, None, None]
    dy = np.floor_divide(77 * d[0] + 150 * d[1] + 29 * d[2] + 128, 256)
    cb, cr = d[2] - dy, d[0] - dy
    D = cb ** 2 + cr ** 2 + np.floor_divide(64 * dy ** 2 + 128, 256)
    mean = D.astype(np.float32) / np.float32(1.0)
    t = np.clip((mean - np.float32(lo * lo)) * np.float32(1.0 / (hi * hi - lo * lo)), np.float32(0), np.float32(1))
    m = (t * t) * (np.float32(3) - np.float32(2) * t)
    want = np.rint(np.float32(255) * m).astype(np.uint8)
    got = MK.key_ref(src, GREEN, lo=lo, hi=hi, luma=luma, radius=0)
    assert np.array_equal(got, want) and 0 < got.mean() < 255 and len(np.unique(got)) > 20


def test_window_is_the_clamped_box():
    b = np.zeros((3, 9, 16), np.uint8)
    b[2, 0, 0] = 100                              # dB = 100 at the corner: dy = (2900 + 128) >> 8 = 11, cb = 89, cr = -11
    D = MK.distance_ref(b, (0, 0, 0))
    assert D[0, 0] == 89 * 89 + 11 * 11 and D.sum() == D[0, 0]
    S = MK.window_sum(D, 1)
    assert S[0, 0] == 4 * D[0, 0] and S[0, 1] == S[1, 0] == 2 * D[0, 0] and S[1, 1] == D[0, 0] and S[2, 2] == 0
    P = MK.plane_of(D, lo=0, hi=np.sqrt(4 * D[0, 0] / 9), radius=1)
    assert P[0, 0] == 255 and 0 < P[1, 1] < P[0, 1] < 255 and P[2, 2] == 0


def planted(dR, dG, dB, key=(100, 100, 100)):
    """a 1 x 8 frame whose every pixel differs from `key` by (dR, dG, dB)"""
    b = np.empty((3, 1, 8), np.uint8)
    for c, d in enumerate((dR, dG, dB)):
        b[c] = key[c] + d
    return of_bytes(b), key


def test_planted_boundaries():
    # dR = 4, dG = 0, dB = 3: dy = (308 + 87 + 128) >> 8 = 2 ... choose differences whose dy is 0 instead: cb = 3, cr = 4, D = 25
    src, key = planted(4, -3, 3)                  # 77 * 4 - 150 * 3 + 29 * 3 + 128 = 73 -> dy = 0
    assert (MK.distance_ref(source_bytes(src), key) == 25).all()
    assert (MK.key_ref(src, key, lo=5, hi=5, radius=0) == 255).all()                           # hard, D = lo^2: at the threshold counts
    src1, _ = planted(4, -3, 2)                   # one level below: 44 -> dy = 0, cb = 2, cr = 4, D = 20
    assert (MK.distance_ref(source_bytes(src1), key) == 20).all()
    assert (MK.key_ref(src1, key, lo=5, hi=5, radius=0) == 0).all()
    assert (MK.key_ref(src, key, lo=3, hi=5, radius=0) == 255).all()                           # D exactly at hi^2
    assert (MK.key_ref(src, key, lo=5, hi=7, radius=0) == 0).all()                             # D exactly at lo^2, soft
    mid = MK.key_ref(src1, key, lo=3, hi=5, radius=0)                                          # (20 - 9) / 16
    t = np.float32(11.0) * np.float32(1.0 / 16.0)
    assert (mid == int(np.rint(np.float32(255) * ((t * t) * (np.float32(3) - np.float32(2) * t))))).all() and 0 < mid[0, 0] < 255
    # the arithmetic shift rounds towards minus infinity: dy of (-1, 0, 0) is (-77 + 128) >> 8 = 0, of (-2, -1, 0) (-304 + 128) >> 8 = -1
    assert (MK.distance_ref(source_bytes(planted(-2, -1, 0)[0]), key, luma=1.0) == 1 + 1 + 1).all()      # cb = 1, cr = -1, dy^2 = 1


def test_integer_bounds_at_the_extreme_triples():
    worst = 0
    for a in itertools.product((0, 255), repeat=6):
        b = np.array(a[:3], np.uint8).reshape(3, 1, 1)
        for luma in (0.0, 1.0):
            D = MK.distance_ref(b, a[3:], luma)   # (asserts D <= MAX_D inside)
            worst = max(worst, int(D.max()))
    assert 0 < worst <= MK.MAX_D == 585225 < 1 << 20
    assert (2 * MK.MAX_RADIUS + 1) ** 2 * MK.MAX_D < 1 << 31
    # a frame of the worst triple through the widest window (plane_of asserts the sum's bound)
    b = np.zeros((3, 12, 16), np.uint8)
    b[0], b[2] = 255, 255
    assert (MK.plane_of(MK.distance_ref(b, (0, 255, 0), 1.0), lo=1024, hi=1024, radius=4) == 0).all()
    assert MK.luma_weight(1.0) == 256 and MK.luma_weight(0.25) == 64 and MK.luma_weight(0.0) == 0
    lo2, inv, hard = MK.key_params(40, 90)
    assert (lo2, inv, hard) == (np.float32(1600.0), np.float32(1.0 / 6500.0), False)
    assert MK.key_params(1024, 1024) == (np.float32(1048576.0), np.float32(0.0), True)


def test_and_or_equal_front_ref():
    src, depth = frame16(3), depth16(4)
    matte = dict(lo=0.3, hi=0.7, keep="far")
    for combine in ("replace", "and", "or"):
        s = dict(MK.DEFAULTS, lo=140.0, hi=190.0, luma=0.25, radius=2, combine=combine, invert=combine == "or")
        P = MK.key_ref(src, GREEN, lo=140.0, hi=190.0, luma=0.25, radius=2, invert=s["invert"])
        assert 20 < P.mean() < 235
        want = MI.front_ref(P, depth, 0.3, 0.7, "far", combine)
        assert np.array_equal(bits(MK.raw_ref(src, GREEN, depth, matte, s)), bits(want))
    ramp = MT.matte_ref(depth, 0.3, 0.7, 0, "far")[0]
    full = dict(MK.DEFAULTS, lo=0.0, hi=0.0, combine="and")                                    # a key that is 255 everywhere
    assert np.array_equal(bits(MK.raw_ref(src, GREEN, depth, matte, full)), bits(ramp))


def test_synthetic_green_screen():
    """the colour defaults on a synthetic frame: 0 on the lit screen, little on the shadowed screen, 255 on skin, dark and white.
    The bounds are worked out by hand.  Lit screen, noise of +-6 per channel: |dy| <= 6, |cb|, |cr| <= 12, D <= 288 < lo^2 = 1600.
    Shadow at 0.6, (0, 106, 38) against (0, 177, 64): dy = (-10650 - 754 + 128) >> 8 = -45, cb = 19, cr = 45, D = 2386 (with
    luma = 0.25: + (64 * 2025 + 128) >> 8 = 506); with the noise cb <= 30, cr <= 56, D <= 4036 -> t <= 0.375, P <= 81."""
    def smooth(D):
        t = (np.float32(D) - np.float32(1600.0)) * np.float32(1.0 / 6500.0)
        return int(np.rint(np.float32(255) * ((t * t) * (np.float32(3) - np.float32(2) * t))))

    rng = np.random.default_rng(5)
    s = {k: MK.DEFAULTS[k] for k in ("lo", "hi", "luma", "radius")}
    for noise in (0, 6):
        b = np.empty((3, 48, 64), np.int64)
        for c in range(3):
            b[c] = GREEN[c]
        b[:, :, 32:] = (b[:, :, 32:] * 0.6).astype(np.int64)              # a band of the screen in shadow
        if noise:
            b += rng.integers(-noise, noise + 1, b.shape)
        for (y, x), rgb in (((8, 8), (224, 172, 140)), ((24, 8), (20, 20, 24)), ((8, 40), (250, 250, 250))):
            b[:, y:y + 8, x:x + 8] = np.array(rgb)[:, None, None]
        src = of_bytes(np.clip(b, 0, 255).astype(np.uint8))
        P, Pl = MK.key_ref(src, GREEN, **s), MK.key_ref(src, GREEN, **dict(s, luma=0.25))
        assert not P[40:, :30].any() and not Pl[40:, :30].any()
        if noise:
            assert 0 < P[40:, 34:].max() <= smooth(4036) == 81
        else:
            assert (P[40:, 34:] == smooth(2386)).all() and smooth(2386) == 10
            assert (Pl[40:, 34:] == smooth(2386 + 506)).all() and smooth(2892) == 26
        for y, x in ((8, 8), (24, 8), (8, 40)):
            assert (P[y + 1:y + 7, x + 1:x + 7] == 255).all()


def test_plate_ref_and_value_errors(tmp_path):
    from PIL import Image

    from live2diff_amd.backdrop import image_ref
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (60, 90, 3), dtype=np.uint8)
    p = tmp_path / "plate.png"
    Image.fromarray(img).save(p)
    want = image_ref(img, H, W, "bilinear").transpose(2, 0, 1)
    for given in (img, Image.fromarray(img), str(p)):
        got = MK.plate_ref(given, H, W, "bilinear")
        assert got.dtype == np.uint8 and got.shape == (3, H, W) and got.flags.c_contiguous and np.array_equal(got, want)
    assert MK.check_settings() == dict(lo=40.0, hi=90.0, luma=0.0, radius=1, combine="replace", invert=False) == MK.DEFAULTS
    assert MK.check_settings(plate=True)["luma"] == 0.25 and MK.check_settings(luma=0.5, plate=True)["luma"] == 0.5
    for kw, name in ((dict(lo=-1), "lo="), (dict(hi=1025), "hi="), (dict(lo=True), "lo="), (dict(lo=91), "lo="), (dict(lo=float("nan")), "lo="),
                     (dict(luma=1.5), "luma="), (dict(luma="0"), "luma="), (dict(radius=5), "radius="), (dict(radius=1.0), "radius="),
                     (dict(radius=True), "radius="), (dict(combine="xor"), "combine="), (dict(invert=1), "invert=")):
        with pytest.raises(ValueError, match="matte key: .*" + name):
            MK.check_settings(**kw)
    for to in ((0, 0, 256), (0, 0), (0.0, 1, 2), (True, 0, 0)):
        with pytest.raises(ValueError, match="to="):
            MK.check_color(to)
    with pytest.raises(ValueError, match="plate is a planar uint8"):
        MK.key_ref(frame16(1), np.zeros((3, H, W + 8), np.uint8), lo=1, hi=2)
    with pytest.raises(ValueError, match="radius="):
        MK.key_ref(frame16(1), GREEN, lo=1, hi=2, radius=5)
    assert "untuned" in MK.__doc__.lower() or "not tuned" in MK.__doc__.lower()


# ----------------------------------------------------------------------------- the builders and the launchers (dry run)
@pytest.fixture
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def test_launcher_checks(dry_run):
    from live2diff_amd import _lib, ops
    assert _lib.OP_MATTE_KEY == 59 and _lib.OP_FRAME_PLANAR_BYTES == 60
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_MATTE_KEY = 59," in hdr and "L2D_OP_FRAME_PLANAR_BYTES = 60," in hdr
    assert all(f"#define L2D_MATTE_KEY_{n} {v} " in hdr for n, v in (
        ("PLATE", ops.MATTE_KEY_PLATE), ("HARD", ops.MATTE_KEY_HARD), ("INVERT", ops.MATTE_KEY_INVERT), ("AND", ops.MATTE_KEY_AND),
        ("OR", ops.MATTE_KEY_OR), ("RAMP_HARD", ops.MATTE_KEY_RAMP_HARD), ("RAMP_FAR", ops.MATTE_KEY_RAMP_FAR)))
    assert f"#define L2D_MATTE_KEY_MAX_R {ops.MATTE_KEY_MAX_R}\n" in hdr and MK.MAX_RADIUS == 4

    def key(**kw):
        args = dict(source=torch.zeros(3, H, W, dtype=torch.float16), out=torch.zeros(H, W), depth=torch.zeros(H, W, dtype=torch.float16),
                    key=GREEN, H=H, W=W, r=1, L=64, lo2=1600.0, inv=float(np.float32(1 / 6500)), hard=False)
        args.update(kw)
        return ops.matte_key(*[args.pop(k) for k in ("source", "out", "depth", "key")], **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    plate = torch.zeros(3, H, W, dtype=torch.uint8)
    op, keep = key(key=plate, combine="or", invert=True, lo32=-0.4, inv32=1.25, far=True, r=4, L=256)
    assert op.kind == 59 and [op.p[j] for j in range(4)] == [t.data_ptr() for t in keep] and op.p[4] is None
    assert [op.i[j] for j in range(8)] == [H, W, 4, ops.MATTE_KEY_PLATE | ops.MATTE_KEY_OR | ops.MATTE_KEY_INVERT | ops.MATTE_KEY_RAMP_FAR,
                                           256, 0, 0, 0]
    assert [op.f[j] for j in range(4)] == [1600.0, float(np.float32(1 / 6500)), float(np.float32(-0.4)), 1.25]
    ops.run((op, keep))
    op, keep = key(lo32=-0.4, inv32=1.25, far=True)                       # (a replacing key: no depth, no ramp)
    assert op.p[2] is None and op.p[3] is None and op.i[3] == 0 and op.f[2] == op.f[3] == 0.0 and [op.i[j] for j in (5, 6, 7)] == list(GREEN)
    for kw in (dict(), dict(r=0), dict(L=0), dict(key=plate), dict(lo2=0.0, inv=0.0, hard=True), dict(combine="and", lo32=0.0, inv32=0.0, ramp_hard=True),
               dict(combine="or", lo32=-0.2, inv32=2.0), dict(invert=True), dict(key=[255, 0, 255])):
        ops.run(key(**kw))
    for call in (lambda: key(source=torch.zeros(3, H, W)), lambda: key(source=torch.zeros(3, H, W + 8, dtype=torch.float16)),
                 lambda: key(out=torch.zeros(H, W, dtype=torch.float16)), lambda: key(out=torch.zeros(H, W + 1)),
                 lambda: key(combine="xor"), lambda: key(combine="and", depth=None), lambda: key(combine="or", depth=torch.zeros(H, W)),
                 lambda: key(r=5), lambda: key(r=-1), lambda: key(r=1.0), lambda: key(L=257), lambda: key(L=-1), lambda: key(key=(0, 0, 256)),
                 lambda: key(key=(0, 0)), lambda: key(key=torch.zeros(3, H, W)), lambda: key(key=torch.zeros(H, W, 3, dtype=torch.uint8)),
                 lambda: key(lo2=-1.0), lambda: key(inv=float("inf")), lambda: key(lo2=float("nan")), lambda: key(inv=0.0),
                 lambda: key(hard=True), lambda: key(H=H, W=W - 4, source=torch.zeros(3, H, W - 4, dtype=torch.float16), out=torch.zeros(H, W - 4))):
        with pytest.raises(ValueError, match="matte_key"):
            call()
    for k, v, match in ((3, 32, "unknown flag bits"), (3, 256, "unknown flag bits"), (3, 24, "two ways to combine"), (3, 64, "ramp flags without"),
                        (0, 0, "non-positive size"), (1, W - 4, "multiple of 8"), (2, 5, "radius"), (2, -1, "radius"), (4, 257, "luma weight"),
                        (4, -1, "luma weight"), (5, 256, "key colour"), (7, -1, "key colour"), (3, ops.MATTE_KEY_HARD, "hard flag"),
                        (3, ops.MATTE_KEY_PLATE, "pointer 3")):
        op, keep = key()
        op.i[k] = v
        bad(match, (op, keep))
    for k, match in ((0, "pointer 0 is null"), (1, "pointer 1 is null"), (2, "pointer 2"), (3, "pointer 3")):
        op, keep = key(key=plate, combine="and", lo32=-0.2, inv32=2.0)
        op.p[k] = None
        bad(match, (op, keep))
    for k, off, match in ((0, 8, "pointer 0 is not 16-byte aligned"), (1, 8, "pointer 1 is not 16-byte aligned"), (2, 8, "pointer 2"), (3, 4, "pointer 3")):
        op, keep = key(key=plate, combine="and", lo32=-0.2, inv32=2.0)
        op.p[k] += off
        bad(match, (op, keep))
    for f, v in ((0, -1.0), (0, float("inf")), (0, float("nan")), (1, -1.0), (1, float("inf")), (1, 0.0)):
        op, keep = key()
        op.f[f] = v
        bad("finite and not negative", (op, keep))
    for kw in (dict(lo32=-1.5), dict(inv32=-1.0), dict(inv32=float("inf")), dict(inv32=0.0), dict(ramp_hard=True)):
        bad("must lie in \\[-1, 1\\]", key(combine="and", **dict(dict(lo32=-0.2, inv32=2.0), **kw)))
    raw = torch.zeros(6 * H * W, dtype=torch.uint8)
    bad("overlaps", key(source=raw.view(torch.float16).view(3, H, W), out=raw[:4 * H * W].view(torch.float32).view(H, W)))
    bad("overlaps", key(combine="or", lo32=-0.2, inv32=2.0, out=raw[:4 * H * W].view(torch.float32).view(H, W),
                        depth=raw[:2 * H * W].view(torch.float16).view(H, W)))
    bad("overlaps", key(key=raw[:3 * H * W].view(3, H, W), out=raw[:4 * H * W].view(torch.float32).view(H, W)))

    # op 60
    def planar(**kw):
        args = dict(source=torch.zeros(3, H, W, dtype=torch.float16), out=torch.zeros(3, H, W, dtype=torch.uint8), H=H, W=W)
        args.update(kw)
        return ops.frame_planar_bytes(args.pop("source"), args.pop("out"), **args)

    op, keep = planar()
    assert op.kind == 60 and [op.p[j] for j in range(3)] == [keep[0].data_ptr(), keep[1].data_ptr(), None] and (op.i[0], op.i[1]) == (H, W)
    ops.run((op, keep))
    for call in (lambda: planar(source=torch.zeros(3, H, W)), lambda: planar(out=torch.zeros(H, W, 3, dtype=torch.uint8)),
                 lambda: planar(out=torch.zeros(3, H, W, dtype=torch.int8)),
                 lambda: planar(W=W - 4, source=torch.zeros(3, H, W - 4, dtype=torch.float16), out=torch.zeros(3, H, W - 4, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="frame_planar_bytes"):
            call()
    for k, v, match in ((0, 0, "non-positive size"), (1, W - 4, "multiple of 8")):
        op, keep = planar()
        op.i[k] = v
        bad(match, (op, keep))
    for k in range(2):
        op, keep = planar()
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
        op, keep = planar()
        op.p[k] += 8
        bad(f"pointer {k} is not 16-byte aligned", (op, keep))
    bad("overlap", planar(source=raw.view(torch.float16).view(3, H, W), out=raw[:3 * H * W].view(3, H, W)))

    # HipMatteKey in a dry run: the records and their order
    mk = MK.HipMatteKey(H, W, device="cpu")
    slot = MT._Slot(H, W, "cpu")
    matte = dict(lo=0.3, hi=0.7, keep="near")
    s = dict(MK.DEFAULTS, to=GREEN)
    records, keep, plane = mk.record(slot, matte, s)
    assert [r.kind for r in records] == [59] and plane is mk.plane and records[0].i[3] == 0
    with pytest.raises(ValueError, match="no plate is set"):
        mk.record(slot, matte, dict(s, to="plate"))
    records, keep, plane = mk.record(slot, matte, dict(s, to="plate", combine="and"), capture=True)
    assert [r.kind for r in records] == [60, 59] and records[0].p[1] == records[1].p[3] == mk.plate.data_ptr()
    assert records[1].i[3] == ops.MATTE_KEY_PLATE | ops.MATTE_KEY_AND and records[1].p[2] == slot.depth.data_ptr()
    assert [r.kind for r in mk.record(slot, matte, dict(s, to="plate"))[0]] == [59]            # the plate stays
    mk.set_plate(np.zeros((3, H, W), np.uint8))
    with pytest.raises(ValueError, match="planar uint8"):
        mk.set_plate(np.zeros((H, W, 3), np.uint8))
    assert mk.key(slot.source, slot.depth, matte, s) is mk.plane


# ----------------------------------------------------------------------------- the wrapper on the mock components (host route)
def call(w, f, **kw):
    torch.manual_seed(77)                        # (the host path draws its re-noising from the global generator)
    return w(f, **kw)


def made(monkeypatch, n=2, matte=dict(lo=0.3, hi=0.7, keep="near", feather=0), drop=None, **setup):
    import pipeline_mocks as M
    torch.manual_seed(123)
    w = build(monkeypatch, n, drop=drop)
    if matte is not None:
        w.set_matte(matte["lo"], matte["hi"], keep=matte["keep"], feather=matte["feather"])
    for name, kw in setup.items():
        getattr(w, "set_" + name)(**kw)
    w.prepare(M.frames(8, seed=7), "a prompt")
    return w


def screen_frames(k, seed=8):
    """frames in [0, 1] that show a green screen with a box of noise (the subject) at a place of the frame's own"""
    import pipeline_mocks as M
    out = []
    for j, f in enumerate(M.frames(k, seed=seed)):
        g = (torch.tensor(GREEN, dtype=torch.float32) / 255.0)[:, None, None].expand(3, M.H, M.W).clone()
        y, x = 6 + 5 * j, 40 - 5 * j
        g[:, y:y + 16, x:x + 16] = f[:, y:y + 16, x:x + 16] * 0.5 + torch.tensor([0.5, 0.0, 0.5])[:, None, None]      # (magenta-ish: far from green)
        out.append(g)
    return out


def by_hand(w, key):
    """the oracles chained by hand beside a wrapper, on the slot the last output was composited with"""
    slot, mt = w._matte_line.last, w.matte
    raw = MK.raw_ref(slot.source, key, slot.depth[None], mt, w.matte_key)
    m0 = raw if w.matte_edge is None else MT.edge_ref(raw, slot.source, **w.matte_edge)
    return MT.composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **mt, plane=m0[None])[0]


@pytest.mark.parametrize("n", [2, 3])
def test_wrapper_the_key_is_delayed_with_its_frame(monkeypatch, n):
    import pipeline_mocks as M
    frames = screen_frames(6)
    w, twin = made(monkeypatch, n), made(monkeypatch, n)
    w.set_matte_key(GREEN)
    assert w.matte_key == dict(MK.DEFAULTS, to=GREEN)
    warm = M.frames(8, seed=7)[-1]
    for k in range(6):
        got = call(w, frames[k])
        plain = call(twin, frames[k])
        styled = egress_ref(w.stream.prev_image_result)[0].numpy()
        j = k - (n - 1)
        src = src_bytes(warm if j < 0 else frames[j])                                          # [H,W,3]
        P = MK.plane_of(MK.distance_ref(np.ascontiguousarray(src.transpose(2, 0, 1)), GREEN), lo=40, hi=90, radius=1)
        assert np.array_equal(got, by_hand(w, GREEN)), k
        assert np.array_equal(got[P == 0], src[P == 0]) and np.array_equal(got[P == 255], styled[P == 255]), k
        assert not np.array_equal(got, plain), k
        if j >= 0:                               # the box of frame j, not of frame k
            y, x = 6 + 5 * j, 40 - 5 * j
            assert (P[y + 1:y + 15, x + 1:x + 15] == 255).all() and not P[:y - 1].any() and not P[:, x + 18:].any(), k
        else:
            assert (P == 255).all()              # the warm-up frame is noise: nothing of it is the key's
    w.clear_matte_key()
    assert w.matte_key is None
    assert np.array_equal(call(w, frames[0]), call(twin, frames[0]))                           # the parent's frame, byte for byte


def test_wrapper_capture_takes_the_frame_of_the_next_output(monkeypatch):
    frames = screen_frames(6)
    w = made(monkeypatch, 2)
    call(w, frames[0])
    w.set_matte_key("capture", lo=20, hi=60, radius=2)
    assert w.matte_key == dict(lo=20.0, hi=60.0, luma=0.25, radius=2, combine="replace", invert=False, to="capture")
    got = call(w, frames[1])                     # output 1 shows frame 0: that frame is the plate, and is keyed against itself
    assert w.matte_key["to"] == "plate"
    plate = np.ascontiguousarray(src_bytes(frames[0]).transpose(2, 0, 1))
    assert np.array_equal(w._key_plate, plate)
    assert np.array_equal(got, src_bytes(frames[0]))                                           # P = 0 everywhere: the real frame
    for k in (2, 3):
        got = call(w, frames[k])                 # frame k - 1 against frame 0: both boxes differ, the screen does not
        assert np.array_equal(w._key_plate, plate) and np.array_equal(got, by_hand(w, plate)), k
        P = MK.key_ref(w._matte_line.last.source, plate, lo=20, hi=60, luma=0.25, radius=2)
        assert 0 < (P == 255).sum() < P.size and (P == 0).sum() > P.size // 2
    w.capture_matte_plate()
    assert w.matte_key["to"] == "capture" and w.matte_key["lo"] == 20.0
    got = call(w, frames[4])
    assert w.matte_key["to"] == "plate" and np.array_equal(w._key_plate, np.ascontiguousarray(src_bytes(frames[3]).transpose(2, 0, 1)))
    assert np.array_equal(got, src_bytes(frames[3]))


def test_wrapper_plate_from_an_image_edge_and_a_dropped_frame(monkeypatch, tmp_path):
    from PIL import Image
    frames = screen_frames(5)
    room = src_bytes(frames[0])                  # a picture of "the empty room" of another size: resampled by plate_ref
    big = np.asarray(Image.fromarray(room).resize((96, 96), Image.BILINEAR))
    p = tmp_path / "room.png"
    Image.fromarray(big).save(p)
    w = made(monkeypatch, 2, drop={2})
    w.stream.inference_time_ema = 0.0            # (a dropped frame waits that long)
    w.set_matte_key(str(p), combine="and", luma=0.5)
    w.set_matte_edge(radius=2, eps=4.0)
    plate = MK.plate_ref(big, 64, 64, "lanczos")
    assert w.matte_key["to"] == "plate" and w.matte_key["luma"] == 0.5 and np.array_equal(w._key_plate, plate)
    got = []
    for k in range(5):
        got.append(call(w, frames[k]))
        if k != 2:
            assert np.array_equal(got[k], by_hand(w, plate)), k
    assert np.array_equal(got[2], got[1]) and w._matte_line.tapped == 4                        # the repeated output re-keys `last`
    with pytest.raises(ValueError, match="cannot|image"):
        bad = tmp_path / "bad.png"
        bad.write_bytes(b"no image")
        w.set_matte_key(str(bad))
    assert w.matte_key["to"] == "plate"          # (a refused call changes nothing)


def test_exclusion_with_masks_a_key_needs_a_matte_and_clear_matte(monkeypatch):
    import pipeline_mocks as M
    w = made(monkeypatch, 2, matte=None)
    f = screen_frames(1)[0]
    mask = np.full((64, 64), 255, np.uint8)
    assert w.matte_key is None
    with pytest.raises(ValueError, match="needs a matte"):
        w.set_matte_key(GREEN)
    with pytest.raises(ValueError, match="no matte key"):
        w.capture_matte_plate()
    w.set_matte(0.3, 0.7)
    w.set_mask(mask)
    with pytest.raises(ValueError, match="(?s)key.*mask|mask.*key"):
        w.set_matte_key(GREEN)
    w.clear_mask()
    w.set_matte_key(GREEN, lo=10, hi=20)
    w._hold_init = False
    w.set_matte_key(GREEN, lo=10, hi=30)
    assert w._hold_init is True                   # any change of the key restarts a hold
    for bad in (lambda: w.set_mask(mask), lambda: w(f, mask=mask), lambda: w.push(f, mask=mask),
                lambda: w.prepare(M.frames(8, seed=7), "a prompt", warmup_masks=[mask] * 8)):
        with pytest.raises(ValueError, match="(?s)key.*mask|mask.*key"):
            bad()
    for kw, name in ((dict(lo=-1), "lo="), (dict(radius=5), "radius="), (dict(combine="nor"), "combine="), (dict(luma=2), "luma=")):
        with pytest.raises(ValueError, match=name):
            w.set_matte_key(GREEN, **kw)
    for to in ((0, 0, 300), None, 5):
        with pytest.raises(ValueError, match="to="):
            w.set_matte_key(to)
    assert w.matte_key == dict(MK.DEFAULTS, lo=10.0, hi=30.0, to=GREEN)
    w.clear_matte()
    assert w.matte_key is None and w._key_dev is None


def test_constructor_keyword(monkeypatch):
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    assert inspect.signature(Wrapper.__init__).parameters["matte_key"].default is None
    p = inspect.signature(Wrapper.set_matte_key).parameters
    assert [k for k in p][1] == "to" and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("lo", "hi", "luma", "radius", "combine", "invert"))
    assert (p["lo"].default, p["hi"].default, p["luma"].default, p["radius"].default, p["combine"].default, p["invert"].default) == \
        (None, None, None, 1, "replace", False)
    real = Wrapper.from_components

    def with_key(value):
        monkeypatch.setattr(Wrapper, "from_components", classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, matte_key=value, **kw)))

    with_key("green")
    with pytest.raises(ValueError, match="matte_key="):
        build(monkeypatch, 2)
    with_key(dict(lo=3))
    with pytest.raises(ValueError, match="matte_key="):
        build(monkeypatch, 2)
    with_key(dict(to=GREEN, lo=-3))
    with pytest.raises(ValueError, match="lo="):
        build(monkeypatch, 2)
    with_key(dict(to=GREEN, hi=120, combine="or"))                                             # (it waits for the first set_matte)
    w = build(monkeypatch, 2)
    assert w.matte_key == dict(MK.DEFAULTS, hi=120.0, combine="or", to=GREEN)
    with_key(dict(to="capture"))
    assert build(monkeypatch, 2).matte_key == dict(MK.PLATE_DEFAULTS, to="capture")
    with_key(None)
    assert build(monkeypatch, 2).matte_key is None
