"""CPU tests (-m "not gpu") of the plate gain (live2diff_amd/matte_key.py): the numpy oracle of
L2D_OP_MATTE_KEY_GAIN_HIST / L2D_OP_MATTE_KEY_GAIN and of L2D_MATTE_KEY_GAIN on ops 59 and 61 -- cases planted and worked out by
hand, a room under a white-balance step, the gain beside the adaptive plate --, the settings, the builders and launchers in a dry
run, `HipMatteKey`'s lists, and `set_matte_key_gain` on the wrapper's host route."""
import inspect
import os

import numpy as np
import pytest
import torch

from live2diff_amd import matte as MT
from live2diff_amd import matte_key as MK
from live2diff_amd.backdrop import frame_of
from live2diff_amd.steady import source_bytes
from test_matte_cpu import build
from test_matte_key_cpu import GREEN, H, W, call, depth16, dry_run, frame16, made, screen_frames  # noqa: F401  (dry_run: the fixture)

KEY = dict(lo=40.0, hi=90.0, luma=0.25, radius=1)          # the plate defaults
LIM, UNITY = 256, 128


def planes(b, k, h=1, w=8):
    """planar uint8 [3,h,w] pairs whose every sample is (b, k)"""
    return np.full((3, h, w), b, np.uint8), np.full((3, h, w), k, np.uint8)


def hist_of(counts):
    """a [3,512] histogram with the same {q: count} on every channel"""
    h = np.zeros((3, MK.GAIN_BINS), np.int64)
    for q, c in counts.items():
        h[:, q] = c
    return h


# ----------------------------------------------------------------------------- planted cases
# (b, k, q) with q = (128 b + (k >> 1)) // k worked out by hand:
#   (100, 33): 12816 = 33 * 388 + 12          (77, 39): 9875 = 39 * 253 + 8          (50, 37): 6418 = 37 * 173 + 17
#   (9, 17): 1160 = 17 * 68 + 4               (251, 16): 32136 = 16 * 2008 + 8 -> bin 511      (200, 33): 25616 = 33 * 776 + 8 -> 511
#   (101, 49): 12952 = 49 * 264 + 16          (7, 17): 904 = 17 * 53 + 3
#   (10, 19): 1289 = 19 * 67 + 16: the floor is 67 where rounding the quotient 67.84 to nearest would give 68
FLOORS = [(100, 33, 388), (77, 39, 253), (50, 37, 173), (9, 17, 68), (251, 16, 511), (200, 33, 511), (101, 49, 264), (7, 17, 53),
          (10, 19, 67)]


def test_a_frame_equal_to_its_plate_measures_unity_and_keys_as_key_ref():
    rng = np.random.default_rng(1)
    plate = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    hist = MK.gain_hist_ref(plate, plate)
    valid = ((plate >= 16) & (plate <= 239)).reshape(3, -1).sum(1)
    assert hist.shape == (3, 512) and np.array_equal(hist[:, UNITY], valid) and hist.sum() == valid.sum()      # b == k: exactly 128
    g, n = MK.gain_of(hist, LIM, 1)
    assert g.tolist() == [UNITY] * 3 and np.array_equal(n, valid)
    src = frame_of(plate)
    assert np.array_equal(MK.gain_plate(plate, g), plate)
    assert np.array_equal(MK.key_ref(src, plate, **KEY, gain=g), MK.key_ref(src, plate, **KEY))
    assert MK.key_ref(src, plate, **KEY, gain=g).max() == 0


def test_five_quarters_is_160_exactly():
    k1 = np.arange(16, 200, 4)[:40]                           # multiples of 4 with 5 k / 4 <= 251
    k = np.broadcast_to(k1[None, None], (3, 1, 40)).astype(np.uint8)
    b = (5 * k.astype(int) // 4).astype(np.uint8)
    assert b.max() <= 251 and np.all(4 * b.astype(int) == 5 * k.astype(int))
    hist = MK.gain_hist_ref(b, k)
    assert np.array_equal(hist[:, 160], [k[0].size] * 3) and hist.sum() == k.size
    assert MK.gain_of(hist, LIM, 1)[0].tolist() == [160] * 3


@pytest.mark.parametrize("b,k,q", FLOORS)
def test_the_floor_by_hand(b, k, q):
    hist = MK.gain_hist_ref(*planes(b, k))
    assert np.array_equal(np.nonzero(hist[0])[0], [q]) and hist[0, q] == 8


def test_the_validity_limits_and_the_saturating_bin():
    for k, ok in ((15, False), (16, True), (239, True), (240, False)):
        assert MK.gain_hist_ref(*planes(100, k)).sum() == (24 if ok else 0), k
    for b, ok in ((3, False), (4, True), (251, True), (252, False)):
        assert MK.gain_hist_ref(*planes(b, 100)).sum() == (24 if ok else 0), b
    hist = MK.gain_hist_ref(*planes(251, 16))                 # 2008 -> 511
    assert hist[:, 511].tolist() == [8] * 3
    hist = MK.gain_hist_ref(*planes(64, 16))                  # (8192 + 8) // 16 = 512 -> 511: the first ratio that saturates
    assert hist[:, 511].tolist() == [8] * 3
    hist = MK.gain_hist_ref(*planes(255, 64))                 # 510 would fit, but b = 255 is clipped
    assert hist.sum() == 0
    # channels are counted apart
    b, k = planes(100, 100)
    b[1], k[2] = 125, 15
    hist = MK.gain_hist_ref(b, k)
    assert hist[0, 128] == 8 and hist[1, 160] == 8 and hist[2].sum() == 0


def test_the_median_a_tie_and_min_count():
    # 2 cum == n exactly at q = 100: the lower median stays there
    assert MK.gain_of(hist_of({100: 5, 140: 5}), LIM, 1)[0].tolist() == [100] * 3
    assert MK.gain_of(hist_of({100: 4, 140: 5}), LIM, 1)[0].tolist() == [140] * 3
    assert MK.gain_of(hist_of({100: 5, 140: 4}), LIM, 1)[0].tolist() == [100] * 3
    assert MK.gain_of(hist_of({100: 1, 120: 1, 140: 1}), LIM, 1)[0].tolist() == [120] * 3
    # n = min_count - 1 against n = min_count
    h = hist_of({150: 7})
    g, n = MK.gain_of(h, LIM, 8)
    assert g.tolist() == [UNITY] * 3 and n.tolist() == [7] * 3
    assert MK.gain_of(h, LIM, 7)[0].tolist() == [150] * 3
    # per channel
    h[1] = 0
    assert MK.gain_of(h, LIM, 7)[0].tolist() == [150, UNITY, 150]
    # no sample at all under min_count 0: the smallest q with 0 >= 0 is 0, clamped to the lower end
    assert MK.gain_of(hist_of({}), LIM, 0)[0].tolist() == [64] * 3
    # the subject past one half takes the median: the docstring says so
    assert "less than half" in " ".join(MK.gain_of.__doc__.split()) and "60 %" in MK.gain_of.__doc__
    assert MK.gain_of(hist_of({160: 4, 300: 6}), 511, 1)[0].tolist() == [300] * 3


def test_both_ends_of_the_clamp_and_the_saturating_plate():
    for lim, lo in ((256, 64), (128, 128), (511, 33), (200, 82), (129, 128)):       # ceil(16384 / lim)
        assert lo == -(-16384 // lim)
        assert MK.gain_of(hist_of({511: 3}), lim, 1)[0].tolist() == [lim] * 3
        assert MK.gain_of(hist_of({1: 3}), lim, 1)[0].tolist() == [lo] * 3
        assert MK.gain_of(hist_of({lim: 3}), lim, 1)[0].tolist() == [lim] * 3 and MK.gain_of(hist_of({lo: 3}), lim, 1)[0].tolist() == [lo] * 3
    assert MK.gain_params(2.0, 1 / 16, 72, 136) == (256, 612) and MK.gain_params(3.99, 0.0, 8, 8) == (511, 0)
    assert MK.gain_params(1.0, 1.0, 8, 8) == (128, 64) and MK.gain_params(2.0, 1 / 3, 1, 8) == (256, 3)
    # k' = min(255, (g k + 64) >> 7)
    k = np.array([[[0, 1, 100, 127, 128, 200, 254, 255]]] * 3, np.uint8)
    assert np.array_equal(MK.gain_plate(k, (128, 128, 128)), k)
    got = MK.gain_plate(k, (256, 511, 32))
    assert got[0, 0].tolist() == [0, 2, 200, 254, 255, 255, 255, 255]
    assert got[1, 0].tolist() == [0, 4, 255, 255, 255, 255, 255, 255]       # (511 + 64) >> 7 = 4
    assert got[2, 0].tolist() == [0, 0, 25, 32, 32, 50, 64, 64]              # (32 * 1 + 64) >> 7 = 0, (8128 + 64) >> 7 = 64
    assert MK.gain_plate(k, (160, 100, 0))[:, 0, 2].tolist() == [125, 78, 0]  # (16000 + 64) >> 7 = 125, (10000 + 64) >> 7 = 78


def test_the_two_bounds():
    assert (MK.GAIN_BINS - 1) * 255 + 64 == 130369 < 1 << 17                # g k + 64
    assert MK.gain_plate(np.full((3, 1, 8), 255, np.uint8), (511, 511, 511)).max() == 255
    src = inspect.getsource(MK.gain_plate) + inspect.getsource(MK.gain_hist_ref) + inspect.getsource(MK.gain_of)
    assert "< 1 << 17" in src and "< 1 << 31" in src                         # the oracle asserts both
    hip = open(os.path.join(os.path.dirname(os.path.abspath(MK.__file__)), "csrc", "matte_key.hip")).read()
    assert "(MKG_BINS - 1) * 255 + 64 < (1 << 17)" in hip and "2^31 / 3" in hip
    for bad in ((128, 128), (128, 128, 512), (128, 128, -1), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="gain"):
            MK.gain_plate(np.zeros((3, 1, 8), np.uint8), bad)
    with pytest.raises(ValueError, match="lim="):
        MK.gain_of(hist_of({}), 127, 0)
    with pytest.raises(ValueError, match="lim="):
        MK.gain_of(hist_of({}), 512, 0)
    with pytest.raises(ValueError, match="min_count="):
        MK.gain_of(hist_of({}), 256, -1)
    with pytest.raises(ValueError, match="histogram"):
        MK.gain_of(np.zeros((3, 511), np.int64), 256, 0)
    with pytest.raises(ValueError, match="shape"):
        MK.gain_hist_ref(np.zeros((3, 1, 8), np.uint8), np.zeros((3, 2, 8), np.uint8))


def test_unity_gain_reproduces_raw_ref_and_raw_adapt_ref():
    rng = np.random.default_rng(5)
    plate = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    state = np.clip(plate.astype(np.int64) * 256 + rng.integers(-200, 201, plate.shape), 0, MK.MAX_STATE).astype(np.uint16)
    matte, depth = dict(lo=0.3, hi=0.7, keep="far"), depth16(4)
    ad = dict(rate=1 / 8, absorb=1 / 64)
    unity = (UNITY,) * 3
    for combine in ("replace", "and", "or"):
        for invert in (False, True):
            ks = dict(KEY, combine=combine, invert=invert, to="plate")
            src = frame16(30)
            assert np.array_equal(MK.raw_ref(src, plate, depth, matte, ks, gain=unity), MK.raw_ref(src, plate, depth, matte, ks))
            a, b = MK.raw_adapt_ref(src, state, depth, matte, ks, ad, gain=unity), MK.raw_adapt_ref(src, state, depth, matte, ks, ad)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # another gain changes the plane, and under the adaptive plate only through the plane's gate: e = 256 b - s stays
    ks = dict(KEY, combine="replace", invert=False, to="plate")
    near = frame_of(np.clip(plate.astype(int) * 5 // 4, 0, 255).astype(np.uint8))
    P, nxt = MK.key_adapt_ref(near, MK.state_of(plate), **KEY, rate=0.5, absorb=0.5, gain=(200, 128, 90))
    P1, nxt1 = MK.key_adapt_ref(near, MK.state_of(plate), **KEY, rate=0.5, absorb=0.5)
    assert not np.array_equal(P, P1) and np.array_equal(nxt, nxt1)           # (equal rates: the gate does not matter)
    assert np.array_equal(P, MK.key_ref(near, MK.gain_plate(plate, (200, 128, 90)), **KEY))
    assert np.array_equal(P, MK.key_ref(near, plate, **KEY, gain=(200, 128, 90)))


# ----------------------------------------------------------------------------- the room under a white-balance step
RH, RW = 72, 136
PERSON = int(0.3 * RW)                            # the left 30 % of the columns


def room():
    """planar int64 [3,72,136]: R = 60 + x, G = 40 + 2 y, B = 200 - x // 2 - y // 2"""
    y, x = np.mgrid[0:RH, 0:RW]
    return np.stack([60 + x, 40 + 2 * y, 200 - x // 2 - y // 2]).astype(np.int64)


def stepped(gains, noise, rng, person=True):
    """the room's bytes times `gains`, rounded, plus uniform noise in -noise .. noise; the left 30 % a person of (200, 150, 120) +- 20"""
    f = np.rint(room() * np.asarray(gains, np.float64)[:, None, None]).astype(np.int64)
    if noise:
        f = f + rng.integers(-noise, noise + 1, f.shape)
    if person:
        f[:, :, :PERSON] = np.array([200, 150, 120])[:, None, None] + rng.integers(-20, 21, (3, RH, PERSON))
    return np.clip(f, 0, 255).astype(np.uint8)


def test_the_room_under_a_white_balance_step():
    rng = np.random.default_rng(0)
    plate = room().astype(np.uint8)
    assert np.array_equal(plate, room())
    b = stepped((1.3, 1.0, 0.8), 4, rng)
    src = frame_of(b)
    assert np.array_equal(source_bytes(src), b)
    r = KEY["radius"]
    wall, person = np.s_[:, PERSON + r:], np.s_[:, :PERSON - r]               # (a window at the border sees both)
    P = MK.key_ref(src, plate, **KEY)
    print("without a gain: share of the wall with P > 0:", float((P[wall] > 0).mean()))
    assert float((P[wall] > 0).mean()) > 0.9
    g, n = MK.measure_gain(b, plate, *MK.gain_params(2.0, 1 / 16, RH, RW))
    P = MK.key_ref(src, plate, **KEY, gain=g)
    D = MK.distance_ref(b, MK.gain_plate(plate, g), KEY["luma"])
    print("gain", g.tolist(), "n", n.tolist(), "largest D on the wall", int(D[wall].max()), "person's mean P", float(P[person].mean()))
    assert g.tolist() == [168, 129, 101]          # 1.3, 1.0 and 0.8 in units of 1 / 128, to within a bin
    assert P[wall].max() == 0 and int(D[wall].max()) < 1600                  # lo^2
    assert float(P[person].mean()) > 200
    # the median's limit: with the person over 60 % of the columns the gains are not the wall's
    wide = b.copy()
    n60 = int(0.6 * RW)
    wide[:, :, :n60] = np.array([200, 150, 120])[:, None, None] + rng.integers(-20, 21, (3, RH, n60))
    g60, _ = MK.measure_gain(wide, plate, *MK.gain_params(2.0, 1 / 16, RH, RW))
    print("at 60 %:", g60.tolist())
    assert max(abs(int(a) - int(c)) for a, c in zip(g60, g)) > 8


def test_the_gain_beside_the_adaptive_plate():
    """no noise, exact integer ratios: after the step the plate absorbs the new exposure at `rate` and the gain walks back to 128"""
    plate = (room() // 4 * 4).astype(np.uint8)    # multiples of 4: 5 / 4 and 3 / 4 of them are integers
    p = plate.astype(np.int64)
    lit = np.stack([p[0] * 5 // 4, p[1], p[2] * 3 // 4])
    assert lit.max() <= 251 and np.array_equal(4 * lit[0], 5 * p[0]) and np.array_equal(4 * lit[2], 3 * p[2])
    before, after = frame_of(plate), frame_of(lit.astype(np.uint8))
    state = MK.state_of(plate)
    lim, min_count = MK.gain_params(2.0, 1 / 16, RH, RW)
    dist = []
    for k in range(44):
        src = before if k < 3 else after
        b = source_bytes(src)
        g, _ = MK.measure_gain(b, MK.plate_bytes(state), lim, min_count)
        P, state = MK.key_adapt_ref(src, state, **KEY, rate=1 / 8, absorb=0.0, gain=g)
        assert P.max() == 0, k                    # the wall stays 0 throughout
        dist.append(int(np.abs(g - UNITY).max()))
        if k < 3:
            assert g.tolist() == [UNITY] * 3
        if k == 3:
            assert g.tolist() == [160, 128, 96]
        if k > 3:
            assert dist[-1] <= dist[-2] + 1, (k, dist)       # never grows by more than one bin
    print("|g - 128| per frame:", dist)
    assert dist[3] == 32 and dist[43] < dist[4] and dist[43] <= 2


# ----------------------------------------------------------------------------- settings
def test_settings_by_keyword():
    assert MK.check_gain() == MK.GAIN_DEFAULTS == dict(limit=2.0, min_share=1 / 16)
    assert MK.check_gain(1, 0) == dict(limit=1.0, min_share=0.0) and MK.check_gain(3.99, 1.0) == dict(limit=3.99, min_share=1.0)
    for kw, name in ((dict(limit=0.99), "limit="), (dict(limit=4.0), "limit="), (dict(limit="2"), "limit="), (dict(limit=True), "limit="),
                     (dict(limit=float("nan")), "limit="), (dict(min_share=-0.1), "min_share="), (dict(min_share=1.01), "min_share="),
                     (dict(min_share=None), "min_share=")):
        with pytest.raises(ValueError, match=name):
            MK.check_gain(**kw)


# ----------------------------------------------------------------------------- the builders and launchers (dry run)
def test_launcher_checks(dry_run):  # noqa: F811
    from live2diff_amd import _lib, ops
    assert _lib.OP_MATTE_KEY_GAIN_HIST == 62 and _lib.OP_MATTE_KEY_GAIN == 63 and _lib.ABI_VERSION == 6
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_MATTE_KEY_GAIN_HIST = 62," in hdr and "L2D_OP_MATTE_KEY_GAIN = 63," in hdr
    assert all(f"#define L2D_MATTE_KEY_{n} {v} " in hdr for n, v in (
        ("GAIN", ops.MATTE_KEY_GAIN), ("GAIN_STATE", ops.MATTE_KEY_GAIN_STATE), ("GAIN_UNITY", ops.MATTE_KEY_GAIN_UNITY),
        ("GAIN_BINS", ops.MATTE_KEY_GAIN_BINS), ("GAIN_BLOCK", ops.MATTE_KEY_GAIN_BLOCK)))
    assert ops.MATTE_KEY_GAIN == 512 and ops.matte_key_gain_blocks(512, 512) == 64 and ops.matte_key_gain_blocks(1, 8) == 1
    assert ops.matte_key_gain_blocks(72, 136) == 3 and ops.matte_key_gain_blocks(64, 64) == 1 and ops.matte_key_gain_blocks(64, 72) == 2
    nblk = ops.matte_key_gain_blocks(H, W)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    src, plate = torch.zeros(3, H, W, dtype=torch.float16), torch.zeros(3, H, W, dtype=torch.uint8)
    state = torch.zeros(3, H, W, dtype=torch.uint16)
    part, rec = torch.zeros(nblk, 3, 512, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    raw = torch.zeros(6 * H * W + 64, dtype=torch.uint8)

    # op 62
    op, keep = ops.matte_key_gain_hist(src, plate, part, H=H, W=W)
    assert op.kind == 62 and [op.p[j] for j in range(3)] == [t.data_ptr() for t in keep] and op.p[3] is None
    assert [op.i[j] for j in range(4)] == [H, W, 0, nblk]
    ops.run((op, keep))
    op, keep = ops.matte_key_gain_hist(src, state, part.view(torch.uint32), H=H, W=W)
    assert op.i[2] == ops.MATTE_KEY_GAIN_STATE and op.p[1] == state.data_ptr()
    ops.run((op, keep))
    ops.run(ops.matte_key_gain_hist(src, state.view(torch.int16), part, H=H, W=W))
    for call_ in (lambda: ops.matte_key_gain_hist(src.float(), plate, part, H=H, W=W),
                  lambda: ops.matte_key_gain_hist(src, plate.float(), part, H=H, W=W),
                  lambda: ops.matte_key_gain_hist(src, plate[:, :, :W - 8], part, H=H, W=W),
                  lambda: ops.matte_key_gain_hist(src, None, part, H=H, W=W),
                  lambda: ops.matte_key_gain_hist(src, plate, part[:1], H=H, W=W) if nblk > 1 else ops.matte_key_gain_hist(src, plate, None, H=H, W=W),
                  lambda: ops.matte_key_gain_hist(src, plate, part.float(), H=H, W=W),
                  lambda: ops.matte_key_gain_hist(src, plate, torch.zeros(nblk + 1, 3, 512, dtype=torch.int32), H=H, W=W),
                  lambda: ops.matte_key_gain_hist(src[:, :, :W - 4].contiguous(), plate[:, :, :W - 4].contiguous(), part, H=H, W=W - 4),
                  lambda: ops.matte_key_gain_hist(src, raw[4:4 + 3 * H * W].view(3, H, W), part, H=H, W=W),                      # misaligned
                  lambda: ops.matte_key_gain_hist(src, raw[8:8 + 6 * H * W].view(torch.uint16).view(3, H, W), part, H=H, W=W),  # 8, not 16
                  lambda: ops.matte_key_gain_hist(src, raw[:3 * H * W].view(3, H, W), raw[:nblk * 6144].view(torch.int32).view(nblk, 3, 512),
                                                  H=H, W=W)):
        with pytest.raises(ValueError, match="matte_key_gain_hist"):
            call_()
    for k, v, match in ((2, 2, "unknown flag bits"), (0, 0, "non-positive size"), (1, W - 4, "multiple of 8"), (3, nblk + 1, "nblk"),
                        (3, 0, "nblk"), (0, H + 64, "nblk")):
        op, keep = ops.matte_key_gain_hist(src, plate, part, H=H, W=W)
        op.i[k] = v
        bad(match, (op, keep))
    for k in range(3):
        op, keep = ops.matte_key_gain_hist(src, plate, part, H=H, W=W)
        op.p[k] = None
        bad("null or misaligned", (op, keep))
    for k, off in ((0, 8), (1, 4), (2, 8)):
        op, keep = ops.matte_key_gain_hist(src, plate, part, H=H, W=W)
        op.p[k] += off
        bad("null or misaligned", (op, keep))
    op, keep = ops.matte_key_gain_hist(src, state, part, H=H, W=W)
    op.p[1] += 8                                  # fine for a plate, not for a state
    bad("null or misaligned", (op, keep))
    for k in (0, 1):
        op, keep = ops.matte_key_gain_hist(src, plate, part, H=H, W=W)
        op.p[2] = op.p[k]
        bad("overlap", (op, keep))

    # op 63
    op, keep = ops.matte_key_gain(part, rec, H=H, W=W, lim=256, min_count=180)
    assert op.kind == 63 and [op.p[j] for j in range(2)] == [part.data_ptr(), rec.data_ptr()] and op.p[2] is None
    assert [op.i[j] for j in range(5)] == [H, W, nblk, 256, 180]
    ops.run((op, keep))
    for kw in (dict(lim=128, min_count=0), dict(lim=511, min_count=H * W)):
        ops.run(ops.matte_key_gain(part, rec, H=H, W=W, **kw))
    for kw, name in ((dict(lim=127), "lim="), (dict(lim=512), "lim="), (dict(lim=2.0), "lim="), (dict(min_count=-1), "min_count="),
                     (dict(min_count=H * W + 1), "min_count="), (dict(min_count=True), "min_count=")):
        with pytest.raises(ValueError, match=name):
            ops.matte_key_gain(part, rec, H=H, W=W, **dict(dict(lim=256, min_count=1), **kw))
    for call_ in (lambda: ops.matte_key_gain(part, rec.float(), H=H, W=W, lim=256, min_count=1),
                  lambda: ops.matte_key_gain(part, torch.zeros(6, dtype=torch.int32), H=H, W=W, lim=256, min_count=1),
                  lambda: ops.matte_key_gain(part, raw[4:36].view(torch.int32), H=H, W=W, lim=256, min_count=1),
                  lambda: ops.matte_key_gain(part, part.view(-1)[:8], H=H, W=W, lim=256, min_count=1),
                  lambda: ops.matte_key_gain(part, rec, H=H, W=W - 4, lim=256, min_count=1),
                  lambda: ops.matte_key_gain(part, rec, H=H + 64, W=W, lim=256, min_count=1)):
        with pytest.raises(ValueError, match="matte_key_gain"):
            call_()
    for k, v, match in ((3, 127, "lim ="), (3, 512, "lim ="), (4, -1, "min_count"), (4, H * W + 1, "min_count"), (2, nblk + 1, "nblk"),
                        (1, W + 4, "multiple of 8"), (0, -1, "non-positive size")):
        op, keep = ops.matte_key_gain(part, rec, H=H, W=W, lim=256, min_count=1)
        op.i[k] = v
        bad(match, (op, keep))
    for k in (0, 1):
        op, keep = ops.matte_key_gain(part, rec, H=H, W=W, lim=256, min_count=1)
        op.p[k] = None
        bad(f"pointer {k} is null", (op, keep))
        op, keep = ops.matte_key_gain(part, rec, H=H, W=W, lim=256, min_count=1)
        op.p[k] += 8
        bad(f"pointer {k} is not 16-byte aligned", (op, keep))
    op, keep = ops.matte_key_gain(part, rec, H=H, W=W, lim=256, min_count=1)
    op.p[1] = op.p[0] + 16
    bad("overlaps", (op, keep))

    # the flag on ops 59 and 61
    kw = dict(H=H, W=W, r=1, L=64, lo2=1600.0, inv=float(np.float32(1 / 6500)), hard=False)
    out, depth = torch.zeros(H, W), torch.zeros(H, W, dtype=torch.float16)
    st2 = torch.zeros(3, H, W, dtype=torch.uint16)
    plain, _ = ops.matte_key(src, out, None, plate, **kw)
    op, keep = ops.matte_key(src, out, None, plate, gain=rec, **kw)
    assert op.kind == 59 and op.i[3] == plain.i[3] | ops.MATTE_KEY_GAIN and op.p[6] == rec.data_ptr() and keep[-1] is rec
    assert plain.p[6] is None and not plain.i[3] & ops.MATTE_KEY_GAIN
    assert [op.p[j] for j in range(6)] == [plain.p[j] for j in range(6)] and [op.f[j] for j in range(4)] == [plain.f[j] for j in range(4)]
    ops.run((op, keep))
    for init in (True, False):
        a = (src, out, depth, plate if init else None, None if init else state, st2)
        plain, _ = ops.matte_key_adapt(*a, a_bg=2048, a_fg=0, combine="and", lo32=-0.2, inv32=2.0, **kw)
        op, keep = ops.matte_key_adapt(*a, a_bg=2048, a_fg=0, combine="and", lo32=-0.2, inv32=2.0, gain=rec, **kw)
        assert op.kind == 61 and op.i[3] == plain.i[3] | ops.MATTE_KEY_GAIN and op.p[6] == rec.data_ptr() and plain.p[6] is None
        assert [op.p[j] for j in range(6)] == [plain.p[j] for j in range(6)] and [op.i[j] for j in (5, 6, 7)] == [2048, 0, 0]
        ops.run((op, keep))
    with pytest.raises(ValueError, match="colour"):
        ops.matte_key(src, out, None, GREEN, gain=rec, **kw)
    inside = raw[:4 * H * W].view(torch.float32).view(H, W)
    for g in (rec.float(), torch.zeros(6, dtype=torch.int32), raw[4:36].view(torch.int32), raw[:32].view(torch.int32), "record"):
        with pytest.raises(ValueError, match="gain"):
            ops.matte_key(src, inside, None, plate, gain=g, **kw)
        with pytest.raises(ValueError, match="gain"):
            ops.matte_key_adapt(src, inside, None, None, state, st2, a_bg=0, a_fg=0, gain=g, **kw)
    with pytest.raises(ValueError, match="gain"):
        ops.matte_key_adapt(src, out, None, None, state, raw[:6 * H * W].view(torch.uint16).view(3, H, W), a_bg=0, a_fg=0,
                            gain=raw[:32].view(torch.int32), **kw)
    # ... and the launchers
    op, keep = ops.matte_key(src, out, None, GREEN, **kw)
    op.i[3] |= ops.MATTE_KEY_GAIN
    op.p[6] = rec.data_ptr()
    bad("colour key", (op, keep + (rec,)))
    for build_ in (lambda: ops.matte_key(src, out, None, plate, gain=rec, **kw),
                   lambda: ops.matte_key_adapt(src, out, None, None, state, st2, a_bg=0, a_fg=0, gain=rec, **kw),
                   lambda: ops.matte_key_adapt(src, out, None, plate, None, st2, a_bg=0, a_fg=0, gain=rec, **kw)):
        op, keep = build_()
        op.p[6] = None
        bad("pointer 6", (op, keep))
        op, keep = build_()
        op.p[6] += 8
        bad("pointer 6", (op, keep))
        op, keep = build_()
        op.p[6] = op.p[1] + 16
        bad("overlaps the gain record", (op, keep))
        op, keep = build_()
        op.i[3] |= 1024
        bad("unknown flag bits", (op, keep))
    op, keep = ops.matte_key_adapt(src, out, None, None, state, st2, a_bg=0, a_fg=0, gain=rec, **kw)
    op.p[6] = op.p[5] + 32
    bad("overlaps the gain record", (op, keep))


def test_hip_matte_key_lists_in_a_dry_run(dry_run):  # noqa: F811
    from live2diff_amd import ops
    mk = MK.HipMatteKey(H, W, device="cpu")
    slot = MT._Slot(H, W, "cpu")
    matte = dict(lo=0.3, hi=0.7, keep="near")
    s = dict(MK.PLATE_DEFAULTS, to="plate")
    ad, gn = dict(rate=1 / 32, absorb=0.0), dict(limit=2.0, min_share=1 / 16)
    with pytest.raises(ValueError, match="no plate is set"):
        mk.record(slot, matte, s, gain=gn)
    with pytest.raises(ValueError, match="needs a plate"):
        mk.record(slot, matte, dict(s, to=GREEN), gain=gn)
    with pytest.raises(ValueError, match="no gain has been measured"):
        mk.current_gain()
    # with the setting off the lists are the parent's
    assert [r.kind for r in mk.record(slot, matte, s, capture=True)[0]] == [60, 59]
    assert mk.partials is None and mk.gain_record is None
    (r59,), keep59, _ = mk.record(slot, matte, s)
    assert r59.kind == 59 and r59.i[3] == ops.MATTE_KEY_PLATE and r59.p[6] is None and len(keep59) == 4
    (r61,), keep61, _ = mk.record(slot, matte, s, adapt=ad)
    assert r61.kind == 61 and not r61.i[3] & ops.MATTE_KEY_GAIN and r61.p[6] is None and len(keep61) == 6
    mk.restart()
    # 62 -> 63 -> 59
    records, keep, plane = mk.record(slot, matte, dict(s, combine="and"), gain=gn)
    assert [r.kind for r in records] == [62, 63, 59] and plane is mk.plane
    h, m, k = records
    nblk = ops.matte_key_gain_blocks(H, W)
    assert tuple(mk.partials.shape) == (nblk, 3, 512) and mk.gain_record.dtype == torch.int32 and mk.gain_record.numel() == 8
    assert h.p[0] == slot.source.data_ptr() and h.p[1] == mk.plate.data_ptr() and h.p[2] == mk.partials.data_ptr()
    assert [h.i[j] for j in range(4)] == [H, W, 0, nblk]
    assert m.p[0] == mk.partials.data_ptr() and m.p[1] == mk.gain_record.data_ptr()
    assert [m.i[j] for j in range(5)] == [H, W, nblk, 256, int(np.ceil(H * W / 16))]
    assert k.i[3] == ops.MATTE_KEY_PLATE | ops.MATTE_KEY_AND | ops.MATTE_KEY_GAIN and k.p[6] == mk.gain_record.data_ptr() and k.p[3] == mk.plate.data_ptr()
    assert any(t is mk.partials for t in keep) and any(t is mk.gain_record for t in keep)
    # 60 -> 62 -> 63 -> 61 (INIT: against the plate just captured), then 62 -> 63 -> 61 against the state read
    records, _, _ = mk.record(slot, matte, s, capture=True, adapt=ad, gain=dict(limit=3.0, min_share=0.5))
    assert [r.kind for r in records] == [60, 62, 63, 61]
    c, h, m, k = records
    assert c.p[1] == h.p[1] == k.p[3] == mk.plate.data_ptr() and h.i[2] == 0 and [m.i[3], m.i[4]] == [384, H * W // 2]
    assert k.i[3] == ops.MATTE_KEY_ADAPT_INIT | ops.MATTE_KEY_GAIN and k.p[6] == mk.gain_record.data_ptr() and k.p[4] is None
    was = mk.cur
    records, _, _ = mk.record(slot, matte, s, adapt=ad, gain=gn)
    assert [r.kind for r in records] == [62, 63, 61]
    h, m, k = records
    assert h.i[2] == ops.MATTE_KEY_GAIN_STATE and h.p[1] == k.p[4] == mk.states[was].data_ptr() and k.p[5] == mk.states[1 - was].data_ptr()
    assert k.i[3] == ops.MATTE_KEY_GAIN and (k.i[5], k.i[6]) == (2048, 0)
    records, _, _ = mk.record(slot, matte, s, adapt=ad, gain=gn, repeated=True)     # a repeated frame measures again, and moves nothing
    assert [r.kind for r in records] == [62, 63, 61] and (records[2].i[5], records[2].i[6]) == (0, 0)
    assert mk.key(slot.source, slot.depth, matte, s, gain=gn) is mk.plane
    g, n = mk.current_gain()
    assert g.shape == (3,) and n.shape == (3,)
    # the caller's buffers
    part, rec = torch.zeros(nblk, 3, 512, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    mine = MK.HipMatteKey(H, W, device="cpu", partials=part, gain_record=rec)
    mine.set_plate(np.zeros((3, H, W), np.uint8))
    records, _, _ = mine.record(slot, matte, s, gain=gn)
    assert records[0].p[2] == part.data_ptr() and records[1].p[1] == records[2].p[6] == rec.data_ptr()


# ----------------------------------------------------------------------------- the wrapper on the mock components (host route)
class ByHand:
    """the oracles chained by hand beside a wrapper: measure, then key, on the slot the last output was composited with"""

    def __init__(self, plate=None):
        self.plate, self.state, self.last = plate, None, None

    def step(self, w, repeated=False):
        slot, mt = w._matte_line.last, w.matte
        b = source_bytes(slot.source)
        if self.plate is None:
            self.plate = b                        # the capturing frame
        s = w.matte_key_gain
        hh, ww = b.shape[1:]
        if w.matte_key_adapt is None:
            self.last = MK.measure_gain(b, self.plate, *MK.gain_params(s["limit"], s["min_share"], hh, ww))
            raw = MK.raw_ref(slot.source, self.plate, slot.depth[None], mt, w.matte_key, gain=self.last[0])
        else:
            if self.state is None:
                self.state = MK.state_of(self.plate)
            self.last = MK.measure_gain(b, MK.plate_bytes(self.state), *MK.gain_params(s["limit"], s["min_share"], hh, ww))
            ad = dict(rate=0.0, absorb=0.0) if repeated else w.matte_key_adapt
            raw, self.state = MK.raw_adapt_ref(slot.source, self.state, slot.depth[None], mt, w.matte_key, ad, gain=self.last[0])
        return MT.composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **mt, plane=raw[None])[0]

    def measured(self, hw):
        g, n = self.last
        return tuple(float(v) / 128.0 for v in g), tuple(float(v) / hw for v in n)


def stepping(frames, at=3, gains=(1.25, 1.0, 0.8)):
    """the screen frames under a white-balance step: from frame `at` on every channel is multiplied by its gain"""
    g = torch.tensor(gains)[:, None, None]
    return [(f * g).clamp(0, 1) if k >= at else f for k, f in enumerate(frames)]


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("adapt", [False, True])
def test_wrapper_capture_with_a_gain(monkeypatch, n, adapt):
    frames = stepping(screen_frames(7))
    w, twin = made(monkeypatch, n), made(monkeypatch, n)
    for x in (w, twin):
        for _ in range(n - 1):                    # (so that the next output shows frame 0, not a warm-up frame of noise)
            call(x, frames[0])
        x.set_matte_key("capture", lo=20, hi=60, radius=2)
        if adapt:
            x.set_matte_key_adapt(rate=0.25)
    w.set_matte_key_gain(limit=1.5, min_share=1 / 8)
    assert w.matte_key_gain == dict(limit=1.5, min_share=1 / 8) and twin.matte_key_gain is None
    with pytest.raises(ValueError, match="no frame has been keyed"):
        w.matte_key_gain_measured()
    with pytest.raises(ValueError, match="no plate gain is set"):
        twin.matte_key_gain_measured()
    hand, differs, stepped_ = ByHand(), False, False
    for k in range(1, 7):
        got, plain = call(w, frames[k]), call(twin, frames[k])
        assert np.array_equal(got, hand.step(w)), k
        hw = w.height * w.width
        assert w.matte_key_gain_measured() == hand.measured(hw), k
        if k == 1:                                # the capturing frame is keyed against itself: unity by construction
            assert np.array_equal(got, plain) and hand.last[0].tolist() == [128] * 3
        differs |= not np.array_equal(got, plain)
        stepped_ |= hand.last[0].tolist() != [128] * 3
    assert differs and stepped_
    # clearing it gives the key's own frames again
    w.clear_matte_key_gain()
    assert w.matte_key_gain is None and w.matte_key is not None
    if not adapt:
        assert np.array_equal(call(w, frames[6]), call(twin, frames[6]))


def test_exclusions_and_clearing(monkeypatch):
    w = made(monkeypatch, 2)
    assert w.matte_key_gain is None
    with pytest.raises(ValueError, match="needs a matte key"):
        w.set_matte_key_gain()
    w.set_matte_key(GREEN)
    with pytest.raises(ValueError, match="colour"):
        w.set_matte_key_gain()
    w.set_matte_key("capture")
    for kw, name in ((dict(limit=0.5), "limit="), (dict(limit=4), "limit="), (dict(min_share=2), "min_share="), (dict(min_share="x"), "min_share=")):
        with pytest.raises(ValueError, match=name):
            w.set_matte_key_gain(**kw)
    assert w.matte_key_gain is None
    w._hold_init = False
    w.set_matte_key_gain(limit=3)
    assert w._hold_init is True and w.matte_key_gain == dict(limit=3.0, min_share=1 / 16)        # any change of it restarts a hold
    with pytest.raises(ValueError, match="(?s)colour.*clear_matte_key_gain"):
        w.set_matte_key(GREEN)                   # a colour while the gain is set
    assert w.matte_key["to"] == "capture" and w.matte_key_gain == dict(limit=3.0, min_share=1 / 16)  # (a refused call changes nothing)
    w.set_matte_key_adapt()                      # with the adaptive plate, in either order
    assert w.matte_key_adapt == MK.ADAPT_DEFAULTS and w.matte_key_gain is not None
    w._hold_init = False
    w.clear_matte_key_gain()
    assert w.matte_key_gain is None and w._hold_init is True and w.matte_key is not None and w.matte_key_adapt is not None
    w.set_matte_key_gain()
    assert w.matte_key_gain == MK.GAIN_DEFAULTS
    w.clear_matte_key_adapt()
    assert w.matte_key_gain == MK.GAIN_DEFAULTS
    w.clear_matte_key()
    assert w.matte_key_gain is None and w.matte_key is None
    w.set_matte_key("capture")
    w.set_matte_key_gain()
    w.clear_matte()
    assert w.matte_key_gain is None and w.matte_key is None


def test_constructor_keyword(monkeypatch):
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    assert inspect.signature(Wrapper.__init__).parameters["matte_key_gain"].default is None
    p = inspect.signature(Wrapper.set_matte_key_gain).parameters
    assert (p["limit"].default, p["min_share"].default) == (2.0, 1 / 16)
    real = Wrapper.from_components

    def with_gain(key, value, **more):
        monkeypatch.setattr(Wrapper, "from_components",
                            classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, matte_key=key, matte_key_gain=value, **more, **kw)))

    with_gain(dict(to="capture"), "auto")
    with pytest.raises(ValueError, match="matte_key_gain="):
        build(monkeypatch, 2)
    with_gain(dict(to="capture"), dict(limit=9))
    with pytest.raises(ValueError, match="limit="):
        build(monkeypatch, 2)
    with_gain(None, dict())
    with pytest.raises(ValueError, match="needs a matte key"):
        build(monkeypatch, 2)
    with_gain(dict(to=GREEN), dict())
    with pytest.raises(ValueError, match="colour"):
        build(monkeypatch, 2)
    with_gain(dict(to="capture"), dict(min_share=1 / 4))
    w = build(monkeypatch, 2)
    assert w.matte_key_gain == dict(limit=2.0, min_share=1 / 4) and w.matte_key["to"] == "capture" and w.matte_key_adapt is None
    with_gain(dict(to="capture"), dict(), matte_key_adapt=dict(rate=1 / 8))
    w = build(monkeypatch, 2)
    assert w.matte_key_gain == MK.GAIN_DEFAULTS and w.matte_key_adapt == dict(rate=1 / 8, absorb=0.0)
    with_gain(dict(to="capture"), None)
    assert build(monkeypatch, 2).matte_key_gain is None
