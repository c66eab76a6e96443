"""CPU tests (-m "not gpu") of the adaptive plate (live2diff_amd/matte_key.py): the numpy oracle of
L2D_OP_MATTE_KEY_ADAPT -- its identities with `key_ref`, updates planted and worked out by hand, a drifting room --, the settings,
the builder and the launcher of op 61 (dry-run), `HipMatteKey`'s lists, and `set_matte_key_adapt` on the wrapper's host route."""
import inspect
import os

import numpy as np
import pytest
import torch

from live2diff_amd import matte as MT
from live2diff_amd import matte_key as MK
from live2diff_amd.backdrop import frame_of
from live2diff_amd.steady import source_bytes
from test_matte_cpu import build, src_bytes
from test_matte_key_cpu import GREEN, H, W, call, dry_run, frame16, made, screen_frames  # noqa: F401  (dry_run: the fixture)

KEY = dict(lo=40.0, hi=90.0, luma=0.25, radius=1)


# ----------------------------------------------------------------------------- identities
def test_zero_rates_leave_the_state_and_give_key_ref_on_every_frame():
    rng = np.random.default_rng(3)
    plate = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    state = MK.state_of(plate)
    assert state.dtype == np.uint16 and np.array_equal(state, plate.astype(np.uint16) * 256)
    assert np.array_equal(MK.plate_bytes(state), plate)                      # (256 k + 128) >> 8 == k
    assert np.array_equal(MK.plate_bytes(np.array([[[127, 128, 383, 384, 65280]]] * 3, np.uint16))[0, 0], [0, 1, 1, 2, 255])
    for k in range(3):
        src = frame16(10 + k)
        for invert in (False, True):
            P, nxt = MK.key_adapt_ref(src, state, **KEY, invert=invert, rate=0.0, absorb=0.0)
            assert np.array_equal(nxt, state) and nxt.dtype == np.uint16
            assert np.array_equal(P, MK.key_ref(src, plate, **KEY, invert=invert))
    # the INIT frame equals key_ref against the plate's bytes whatever the rates, and the state then moves
    near = frame_of(np.clip(plate.astype(int) + rng.integers(-20, 21, plate.shape), 0, 255).astype(np.uint8))
    P, nxt = MK.key_adapt_ref(near, MK.state_of(plate), **KEY, rate=0.5, absorb=0.25)
    assert np.array_equal(P, MK.key_ref(near, plate, **KEY)) and not np.array_equal(nxt, state)
    # a moved state keys as its bytes do
    P2, _ = MK.key_adapt_ref(frame16(20), nxt, **KEY)
    assert np.array_equal(P2, MK.key_ref(frame16(20), MK.plate_bytes(nxt), **KEY))
    # raw_adapt_ref adds front_ref as raw_ref does
    from test_matte_key_cpu import depth16
    matte, depth = dict(lo=0.3, hi=0.7, keep="far"), depth16(4)
    ks = dict(KEY, combine="and", invert=True, to="plate")
    raw, n3 = MK.raw_adapt_ref(frame16(20), nxt, depth, matte, ks, dict(rate=1 / 32, absorb=0.0))
    assert np.array_equal(raw, MK.raw_ref(frame16(20), MK.plate_bytes(nxt), depth, matte, ks))
    assert np.array_equal(n3, MK.key_adapt_ref(frame16(20), nxt, **KEY, invert=True)[1])     # the gate is P in front of `invert`


# ----------------------------------------------------------------------------- planted updates, worked out by hand
# One pixel, the same in all three channels and in all 8 pixels of a 1 x 8 frame, under luma = 1 and radius 0: dR = dG = dB = d = b
# - k gives dy = d, cb = cr = 0 and D = d^2, so `lo` and `hi` are levels of d itself.  s: the state word, b: the source's byte, and
# by hand: k = (s + 128) >> 8, P0, a = (a_bg (255 - P0) + a_fg P0 + 127) // 255, e = 256 b - s, s' = s + ((a e + 32768) >> 16).
HARD = dict(lo=5.0, hi=5.0)
SOFT = dict(lo=0.0, hi=70.6)           # d = 50: t = 2500 / 70.6^2 = 0.5016, m = t t (3 - 2 t) = 0.5024, P0 = rint(128.1) = 128
PLANTED = [
    # a = 32768: (a e + 32768) >> 16 = floor((e + 1) / 2)
    dict(name="e = -2: -32768 >> 16 is -1, towards minus infinity (a division would give 0)", s=258, b=1, rate=0.5, absorb=0.0, **HARD, P0=0, want=257),
    dict(name="e = -3: a e + 32768 = -65536 exactly", s=259, b=1, rate=0.5, absorb=0.0, **HARD, P0=0, want=258),
    dict(name="s = 0, b = 255: 32768 * 65281 >> 16 = 32640", s=0, b=255, rate=0.5, absorb=0.5, **HARD, P0=255, want=32640),
    dict(name="s = 65280, b = 0: 32768 * -65279 >> 16 = -32640", s=65280, b=0, rate=0.5, absorb=0.5, **HARD, P0=255, want=32640),
    # a_bg = 2048
    dict(name="P0 = 0: a = 2048, e = -100, (-204800 + 32768) >> 16 = -3", s=25700, b=100, rate=1 / 32, absorb=0.0, **HARD, P0=0, want=25697),
    dict(name="P0 = 0, absorb = rate: the same", s=25700, b=100, rate=1 / 32, absorb=1 / 32, **HARD, P0=0, want=25697),
    dict(name="P0 = 128: a = (2048 * 127 + 127) // 255 = 1020, e = 12800, 13088768 >> 16 = 199", s=25600, b=150, rate=1 / 32, absorb=0.0, **SOFT,
         P0=128, want=25799),
    dict(name="P0 = 128, absorb = rate: a = 2048, 26247168 >> 16 = 400", s=25600, b=150, rate=1 / 32, absorb=1 / 32, **SOFT, P0=128, want=26000),
    dict(name="P0 = 255: a = 0, nothing moves", s=5120, b=220, rate=1 / 32, absorb=0.0, **HARD, P0=255, want=5120),
    dict(name="P0 = 255, absorb = rate: e = 51200, (104857600 + 32768) >> 16 = 1600", s=5120, b=220, rate=1 / 32, absorb=1 / 32, **HARD, P0=255,
         want=6720),
    # a = 64: |e| < 32768 / 64 = 512 moves nothing
    dict(name="e = 511: 65472 >> 16 = 0", s=25089, b=100, rate=1 / 1024, absorb=0.0, **HARD, P0=0, want=25089),
    dict(name="e = 512: 65536 >> 16 = 1", s=25088, b=100, rate=1 / 1024, absorb=0.0, **HARD, P0=0, want=25089),
    dict(name="e = -512: 0 >> 16 = 0", s=26112, b=100, rate=1 / 1024, absorb=0.0, **HARD, P0=0, want=26112),
    dict(name="e = -513: -64 >> 16 = -1", s=26113, b=100, rate=1 / 1024, absorb=0.0, **HARD, P0=0, want=26112),
]


def planted_frame(case):
    """(source fp16 [3,1,8], state uint16 [3,1,8], the key's keywords) of one planted case"""
    src = frame_of(np.full((3, 1, 8), case["b"], np.uint8))
    return src, np.full((3, 1, 8), case["s"], np.uint16), dict(lo=case["lo"], hi=case["hi"], luma=1.0, radius=0)


@pytest.mark.parametrize("case", PLANTED, ids=[c["name"].split(":")[0] for c in PLANTED])
def test_planted_updates(case):
    src, state, kw = planted_frame(case)
    for invert in (False, True):                 # the gate is taken in front of `invert`
        P, nxt = MK.key_adapt_ref(src, state, **kw, invert=invert, rate=case["rate"], absorb=case["absorb"])
        assert np.all(P == (255 - case["P0"] if invert else case["P0"])), (case["name"], P)
        assert np.all(nxt == case["want"]), (case["name"], nxt)


def test_rates_and_bounds_at_the_extremes():
    assert MK.adapt_params(0.0, 0.0) == (0, 0) and MK.adapt_params(0.5, 0.5) == (32768, 32768)
    assert MK.adapt_params(1 / 32, 0.0) == (2048, 0) and MK.adapt_params(1 / 256, 1 / 1024) == (256, 64)
    assert MK.adapt_params(1e-5) == (1, 0)       # rint(0.65536)
    assert MK.MAX_STATE == 65280 and 32768 * MK.MAX_STATE + 32768 == 2139127808 < 2 ** 31
    # every corner of (s, b, P0) at the largest rates: the oracle's own assertions hold, and the state stays in range
    s = np.array([0, 65280, 0, 65280], np.uint16).reshape(1, 1, 4).repeat(3, 0)
    b = np.array([255, 0, 0, 255], np.uint8).reshape(1, 1, 4).repeat(3, 0)
    for P0 in (0, 128, 255):
        n = MK.adapt_ref(s, b, np.full((1, 4), P0, np.uint8), 32768, 32768)
        assert np.array_equal(n[0, 0], [32640, 32640, 0, 65280])
    with pytest.raises(ValueError, match="a_bg"):
        MK.adapt_ref(s, b, np.zeros((1, 4), np.uint8), 32769, 0)
    with pytest.raises(ValueError, match="a_fg"):
        MK.adapt_ref(s, b, np.zeros((1, 4), np.uint8), 0, -1)
    with pytest.raises(ValueError, match="state"):
        MK.adapt_ref(s.astype(np.uint8), b, np.zeros((1, 4), np.uint8), 0, 0)
    with pytest.raises(ValueError, match="state"):
        MK.plate_bytes(np.full((3, 1, 8), 65281, np.uint16))


# ----------------------------------------------------------------------------- the point of the feature
ROOM_FRAMES = 40
BOX = np.array([200, 30, 220], np.uint8)          # nothing like the wall


def room(t, box=True, noise=2):
    """planar uint8 [3,40,72] bytes of the room at frame t, and the box's column or None.  A gradient with noise of +-2 levels
    of the frame's own under a lamp that warms up: red rises by one byte level per frame, green by half, blue falls by three
    quarters.  (A neutral brightening cannot serve: under the plate's default luma of 0.25 its D is dy^2 / 4, which passes lo^2 =
    1600 only 80 levels away; a colour cast of 40 levels is far outside: D(40, 20, -30) = 50^2 + 20^2 + 100 = 3000.)  The plate
    lags a drift of one level per frame by 32 (1 - (31 / 32)^t) levels at rate 1 / 32 -- 23 of the 40 --, a few more where the box
    has covered it, and D falls with the square: about 3000 (28 / 40)^2 = 1470, below 1600."""
    rng = np.random.default_rng(5000 + t)
    base = 90 + np.arange(W)[None, None, :] * 0.5 + np.arange(H)[None, :, None] * 0.25 + np.zeros((3, 1, 1))
    b = base + np.array([1.0, 0.5, -0.75])[:, None, None] * t + rng.integers(-noise, noise + 1, (3, H, W))
    b = np.floor(b).astype(np.uint8)
    x = None
    if box and 8 <= t < 36:
        x = 2 * (t - 8)
        b[:, 12:28, x:x + 16] = BOX[:, None, None]
    return b, x


def test_the_plate_follows_a_drifting_room():
    plate = room(0, box=False)[0]
    state = MK.state_of(plate)
    static_bg = None
    for t in range(1, ROOM_FRAMES + 1):
        b, x = room(t)
        src = frame_of(b)
        bg = np.ones((H, W), bool)
        if x is not None:
            bg[10:30, max(0, x - 2):x + 18] = False              # the box and the window's reach around it
        static = MK.key_ref(src, plate, **KEY)
        P, state = MK.key_adapt_ref(src, state, **KEY)           # the defaults: rate 1 / 32, absorb 0
        static_bg = float((static[bg] > 0).mean())
        assert not P[bg].any(), t                                # with adaptation the wall stays wall on every frame
        if x is not None:
            assert (P[13:27, x + 1:x + 15] == 255).all(), t      # and the box stays subject
            assert (static[13:27, x + 1:x + 15] == 255).all(), t
    assert static_bg > 0.9                                       # against the frozen plate the wall has turned into subject
    # the plate under the box's path holds no trace of the box: it is the room of this moment, as far behind as the lag says
    k = MK.plate_bytes(state).astype(int)
    clean = room(ROOM_FRAMES, box=False, noise=0)[0].astype(int)
    assert np.abs(k - clean).max() <= 30 and np.abs(k - clean)[:, 12:28].max() <= 30
    assert np.abs(k - BOX.astype(int)[:, None, None]).max(axis=0).min() >= 60


# ----------------------------------------------------------------------------- settings, op 61 in a dry run, HipMatteKey's lists
def test_check_adapt_names_the_keyword():
    assert MK.check_adapt() == dict(rate=1 / 32, absorb=0.0) == MK.ADAPT_DEFAULTS
    assert MK.check_adapt(0.5, 0) == dict(rate=0.5, absorb=0.0)
    for kw, name in ((dict(rate=0.51), "rate="), (dict(rate=-0.1), "rate="), (dict(rate=True), "rate="), (dict(rate="fast"), "rate="),
                     (dict(rate=float("nan")), "rate="), (dict(absorb=0.6), "absorb="), (dict(absorb=-1), "absorb="), (dict(absorb=None), "absorb=")):
        with pytest.raises(ValueError, match=name):
            MK.check_adapt(**kw)
        with pytest.raises(ValueError, match=name):
            MK.adapt_params(**dict(dict(rate=0.1, absorb=0.0), **kw))


def test_launcher_checks(dry_run):  # noqa: F811
    from live2diff_amd import _lib, ops
    assert _lib.OP_MATTE_KEY_ADAPT == 61
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l2d.h")).read()
    assert "L2D_OP_MATTE_KEY_ADAPT = 61," in hdr
    assert f"#define L2D_MATTE_KEY_ADAPT_INIT {ops.MATTE_KEY_ADAPT_INIT} " in hdr and f"#define L2D_MATTE_KEY_MAX_RATE {ops.MATTE_KEY_MAX_RATE} " in hdr

    def st():
        return torch.zeros(3, H, W, dtype=torch.uint16)

    def adapt(**kw):
        args = dict(source=torch.zeros(3, H, W, dtype=torch.float16), out=torch.zeros(H, W), depth=torch.zeros(H, W, dtype=torch.float16),
                    plate=None, state_in=st(), state_out=st(), H=H, W=W, r=1, L=64, lo2=1600.0, inv=float(np.float32(1 / 6500)), hard=False,
                    a_bg=2048, a_fg=0)
        args.update(kw)
        return ops.matte_key_adapt(*[args.pop(k) for k in ("source", "out", "depth", "plate", "state_in", "state_out")], **args)

    def bad(match, op):
        with pytest.raises(_lib.L2DError, match=match):
            ops.run(op)

    plate = torch.zeros(3, H, W, dtype=torch.uint8)
    # STATE: no plate, the state read in p4
    op, keep = adapt(combine="or", invert=True, lo32=-0.4, inv32=1.25, far=True, r=4, L=256, a_bg=32768, a_fg=64, plate=plate)
    assert op.kind == 61 and [op.p[j] for j in range(6)] == [None if t is None else t.data_ptr() for t in keep] and op.p[3] is None
    assert op.p[4] == keep[4].data_ptr() and op.p[5] == keep[5].data_ptr() and op.p[6] is None
    assert [op.i[j] for j in range(8)] == [H, W, 4, ops.MATTE_KEY_OR | ops.MATTE_KEY_INVERT | ops.MATTE_KEY_RAMP_FAR, 256, 32768, 64, 0]
    assert [op.f[j] for j in range(4)] == [1600.0, float(np.float32(1 / 6500)), float(np.float32(-0.4)), 1.25]
    ops.run((op, keep))
    # INIT: the plate in p3, no state read
    op, keep = adapt(plate=plate, state_in=None)
    assert op.p[2] is None and op.p[3] == plate.data_ptr() and op.p[4] is None and op.i[3] == ops.MATTE_KEY_ADAPT_INIT
    assert (op.i[5], op.i[6]) == (2048, 0)
    ops.run((op, keep))
    for kw in (dict(), dict(r=0), dict(L=0), dict(lo2=0.0, inv=0.0, hard=True), dict(combine="and", lo32=0.0, inv32=0.0, ramp_hard=True),
               dict(invert=True), dict(a_bg=0, a_fg=0), dict(a_bg=32768, a_fg=32768), dict(state_in=st().view(torch.int16)),
               dict(plate=plate, state_in=None, combine="or", lo32=-0.2, inv32=2.0)):
        ops.run(adapt(**kw))
    raw = torch.zeros(6 * H * W + 64, dtype=torch.uint8)
    inside = raw[:6 * H * W].view(torch.uint16).view(3, H, W)
    for call_ in (lambda: adapt(source=torch.zeros(3, H, W)), lambda: adapt(out=torch.zeros(H, W + 1)), lambda: adapt(combine="xor"),
                  lambda: adapt(combine="and", depth=None), lambda: adapt(r=5), lambda: adapt(L=257), lambda: adapt(lo2=-1.0),
                  lambda: adapt(hard=True),                                            # ... everything `matte_key` refuses
                  lambda: adapt(a_bg=32769), lambda: adapt(a_bg=-1), lambda: adapt(a_fg=32769), lambda: adapt(a_fg=0.5), lambda: adapt(a_bg=True),
                  lambda: adapt(state_out=None), lambda: adapt(state_out=torch.zeros(3, H, W, dtype=torch.uint8)),
                  lambda: adapt(state_in=torch.zeros(3, H, W, dtype=torch.float16)), lambda: adapt(state_out=torch.zeros(H, W, 3, dtype=torch.uint16)),
                  lambda: adapt(state_out=raw[8:8 + 6 * H * W].view(torch.uint16).view(3, H, W)),      # misaligned
                  lambda: adapt(state_in=None), lambda: adapt(state_in=None, plate=GREEN),              # INIT without a plate
                  lambda: adapt(plate=torch.zeros(3, H, W), state_in=None),
                  lambda: adapt(state_in=inside, state_out=inside),
                  lambda: adapt(source=raw[:6 * H * W].view(torch.float16).view(3, H, W), state_out=inside),
                  lambda: adapt(out=raw[:4 * H * W].view(torch.float32).view(H, W), state_out=inside),
                  lambda: adapt(out=raw[:4 * H * W].view(torch.float32).view(H, W), state_in=inside),
                  lambda: adapt(combine="and", lo32=-0.2, inv32=2.0, depth=raw[:2 * H * W].view(torch.float16).view(H, W), state_out=inside),
                  lambda: adapt(plate=raw[:3 * H * W].view(3, H, W), state_in=None, state_out=inside)):
        with pytest.raises(ValueError, match="matte_key"):
            call_()
    # the launcher refuses the same of a record built by hand
    for k, v, match in ((3, 32, "unknown flag bits"), (3, 512, "unknown flag bits"), (3, 24, "two ways to combine"), (3, 64, "ramp flags without"),
                        (0, 0, "non-positive size"), (1, W - 4, "multiple of 8"), (2, 5, "radius"), (4, 257, "luma weight"),
                        (3, ops.MATTE_KEY_HARD, "hard flag"), (5, 32769, "rates"), (5, -1, "rates"), (6, 32769, "rates"), (6, -1, "rates"),
                        (3, ops.MATTE_KEY_ADAPT_INIT, "pointer 3")):
        op, keep = adapt()
        op.i[k] = v
        bad(match, (op, keep))
    for k, match in ((0, "pointer 0 is null"), (1, "pointer 1 is null"), (2, "pointer 2"), (4, "pointer 4"), (5, "pointer 5")):
        op, keep = adapt(combine="and", lo32=-0.2, inv32=2.0)
        op.p[k] = None
        bad(match, (op, keep))
    for k in (4, 5):
        op, keep = adapt()
        op.p[k] += 8
        bad(f"pointer {k}", (op, keep))
    op, keep = adapt(plate=plate, state_in=None)
    op.p[3] += 4
    bad("pointer 3", (op, keep))
    for f, v in ((0, -1.0), (1, float("inf")), (1, 0.0)):
        op, keep = adapt()
        op.f[f] = v
        bad("finite and not negative", (op, keep))
    for name, j in (("state read", 4), ("source", 0), ("plane", 1), ("depth", 2), ("plate", 3)):
        op, keep = adapt(combine="and", lo32=-0.2, inv32=2.0, **(dict(plate=plate, state_in=None) if j == 3 else {}))
        op.p[5] = op.p[j]
        bad("overlaps", (op, keep))
    op, keep = adapt()
    op.p[1] = op.p[4]
    bad("overlaps", (op, keep))

    # HipMatteKey in a dry run: the lists, the ping-pong and the rates of a repeated frame
    mk = MK.HipMatteKey(H, W, device="cpu")
    slot = MT._Slot(H, W, "cpu")
    matte = dict(lo=0.3, hi=0.7, keep="near")
    s = dict(MK.PLATE_DEFAULTS, to="plate")
    ad = dict(rate=1 / 32, absorb=1 / 1024)
    with pytest.raises(ValueError, match="no plate is set"):
        mk.record(slot, matte, s, adapt=ad)
    with pytest.raises(ValueError, match="needs a plate"):
        mk.record(slot, matte, dict(s, to=GREEN), adapt=ad)
    records, keep, plane = mk.record(slot, matte, dict(s, combine="and"), capture=True, adapt=ad)
    assert [r.kind for r in records] == [60, 61] and plane is mk.plane
    first = records[1]
    assert records[0].p[1] == first.p[3] == mk.plate.data_ptr() and first.p[4] is None and first.p[5] == mk.states[mk.cur].data_ptr()
    assert first.i[3] == ops.MATTE_KEY_ADAPT_INIT | ops.MATTE_KEY_AND and (first.i[5], first.i[6]) == (2048, 64)
    assert mk.states[0].dtype == torch.uint16 and tuple(mk.states[0].shape) == (3, H, W)
    was = mk.cur
    (second,), _, _ = mk.record(slot, matte, s, adapt=ad)
    assert second.kind == 61 and second.i[3] == 0 and second.p[3] is None
    assert second.p[4] == mk.states[was].data_ptr() and second.p[5] == mk.states[1 - was].data_ptr() and mk.cur == 1 - was
    (third,), _, _ = mk.record(slot, matte, s, adapt=ad, repeated=True)                        # a repeated frame: both rates 0
    assert third.kind == 61 and (third.i[5], third.i[6]) == (0, 0) and third.p[4] == second.p[5] and third.p[5] == second.p[4]
    assert [r.kind for r in mk.record(slot, matte, s)[0]] == [59]                              # without `adapt`: the lists of before
    assert [r.kind for r in mk.record(slot, matte, s, capture=True)[0]] == [60, 59]
    (again,), _, _ = mk.record(slot, matte, s, adapt=ad)                                       # a capture restarts the state
    assert again.i[3] == ops.MATTE_KEY_ADAPT_INIT and again.p[4] is None
    mk.record(slot, matte, s, adapt=ad)
    mk.set_plate(np.zeros((3, H, W), np.uint8))                                                # and so does a new plate
    assert mk.record(slot, matte, s, adapt=ad)[0][0].i[3] == ops.MATTE_KEY_ADAPT_INIT
    mk.restart()
    assert mk.record(slot, matte, s, adapt=ad)[0][0].i[3] == ops.MATTE_KEY_ADAPT_INIT
    assert mk.key(slot.source, slot.depth, matte, s, adapt=ad) is mk.plane


# ----------------------------------------------------------------------------- the wrapper on the mock components (host route)
class ByHand:
    """the oracles chained by hand beside a wrapper: the state of its own, fed the slot the last output was composited with"""

    def __init__(self, plate=None):
        self.state = None if plate is None else MK.state_of(plate)

    def step(self, w, repeated=False):
        slot, mt = w._matte_line.last, w.matte
        if self.state is None:
            self.state = MK.state_of(source_bytes(slot.source))                                # the capturing frame
        ad = dict(rate=0.0, absorb=0.0) if repeated else w.matte_key_adapt
        raw, self.state = MK.raw_adapt_ref(slot.source, self.state, slot.depth[None], mt, w.matte_key, ad)
        m0 = raw if w.matte_edge is None else MT.edge_ref(raw, slot.source, **w.matte_edge)
        return MT.composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], **mt, plane=m0[None])[0]

    def plate(self):
        return np.ascontiguousarray(MK.plate_bytes(self.state).transpose(1, 2, 0))


def drifting(frames, step=0.03):
    """the screen frames under a light that changes: frame k is raised by k `step` in red and lowered in blue"""
    return [(f + torch.tensor([k * step, 0.0, -k * step])[:, None, None]).clamp(0, 1) for k, f in enumerate(frames)]


@pytest.mark.parametrize("n", [2, 3])
def test_wrapper_capture_with_adaptation(monkeypatch, n):
    frames = drifting(screen_frames(7))
    w, twin = made(monkeypatch, n), made(monkeypatch, n)
    for x in (w, twin):
        for _ in range(n - 1):                    # (so that the next output shows frame 0, not a warm-up frame of noise)
            call(x, frames[0])
        x.set_matte_key("capture", lo=20, hi=60, radius=2)
    with pytest.raises(ValueError, match="no plate yet"):
        w.matte_key_plate()
    w.set_matte_key_adapt(rate=0.25, absorb=1 / 64)
    assert w.matte_key_adapt == dict(rate=0.25, absorb=1 / 64) and twin.matte_key_adapt is None
    hand, moved = ByHand(), False
    for k in range(1, 7):
        got, frozen = call(w, frames[k]), call(twin, frames[k])
        if k == 1:                                # the capturing frame is keyed against itself: the plate is its source
            captured = source_bytes(w._matte_line.last.source)
            assert np.array_equal(got, frozen)
        assert np.array_equal(got, hand.step(w)), k
        assert np.array_equal(w.matte_key_plate(), hand.plate()), k
        assert np.array_equal(twin.matte_key_plate(), captured.transpose(1, 2, 0)), k           # without adaptation the plate stays
        moved |= not np.array_equal(got, frozen)
    assert moved and not np.array_equal(hand.plate(), captured.transpose(1, 2, 0))
    assert w._key_state.dtype == np.uint16
    # a change of the rates keeps the plate; a new capture starts it again
    w.set_matte_key_adapt(rate=0.5)
    assert np.array_equal(w.matte_key_plate(), hand.plate())
    w.capture_matte_plate()
    call(w, frames[0])
    hand = ByHand(source_bytes(w._matte_line.last.source))
    hand.step(w)
    assert np.array_equal(w.matte_key_plate(), hand.plate())


def test_wrapper_plate_from_a_file_and_a_dropped_frame(monkeypatch, tmp_path):
    from PIL import Image
    frames = drifting(screen_frames(5))
    room_ = src_bytes(frames[0])
    p = tmp_path / "room.png"
    Image.fromarray(room_).save(p)
    w = made(monkeypatch, 2, drop={2})
    w.stream.inference_time_ema = 0.0            # (a dropped frame waits that long)
    w.set_matte_key(str(p), combine="and", luma=0.5)
    w.set_matte_key_adapt()
    w.set_matte_edge(radius=2, eps=4.0)
    plate = MK.plate_ref(room_, 64, 64, "lanczos")
    assert w.matte_key_adapt == MK.ADAPT_DEFAULTS and np.array_equal(w.matte_key_plate(), plate.transpose(1, 2, 0))
    hand = ByHand(plate)
    for k in range(5):
        before = None if k == 0 else w.matte_key_plate()
        state = None if w._key_state is None else w._key_state.copy()
        got = call(w, frames[k])
        assert np.array_equal(got, hand.step(w, repeated=k == 2)), k
        assert np.array_equal(w.matte_key_plate(), hand.plate()), k
        if k == 2:                               # the dropped frame re-keys `last` and leaves the state alone
            assert np.array_equal(w._key_state, state) and np.array_equal(w.matte_key_plate(), before)
        elif k >= 3:                             # (output 0 shows a warm-up frame, all subject; output 1 the plate's own frame)
            assert not np.array_equal(w._key_state, state), k
    assert w._matte_line.tapped == 4
    w.set_matte_key(str(p))                      # a new image starts the plate again
    assert w._key_state is None and np.array_equal(w.matte_key_plate(), plate.transpose(1, 2, 0)) and w.matte_key_adapt == MK.ADAPT_DEFAULTS


def test_exclusions_and_clearing(monkeypatch):
    w = made(monkeypatch, 2)
    assert w.matte_key_adapt is None
    with pytest.raises(ValueError, match="needs a matte key"):
        w.set_matte_key_adapt()
    with pytest.raises(ValueError, match="no matte key"):
        w.matte_key_plate()
    w.set_matte_key(GREEN)
    with pytest.raises(ValueError, match="colour"):
        w.set_matte_key_adapt()
    with pytest.raises(ValueError, match="no matte key against a plate"):
        w.matte_key_plate()
    w.set_matte_key("capture")
    for kw, name in ((dict(rate=0.6), "rate="), (dict(rate=-1), "rate="), (dict(absorb=0.75), "absorb="), (dict(absorb="x"), "absorb=")):
        with pytest.raises(ValueError, match=name):
            w.set_matte_key_adapt(**kw)
    assert w.matte_key_adapt is None
    w._hold_init = False
    w.set_matte_key_adapt(rate=0.125)
    assert w._hold_init is True and w.matte_key_adapt == dict(rate=0.125, absorb=0.0)           # any change of it restarts a hold
    with pytest.raises(ValueError, match="(?s)colour.*clear_matte_key_adapt"):
        w.set_matte_key(GREEN)                   # a colour while adaptation is set
    assert w.matte_key["to"] == "capture" and w.matte_key_adapt == dict(rate=0.125, absorb=0.0)  # (a refused call changes nothing)
    w._hold_init = False
    w.clear_matte_key_adapt()
    assert w.matte_key_adapt is None and w._hold_init is True and w.matte_key is not None
    w.set_matte_key(GREEN)
    w.set_matte_key("capture")
    w.set_matte_key_adapt()
    w.clear_matte_key()
    assert w.matte_key_adapt is None and w.matte_key is None and w._key_state is None
    w.set_matte_key("capture")
    w.set_matte_key_adapt()
    w.clear_matte()
    assert w.matte_key_adapt is None and w.matte_key is None


def test_constructor_keyword(monkeypatch):
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    assert inspect.signature(Wrapper.__init__).parameters["matte_key_adapt"].default is None
    p = inspect.signature(Wrapper.set_matte_key_adapt).parameters
    assert (p["rate"].default, p["absorb"].default) == (1 / 32, 0.0)
    real = Wrapper.from_components

    def with_adapt(key, value):
        monkeypatch.setattr(Wrapper, "from_components",
                            classmethod(lambda cls, pipe, **kw: real.__func__(cls, pipe, matte_key=key, matte_key_adapt=value, **kw)))

    with_adapt(dict(to="capture"), "slow")
    with pytest.raises(ValueError, match="matte_key_adapt="):
        build(monkeypatch, 2)
    with_adapt(dict(to="capture"), dict(rate=2))
    with pytest.raises(ValueError, match="rate="):
        build(monkeypatch, 2)
    with_adapt(None, dict())
    with pytest.raises(ValueError, match="needs a matte key"):
        build(monkeypatch, 2)
    with_adapt(dict(to=GREEN), dict())
    with pytest.raises(ValueError, match="colour"):
        build(monkeypatch, 2)
    with_adapt(dict(to="capture"), dict(absorb=1 / 256))
    w = build(monkeypatch, 2)
    assert w.matte_key_adapt == dict(rate=1 / 32, absorb=1 / 256) and w.matte_key["to"] == "capture"
    with_adapt(dict(to="capture"), None)
    assert build(monkeypatch, 2).matte_key_adapt is None
