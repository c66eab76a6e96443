"""GPU tests of the adaptive plate (L2D_OP_MATTE_KEY_ADAPT in csrc/matte_key.hip, live2diff_amd/matte_key.py, DESIGN.md section
8.z18): op 61 against `front_ref(key_adapt_ref(...))` on every bit of the plane and every word of the next state, behind guard
bands; the planted updates of the CPU file; a sequence through the ping-pong records; op 59 on the state's bytes; the composites'
whole lists 60 -> 61 -> 43 and 61 -> 54 -> 49 -> 57 -> 47; and the wrapper on synthetic weights, byte for byte what the host route
computes.  There is no tolerance anywhere."""
import numpy as np
import pytest
import torch

from live2diff_amd import backdrop as BD
from live2diff_amd import mask_io as MI
from live2diff_amd import matte as MT
from live2diff_amd import matte_key as MK
from live2diff_amd import ops
from live2diff_amd.steady import source_bytes
from test_gpu_mask import RAMPS, Slot, _setup, dev, differ
from test_gpu_matte_key import SIZES, THRESHOLDS, scene, screen_u8
from test_matte_key_adapt_cpu import PLANTED, planted_frame
from test_matte_key_cpu import frame16

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # floats in front of and behind the plane, 16-bit words around the state: pre-filled and checked
SENTINEL = 0xA5A5                # above 65280: no state word
RATES = [(0.0, 0.0), (1 / 32, 0.0), (0.5, 0.5), (1 / 256, 1 / 1024)]
MATTE = dict(lo=RAMPS["soft"][0], hi=RAMPS["soft"][1], keep="near")


def words(t):
    """a device tensor of 16-bit words (the int16 tensor of their bits) on the host, as uint16"""
    return t.cpu().numpy().view(np.uint16)


def to_words(a):
    return dev(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16))


def state_near(plate, seed):
    """a state whose bytes are the plate's or a neighbour's: 256 k + anything in -200 .. 200, inside 0 .. 65280"""
    rng = np.random.default_rng(seed)
    s = plate.astype(np.int64) * 256 + rng.integers(-200, 201, plate.shape)
    return np.clip(s, 0, MK.MAX_STATE).astype(np.uint16)


def run61(src, plane, depth, plate, s_in, s_out, H, W, ks, rates, matte=MATTE):
    """one launch of op 61; `s_in` None: INIT, from `plate`"""
    lo2, inv, hard = MK.key_params(ks["lo"], ks["hi"])
    kw = {}
    if ks["combine"] != "replace":
        lo32, inv32, ramp_hard = MT.matte_params(matte["lo"], matte["hi"])
        kw = dict(lo32=lo32, inv32=inv32, ramp_hard=ramp_hard, far=matte["keep"] == "far")
    a_bg, a_fg = MK.adapt_params(*rates)
    ops.run(ops.matte_key_adapt(src, plane, depth, plate if s_in is None else None, s_in, s_out, H=H, W=W, r=ks["radius"],
                                L=MK.luma_weight(ks["luma"]), lo2=lo2, inv=inv, hard=hard, a_bg=a_bg, a_fg=a_fg, combine=ks["combine"],
                                invert=ks["invert"], **kw))


class Guarded:
    """the plane NaN-filled between guard floats, the state out between sentinel words"""

    def __init__(self, H, W):
        self.H, self.W, n = H, W, H * W
        self.fbuf = torch.empty(GUARD + n + GUARD, dtype=torch.float32, device=DEV)
        self.plane = self.fbuf[GUARD:GUARD + n].view(H, W)
        self.fill = to_words(np.full(GUARD + 3 * n + GUARD, SENTINEL, np.uint16))
        self.sbuf = torch.empty_like(self.fill)
        self.state = self.sbuf[GUARD:GUARD + 3 * n].view(3, H, W)

    def reset(self):
        self.fbuf.fill_(float("nan"))            # an unwritten pixel shows
        self.sbuf.copy_(self.fill)

    def check(self, tag, want_plane, want_state):
        got, st = self.fbuf.cpu().numpy(), words(self.sbuf)
        bad = differ(tag + " plane", got[GUARD:-GUARD].reshape(self.H, self.W), want_plane)
        bad += differ(tag + " state", st[GUARD:-GUARD].reshape(3, self.H, self.W), want_state)
        assert np.all(np.isnan(got[:GUARD])) and np.all(np.isnan(got[-GUARD:])), tag
        assert np.all(st[:GUARD] == SENTINEL) and np.all(st[-GUARD:] == SENTINEL), tag
        return bad


# ----------------------------------------------------------------------------- op 61 against the oracle
@pytest.mark.parametrize("shape", SIZES)
def test_op61_equals_the_oracle_on_every_bit(shape):
    H, W = shape
    src, plate, depth = scene(shape)
    b = source_bytes(src)
    s_dev, d_dev, p_dev = dev(src), dev(depth), dev(plate)
    state = state_near(plate, H + W)
    st_dev = to_words(state)
    g = Guarded(H, W)
    bad = cases = moved = 0
    for variant in ("init", "state"):
        s0 = MK.state_of(plate) if variant == "init" else state
        for radius in (0, 1, 4):
            for thr, (lo, hi) in THRESHOLDS.items():
                for luma in (0.0, 0.25):
                    P0 = MK.plane_of(MK.distance_ref(b, MK.plate_bytes(s0), luma), lo=lo, hi=hi, radius=radius)
                    for rates in RATES:
                        nxt = MK.adapt_ref(s0, b, P0, *MK.adapt_params(*rates))
                        moved += not np.array_equal(nxt, s0)
                        for invert in (False, True):
                            P = (np.uint8(255) - P0) if invert else P0
                            for combine in ("replace", "and", "or"):
                                ks = dict(lo=lo, hi=hi, luma=luma, radius=radius, combine=combine, invert=invert)
                                g.reset()
                                run61(s_dev, g.plane, d_dev, p_dev, None if variant == "init" else st_dev, g.state, H, W, ks, rates)
                                want = MI.front_ref(P, depth, MATTE["lo"], MATTE["hi"], MATTE["keep"], combine)
                                bad += g.check(f"{shape} {variant} r {radius} {thr} luma {luma} rates {rates} invert {invert} {combine}", want, nxt)
                                cases += 1
    assert np.array_equal(words(st_dev), state) and np.array_equal(p_dev.cpu().numpy(), plate)       # what is read stays as it was
    assert bad == 0 and cases == 2 * 3 * 2 * 2 * 4 * 2 * 3
    assert moved >= 2 * 3 * 2 * 2 * 2            # (every rate but (0, 0) moves something, at least under one of the two variants)


@pytest.mark.parametrize("case", PLANTED, ids=[c["name"].split(":")[0] for c in PLANTED])
def test_op61_planted_updates(case):
    src, state, kw = planted_frame(case)
    g = Guarded(1, 8)
    for invert in (False, True):
        g.reset()
        ks = dict(kw, combine="replace", invert=invert)
        run61(dev(src), g.plane, None, None, to_words(state), g.state, 1, 8, ks, (case["rate"], case["absorb"]))
        P = 255 - case["P0"] if invert else case["P0"]
        want = np.full((1, 8), np.float32(P) / np.float32(255.0), np.float32)
        assert g.check(case["name"], want, np.full((3, 1, 8), case["want"], np.uint16)) == 0


# ----------------------------------------------------------------------------- a sequence through the ping-pong records
def drifting_scene(k, H=37, W=136):
    """the frame k of a sequence: the scene's plate under a light that warms by 3 levels a frame, with noise of the frame's own, and a
    box of anything that moves 9 pixels a frame"""
    _, plate, _ = scene((H, W))
    rng = np.random.default_rng(100 + k)
    b = plate.astype(np.int64) + np.array([3, 1, -2])[:, None, None] * k + rng.integers(-2, 3, plate.shape)
    b = np.clip(b, 0, 255).astype(np.uint8)
    b[:, 8:24, 10 + 9 * k:34 + 9 * k] = rng.integers(0, 256, (3, 16, 24), dtype=np.uint8)
    return BD.frame_of(b)


def test_a_sequence_through_the_ping_pong_records():
    H, W = 37, 136
    _, plate, depth = scene((H, W))
    ks = dict(lo=20.0, hi=60.0, luma=0.25, radius=2, combine="or", invert=False)
    rates = (1 / 8, 1 / 256)
    g = [Guarded(H, W), Guarded(H, W)]
    d_dev, p_dev = dev(depth), dev(plate)
    state, planes = MK.state_of(plate), set()
    for k in range(8):
        src = drifting_scene(k)
        s_dev = dev(src)
        P, nxt = MK.key_adapt_ref(src, state, lo=ks["lo"], hi=ks["hi"], luma=ks["luma"], radius=ks["radius"], rate=rates[0], absorb=rates[1])
        want = MI.front_ref(P, depth, MATTE["lo"], MATTE["hi"], MATTE["keep"], "or")
        out, before = g[k % 2], g[1 - k % 2]
        for again in range(2):                   # the same input: the same plane and the same next state
            out.reset()
            run61(s_dev, out.plane, d_dev, p_dev, None if k == 0 else before.state, out.state, H, W, ks, rates)
            assert out.check(f"frame {k} run {again}", want, nxt) == 0
            if k:
                assert np.array_equal(words(before.state), state), k                             # the record read is not written
        # op 59 on the state's bytes gives op 61's plane
        mk = MK.HipMatteKey(H, W, device=DEV)
        mk.set_plate(MK.plate_bytes(state))
        p59 = mk.key(s_dev, d_dev, MATTE, dict(ks, to="plate")).cpu().numpy()
        assert differ(f"op 59 against op 61, frame {k}", p59, out.plane.cpu().numpy()) == 0
        planes.add(P.tobytes())
        assert k == 0 or not np.array_equal(nxt, state)
        state = nxt
    assert len(planes) == 8 and 0.02 < float((P == 255).mean()) < 0.5 and float((P == 0).mean()) > 0.3


# ----------------------------------------------------------------------------- the composites' whole lists
def test_one_list_60_61_43_and_61_54_49_57_47(monkeypatch):
    """`HipMatte.composite` with a capturing adaptive key, and `HipMatteUp.composite` with an adaptive key, a blurred backdrop, the
    edge refit and the hold in ONE list, against raw_adapt_ref -> edge_ref -> hold_ref -> composite_ref / composite_up_ref by hand"""
    from live2diff_amd import _lib
    from live2diff_amd.resize import CameraBuffer
    H, W, Ho, Wo = 40, 72, 52, 100
    matte = dict(lo=0.3, hi=0.7, keep="far", feather=2, show=False)
    edge, hold = dict(radius=2, eps=4.0), MT.check_hold(search=0)
    bd = BD.check_settings("blur", 2, 2)
    rng = np.random.default_rng(21)
    S8, C8 = (rng.integers(0, 256, (Ho, Wo, 3), dtype=np.uint8) for _ in range(2))
    kinds = {v: k for k, v in vars(_lib).items() if k.startswith("OP_")}
    lists, run = [], _lib.OpList.run
    monkeypatch.setattr(_lib.OpList, "run", lambda self, *a, **k: (lists.append([op.kind for op in self._ops]), run(self, *a, **k))[1])

    src, plate, depth = scene((H, W))
    mk, mk_up = MK.HipMatteKey(H, W, device=DEV), MK.HipMatteKey(H, W, device=DEV)
    mk_up.set_plate(plate)
    mt, up = MT.HipMatte(H, W, device=DEV), MT.HipMatteUp(H, W, Ho, Wo, device=DEV)
    hd = MT.HipMatteHold(H, W, device=DEV)
    back = BD.HipBackdrop(H, W, device=DEV)
    ks = dict(to="plate", lo=10.0, hi=150.0, luma=0.25, radius=2, combine="and", invert=True)
    ku = dict(to="plate", lo=10.0, hi=150.0, luma=0.0, radius=1, combine="or", invert=False)
    ad, ad_up = dict(rate=1 / 8, absorb=1 / 64), dict(rate=0.5, absorb=0.0)
    st = st_up = hstate = None
    for k in range(3):
        styled = frame16(30 + k, H, W)
        source = torch.from_numpy(np.roll(src, 5 * k, axis=2).copy())      # the scene, panned
        slot = Slot(source, depth)
        if k == 0:                               # the first frame is the plate: captured in the same list
            st = MK.state_of(source_bytes(source))
            st_up = MK.state_of(plate)
        raw, st = MK.raw_adapt_ref(source, st, depth, matte, ks, ad)
        want = MT.composite_ref(styled[None], source[None], None, **matte, plane=raw[None])[0]
        del lists[:]
        got = mt.composite(styled.to(DEV), slot, matte, mask=mk.record(slot, matte, ks, capture=k == 0, adapt=ad)).copy()
        assert [kinds[x] for x in lists[0]] == (["OP_FRAME_PLANAR_BYTES"] if k == 0 else []) + ["OP_MATTE_KEY_ADAPT", "OP_FRAME_MATTE"]
        assert differ(f"43, frame {k}", got, want) == 0
        assert np.array_equal(mk.current_plate(), MK.plate_bytes(st).transpose(1, 2, 0)), k
        assert k == 0 or (raw.min() == 0.0 and raw.max() == 1.0 and len(np.unique(raw)) > 8)     # both sides, and the soft part between
        # at the output size, with everything that reads the plane behind it
        slot.camera = CameraBuffer(dev(C8), (Ho, Wo, "lanczos"))
        raw_up, st_up = MK.raw_adapt_ref(source, st_up, depth, matte, ku, ad_up)
        h, hstate, _ = MT.hold_ref(MT.edge_ref(raw_up, source, **edge), source, hstate, init=k == 0, **hold)
        kept = BD.output_ref(bd, None, source, depth, matte, Ho, Wo, "lanczos", plane=raw_up)
        want = MT.composite_up_ref(S8, C8, None, **matte, plane=h[None], backdrop=kept)[0]
        front = mk_up.record(slot, matte, ku, adapt=ad_up)
        del lists[:]
        got = up.composite(dev(S8), slot, matte, edge=edge, hold=MT.HoldStep(hd, hold, k == 0, False), mask=front,
                           backdrop=back.output(slot, matte, bd, Ho, Wo, None, "lanczos", plane=front[2])).copy()
        assert [kinds[x] for x in lists[0] if kinds[x] != "OP_FRAME_RESIZE"] == [      # (the blurred frame is resampled to the output size)
            "OP_MATTE_KEY_ADAPT", "OP_FRAME_BACKDROP_BLUR", "OP_FRAME_MATTE_EDGE", "OP_FRAME_MATTE_HOLD", "OP_FRAME_MATTE_UP"]
        assert differ(f"47, frame {k}", got, want) == 0
        assert np.array_equal(mk_up.current_plate(), MK.plate_bytes(st_up).transpose(1, 2, 0)), k


# ----------------------------------------------------------------------------- the wrapper on the device
def test_wrapper_adapts_on_device():
    from test_matte_cpu import DropFilter
    wrapper, _ = _setup()
    rng = np.random.default_rng(9)
    frames = screen_u8(7, 3).astype(np.int64)
    for k in range(7):                           # the light warms by 4 levels a frame
        frames[k] += np.array([4 * k, 0, -4 * k])[None, None]
    frames = np.clip(frames + rng.integers(-1, 2, frames.shape), 0, 255).astype(np.uint8)
    w = wrapper(enable_similar_image_filter=True)
    w.stream.similar_filter = DropFilter({4})    # the fifth frame from here on is dropped
    w(frames[0])
    w.set_matte_key("capture", lo=20, hi=60)
    w.set_matte_key_adapt(rate=0.25, absorb=1 / 64)
    state, last, moved = None, None, 0
    for k in range(1, 7):
        w.stream.inference_time_ema = 0.0        # (a dropped frame waits that long)
        got = w(frames[k])
        slot, mt = w._matte_line.last, w.matte
        source, depth = slot.source.cpu(), slot.depth.cpu()
        if state is None:
            state = MK.state_of(source_bytes(source))
        dropped = k == 4
        before = state
        raw, state = MK.raw_adapt_ref(source, state, depth[None], mt, w.matte_key, dict(rate=0.0, absorb=0.0) if dropped else w.matte_key_adapt)
        want = MT.composite_ref(w.stream.prev_image_result.cpu(), source[None], depth[None], **mt, plane=raw[None])[0]
        assert differ(f"output {k}", got, want) == 0
        assert np.array_equal(w.matte_key_plate(), MK.plate_bytes(state).transpose(1, 2, 0)), k
        assert np.array_equal(words(w._key_dev.states[w._key_dev.cur].view(torch.int16)), state), k
        if dropped:
            assert np.array_equal(state, before)
        moved += not np.array_equal(state, before)
        last = raw
    assert moved >= 3 and 0.02 < float((last == 1.0).mean()) < 0.6 and float((last == 0.0).mean()) > 0.3
    w.clear_matte_key_adapt()
    assert w.matte_key_adapt is None
    w(frames[0])                                 # (the key's own launch again)
