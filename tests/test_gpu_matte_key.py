"""GPU tests of the matte key (csrc/matte_key.hip, live2diff_amd/matte_key.py): ops 59 and 60 against
`front_ref(key_ref(...))` and `source_bytes` on every bit behind guard bands, the composites' whole lists 59 -> 54 -> 49 -> 57 ->
43 and 60 -> 59 -> 47 against the oracles chained by hand, and the wrapper on synthetic weights: a colour key, a plate from an
image and a captured plate, byte for byte what the host route computes.  There is no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from live2diff_amd import backdrop as BD
from live2diff_amd import mask_io as MI
from live2diff_amd import matte as MT
from live2diff_amd import matte_key as MK
from live2diff_amd.steady import source_bytes
from test_gpu_mask import RAMPS, Slot, _setup, dev, differ
from test_matte_key_cpu import GREEN, depth16, frame16, planted

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # floats (bytes for op 60) in front of and behind the output, pre-filled and checked

# (1, 8): one lane's worth of pixels; (19, 72) and (37, 136): partial 16 x 64 tiles on both axes and two / three tiles along each;
# (40, 72): the size of the CPU tests.  A halo of 4 crosses every tile border of the larger three.
SIZES = [(1, 8), (19, 72), (37, 136), (40, 72)]
THRESHOLDS = {"soft": (10.0, 150.0), "hard": (100.0, 100.0)}


@functools.lru_cache(maxsize=None)
def scene(shape):
    """(source fp16 [3,H,W], plate uint8 [3,H,W], depth fp16 [H,W]) of one size, read-only: whole cells in which the source is the
    key (the colour, or the plate) with noise of a few levels -- D near the thresholds --, and cells of anything else; one cell
    keeps raw fp16 noise that leaves [-1, 1], so the byte's clamp is exercised"""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    cell = 8
    is_key = np.kron(rng.random(((H + cell - 1) // cell, (W + cell - 1) // cell)) < 0.5, np.ones((cell, cell), dtype=bool))[:H, :W]
    plate = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    half = np.arange(W)[None] < W // 2
    plate[:, is_key & half] = np.array(GREEN, np.uint8)[:, None]          # in the left half the plate is the colour: both variants bite
    near = np.clip(plate.astype(np.int64) + rng.integers(-12, 13, plate.shape), 0, 255).astype(np.uint8)
    b = np.where(is_key[None], near, rng.integers(0, 256, (3, H, W), dtype=np.uint8))
    src = BD.frame_of(b).copy()
    wild = frame16(H + W, H, W).numpy()
    src[:, :, -8:] = np.where(np.arange(H)[None, :, None] < 8, wild[:, :, -8:], src[:, :, -8:])
    depth = depth16(H + 2 * W, H, W)
    for a in (src, plate, depth):
        a.setflags(write=False)
    return src, plate, depth


def settings(to, thr, luma, radius, combine="replace", invert=False):
    lo, hi = THRESHOLDS[thr]
    return dict(to=to, lo=lo, hi=hi, luma=luma, radius=radius, combine=combine, invert=invert)


# ----------------------------------------------------------------------------- ops 59 and 60
@pytest.mark.parametrize("shape", SIZES)
def test_op59_equals_the_oracle_on_every_bit(shape):
    H, W = shape
    src, plate, depth = scene(shape)
    s_dev, d_dev = dev(src), dev(depth)
    buf = torch.empty(GUARD + H * W + GUARD, dtype=torch.float32, device=DEV)
    mk = MK.HipMatteKey(H, W, device=DEV, plane=buf[GUARD:GUARD + H * W].view(H, W))
    mk.set_plate(plate)
    bad = cases = varied = 0
    for variant, key in (("color", GREEN), ("plate", plate)):
        for radius in (0, 1, 4):
            for thr, (lo, hi) in THRESHOLDS.items():
                for luma in (0.0, 0.25, 1.0):
                    D = MK.distance_ref(source_bytes(src), key, luma)
                    for invert in (False, True):
                        P = MK.plane_of(D, lo=lo, hi=hi, radius=radius, invert=invert)
                        varied += len(np.unique(P)) > 2
                        for combine, keep, ramp in (("replace", "near", "soft"), ("and", "near", "soft"), ("and", "far", "hard"),
                                                    ("or", "far", "soft"), ("or", "near", "hard")):
                            buf.fill_(float("nan"))                        # an unwritten pixel shows
                            matte = dict(lo=RAMPS[ramp][0], hi=RAMPS[ramp][1], keep=keep)
                            mk.key(s_dev, d_dev, matte, settings(GREEN if variant == "color" else "plate", thr, luma, radius, combine, invert))
                            got = buf.cpu().numpy()
                            want = MI.front_ref(P, depth, matte["lo"], matte["hi"], keep, combine)
                            bad += differ(f"{shape} {variant} r {radius} {thr} luma {luma} invert {invert} {combine} {keep} {ramp}",
                                          got[GUARD:-GUARD].reshape(H, W), want)
                            assert np.all(np.isnan(got[:GUARD])) and np.all(np.isnan(got[-GUARD:]))
                            cases += 1
    assert bad == 0 and cases == 2 * 3 * 2 * 3 * 2 * 5
    assert varied >= 6 or shape == (1, 8)        # soft cases hold values strictly between 0 and 255


def test_op59_planted_boundaries_and_repeated_launches():
    matte = dict(lo=0.3, hi=0.7, keep="near")
    for (dR, dG, dB), lo, hi, want in (((4, -3, 3), 5, 5, 1.0), ((4, -3, 2), 5, 5, 0.0), ((4, -3, 3), 3, 5, 1.0), ((4, -3, 3), 5, 7, 0.0)):
        src, key = planted(dR, dG, dB)
        mk = MK.HipMatteKey(1, 8, device=DEV)
        s = dict(to=key, lo=lo, hi=hi, luma=0.0, radius=0, combine="replace", invert=False)
        got = mk.key(dev(src), None, matte, s).cpu().numpy()
        assert np.array_equal(got, np.full((1, 8), want, np.float32)), (dR, dG, dB, lo, hi)
        assert differ("planted", got, MK.raw_ref(src, key, None, matte, s)) == 0
        for form in ("plate", "captured"):       # the same through a plate filled with the colour, and keyed against its own capture
            if form == "plate":
                mk.set_plate(np.ascontiguousarray(np.broadcast_to(np.array(key, np.uint8)[:, None, None], (3, 1, 8))))
                assert np.array_equal(mk.key(dev(src), None, matte, dict(s, to="plate")).cpu().numpy(), got)
            else:
                own = mk.key(dev(src), None, matte, dict(s, to="plate"), capture=True).cpu().numpy()
                assert np.array_equal(own, np.zeros((1, 8), np.float32))
    # repeated launches: identical bits
    H, W = 37, 136
    src, plate, depth = scene((H, W))
    mk = MK.HipMatteKey(H, W, device=DEV)
    mk.set_plate(plate)
    s = settings("plate", "soft", 0.25, 4, "and")
    first = mk.key(dev(src), dev(depth), matte, s).clone()
    for _ in range(3):
        assert torch.equal(mk.key(dev(src), dev(depth), matte, s), first)


@pytest.mark.parametrize("shape", SIZES)
def test_op60_equals_source_bytes(shape):
    from live2diff_amd import ops
    H, W = shape
    src = scene(shape)[0]
    buf = torch.full((GUARD + 3 * H * W + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    ops.run(ops.frame_planar_bytes(dev(src), buf[GUARD:GUARD + 3 * H * W].view(3, H, W), H=H, W=W))
    got = buf.cpu().numpy()
    assert differ(f"op 60 {shape}", got[GUARD:-GUARD].reshape(3, H, W), source_bytes(src)) == 0
    assert np.all(got[:GUARD] == 0xA5) and np.all(got[-GUARD:] == 0xA5)


# ----------------------------------------------------------------------------- the composites' whole lists
def test_one_list_59_54_49_57_43_and_60_59_47(monkeypatch):
    """`HipMatte.composite` with a key, a blurred backdrop, the edge refit and the hold in ONE list, and `HipMatteUp.composite`
    with a capturing key, against raw_ref -> edge_ref -> hold_ref -> composite_ref(plane=) / composite_up_ref by hand"""
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
    mt, up = MT.HipMatte(H, W, device=DEV), MT.HipMatteUp(H, W, Ho, Wo, device=DEV)
    hd = MT.HipMatteHold(H, W, device=DEV)
    back = BD.HipBackdrop(H, W, device=DEV)
    ks = settings(GREEN, "soft", 0.25, 2, "and", True)
    ku = settings("plate", "soft", 0.0, 1, "or")
    state = up_plate = None
    for k in range(3):
        styled = frame16(30 + k, H, W)
        source = torch.from_numpy(np.roll(src, 5 * k, axis=2).copy())      # the scene, panned
        slot = Slot(source, depth)
        raw = MK.raw_ref(source, GREEN, depth, matte, ks)
        h, state, _ = MT.hold_ref(MT.edge_ref(raw, source, **edge), source, state, init=k == 0, **hold)
        bdrop = BD.stream_ref(bd, None, source, depth, matte, plane=raw)
        want = MT.composite_ref(styled[None], source[None], None, **matte, plane=h[None], backdrop=bdrop[None])[0]
        front = mk.record(slot, matte, ks)
        del lists[:]
        got = mt.composite(styled.to(DEV), slot, matte, edge=edge, hold=MT.HoldStep(hd, hold, k == 0, False), mask=front,
                           backdrop=back.stream(slot, matte, bd, plane=front[2])).copy()
        assert [kinds[x] for x in lists[0]] == ["OP_MATTE_KEY", "OP_FRAME_BACKDROP_BLUR", "OP_FRAME_MATTE_EDGE", "OP_FRAME_MATTE_HOLD",
                                               "OP_FRAME_MATTE"]
        assert differ(f"43, frame {k}", got, want) == 0
        # at the output size: the first frame captures the plate in the same list, the later ones are keyed against it
        slot.camera = CameraBuffer(dev(C8), (Ho, Wo, "lanczos"))
        if k == 0:
            up_plate = source_bytes(source)
        del lists[:]
        got = up.composite(dev(S8), slot, matte, mask=mk_up.record(slot, matte, ku, capture=k == 0)).copy()
        assert [kinds[x] for x in lists[0]] == (["OP_FRAME_PLANAR_BYTES"] if k == 0 else []) + ["OP_MATTE_KEY", "OP_FRAME_MATTE_UP"]
        assert np.array_equal(mk_up.plate.cpu().numpy(), up_plate)
        raw_up = MK.raw_ref(source, up_plate, depth, matte, ku)
        assert k == 0 or 0.02 < float((raw_up == 1.0).mean()) < 0.98
        assert differ(f"47, frame {k}", got, MT.composite_up_ref(S8, C8, None, **matte, plane=raw_up[None])[0]) == 0
    # without edge and hold the composite reads op 59's plane itself; `show` shows it
    shown = mt.composite(styled.to(DEV), slot, dict(matte, feather=0, show=True), mask=mk.record(slot, matte, ks)).copy()
    assert np.array_equal(shown[..., 0], np.rint(raw * np.float32(255)).astype(np.uint8)) and np.array_equal(shown[..., 0], shown[..., 2])


# ----------------------------------------------------------------------------- the wrapper on the device
def screen_u8(n, seed, Hs=96, Ws=128):
    """uint8 [n,Hs,Ws,3] camera frames: a green screen with noise of +-6 and a box of anything at a place of the frame's own"""
    rng = np.random.default_rng(seed)
    f = np.clip(np.array(GREEN)[None, None, None] + rng.integers(-6, 7, (n, Hs, Ws, 3)), 0, 255).astype(np.uint8)
    for k in range(n):
        y, x = 10 + 9 * k, 70 - 9 * k
        f[k, y:y + 32, x:x + 32] = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    return f


def host_route(w, key):
    """what the host route computes of the slot and the styled frame the last output was composited with"""
    slot, mt = w._matte_line.last, w.matte
    source, depth = slot.source.cpu(), slot.depth.cpu()
    raw = MK.raw_ref(source, key, depth[None], mt, w.matte_key)
    return MT.composite_ref(w.stream.prev_image_result.cpu(), source[None], depth[None], **mt, plane=raw[None])[0], raw


def test_wrapper_keys_on_device():
    wrapper, _ = _setup()
    frames = screen_u8(6, 3)
    w, twin = wrapper(), wrapper()
    w.set_matte_key(GREEN)
    for k in range(3):                           # a colour key: output k is keyed of frame k - 1's source
        got, plain = w(frames[k]), twin(frames[k])
        want, raw = host_route(w, GREEN)
        assert differ(f"colour {k}", got, want) == 0
        if k:
            assert 0.05 < float((raw == 1.0).mean()) < 0.5 and float((raw == 0.0).mean()) > 0.4 and not np.array_equal(got, plain), k
    w.set_matte_key(frames[0], combine="and")    # a plate from an image: frame 0 through `plate_ref`
    plate = MK.plate_ref(frames[0], 64, 64, "lanczos")
    for k in range(3, 5):
        got = w(frames[k])
        assert np.array_equal(w._key_dev.plate.cpu().numpy(), plate) and w.matte_key["to"] == "plate"
        assert differ(f"image {k}", got, host_route(w, plate)[0]) == 0
    w.set_matte_key("capture", lo=20, hi=60)     # a captured plate: the source of the next output, frame 4
    assert w.matte_key["to"] == "capture"
    got = w(frames[5])
    captured = source_bytes(w._matte_line.last.source.cpu())
    assert w.matte_key["to"] == "plate" and np.array_equal(w._key_dev.plate.cpu().numpy(), captured)
    want, raw = host_route(w, captured)
    assert differ("capturing frame", got, want) == 0 and not raw.any()
    for k in (0, 1):
        got = w(frames[k])
        assert np.array_equal(w._key_dev.plate.cpu().numpy(), captured)
        want, raw = host_route(w, captured)
        assert differ(f"captured {k}", got, want) == 0
    assert 0.05 < float((raw == 1.0).mean()) < 0.6 and float((raw == 0.0).mean()) > 0.3
    w.clear_matte_key()
    assert w.matte_key is None and w._key_dev is None
    w(frames[2])                                 # (the plain matte route again)
