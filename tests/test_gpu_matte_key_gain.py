"""GPU tests of the plate gain (csrc/matte_key.hip, live2diff_amd/matte_key.py): L2D_OP_MATTE_KEY_GAIN_HIST
against `gain_hist_ref` block by block behind guard words, L2D_OP_MATTE_KEY_GAIN on planted and on real partials against `gain_of`,
ops 59 and 61 under L2D_MATTE_KEY_GAIN against the oracle for planted records, the lists 62 -> 63 -> 59 and 60 -> 62 -> 63 -> 61 over
a room whose white balance steps, and the wrapper on synthetic weights, byte for byte what the host route computes.  There is no
tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from live2diff_amd import mask_io as MI
from live2diff_amd import matte as MT
from live2diff_amd import matte_key as MK
from live2diff_amd import ops
from live2diff_amd.backdrop import frame_of
from live2diff_amd.steady import source_bytes
from test_gpu_mask import RAMPS, _setup, dev, differ
from test_gpu_matte_key import SIZES, THRESHOLDS, scene, screen_u8
from test_gpu_matte_key_adapt import Guarded, run61, state_near, to_words, words
from test_matte_key_gain_cpu import PERSON, RH, RW, room, stepped

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # words in front of and behind the partials and the record, pre-filled and checked
FILL = -1                        # 0xFFFFFFFF: no count
BLOCK, BINS = ops.MATTE_KEY_GAIN_BLOCK, ops.MATTE_KEY_GAIN_BINS
MATTE = dict(lo=RAMPS["soft"][0], hi=RAMPS["soft"][1], keep="near")
# 72 x 136 = 9,792 pixels: two whole blocks of 4,096 and a ragged one of 1,600
HIST_SIZES = SIZES + [(RH, RW)]
RECORDS = [(32, 100, 128), (100, 128, 160), (128, 160, 511), (160, 511, 32), (511, 32, 100), (128, 128, 128)]


@functools.lru_cache(maxsize=None)
def gain_scene(shape):
    """(source fp16 [3,H,W], plate uint8 [3,H,W]) of one size, read-only.  The plate is anything, its clipped and near-black bytes
    included; the source in 8 x 8 cells: the plate itself, the plate times 5 / 4, 3 / 4 or 5 (which saturates bin 511 and the
    byte), the plate with noise of a few levels, anything, black or white, and raw fp16 noise that leaves [-1, 1]"""
    H, W = shape
    rng = np.random.default_rng(7000 + H * 1000 + W)
    plate = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    p = plate.astype(np.int64)
    kinds = [p, p * 5 // 4, p * 3 // 4, p * 5, p + rng.integers(-6, 7, p.shape), rng.integers(0, 256, p.shape),
             np.where(rng.random(p.shape) < 0.5, 0, 255)]
    cell = np.kron(rng.integers(0, len(kinds) + 1, ((H + 7) // 8, (W + 7) // 8)), np.ones((8, 8), dtype=np.int64))[:H, :W]
    b = np.zeros_like(p)
    for j, kind in enumerate(kinds):
        b = np.where(cell[None] == j, kind, b)
    src = np.array(frame_of(np.clip(b, 0, 255).astype(np.uint8)))
    wild = (rng.standard_normal((3, H, W)) * 1.5).astype(np.float16)
    src = np.where(cell[None] == len(kinds), wild, src)
    src.setflags(write=False)
    plate.setflags(write=False)
    return torch.from_numpy(src.copy()), plate


class Counts:
    """the partials and the record between guard words, pre-filled with 0xFFFFFFFF"""

    def __init__(self, H, W):
        self.nblk = ops.matte_key_gain_blocks(H, W)
        n = self.nblk * 3 * BINS
        self.pbuf = torch.empty(GUARD + n + GUARD, dtype=torch.int32, device=DEV)
        self.partials = self.pbuf[GUARD:GUARD + n].view(self.nblk, 3, BINS)
        self.rbuf = torch.empty(GUARD + 8 + GUARD, dtype=torch.int32, device=DEV)
        self.record = self.rbuf[GUARD:GUARD + 8]

    def reset(self):
        self.pbuf.fill_(FILL)
        self.rbuf.fill_(FILL)

    def counts(self):
        got = self.pbuf.cpu().numpy()
        assert np.all(got[:GUARD] == FILL) and np.all(got[-GUARD:] == FILL)
        return got[GUARD:-GUARD].reshape(self.nblk, 3, BINS).astype(np.int64)

    def rec(self):
        got = self.rbuf.cpu().numpy()
        assert np.all(got[:GUARD] == FILL) and np.all(got[-GUARD:] == FILL)
        return got[GUARD:-GUARD].astype(np.int64)


def blocks_ref(b, k):
    """int64 [nblk,3,512]: `gain_hist_ref` of every run of 4,096 pixels"""
    b, k = b.reshape(3, 1, -1), k.reshape(3, 1, -1)
    n = b.shape[2]
    return np.stack([MK.gain_hist_ref(b[:, :, i:i + BLOCK], k[:, :, i:i + BLOCK]) for i in range(0, n, BLOCK)])


# ----------------------------------------------------------------------------- op 62
@pytest.mark.parametrize("shape", HIST_SIZES)
def test_op62_equals_the_oracle_block_by_block(shape):
    H, W = shape
    src, plate = gain_scene(shape)
    b = source_bytes(src)
    state = state_near(plate, H + W)
    c = Counts(H, W)
    assert c.nblk == (3 if shape == (RH, RW) else -(-H * W // BLOCK))
    s_dev, p_dev, st_dev = src.to(DEV), dev(plate), to_words(state)
    for name, key_dev, k in (("plate", p_dev, plate), ("state", st_dev, MK.plate_bytes(state))):
        want = blocks_ref(b, k)
        assert np.array_equal(want.sum(0), MK.gain_hist_ref(b, k))
        if H * W >= 64:                          # the scene reaches unity, both scaled cells, the saturating bin and invalid samples
            total = want.sum(0)
            assert total[:, 128].min() > 0 and total[:, 160].min() > 0 and total[:, 96].min() > 0 and total[:, 511].min() > 0
            assert 0 < total.sum() < 3 * H * W
        for again in range(2):                   # a repeated launch: the same counts, nothing accumulated
            c.reset()
            ops.run(ops.matte_key_gain_hist(s_dev, key_dev, c.partials, H=H, W=W))
            assert differ(f"op 62 {shape} {name} run {again}", c.counts(), want) == 0
    assert np.array_equal(words(st_dev), state) and np.array_equal(p_dev.cpu().numpy(), plate)       # what is read stays as it was


# ----------------------------------------------------------------------------- op 63
def spread(hist, nblk, rng):
    """partials [nblk,3,512] of anything that sum to `hist`"""
    parts = np.zeros((nblk, 3, BINS), np.int64)
    left = hist.copy()
    for i in range(nblk - 1):
        parts[i] = rng.integers(0, left + 1)
        left -= parts[i]
    parts[nblk - 1] = left
    return parts


def planted_hists():
    def of(counts, zero=None):
        h = np.zeros((3, BINS), np.int64)
        for q, n in counts.items():
            h[:, q] = n
        if zero is not None:
            h[zero] = 0
        return h
    yield "a tie", of({100: 5, 140: 5}), 256, 1
    yield "below the tie", of({100: 4, 140: 5}), 256, 1
    yield "above the tie", of({100: 5, 140: 4}), 256, 1
    yield "three", of({100: 1, 120: 1, 140: 1}), 256, 1
    yield "n = min_count - 1", of({150: 7}), 256, 8
    yield "n = min_count", of({150: 7}), 256, 7
    yield "one channel empty", of({150: 7}, zero=1), 256, 7
    yield "no sample, min_count 0", of({}), 256, 0
    yield "the subject past one half", of({160: 4, 300: 6}), 511, 1
    yield "bin 0", of({0: 3, 200: 2}), 256, 1
    yield "bin 511", of({511: 3, 5: 2}), 511, 1
    yield "large counts", of({127: 3000, 128: 3264, 129: 3264}), 256, RH * RW // 16
    for lim in (256, 128, 511, 200, 129):
        yield f"upper clamp {lim}", of({511: 3}), lim, 1
        yield f"lower clamp {lim}", of({1: 3}), lim, 1


def test_op63_on_planted_and_real_partials():
    H, W = RH, RW
    c = Counts(H, W)
    rng = np.random.default_rng(63)
    cases = 0
    for name, hist, lim, min_count in planted_hists():
        g, n = MK.gain_of(hist, lim, min_count)
        for again in range(2):
            c.reset()
            c.partials.copy_(dev(spread(hist, c.nblk, rng).astype(np.int32)))
            ops.run(ops.matte_key_gain(c.partials, c.record, H=H, W=W, lim=lim, min_count=min_count))
            assert c.rec().tolist() == g.tolist() + n.tolist() + [0, 0], (name, again)
        cases += 1
    assert cases == 22
    # real ones: the scene's and the room's, under a few settings
    src, plate = gain_scene((H, W))
    b = source_bytes(src)
    rb = stepped((1.3, 1.0, 0.8), 4, np.random.default_rng(0))
    seen = set()
    for s, bb, kk in ((src.to(DEV), b, plate), (dev(frame_of(rb)), rb, room().astype(np.uint8))):
        for lim, min_count in ((256, H * W // 16), (140, 1), (511, H * W), (128, 0)):
            c.reset()
            ops.run(ops.matte_key_gain_hist(s, dev(kk), c.partials, H=H, W=W))
            ops.run(ops.matte_key_gain(c.partials, c.record, H=H, W=W, lim=lim, min_count=min_count))
            g, n = MK.measure_gain(bb, kk, lim, min_count)
            assert c.rec().tolist() == g.tolist() + n.tolist() + [0, 0], (lim, min_count)
            seen.add(tuple(g.tolist()))
    assert (168, 129, 101) in seen and len(seen) >= 4


# ----------------------------------------------------------------------------- ops 59 and 61 under the flag
def run59(src, plane, depth, plate, H, W, ks, gain=None, matte=MATTE):
    lo2, inv, hard = MK.key_params(ks["lo"], ks["hi"])
    kw = {}
    if ks["combine"] != "replace":
        lo32, inv32, ramp_hard = MT.matte_params(matte["lo"], matte["hi"])
        kw = dict(lo32=lo32, inv32=inv32, ramp_hard=ramp_hard, far=matte["keep"] == "far")
    if gain is not None:
        kw["gain"] = gain
    ops.run(ops.matte_key(src, plane, depth, plate, H=H, W=W, r=ks["radius"], L=MK.luma_weight(ks["luma"]), lo2=lo2, inv=inv, hard=hard,
                          combine=ks["combine"], invert=ks["invert"], **kw))


def run61g(src, plane, depth, plate, s_in, s_out, H, W, ks, rates, gain, matte=MATTE):
    """`run61` with the gain record"""
    lo2, inv, hard = MK.key_params(ks["lo"], ks["hi"])
    kw = {}
    if ks["combine"] != "replace":
        lo32, inv32, ramp_hard = MT.matte_params(matte["lo"], matte["hi"])
        kw = dict(lo32=lo32, inv32=inv32, ramp_hard=ramp_hard, far=matte["keep"] == "far")
    a_bg, a_fg = MK.adapt_params(*rates)
    ops.run(ops.matte_key_adapt(src, plane, depth, plate if s_in is None else None, s_in, s_out, H=H, W=W, r=ks["radius"],
                                L=MK.luma_weight(ks["luma"]), lo2=lo2, inv=inv, hard=hard, a_bg=a_bg, a_fg=a_fg, combine=ks["combine"],
                                invert=ks["invert"], gain=gain, **kw))


@pytest.mark.parametrize("shape", [(19, 72), (37, 136)])
def test_ops_59_and_61_under_the_flag_equal_the_oracle(shape):
    H, W = shape
    src, plate, depth = scene(shape)
    b = source_bytes(src)
    state = state_near(plate, H + W)
    s_dev, d_dev, p_dev, st_dev = dev(src), dev(depth), dev(plate), to_words(state)
    g, plain = Guarded(H, W), Guarded(H, W)
    rates = (1 / 8, 1 / 256)
    a = MK.adapt_params(*rates)
    bad = cases = varied = 0
    for rec in RECORDS:
        r_dev = dev(np.array(rec + (0, 0, 0, 0, 0), np.int32))
        for variant in ("59", "init", "state"):
            s0 = None if variant == "59" else (MK.state_of(plate) if variant == "init" else state)
            k = plate if variant != "state" else MK.plate_bytes(state)
            kg = MK.gain_plate(k, rec)
            for radius in (0, 1, 4):
                for thr, (lo, hi) in THRESHOLDS.items():
                    P0 = MK.plane_of(MK.distance_ref(b, kg, 0.25), lo=lo, hi=hi, radius=radius)
                    varied += not np.array_equal(P0, MK.plane_of(MK.distance_ref(b, k, 0.25), lo=lo, hi=hi, radius=radius))
                    nxt = None if s0 is None else MK.adapt_ref(s0, b, P0, *a)
                    for invert in (False, True):
                        P = (np.uint8(255) - P0) if invert else P0
                        for combine in ("replace", "and", "or"):
                            ks = dict(lo=lo, hi=hi, luma=0.25, radius=radius, combine=combine, invert=invert)
                            want = MI.front_ref(P, depth, MATTE["lo"], MATTE["hi"], MATTE["keep"], combine)
                            tag = f"{shape} {rec} {variant} r {radius} {thr} invert {invert} {combine}"
                            g.reset()
                            if variant == "59":
                                run59(s_dev, g.plane, d_dev, p_dev, H, W, ks, gain=r_dev)
                                bad += differ(tag, g.fbuf.cpu().numpy()[64:-64].reshape(H, W), want)
                                got = g.fbuf.cpu().numpy()
                                assert np.all(np.isnan(got[:64])) and np.all(np.isnan(got[-64:])), tag
                            else:
                                run61g(s_dev, g.plane, d_dev, p_dev, None if variant == "init" else st_dev, g.state, H, W, ks, rates, r_dev)
                                bad += g.check(tag, want, nxt)
                            if rec == (128, 128, 128):           # unity: the unflagged launch, bit for bit
                                plain.reset()
                                if variant == "59":
                                    run59(s_dev, plain.plane, d_dev, p_dev, H, W, ks)
                                else:
                                    run61(s_dev, plain.plane, d_dev, p_dev, None if variant == "init" else st_dev, plain.state, H, W, ks, rates)
                                    assert torch.equal(plain.state, g.state), tag
                                assert torch.equal(plain.plane.view(torch.int32), g.plane.view(torch.int32)), tag
                            cases += 1
    assert np.array_equal(words(st_dev), state) and np.array_equal(p_dev.cpu().numpy(), plate)       # what is read stays as it was
    assert bad == 0 and cases == 6 * 3 * 3 * 2 * 2 * 3
    assert varied >= 5 * 3 * 3                   # every record but unity changes a plane


# ----------------------------------------------------------------------------- the lists over a room whose white balance steps
def room_frames():
    """six frames of the room, the white balance stepping at frame 3; the person walks in with the step"""
    rng = np.random.default_rng(0)
    return [frame_of(stepped((1.0, 1.0, 1.0) if k < 3 else (1.3, 1.0, 0.8), 2, rng, person=k >= 3)) for k in range(6)]


KS = dict(to="plate", lo=40.0, hi=90.0, luma=0.25, radius=1, combine="replace", invert=False)
GAIN = dict(limit=2.0, min_share=1 / 16)


def test_the_list_62_63_59(monkeypatch):
    from live2diff_amd import _lib
    lists, run = [], _lib.OpList.run
    monkeypatch.setattr(_lib.OpList, "run", lambda self, *a, **k: (lists.append([op.kind for op in self._ops]), run(self, *a, **k))[1])
    plate = room().astype(np.uint8)
    lim, min_count = MK.gain_params(GAIN["limit"], GAIN["min_share"], RH, RW)
    mk, frozen = MK.HipMatteKey(RH, RW, device=DEV), MK.HipMatteKey(RH, RW, device=DEV)
    mk.set_plate(plate)
    frozen.set_plate(plate)
    for k, src in enumerate(room_frames()):
        s_dev = dev(src)
        g, n = MK.measure_gain(source_bytes(src), plate, lim, min_count)
        want = MK.raw_ref(src, plate, None, MATTE, KS, gain=g)
        for again in range(2):
            del lists[:]
            got = mk.key(s_dev, None, MATTE, KS, gain=GAIN).cpu().numpy()
            assert lists == [[62, 63, 59]]
            assert differ(f"frame {k} run {again}", got, want) == 0
            gg, nn = mk.current_gain()
            assert gg.tolist() == g.tolist() and nn.tolist() == n.tolist(), k
        wall = got[:, PERSON + 1:]
        assert wall.max() == 0.0, k              # the wall stays background through the step
        if k >= 3:
            assert np.abs(g - np.array([166, 128, 102])).max() <= 3         # 1.3, 1.0 and 0.8 in units of 1 / 128, within a few bins
            assert got[:, :PERSON - 1].mean() > 200 / 255
            del lists[:]
            without = frozen.key(s_dev, None, MATTE, KS).cpu().numpy()
            assert lists == [[59]] and float((without[:, PERSON + 1:] > 0).mean()) > 0.9          # and without the gain it does not


def test_the_lists_60_62_63_61_and_62_63_61(monkeypatch):
    from live2diff_amd import _lib
    lists, run = [], _lib.OpList.run
    monkeypatch.setattr(_lib.OpList, "run", lambda self, *a, **k: (lists.append([op.kind for op in self._ops]), run(self, *a, **k))[1])
    lim, min_count = MK.gain_params(GAIN["limit"], GAIN["min_share"], RH, RW)
    ad = dict(rate=1 / 8, absorb=0.0)
    mk = MK.HipMatteKey(RH, RW, device=DEV)
    state, gains = None, []
    for k, src in enumerate(room_frames()):
        b = source_bytes(src)
        if state is None:
            state = MK.state_of(b)               # the first frame is the plate: captured in the same list
        g, n = MK.measure_gain(b, MK.plate_bytes(state), lim, min_count)
        raw, state = MK.raw_adapt_ref(src, state, None, MATTE, KS, ad, gain=g)
        del lists[:]
        got = mk.key(dev(src), None, MATTE, KS, capture=k == 0, adapt=ad, gain=GAIN).cpu().numpy()
        assert lists == [[60, 62, 63, 61] if k == 0 else [62, 63, 61]]
        assert differ(f"frame {k}", got, raw) == 0
        gg, nn = mk.current_gain()
        assert gg.tolist() == g.tolist() and nn.tolist() == n.tolist(), k
        assert np.array_equal(words(mk.states[mk.cur].view(torch.int16)), state), k
        assert got[:, PERSON + 1:].max() == 0.0, k
        gains.append(g.tolist())
    assert gains[0] == [128] * 3                 # a capturing frame measures unity by construction
    assert abs(gains[3][0] - 166) <= 3 and abs(gains[3][2] - 102) <= 3 and gains[5][0] < gains[3][0] and gains[5][2] > gains[3][2]


# ----------------------------------------------------------------------------- the wrapper on the device
def host_route(w, hand):
    """what the host route computes of the slot and the styled frame the last output was composited with; `hand`: {plate, state}"""
    slot, mt = w._matte_line.last, w.matte
    source, depth = slot.source.cpu(), slot.depth.cpu()
    b = source_bytes(source)
    if hand.get("plate") is None:
        hand["plate"] = b
    s = w.matte_key_gain
    p = MK.gain_params(s["limit"], s["min_share"], *b.shape[1:])
    if w.matte_key_adapt is None:
        hand["last"] = MK.measure_gain(b, hand["plate"], *p)
        raw = MK.raw_ref(source, hand["plate"], depth[None], mt, w.matte_key, gain=hand["last"][0])
    else:
        if hand.get("state") is None:
            hand["state"] = MK.state_of(hand["plate"])
        hand["last"] = MK.measure_gain(b, MK.plate_bytes(hand["state"]), *p)
        raw, hand["state"] = MK.raw_adapt_ref(source, hand["state"], depth[None], mt, w.matte_key, w.matte_key_adapt, gain=hand["last"][0])
    return MT.composite_ref(w.stream.prev_image_result.cpu(), source[None], depth[None], **mt, plane=raw[None])[0], raw


def test_wrapper_measures_on_device():
    wrapper, _ = _setup()
    frames = screen_u8(7, 3).astype(np.float64)
    frames[3:] *= np.array([1.25, 0.9, 1.3])[None, None, None]           # the white balance steps at frame 3
    frames = np.clip(np.rint(frames), 0, 255).astype(np.uint8)
    w = wrapper()
    w.set_matte_key(frames[0], lo=20, hi=60)     # a plate from an image: frame 0 through `plate_ref`
    w.set_matte_key_gain(limit=1.5, min_share=1 / 32)
    hand = dict(plate=MK.plate_ref(frames[0], 64, 64, "lanczos"))
    stepped_ = 0
    for k in range(1, 6):
        got = w(frames[k])
        want, raw = host_route(w, hand)
        assert differ(f"image {k}", got, want) == 0
        g, n = hand["last"]
        assert w.matte_key_gain_measured() == (tuple(float(v) / 128 for v in g), tuple(float(v) / 4096 for v in n)), k
        stepped_ += g.tolist() != [128] * 3
    assert stepped_ >= 2 and raw.max() == 1.0 and float((raw == 0.0).mean()) > 0.3
    w.set_matte_key("capture", lo=20, hi=60)     # a captured plate under the adaptive plate: the source of the next output
    w.set_matte_key_adapt(rate=0.25)
    assert w.matte_key_gain == dict(limit=1.5, min_share=1 / 32)         # (a new key keeps the setting beside it)
    hand = dict()
    for k in (6, 0, 1, 2):
        got = w(frames[k])
        want, raw = host_route(w, hand)
        assert differ(f"captured {k}", got, want) == 0
        g, n = hand["last"]
        assert w.matte_key_gain_measured()[0] == tuple(float(v) / 128 for v in g), k
        assert np.array_equal(words(w._key_dev.states[w._key_dev.cur].view(torch.int16)), hand["state"]), k
        if k == 6:
            assert g.tolist() == [128] * 3 and not raw.any()
    assert g.tolist() != [128] * 3
    w.clear_matte_key_gain()
    assert w.matte_key_gain is None
    w(frames[3])                                 # (the adaptive key's own launch again)
