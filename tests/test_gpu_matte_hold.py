"""-m gpu: L2D_OP_FRAME_MATTE_HOLD (csrc/matte_hold.hip), behind L2D_OP_FRAME_MOTION where it follows, against `matte.hold_ref`,
bit for bit on the held plane, the state and the field, frame by frame over the sequences of tests/test_matte_hold_cpu.py (a
pan, a still stretch, a hard cut, a pan with fresh content); both input forms (the depth ramp near / far / hard, op 49's plane);
the records and the field inside guarded, poisoned buffers; two runs with the same bits; the held plane through op 43, op 47 and
in front of the JPEG encoder; and `set_matte_hold` on the wrapper with small native components against the host route."""
import numpy as np
import pytest
import torch

from test_matte_hold_cpu import EDGE, FORMS, MATTE, depths, oracle
from test_steady_cpu import bits
from test_steady_follow_cpu import K, sequence

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (8, 8) smaller than a tile and a window; (20, 40) a partial block row; (24, 40) no multiple of the 16 x 64 tile; (40, 72) and
# (48, 136) several tiles and strips; (64, 64) whole tiles
SHAPES = [(8, 8), (20, 40), (24, 40), (40, 72), (48, 136), (64, 64)]
RADII = [0, 2, 8]
SEARCHES = [0, 1, 4, 8]


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def differ(tag, got, want):
    """the number of values whose bits differ; prints where before the caller asserts"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    bad = bits(got) != bits(want)
    n = int(bad.sum())
    if n:
        at = np.argwhere(bad)[:4]
        print(f"{tag}: {n} of {want.size} values differ, first at {at.tolist()}: got {got[bad][:4]} want {want[bad][:4]}")
    return n


class Slot:
    def __init__(self, source, depth):
        self.source, self.depth = dev(source), dev(depth)


def settings_of(form):
    lo, hi = (0.5, 0.5) if form == "hard" else MATTE
    return dict(lo=lo, hi=hi, keep="far" if form in ("far", "plane") else "near", feather=0, show=False)


def hold_of(radius, search, **kw):
    return dict(lo=kw.get("lo", 2.0), hi=kw.get("hi", 10.0), strength=kw.get("strength", 0.8), radius=radius, search=search,
                bias=kw.get("bias", 256))


def frame_ops(hd, edge, slot, form, hold, init):
    """one frame's launches as the composites build them: op 49 for the plane form, then the hold's"""
    from live2diff_amd import _lib
    pl = _lib.OpList()
    plane = None
    if form == "plane":
        op, keep = edge.op(slot, settings_of(form), EDGE)
        pl.append(op, *keep)
        plane = edge.plane
    held = hd.append(pl, slot, settings_of(form), hold, plane, init=init)
    pl.run()
    return held


def run_sequence(H, W, form, radius, search, hd=None, frames=K, **kw):
    """`HipMatteHold` over the sequence against the oracle, frame by frame: the number of differing values"""
    from live2diff_amd import matte as MT
    sources, _ = sequence(H, W)
    ms, hs, states, fields = oracle(H, W, form, radius, search, **kw)
    hd = MT.HipMatteHold(H, W, device=DEV) if hd is None else hd
    edge = MT.HipMatteEdge(H, W, device=DEV) if form == "plane" else None
    hold, n = hold_of(radius, search, **kw), 0
    for k in range(frames):
        held = frame_ops(hd, edge, Slot(sources[k], depths(H, W)[k]), form, hold, k == 0)
        torch.cuda.synchronize()
        plane, by = hd.state
        tag = f"{(H, W)} {form} r={radius} search={search} {kw} frame {k}"
        assert held is plane
        if k and search:
            n += differ(f"{tag}: field", hd.field.cpu().numpy(), fields[k])
        n += differ(f"{tag}: held plane", held.cpu().numpy(), hs[k])
        n += differ(f"{tag}: state plane", plane.cpu().numpy(), states[k][0])
        n += differ(f"{tag}: state bytes", by.cpu().numpy(), states[k][1])
    return n


@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_hold_ref(shape, radius, search):
    """every shape, radius and search; the input form rotates through the four so that each meets every value of each"""
    form = FORMS[(SHAPES.index(shape) + RADII.index(radius) + SEARCHES.index(search)) % len(FORMS)]
    assert run_sequence(*shape, form, radius, search) == 0


@pytest.mark.parametrize("search", [0, 4])
@pytest.mark.parametrize("form", FORMS)
def test_every_input_form(form, search):
    assert run_sequence(24, 40, form, 2, search) == 0
    assert run_sequence(40, 72, form, 2, search) == 0
    ms, hs, _, fields = oracle(40, 72, form, 2, search)
    assert not np.array_equal(hs[2], ms[2]) and np.array_equal(hs[0], ms[0]) and (not search or fields[1].any())


def test_hard_motion_ramp_and_strength_ends():
    assert run_sequence(40, 72, "near", 3, 4, lo=4, hi=4) == 0                   # a step: t = dbar >= lo
    assert run_sequence(40, 72, "plane", 0, 0, lo=4, hi=4, strength=1.0) == 0
    assert run_sequence(24, 40, "far", 2, 8, strength=0.0, bias=0) == 0          # a == 1 everywhere: m0's own bits


@pytest.mark.parametrize("shape,form,radius,search", [((24, 40), "near", 2, 8), ((40, 72), "plane", 8, 8), ((20, 40), "far", 0, 0)])
def test_records_and_field_need_no_zeroing_and_stay_in_bounds(shape, form, radius, search):
    """both (plane, bytes) records and the field live inside larger buffers, NaN-filled and 0xA5-filled: three frames from `init` on
    equal the oracle, and every guard element before and behind them is as it was"""
    from live2diff_amd import matte as MT
    H, W = shape
    n, G = H * W, 4096                                                    # (G elements: the records stay 16-byte aligned)
    floats = torch.full((5 * G + 2 * n,), float("nan"), dtype=torch.float32, device=DEV)
    raw = torch.full((5 * G + 6 * n,), 0xA5, dtype=torch.uint8, device=DEV)
    at, bat = [2 * G, 3 * G + n], [2 * G, 3 * G + 3 * n]
    records = [(floats[o:o + n].view(H, W), raw[b:b + 3 * n].view(3, H, W)) for o, b in zip(at, bat)]
    Hb, Wb = (H + 7) // 8, W // 8
    nf, fat = 2 * Hb * Wb, G + 1                                          # (the field takes any alignment: an odd address)
    vec = torch.full((2 * G + nf + 1,), -91, dtype=torch.int8, device=DEV)          # 0xA5 as int8
    hd = MT.HipMatteHold(H, W, device=DEV, records=records, field=vec[fat:fat + nf].view(Hb, Wb, 2))
    assert run_sequence(H, W, form, radius, search, hd=hd, frames=3) == 0
    f, b, v = floats.cpu().numpy(), raw.cpu().numpy(), vec.cpu().numpy()
    inside, binside = np.zeros(f.size, dtype=bool), np.zeros(b.size, dtype=bool)
    for o, bo in zip(at, bat):
        inside[o:o + n] = True
        binside[bo:bo + 3 * n] = True
    assert np.isnan(f[~inside]).all() and (b[~binside] == 0xA5).all() and not np.isnan(f[inside]).any()
    assert (v[:fat] == -91).all() and (v[fat + nf:] == -91).all()
    assert (np.abs(v[fat:fat + nf].astype(int)).max() <= search) if search else (v == -91).all()


def test_two_runs_give_the_same_bits():
    from live2diff_amd import matte as MT
    H, W = 48, 136
    sources, _ = sequence(H, W)
    runs = []
    for _ in range(2):
        hd, edge, got = MT.HipMatteHold(H, W, device=DEV), MT.HipMatteEdge(H, W, device=DEV), []
        for k in range(K):
            held = frame_ops(hd, edge, Slot(sources[k], depths(H, W)[k]), "plane", hold_of(2, 8, bias=0), k == 0)
            got.append((held.cpu().numpy().copy(), hd.state[1].cpu().numpy().copy(), None if k == 0 else hd.field.cpu().numpy().copy()))
        runs.append(got)
    for k in range(K):
        assert np.array_equal(bits(runs[0][k][0]), bits(runs[1][k][0])) and np.array_equal(runs[0][k][1], runs[1][k][1])
        assert k == 0 or np.array_equal(runs[0][k][2], runs[1][k][2])


@pytest.mark.parametrize("form", ["near", "plane"])
def test_held_plane_through_the_composites_and_the_encoder(form):
    """`HipMatte.composite` (op 43, feather 0 and 4), `HipMatteUp.composite` (op 47) and the JPEG encoder behind the held plane"""
    from live2diff_amd import jpeg
    from live2diff_amd import matte as MT
    from live2diff_amd.jpeg_io import HipJpegEncoder
    from live2diff_amd.resize import CameraBuffer
    H, W, Ho, Wo = 64, 128, 96, 160
    sources, styled = sequence(H, W)
    ms, hs, _, _ = oracle(H, W, form, 2, 4)
    rng = np.random.default_rng(3)
    S8, C8 = (rng.integers(0, 256, (Ho, Wo, 3), dtype=np.uint8) for _ in range(2))
    edge = EDGE if form == "plane" else None
    for feather in (0, 4):
        settings = dict(settings_of(form), feather=feather)
        mt, up, hd = MT.HipMatte(H, W, device=DEV), MT.HipMatteUp(H, W, Ho, Wo, device=DEV), MT.HipMatteHold(H, W, device=DEV)
        for k in range(3):
            slot = Slot(sources[k], depths(H, W)[k])
            step = MT.HoldStep(hd, hold_of(2, 4), k == 0, False)
            got = mt.composite(dev(styled[k]), slot, settings, edge=edge, hold=step).copy()
            want = MT.composite_ref(styled[k][None], sources[k][None], None, **settings, plane=hs[k][None])[0]
            assert np.array_equal(got, want), (feather, k)
        assert not np.array_equal(hs[2], ms[2])
        # the same held plane again (a repeated frame moves nothing), at the output size and in front of the encoder
        cur = hd._cur
        slot.camera = CameraBuffer(dev(C8), (Ho, Wo, "lanczos"))
        again = MT.HoldStep(hd, hold_of(2, 4), False, True)
        got = up.composite(dev(S8), slot, settings, edge=edge, hold=again).copy()
        assert hd._cur == cur
        assert np.array_equal(got, MT.composite_up_ref(S8, C8, None, **settings, plane=hs[2][None])[0]), feather
        u8 = mt.composite(dev(styled[2]), slot, settings, to_host=False, edge=edge, hold=again)
        enc = HipJpegEncoder(H, W, 75, device=DEV)
        want = MT.composite_ref(styled[2][None], sources[2][None], None, **settings, plane=hs[2][None])[0]
        assert enc.encode(u8) == jpeg.encode_ref(want, 75)


# ----------------------------------------------------------------------------- the wrapper on the device
FRAME_OPS = ("OP_FRAME_EGRESS", "OP_FRAME_MATTE", "OP_FRAME_MATTE_EDGE", "OP_FRAME_MOTION", "OP_FRAME_MATTE_HOLD")


def test_wrapper_hold_on_device(monkeypatch):
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd import _lib
    from live2diff_amd import matte as MT
    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    from test_matte_cpu import DropFilter
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    parts = Parts(ucfg, ccfg, H, W, 2)
    warm = u8_frames(8, H, W, seed=1)
    # a still camera with a little noise, then a pan: one picture of 4 x 4 cells at the stream's own size
    big = np.kron(u8_frames(1, 32, 32, seed=2)[0], np.ones((4, 4, 1), dtype=np.uint8))
    rng = np.random.default_rng(4)
    offs = [(0, 0), (0, 0), (0, 0), (0, 0), (2, -3), (4, -6), (4, -6), (4, -6)]
    frames = np.stack([np.clip(big[20 + oy:20 + oy + H, 30 + ox:30 + ox + W].astype(int) + rng.integers(-1, 2, (H, W, 3)), 0, 255)
                       for oy, ox in offs]).astype(np.uint8)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)
    MATTE_SET = dict(lo=0.3, hi=0.7, keep="far", feather=2, show=False)

    kinds = {v: k for k, v in vars(_lib).items() if k.startswith("OP_")}
    ran, run = [], _lib.OpList.run

    def recording(self, *a, **k):
        ran.extend(kinds[op.kind] for op in self._ops if kinds[op.kind] in FRAME_OPS)
        return run(self, *a, **k)

    monkeypatch.setattr(_lib.OpList, "run", recording)
    torch.manual_seed(0)                         # `prepare` draws init_noise and the warm-up re-noising from the global generators
    pipe = parts.pipe()
    pipe.similar_filter = DropFilter({3})        # the fourth frame is dropped
    w = Wrapper.from_components(pipe, output_type="u8", seed=SEED, device=DEV, matte_hold=dict(search=4), enable_similar_image_filter=True,
                                **kw)
    w.set_matte(MATTE_SET["lo"], MATTE_SET["hi"], keep="far", feather=2)
    w.prepare(warm, PROMPT)
    assert w.matte_hold == dict(lo=2.0, hi=10.0, strength=0.8, radius=2, search=4, bias=256) and w.matte == MATTE_SET
    state, last, held_frames = None, None, 0
    for t, f in enumerate(frames):
        if t == 5:
            w.clear_matte_hold()                 # the matte of the frame alone
        if t == 6:
            w.set_matte_hold(search=4)           # set again mid-stream: an init frame
            w.set_matte_edge(**EDGE)
            state = None
        del ran[:]
        w.stream.inference_time_ema = 0.0        # (a dropped frame waits that long)
        out = w(f)
        slot = w._matte_line.last
        source, depth = slot.source.cpu(), slot.depth.cpu()
        edge = w.matte_edge
        if t == 3:                               # the dropped frame: the output before, no launch of the hold, no state moved
            assert ran == ["OP_FRAME_MATTE"] and np.array_equal(out, last), ran
            continue
        if t == 5:
            assert ran == ["OP_FRAME_MATTE"], ran
            want = MT.composite_ref(w.stream.prev_image_result.cpu(), source[None], depth[None], **MATTE_SET)[0]
        else:
            init = state is None
            front = (["OP_FRAME_MATTE_EDGE"] if edge else []) + ([] if init else ["OP_FRAME_MOTION"])
            assert ran == front + ["OP_FRAME_MATTE_HOLD", "OP_FRAME_MATTE"], (t, ran)
            m0 = MT.matte_ref(depth[None], 0.3, 0.7, 0, "far", edge=edge, source=source[None] if edge else None)[0]
            h, state, field = MT.hold_ref(m0, source, state, init=init, **w.matte_hold)
            want = MT.composite_ref(w.stream.prev_image_result.cpu(), source[None], depth[None], **MATTE_SET, plane=h[None])[0]
            dev_state = w._hold_dev.state
            assert np.array_equal(bits(dev_state[0].cpu().numpy()), bits(state[0])) and np.array_equal(dev_state[1].cpu().numpy(), state[1]), t
            if not init:
                assert np.array_equal(w._hold_dev.field.cpu().numpy(), field), t
                held_frames += not np.array_equal(h, m0)
        assert out.dtype == np.uint8 and out.shape == (H, W, 3) and np.array_equal(out, want), t
        last = out
    assert held_frames >= 3
