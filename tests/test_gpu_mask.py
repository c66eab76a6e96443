"""GPU tests of the matte from the caller (csrc/mask_in.hip, live2diff_amd/mask_io.py): op 58 against
`front_ref(mask_ref(...))` on every bit, ops 49 and 54 under their plane flags against `edge_ref` and `blur_ref(plane=)`, the
composites' whole lists 58 -> 49 -> 57 -> 43 / 47 against the oracles composed by hand, and the wrapper on synthetic weights:
a different binary mask per frame, `__call__` and `push` / `pop`, device and host masks, the pool in steady state.  There is no
tolerance anywhere: 255 r has exact ties, so the kernel has to match r bit for bit."""
import functools

import numpy as np
import pytest
import torch

from live2diff_amd import backdrop as BD
from live2diff_amd import mask_io as MI
from live2diff_amd import matte as MT
from test_mask_cpu import bits, depth16, frame16, soft

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # floats in front of and behind the plane, pre-filled and checked

# outputs: 40 x 72 has partial tiles of the 16 x 32 tile on both axes, 64 x 64 whole ones.  Masks: 1 : 1; an up-scale with exact
# ties of 255 r; scale 8 with 17 taps; a crop offset; 512 x 512 (scale 8 to 64 x 64).  A pair `frame_io.geometry` refuses (the
# 40 x 72 window does not lie inside a square mask's image) is not a case.
PAIRS = [((40, 72), (40, 72)), ((40, 72), (30, 54)), ((40, 72), (320, 576)), ((64, 64), (64, 96)), ((64, 64), (512, 512)),
         ((64, 64), (30, 54))]
RAMPS = {"soft": (0.3, 0.7), "hard": (0.5, 0.5)}


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)            # (a copy: the cached masks are read-only)


def differ(tag, got, want):
    """the number of values whose bits differ; prints where before the caller asserts"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    bad = (bits(got) != bits(want)) if got.dtype == np.float32 else (got != want)
    n = int(bad.sum())
    if n:
        at = np.argwhere(bad)[:4]
        print(f"{tag}: {n} of {want.size} values differ, first at {at.tolist()}: got {got[bad][:4]} want {want[bad][:4]}")
    return n


@functools.lru_cache(maxsize=None)
def masks_of(shape):
    """{name: mask} of one size, read-only: random and binary masks of the three sample types; the float one holds NaN,
    infinities and values outside [0, 1]"""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    binary = rng.random(shape) < 0.5
    wild = (rng.random(shape) * 1.6 - 0.3).astype(np.float32)
    wild[rng.random(shape) < 0.02] = np.nan
    wild[rng.random(shape) < 0.01] = np.inf
    wild[rng.random(shape) < 0.01] = -np.inf
    out = {"u8 random": rng.integers(0, 256, shape, dtype=np.uint8), "u8 binary": binary.astype(np.uint8) * np.uint8(255),
           "u16 random": rng.integers(0, 65536, shape).astype(np.uint16), "u16 binary": binary.astype(np.uint16) * np.uint16(65535),
           "f32 wild": wild, "f32 binary": binary.astype(np.float32)}
    for m in out.values():
        m.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def plane_ref(shape, name, out, invert):
    P = MI.mask_ref(masks_of(shape)[name], *out, invert)
    P.setflags(write=False)
    return P


def to_dev(m):
    """a mask on the device; uint16 as the int16 tensor of its bits"""
    return dev(m.view(np.int16) if m.dtype == np.uint16 else m)


# ----------------------------------------------------------------------------- op 58
@pytest.mark.parametrize("out,shape", PAIRS)
def test_op58_equals_the_oracle_on_every_bit(out, shape):
    H, W = out
    depth = depth16(7, H, W)
    ing = MI.HipMaskIngest(H, W, device=DEV)
    d = dev(depth)
    buf = torch.empty(GUARD + H * W + GUARD, dtype=torch.float32, device=DEV)
    plane = buf[GUARD:GUARD + H * W].view(H, W)
    bad = cases = 0
    for name, m in masks_of(shape).items():
        md = to_dev(m)
        for invert in (False, True):
            P = plane_ref(shape, name, out, invert)
            for combine in MI.COMBINES:
                for keep in ("near", "far"):
                    for ramp, (lo, hi) in RAMPS.items():
                        if combine == "replace" and (keep, ramp) != ("near", "soft"):
                            continue                                   # (a replacing mask reads neither)
                        buf.fill_(float("nan"))                        # an unwritten pixel shows
                        matte = dict(lo=lo, hi=hi, keep=keep)
                        ing.ingest(md, d, matte, dict(combine=combine, invert=invert), out=plane)
                        got = buf.cpu().numpy()
                        want = MI.front_ref(P, depth, lo, hi, keep, combine)
                        bad += differ(f"{shape} -> {out} {name} {combine} invert {invert} {keep} {ramp}", got[GUARD:-GUARD].reshape(H, W), want)
                        assert np.all(np.isnan(got[:GUARD])) and np.all(np.isnan(got[-GUARD:]))
                        cases += 1
    assert bad == 0 and cases == 6 * 2 * 9
    assert ing.allocated <= 3                    # (one buffer per element size at most: the pool serves every later mask)


def test_op58_ties_constants_and_containers():
    """the ties case by name; constant masks come back exactly 0 or 1; a host mask, a device mask, bool and fp16 give the same bits"""
    H, W = 40, 72
    rng = np.random.default_rng(0)
    m = rng.integers(0, 256, (30, 54), dtype=np.uint8)
    ing = MI.HipMaskIngest(H, W, device=DEV)
    rep = dict(combine="replace", invert=False)
    want = MI.front_ref(MI.mask_ref(m, H, W), None, 0, 1)
    for form in (m, torch.from_numpy(m), dev(m)):
        assert differ("ties", ing.ingest(form, None, {}, rep).cpu().numpy(), want) == 0
    for shape in ((30, 54), (320, 576)):
        for dtype, top in ((np.uint8, 255), (np.uint16, 65535), (np.float32, 1.0)):
            one = ing.ingest(np.full(shape, top, dtype), None, {}, rep).cpu().numpy()
            assert np.array_equal(bits(one), bits(np.ones((H, W)))), (shape, dtype)
            zero = ing.ingest(np.zeros(shape, dtype), None, {}, rep).cpu().numpy()
            assert np.array_equal(bits(zero), bits(np.zeros((H, W)))), (shape, dtype)
    b = rng.random((30, 54)) < 0.5
    want = MI.front_ref(MI.mask_ref(b, H, W), None, 0, 1)
    for form in (b, dev(b), dev(b.astype(np.float16))):
        assert differ("bool / fp16", ing.ingest(form, None, {}, rep).cpu().numpy(), want) == 0
    with pytest.raises(ValueError, match="^mask: "):
        ing.ingest(np.zeros((64, 64), np.uint8), None, {}, rep)
    # every buffer came back, and the same masks again allocate nothing
    grown = ing.allocated
    assert len(ing.free) == grown and ing.pending is None
    for shape in ((30, 54), (320, 576)):
        for dtype in (np.uint8, np.uint16, np.float32):
            ing.ingest(np.zeros(shape, dtype), None, {}, rep)
    assert ing.allocated == grown == len(ing.free)


# ----------------------------------------------------------------------------- ops 49 and 54 under their plane flags
def raw_plane(H, W, seed):
    """a raw matte as op 58 writes it (byte levels over 255), fp32 [H,W]: a soft blob with noise"""
    return MI.front_ref(MI.mask_ref(soft(seed, (H, W)), H, W), None, 0, 1)


@pytest.mark.parametrize("shape", [(40, 72), (24, 40)])
@pytest.mark.parametrize("radius", [1, 8])
def test_op49_reads_the_plane(shape, radius):
    from live2diff_amd import ops
    H, W = shape
    source, raw = frame16(11, H, W), raw_plane(H, W, 12)
    buf = torch.full((GUARD + H * W + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    for eps in (1.0, 10.0):
        ops.run(ops.frame_matte_edge(source.to(DEV), None, buf[GUARD:GUARD + H * W].view(H, W), H=H, W=W, r=radius, E=MT.edge_E(radius, eps),
                                     plane=dev(raw)))
        got = buf.cpu().numpy()
        assert differ(f"op 49 plane {shape} r {radius} eps {eps}", got[GUARD:-GUARD].reshape(H, W), MT.edge_ref(raw, source, radius, eps)) == 0
        assert np.all(np.isnan(got[:GUARD])) and np.all(np.isnan(got[-GUARD:]))


@pytest.mark.parametrize("shape", [(40, 72), (24, 40)])
def test_op54_reads_the_plane(shape):
    from live2diff_amd import ops
    H, W = shape
    source, raw = frame16(13, H, W), raw_plane(H, W, 14)
    out = torch.full((3, H, W), float("nan"), dtype=torch.float16, device=DEV)
    ops.run(ops.frame_backdrop_blur(source.to(DEV), None, out, H=H, W=W, r=BD.MAX_RADIUS, passes=BD.MAX_PASSES, plane=dev(raw)))
    want = BD.frame_of(BD.blur_ref(source, None, 0, 1, "near", BD.MAX_RADIUS, BD.MAX_PASSES, plane=raw))
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert not np.array_equal(want, BD.frame_of(BD.blur_ref(source, depth16(1, H, W), 0.3, 0.7, "near", BD.MAX_RADIUS, BD.MAX_PASSES)))


# ----------------------------------------------------------------------------- the composites' whole lists
class Slot:
    def __init__(self, source, depth, mask=None):
        self.source, self.depth, self.mask, self.camera = source.to(DEV), dev(depth), mask, None


@pytest.mark.parametrize("combine", ["replace", "and"])
def test_one_list_58_49_57_43_and_47(monkeypatch, combine):
    """`HipMatte.composite` and `HipMatteUp.composite` with a mask, the edge refit, the hold and a blurred backdrop in ONE list
    each, against front_ref -> edge_ref -> hold_ref -> composite_ref(plane=) by hand; 47 at an output size with partial tiles"""
    from live2diff_amd import _lib
    from live2diff_amd.resize import CameraBuffer
    H, W, Ho, Wo = 40, 72, 52, 100
    matte = dict(lo=0.3, hi=0.7, keep="far", feather=2, show=False)
    mi = dict(combine=combine, invert=True)
    edge, hold = dict(radius=2, eps=4.0), MT.check_hold(search=0)
    bd = BD.check_settings("blur", 2, 2)
    rng = np.random.default_rng(21)
    S8, C8 = (rng.integers(0, 256, (Ho, Wo, 3), dtype=np.uint8) for _ in range(2))
    kinds = {v: k for k, v in vars(_lib).items() if k.startswith("OP_")}
    lists, run = [], _lib.OpList.run
    monkeypatch.setattr(_lib.OpList, "run", lambda self, *a, **k: (lists.append([op.kind for op in self._ops]), run(self, *a, **k))[1])

    ing = MI.HipMaskIngest(H, W, device=DEV)
    mt, up = MT.HipMatte(H, W, device=DEV), MT.HipMatteUp(H, W, Ho, Wo, device=DEV)
    hd, hd_up = MT.HipMatteHold(H, W, device=DEV), MT.HipMatteHold(H, W, device=DEV)
    back = BD.HipBackdrop(H, W, device=DEV)
    state = None
    for k in range(3):
        styled, source, depth = frame16(30 + k, H, W), frame16(40 + k, H, W), depth16(50 + k, H, W)
        mask = (soft(60 + k, (30, 54)) * 255).clip(0, 255).astype(np.uint8)
        slot = Slot(source, depth, ing.stage(mask))
        raw = MI.raw_ref(mask, depth, matte, mi, H, W)
        h, state, _ = MT.hold_ref(MT.edge_ref(raw, source, **edge), source, state, init=k == 0, **hold)
        bdrop = BD.stream_ref(bd, None, source, depth, matte, plane=raw)
        want = MT.composite_ref(styled[None], source[None], None, **matte, plane=h[None], backdrop=bdrop[None])[0]
        op, keep = ing.record(slot.mask, slot.depth, matte, mi)
        front = (op, keep, ing.plane)
        del lists[:]
        got = mt.composite(styled.to(DEV), slot, matte, edge=edge, hold=MT.HoldStep(hd, hold, k == 0, False), mask=front,
                           backdrop=back.stream(slot, matte, bd, plane=ing.plane)).copy()
        assert [kinds[x] for x in lists[0]] == ["OP_MASK_INGEST", "OP_FRAME_BACKDROP_BLUR", "OP_FRAME_MATTE_EDGE", "OP_FRAME_MATTE_HOLD",
                                               "OP_FRAME_MATTE"]
        assert differ(f"43, frame {k}", got, want) == 0
        # at the output size: the same held plane sampled bilinearly, over the camera's bytes
        slot.camera = CameraBuffer(dev(C8), (Ho, Wo, "lanczos"))
        del lists[:]
        got = up.composite(dev(S8), slot, matte, edge=edge, hold=MT.HoldStep(hd_up, hold, k == 0, False), mask=front).copy()
        assert [kinds[x] for x in lists[0]] == ["OP_MASK_INGEST", "OP_FRAME_MATTE_EDGE", "OP_FRAME_MATTE_HOLD", "OP_FRAME_MATTE_UP"]
        assert differ(f"47, frame {k}", got, MT.composite_up_ref(S8, C8, None, **matte, plane=h[None])[0]) == 0
        ing.give_back(slot.mask)
    # without edge and hold the composite reads op 58's plane itself; `show` shows it
    shown = mt.composite(styled.to(DEV), slot, dict(matte, feather=0, show=True), mask=front).copy()
    assert np.array_equal(shown[..., 0], np.rint(raw * np.float32(255)).astype(np.uint8)) and np.array_equal(shown[..., 0], shown[..., 2])


# ----------------------------------------------------------------------------- the wrapper on the device
def _setup(N=2):
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    parts = Parts(ucfg, ccfg, H, W, N)
    warm = u8_frames(8, 96, 128, seed=1)
    frames = u8_frames(6, 96, 128, seed=2)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(warmup_masks=None, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, **kw, **more)
        w.set_matte(0.3, 0.7, keep="near", feather=0)
        w.prepare(warm, PROMPT, **({} if warmup_masks is None else {"warmup_masks": warmup_masks}))
        return w

    return wrapper, frames


def cells(seed, shape=(96, 128), cell=16):
    """a binary byte mask of whole cells, so that most pixels of the resampled plane stay exactly 0 or 255"""
    rng = np.random.default_rng(seed)
    small = rng.random((shape[0] // cell, shape[1] // cell)) < 0.5
    return np.kron(small, np.ones((cell, cell), dtype=bool)).astype(np.uint8) * np.uint8(255)


def check_output(tag, got, styled, source, mask):
    """the output against its own frame's mask: the styled bytes where the mask is 255, that frame's source bytes where it is 0,
    and the whole frame against the composite oracle"""
    from live2diff_amd.frame_io import egress_ref
    P = MI.mask_ref(mask, 64, 64)
    assert int((P == 255).sum()) > 300 and int((P == 0).sum()) > 300
    s8, c8 = egress_ref(styled.cpu())[0].numpy(), egress_ref(source.cpu()[None])[0].numpy()
    assert np.array_equal(got[P == 255], s8[P == 255]) and np.array_equal(got[P == 0], c8[P == 0]), tag
    want = MT.composite_ref(styled.cpu(), source.cpu()[None], None, 0.3, 0.7, 0, "near", plane=MI.front_ref(P, None, 0, 1)[None])[0]
    assert differ(tag, got, want) == 0


def test_wrapper_masks_on_device():
    wrapper, frames = _setup()
    masks = [cells(80 + k) for k in range(6)]
    warm_masks = [cells(90 + j) for j in range(8)]
    w, wd, twin = wrapper(warm_masks), wrapper(warm_masks), wrapper()
    assert w.mask_input == MI.DEFAULTS and not w.mask
    # __call__, N = 2: output k is cut by the mask of frame k - 1 (the first by the last warm-up mask); frame 3 brings none.
    # `wd` gets the same masks as device tensors: the same bytes.
    for k in range(6):
        kw = {} if k == 3 else {"mask": masks[k]}
        got, plain = w(frames[k], **kw), twin(frames[k])
        same = wd(frames[k], **({} if k == 3 else {"mask": dev(masks[k])}))
        assert np.array_equal(got, same), k
        m = warm_masks[-1] if k == 0 else masks[k - 1]
        if k == 4:                               # frame 3 had no mask: the ramp alone, the parent's bytes
            assert np.array_equal(got, plain), k
            continue
        check_output(f"call {k}", got, w.stream.prev_image_result, w._matte_line.last.source, m)
        assert not np.array_equal(got, plain), k
    # in steady state the pool does not grow
    grown = w._mask_tap.allocated
    for k in range(4):
        w(frames[k], mask=masks[k])
    assert w._mask_tap.allocated == grown <= 4

    # push / pop with one frame in flight
    wp = wrapper(warm_masks, frame_pipelining=True)
    styled, pop = [], wp.stream.pop

    def keeping():
        x = pop()
        styled.append(x.clone())
        return x

    wp.stream.pop = keeping
    out, sources = [], []
    wp.push(frames[0], mask=masks[0])
    for i in range(4):
        if i + 1 < 4:
            wp.push(frames[i + 1], mask=masks[i + 1])
        out.append(wp.pop().copy())
        sources.append(wp._matte_line.last.source.clone())
    torch.cuda.synchronize()
    for i, got in enumerate(out):
        check_output(f"push / pop {i}", got, styled[i], sources[i], warm_masks[-1] if i == 0 else masks[i - 1])
    assert wp._mask_tap.allocated <= 5
