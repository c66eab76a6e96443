"""-m gpu: L2D_OP_FRAME_STEADY (csrc/steady.hip) against `steady.steady_ref`, bit for bit on the fp16 frame and on the byte state,
frame by frame over the sequences of tests/test_steady_cpu.py; the state inside guarded, poisoned buffers; the steady frame
through the outlets (egress, matte, JPEG encoder); and `set_steady` on the wrapper with small native components against the
host route."""
import numpy as np
import pytest
import torch

from test_steady_cpu import HI, K, LO, RADII, STRENGTH, bits, oracle, sequence

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (8, 8) smaller than the halo of every radius; (24, 40) no multiple of the 16 x 64 tile, the edge 8-pixel group outside the image;
# (40, 72) and (48, 136) several tiles on both axes with a partial last one; (64, 64) whole tiles
SHAPES = [(8, 8), (24, 40), (40, 72), (48, 136), (64, 64)]


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


def run_sequence(H, W, r, **kw):
    """`HipSteady` over the sequence against the oracle, frame by frame: the number of differing values"""
    from live2diff_amd import steady as SD
    sources, styled = sequence(H, W)
    outs, states = oracle(H, W, r, **kw)
    settings = dict(lo=kw.get("lo", LO), hi=kw.get("hi", HI), strength=kw.get("strength", STRENGTH), radius=r, show=kw.get("show", False))
    st = SD.HipSteady(H, W, device=DEV)
    n = 0
    for k in range(K):
        out = st.steady(dev(styled[k]), dev(sources[k]), settings, init=k == 0)
        torch.cuda.synchronize()
        frame, by = st.state
        n += differ(f"{(H, W)} r={r} {kw} frame {k}: output", out.cpu().numpy(), outs[k])
        n += differ(f"{(H, W)} r={r} {kw} frame {k}: state frame", frame[0].cpu().numpy(), states[k][0])
        n += differ(f"{(H, W)} r={r} {kw} frame {k}: state bytes", by.cpu().numpy(), states[k][1])
    return n


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_steady_ref(shape, r):
    assert run_sequence(*shape, r) == 0


def test_kernel_equals_steady_ref_hard_and_show():
    assert run_sequence(40, 72, 3, lo=4, hi=4) == 0                       # a step: t = dbar >= lo
    assert run_sequence(40, 72, 0, lo=4, hi=4, strength=1.0) == 0
    assert run_sequence(48, 136, 3, show=True) == 0                       # the picture of w; the state stays the blend
    assert run_sequence(24, 40, 0, show=True) == 0
    outs, states = oracle(48, 136, 3, show=True)
    assert not np.array_equal(outs[1][0], states[1][0]) and np.array_equal(outs[0][0], states[0][0])


@pytest.mark.parametrize("shape,r", [((24, 40), 0), ((40, 72), 8)])
def test_state_needs_no_zeroing_and_stays_in_bounds(shape, r):
    """both (out, bytes) records live inside larger buffers, NaN-filled and 0xA5-filled: three frames from `init` on equal the
    oracle, and every guard element before and behind the records is as it was"""
    from live2diff_amd import steady as SD
    H, W = shape
    n, G = 3 * H * W, 4096                                                # (G elements: the records stay 16-byte aligned)
    halves = torch.full((5 * G + 2 * n,), float("nan"), dtype=torch.float16, device=DEV)
    raw = torch.full((5 * G + 2 * n,), 0xA5, dtype=torch.uint8, device=DEV)
    at = [2 * G, 3 * G + n]
    records = [(halves[o:o + n].view(1, 3, H, W), raw[o:o + n].view(3, H, W)) for o in at]
    st = SD.HipSteady(H, W, device=DEV, records=records)
    sources, styled = sequence(H, W)
    outs, states = oracle(H, W, r)
    settings = dict(lo=LO, hi=HI, strength=STRENGTH, radius=r, show=False)
    bad = 0
    for k in range(3):
        out = st.steady(dev(styled[k]), dev(sources[k]), settings, init=k == 0)
        torch.cuda.synchronize()
        bad += differ(f"frame {k}: output", out.cpu().numpy(), outs[k])
        bad += differ(f"frame {k}: state bytes", st.state[1].cpu().numpy(), states[k][1])
    assert bad == 0
    h, b = halves.cpu().numpy(), raw.cpu().numpy()
    inside = np.zeros(5 * G + 2 * n, dtype=bool)
    for o in at:
        inside[o:o + n] = True
    assert np.isnan(h[~inside]).all() and (b[~inside] == 0xA5).all()
    assert not np.isnan(h[inside]).any()


def test_steady_frame_through_the_outlets():
    """op 35, op 43 and the JPEG encoder consume the steady frame unchanged"""
    from live2diff_amd import jpeg, ops
    from live2diff_amd import steady as SD
    from live2diff_amd.frame_io import egress_ref
    from live2diff_amd.jpeg_io import HipJpegEncoder
    from live2diff_amd.matte import composite_ref, matte_params
    H, W = 64, 128
    sources, styled = sequence(H, W)
    settings = dict(lo=LO, hi=HI, strength=STRENGTH, radius=2, show=False)
    st = SD.HipSteady(H, W, device=DEV)
    st.steady(dev(styled[0]), dev(sources[0]), settings, init=True)
    out = st.steady(dev(styled[1]), dev(sources[1]), settings)
    outs, _ = oracle(H, W, 2)
    want = torch.from_numpy(np.array(outs[1]))
    assert not np.array_equal(outs[1][0], styled[1])
    u8 = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
    ops.run(ops.frame_egress(out, u8, B=1, H=H, W=W))
    assert np.array_equal(u8.cpu().numpy(), egress_ref(want).numpy())
    depth = torch.linspace(-1, 1, H * W).view(1, H, W).half()
    lo32, inv32, hard = matte_params(0.3, 0.7)
    src16 = torch.from_numpy(np.array(sources[1]))[None]
    ops.run(ops.frame_matte(out, src16.to(DEV), depth.to(DEV), u8, B=1, H=H, W=W, lo32=lo32, inv32=inv32, hard=hard, r=3))
    assert np.array_equal(u8.cpu().numpy(), composite_ref(want, src16, depth, 0.3, 0.7, feather=3))
    enc = HipJpegEncoder(H, W, 75, device=DEV)
    assert enc.encode(out[0]) == jpeg.encode_ref(egress_ref(want)[0].numpy(), 75)


# ----------------------------------------------------------------------------- the wrapper on the device
FRAME_OPS = ("OP_FRAME_EGRESS", "OP_FRAME_MATTE", "OP_FRAME_MOMENTS", "OP_COLOR_LOCK", "OP_FRAME_RESIZE", "OP_FRAME_MATTE_UP",
             "OP_FRAME_STEADY")


def test_wrapper_steady_on_device(monkeypatch):
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd import _lib
    from live2diff_amd import color_lock as CL
    from live2diff_amd import steady as SD
    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.frame_io import egress_ref
    from live2diff_amd.matte import composite_ref
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    N = 2
    parts = Parts(ucfg, ccfg, H, W, N)
    warm = u8_frames(8, 96, 128, seed=1)
    # a camera that holds most of the picture still: one frame of `u8_frames`, a band of fresh content that moves along
    fresh = u8_frames(6, 96, 128, seed=2)
    frames = np.stack([fresh[0]] * 6)
    for k in range(1, 6):
        frames[k, :, 16 * k:16 * k + 32] = fresh[k, :, 16 * k:16 * k + 32]
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)
    SET = dict(lo=2.0, hi=10.0, strength=0.8, radius=2, show=False)

    kinds = {v: k for k, v in vars(_lib).items() if k.startswith("OP_")}
    ran, run = [], _lib.OpList.run

    def recording(self, *a, **k):
        ran.extend(kinds[op.kind] for op in self._ops if kinds[op.kind] in FRAME_OPS)
        return run(self, *a, **k)

    monkeypatch.setattr(_lib.OpList, "run", recording)

    def wrapper(steady=False, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, **kw, **more)
        if steady:
            w.set_steady(2, 10, strength=0.8, radius=2)
        w.prepare(warm, PROMPT)
        return w

    twin, w = wrapper(), wrapper(True)
    assert w.steady == SET and twin.steady is None
    state, got = None, []
    for t, f in enumerate(frames):
        del ran[:]
        out, plain = w(f), twin(f)
        assert ran == ["OP_FRAME_STEADY", "OP_FRAME_EGRESS", "OP_FRAME_EGRESS"], ran
        want, state = SD.steady_ref(w.stream.prev_image_result, w._matte_line.last.source, state, init=t == 0, **SET)
        assert out.dtype == np.uint8 and out.shape == (H, W, 3)
        assert np.array_equal(out, egress_ref(torch.from_numpy(want))[0].numpy()), t
        dev_state = w._steady_dev.state
        assert np.array_equal(bits(dev_state[0][0].cpu().numpy()), bits(state[0])) and np.array_equal(dev_state[1].cpu().numpy(), state[1])
        # the init frame passes (so does, in all likelihood, the next: its source follows the unrelated last warm-up frame)
        assert np.array_equal(out, plain) if t == 0 else t == 1 or not np.array_equal(out, plain), t
        got.append(out)
    # behind a colour lock to "source" and in front of a matte
    w.set_color_lock("source")
    w.set_matte(0.3, 0.7, feather=2)
    for f in frames[:3]:
        del ran[:]
        out = w(f)
        twin(f)
        assert ran[:4] == ["OP_FRAME_MOMENTS", "OP_COLOR_LOCK", "OP_FRAME_STEADY", "OP_FRAME_MATTE"] and ran[4:] == ["OP_FRAME_EGRESS"], ran
        slot = w._matte_line.last
        locked, _ = CL.lock_ref(w.stream.prev_image_result, None, mode="source", source=slot.source)
        want, state = SD.steady_ref(locked, slot.source, state, **SET)
        assert np.array_equal(out, composite_ref(torch.from_numpy(want), slot.source[None], slot.depth[None], 0.3, 0.7, feather=2)[0])
    # cleared: no launch of it is left, and without the lock and the matte the outputs are the twin's again
    w.clear_steady()
    assert w.steady is None and w._steady_dev is None and w._matte_line is not None
    del ran[:]
    w(frames[3])
    twin(frames[3])
    assert "OP_FRAME_STEADY" not in ran and ran[:3] == ["OP_FRAME_MOMENTS", "OP_COLOR_LOCK", "OP_FRAME_MATTE"], ran
    w.clear_matte()
    w.clear_color_lock()
    assert w._matte_line is None and w.stream.matte_tap is None
    for f in frames[4:6]:
        del ran[:]
        assert np.array_equal(w(f), twin(f))
        assert ran == ["OP_FRAME_EGRESS", "OP_FRAME_EGRESS"], ran
    # push / pop: the same bytes as __call__ gave
    wp = wrapper(True, frame_pipelining=True)
    outs = []
    wp.push(frames[0])
    for i in range(len(frames)):
        if i + 1 < len(frames):
            wp.push(frames[i + 1])
        outs.append(wp.pop())
    torch.cuda.synchronize()
    for i in range(len(frames)):
        assert np.array_equal(outs[i], got[i]), f"push / pop frame {i} differs from __call__"
