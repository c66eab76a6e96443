"""-m gpu: L2D_OP_FRAME_MOTION and L2D_OP_FRAME_STEADY_FOLLOW (csrc/steady_follow.hip) against `steady.motion_ref` and
`steady.follow_ref`, bit for bit on the field, the fp16 frame and the byte state, frame by frame over the sequences of
tests/test_steady_follow_cpu.py (a pan, a still stretch, a hard cut); a still sequence against op 48; the records and the field
inside guarded, poisoned buffers; two runs with the same bits; the followed frame through the outlets; and `set_steady_follow`
on the wrapper with small native components against the host route."""
import numpy as np
import pytest
import torch

from test_steady_cpu import bits
from test_steady_follow_cpu import HI, K, LO, STRENGTH, oracle, sequence

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (8, 8) one block, smaller than every window and halo; (20, 40) a partial block row; (24, 40) no multiple of the 16 x 64 tile and a
# strip of five blocks; (40, 72) and (48, 136) two strips (9 and 17 blocks: a strip of one) and several tiles; (64, 64) whole ones
SHAPES = [(8, 8), (20, 40), (24, 40), (40, 72), (48, 136), (64, 64)]


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


def settings_of(r, kw):
    return dict(lo=kw.get("lo", LO), hi=kw.get("hi", HI), strength=kw.get("strength", STRENGTH), radius=r, show=kw.get("show", False))


def run_sequence(H, W, R, bias, r, st=None, frames=K, **kw):
    """`HipSteady` with `follow=` over the sequence against the oracle, frame by frame: the number of differing values"""
    from live2diff_amd import steady as SD
    sources, styled = sequence(H, W)
    outs, states, fields = oracle(H, W, R, bias, r, **kw)
    st = SD.HipSteady(H, W, device=DEV) if st is None else st
    follow, n = dict(search=R, bias=bias), 0
    for k in range(frames):
        out = st.steady(dev(styled[k]), dev(sources[k]), settings_of(r, kw), init=k == 0, follow=follow)
        torch.cuda.synchronize()
        frame, by = st.state
        tag = f"{(H, W)} R={R} bias={bias} r={r} {kw} frame {k}"
        if k:
            n += differ(f"{tag}: field", st.field.cpu().numpy(), fields[k])
        n += differ(f"{tag}: output", out.cpu().numpy(), outs[k])
        n += differ(f"{tag}: state frame", frame[0].cpu().numpy(), states[k][0])
        n += differ(f"{tag}: state bytes", by.cpu().numpy(), states[k][1])
    return n


@pytest.mark.parametrize("bias", [0, 256])
@pytest.mark.parametrize("r", [0, 2, 8])
@pytest.mark.parametrize("R", [1, 4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_follow_ref(shape, R, r, bias):
    assert run_sequence(*shape, R, bias, r) == 0


def test_kernels_equal_follow_ref_hard_and_show():
    assert run_sequence(40, 72, 4, 256, 3, lo=4, hi=4) == 0                  # a step: t = dbar >= lo
    assert run_sequence(40, 72, 8, 0, 0, lo=4, hi=4, strength=1.0) == 0
    assert run_sequence(48, 136, 4, 256, 3, show=True) == 0                  # the picture of w; the state stays the blend
    assert run_sequence(24, 40, 1, 256, 0, show=True) == 0
    outs, states, fields = oracle(48, 136, 4, 256, 3, show=True)
    assert not np.array_equal(outs[1][0], states[1][0]) and np.array_equal(outs[0][0], states[0][0]) and fields[1].any()


def test_still_sequence_equals_op_48():
    """one source frame over and over: the field is zero, and every output, state frame and state byte is op 48's"""
    from live2diff_amd import steady as SD
    H, W = 40, 72
    sources, styled = sequence(H, W)
    for r in (0, 2, 8):
        settings = settings_of(r, {})
        a, b = SD.HipSteady(H, W, device=DEV), SD.HipSteady(H, W, device=DEV)
        bad = 0
        for k in range(4):
            fo = a.steady(dev(styled[k]), dev(sources[0]), settings, init=k == 0, follow=dict(search=8, bias=256))
            so = b.steady(dev(styled[k]), dev(sources[0]), settings, init=k == 0)
            torch.cuda.synchronize()
            bad += differ(f"r={r} frame {k}: output", fo.cpu().numpy(), so.cpu().numpy())
            bad += differ(f"r={r} frame {k}: state frame", a.state[0].cpu().numpy(), b.state[0].cpu().numpy())
            bad += differ(f"r={r} frame {k}: state bytes", a.state[1].cpu().numpy(), b.state[1].cpu().numpy())
            assert k == 0 or not a.field.cpu().numpy().any()
            assert k == 0 or not np.array_equal(fo.cpu().numpy()[0], styled[k])
        assert bad == 0 and b.field is None


@pytest.mark.parametrize("shape,R,r", [((24, 40), 8, 2), ((40, 72), 8, 8)])
def test_state_and_field_need_no_zeroing_and_stay_in_bounds(shape, R, r):
    """both (out, bytes) records and the field live inside larger buffers, NaN-filled and 0xA5-filled: three frames from `init` on
    equal the oracle, and every guard element before and behind them is as it was"""
    from live2diff_amd import steady as SD
    H, W = shape
    n, G = 3 * H * W, 4096                                                # (G elements: the records stay 16-byte aligned)
    halves = torch.full((5 * G + 2 * n,), float("nan"), dtype=torch.float16, device=DEV)
    raw = torch.full((5 * G + 2 * n,), 0xA5, dtype=torch.uint8, device=DEV)
    at = [2 * G, 3 * G + n]
    records = [(halves[o:o + n].view(1, 3, H, W), raw[o:o + n].view(3, H, W)) for o in at]
    Hb, Wb = (H + 7) // 8, W // 8
    nf, fat = 2 * Hb * Wb, G + 1                                          # (the field takes any alignment: an odd address)
    vec = torch.full((2 * G + nf + 1,), -91, dtype=torch.int8, device=DEV)          # 0xA5 as int8
    st = SD.HipSteady(H, W, device=DEV, records=records, field=vec[fat:fat + nf].view(Hb, Wb, 2))
    assert run_sequence(H, W, R, 256, r, st=st, frames=3) == 0
    h, b, v = halves.cpu().numpy(), raw.cpu().numpy(), vec.cpu().numpy()
    inside = np.zeros(5 * G + 2 * n, dtype=bool)
    for o in at:
        inside[o:o + n] = True
    assert np.isnan(h[~inside]).all() and (b[~inside] == 0xA5).all()
    assert not np.isnan(h[inside]).any()
    assert (v[:fat] == -91).all() and (v[fat + nf:] == -91).all() and np.abs(v[fat:fat + nf].astype(int)).max() <= R


def test_two_runs_give_the_same_bits():
    from live2diff_amd import steady as SD
    H, W = 48, 136
    sources, styled = sequence(H, W)
    settings, follow = settings_of(2, {}), dict(search=8, bias=0)
    runs = []
    for _ in range(2):
        st, got = SD.HipSteady(H, W, device=DEV), []
        for k in range(K):
            out = st.steady(dev(styled[k]), dev(sources[k]), settings, init=k == 0, follow=follow)
            got.append((out.cpu().numpy().copy(), st.state[1].cpu().numpy().copy(), None if k == 0 else st.field.cpu().numpy().copy()))
        runs.append(got)
    for k in range(K):
        assert np.array_equal(bits(runs[0][k][0]), bits(runs[1][k][0])) and np.array_equal(runs[0][k][1], runs[1][k][1])
        assert k == 0 or np.array_equal(runs[0][k][2], runs[1][k][2])


def test_followed_frame_through_the_outlets():
    """op 35, op 43 and the JPEG encoder consume the followed frame unchanged"""
    from live2diff_amd import jpeg, ops
    from live2diff_amd import steady as SD
    from live2diff_amd.frame_io import egress_ref
    from live2diff_amd.jpeg_io import HipJpegEncoder
    from live2diff_amd.matte import composite_ref, matte_params
    H, W = 64, 128
    sources, styled = sequence(H, W)
    settings, follow = settings_of(2, {}), dict(search=4, bias=256)
    st = SD.HipSteady(H, W, device=DEV)
    st.steady(dev(styled[0]), dev(sources[0]), settings, init=True, follow=follow)
    out = st.steady(dev(styled[1]), dev(sources[1]), settings, follow=follow)
    outs, _, fields = oracle(H, W, 4, 256, 2)
    want = torch.from_numpy(np.array(outs[1]))
    assert not np.array_equal(outs[1][0], styled[1]) and fields[1].any()
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
FRAME_OPS = ("OP_FRAME_EGRESS", "OP_FRAME_STEADY", "OP_FRAME_MOTION", "OP_FRAME_STEADY_FOLLOW")


def test_wrapper_follow_on_device(monkeypatch):
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd import _lib
    from live2diff_amd import steady as SD
    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.frame_io import egress_ref
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    parts = Parts(ucfg, ccfg, H, W, 2)
    warm = u8_frames(8, H, W, seed=1)
    # a camera that pans by (2, -3) per frame over one picture of 4 x 4 cells, at the stream's own size
    big = np.kron(u8_frames(1, 32, 32, seed=2)[0], np.ones((4, 4, 1), dtype=np.uint8))
    frames = np.stack([big[20 + 2 * k:20 + 2 * k + H, 30 - 3 * k:30 - 3 * k + W] for k in range(6)])
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)
    SET, FOLLOW = dict(lo=2.0, hi=10.0, strength=0.8, radius=2, show=False), dict(search=4, bias=256)

    kinds = {v: k for k, v in vars(_lib).items() if k.startswith("OP_")}
    ran, run = [], _lib.OpList.run

    def recording(self, *a, **k):
        ran.extend(kinds[op.kind] for op in self._ops if kinds[op.kind] in FRAME_OPS)
        return run(self, *a, **k)

    monkeypatch.setattr(_lib.OpList, "run", recording)
    torch.manual_seed(0)                         # `prepare` draws init_noise and the warm-up re-noising from the global generators
    w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, steady=dict(), steady_follow=dict(), **kw)
    w.prepare(warm, PROMPT)
    assert w.steady == SET and w.steady_follow == FOLLOW
    state, vectors = None, 0
    for t, f in enumerate(frames):
        if t == 4:
            w.clear_steady_follow()              # op 48 again, from the same state
        del ran[:]
        out = w(f)
        follow = t not in (0, 4)
        assert ran == (["OP_FRAME_MOTION", "OP_FRAME_STEADY_FOLLOW"] if follow else ["OP_FRAME_STEADY"]) + ["OP_FRAME_EGRESS"], (t, ran)
        source = w._matte_line.last.source
        if t == 4:
            want, state = SD.steady_ref(w.stream.prev_image_result, source, state, **SET)
        else:
            want, state, field = SD.follow_ref(w.stream.prev_image_result, source, state, init=t == 0, **FOLLOW, **SET)
            if follow:
                assert np.array_equal(w._steady_dev.field.cpu().numpy(), field), t
                vectors += bool(field.any())
        if t == 4:
            w.set_steady_follow()
        assert out.dtype == np.uint8 and out.shape == (H, W, 3)
        assert np.array_equal(out, egress_ref(torch.from_numpy(want))[0].numpy()), t
        dev_state = w._steady_dev.state
        assert np.array_equal(bits(dev_state[0][0].cpu().numpy()), bits(state[0])) and np.array_equal(dev_state[1].cpu().numpy(), state[1])
    assert vectors >= 2                          # the pan is seen (frame 1 follows the unrelated last warm-up frame)
