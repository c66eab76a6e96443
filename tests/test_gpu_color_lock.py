"""-m gpu: L2D_OP_FRAME_MOMENTS + L2D_OP_COLOR_LOCK (csrc/colorlock.hip) against `color_lock.lock_ref`, bit for bit on the fp16 frame,
the fp64 state record and the fp32 coefficient record; the partial sums; the locked frame through the outlets (egress, matte, JPEG
encoder); and `set_color_lock` on the wrapper with small native components against the host route."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

BLOCK = 4096                                    # ops.COLOR_LOCK_BLOCK_PIXELS (asserted below)
# (8, 8) smaller than a block of either kernel; (24, 40) not a whole number of lane groups per block; (65, 64) one full moments
# block and a 64-pixel tail; (64, 128) two moments blocks, four blocks of the lock kernel
SHAPES = [(8, 8), (24, 40), ((BLOCK + 64) // 64, 64), (64, 128)]
KINDS = ["gauss", "plus_one", "minus_one", "beyond", "near_flat"]
STRENGTHS = [1.0, 0.37]


@functools.lru_cache(maxsize=None)
def gauss(H, W, seed):
    """activation-like: N(offset, sigma) per channel, sigma 0.1 .. 0.25, offset within +-0.3"""
    rng = np.random.default_rng(seed * 100003 + H * 1009 + W)
    x = (rng.standard_normal((3, H, W)) * rng.uniform(0.1, 0.25, (3, 1, 1)) + rng.uniform(-0.3, 0.3, (3, 1, 1))).astype(np.float16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def frame(kind, H, W):
    if kind == "gauss":
        return gauss(H, W, 1)
    if kind == "plus_one":                      # S2 at its maximum
        x = np.full((3, H, W), 1.0, dtype=np.float16)
    elif kind == "minus_one":                   # flat: variance 0
        x = np.full((3, H, W), -1.0, dtype=np.float16)
    elif kind == "beyond":                      # values outside [-1, 1], fp16 subnormals, both zeros
        rng = np.random.default_rng(H * 31 + W)
        x = (rng.standard_normal((3, H, W)) * 0.9).astype(np.float16)
        plant = np.array([-1.0, 1.0, 0.0, -0.0, 1.5, -2.0, 6e-8, -6e-8, 3e-5, 0.99951171875, 7.0, -60000.0], dtype=np.float16)
        x.reshape(3, -1)[:, 3:3 + len(plant)] = plant
        x.reshape(3, -1)[:, -len(plant):] = plant[::-1]
    else:                                       # near-flat: a lively target drives the gain into its clamp at 4
        rng = np.random.default_rng(H * 37 + W)
        x = (0.1 + 0.004 * rng.standard_normal((3, H, W))).astype(np.float16)
    x.setflags(write=False)
    return x


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def dev16(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def read(lock):
    torch.cuda.synchronize()
    return lock.out.cpu().numpy(), lock.state.cpu().numpy(), lock.coef.cpu().numpy()


def same(tag, got, want):
    """every record bit for bit; prints what differs before it asserts"""
    ok = True
    for name, g, w in zip(("frame", "state", "coefficients"), got, want):
        n = int((bits(g) != bits(w)).sum())
        if n:
            ok = False
            print(f"{tag}: {name}: {n} of {w.size} values differ; got {g.reshape(-1)[:6]} want {w.reshape(-1)[:6]}")
    return ok


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_lock_ref(shape, kind):
    from live2diff_amd import color_lock as CL
    from live2diff_amd import ops
    assert ops.COLOR_LOCK_BLOCK_PIXELS == BLOCK
    H, W = shape
    x, target = frame(kind, H, W), gauss(H, W, 2)
    xd, td = dev16(x), dev16(target)
    lock = CL.HipColorLock(H, W, device=DEV)
    ok = True
    for a in STRENGTHS:
        # "source": the target is the second tensor of the moments launch
        s = dict(mode="source", strength=a, rate=0.1)
        lock.lock(xd, td, s)
        want = CL.lock_ref(x, None, mode="source", strength=a, source=target, with_coefficients=True)
        ok &= same(f"{shape} {kind} source a={a}", read(lock), want)
        if kind == "near_flat" and a == 1.0:
            assert np.array_equal(want[2][:, 0], np.full(3, 4.0, np.float32))
        if kind == "minus_one":
            assert np.array_equal(want[2][:, 0], np.ones(3, np.float32))
        # a frozen reference: the state goes through both records unchanged
        ref = CL.moments_ref(target)
        lock.load_state(ref)
        s = dict(mode="image", strength=a, rate=0.1)
        for k in range(2):
            lock.lock(xd, None, s)
            want = CL.lock_ref(x, ref, mode="image", strength=a, with_coefficients=True)
            ok &= same(f"{shape} {kind} image a={a} call {k}", read(lock), want)
        # "ema": three successive frames through the ping-pong, the first one copies
        s = dict(mode="ema", strength=a, rate=0.3)
        state = None
        for k, f in enumerate((gauss(H, W, 3), x, gauss(H, W, 4))):
            lock.lock(dev16(f), None, s, init=k == 0)
            want = CL.lock_ref(f, state, mode="ema", strength=a, rate=0.3, init=k == 0, with_coefficients=True)
            state = want[1]
            ok &= same(f"{shape} {kind} ema a={a} frame {k}", read(lock), want)
    assert ok


@pytest.mark.parametrize("shape", SHAPES)
def test_partials_are_exact_and_need_no_zeroing(shape):
    """every partial is written by every launch: poisoned buffers give the same records, two runs agree bit for bit, and the
    partials are the per-block integer sums of the egress bytes"""
    from live2diff_amd import color_lock as CL
    from live2diff_amd.frame_io import egress_ref
    H, W = shape
    x, target = frame("beyond", H, W), frame("plus_one", H, W)
    xd, td = dev16(x), dev16(target)
    s = dict(mode="source", strength=1.0, rate=0.1)
    runs = []
    for fill in (0, -1, -1):                                                   # (-1: 0xFF in every byte)
        lock = CL.HipColorLock(H, W, device=DEV)
        lock.partials.fill_(fill)
        lock.out.fill_(float("nan"))
        lock.lock(xd, td, s)
        runs.append(read(lock) + (lock.partials.cpu().numpy().astype(np.int64) & 0xFFFFFFFF,))
    for r in runs[1:]:
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(r, runs[0]))
    nblk = lock.nblk
    assert nblk == -(-H * W // BLOCK)
    for t, f in enumerate((x, target)):
        b = egress_ref(torch.from_numpy(np.array(f)))[0].numpy().astype(np.int64).reshape(-1, 3)
        for k in range(nblk):
            blk = b[k * BLOCK:(k + 1) * BLOCK]
            assert np.array_equal(runs[0][3][t, k], np.concatenate([blk.sum(0), (blk * blk).sum(0)])), (t, k)
    S1, S2, _ = CL.sums_ref(target)
    assert np.array_equal(runs[0][3][1].sum(0), np.concatenate([S1, S2])) and int(S2[0]) == 65025 * H * W


def test_locked_frame_through_the_outlets():
    """op 35, op 43 and the JPEG encoder consume the locked frame unchanged"""
    from live2diff_amd import color_lock as CL
    from live2diff_amd import jpeg, ops
    from live2diff_amd.frame_io import egress_ref
    from live2diff_amd.jpeg_io import HipJpegEncoder
    from live2diff_amd.matte import composite_ref, matte_params
    H, W = 64, 128
    x, source = frame("gauss", H, W), gauss(H, W, 2)
    lock = CL.HipColorLock(H, W, device=DEV)
    out = lock.lock(dev16(x), dev16(source), dict(mode="source", strength=1.0, rate=0.1))
    want = torch.from_numpy(CL.lock_ref(x, None, mode="source", source=source)[0])
    u8 = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
    ops.run(ops.frame_egress(out, u8, B=1, H=H, W=W))
    assert np.array_equal(u8.cpu().numpy(), egress_ref(want).numpy())
    depth = torch.linspace(-1, 1, H * W).view(1, H, W).half()
    lo32, inv32, hard = matte_params(0.3, 0.7)
    src16 = torch.from_numpy(np.array(source))[None]
    ops.run(ops.frame_matte(out, src16.to(DEV), depth.to(DEV), u8, B=1, H=H, W=W, lo32=lo32, inv32=inv32, hard=hard, r=3))
    assert np.array_equal(u8.cpu().numpy(), composite_ref(want, src16, depth, 0.3, 0.7, feather=3))
    enc = HipJpegEncoder(H, W, 75, device=DEV)
    assert enc.encode(out[0]) == jpeg.encode_ref(egress_ref(want)[0].numpy(), 75)


# ----------------------------------------------------------------------------- the wrapper on the device
def test_wrapper_color_lock_on_device():
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd import color_lock as CL
    from live2diff_amd import jpeg
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
    frames = u8_frames(6, 96, 128, seed=2)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(lock=None, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, **kw, **more)
        if lock is not None:
            w.set_color_lock(*lock)
        w.prepare(warm, PROMPT)
        return w

    def host(w, **kw):
        """the CPU route's frame for the output the stream made last"""
        locked, state = CL.lock_ref(w.stream.prev_image_result, **kw)
        return torch.from_numpy(locked), state

    twin, w = wrapper(), wrapper(("source", 0.8))
    # "source": the delay line's slot is the target; the device never reads anything back
    for t, f in enumerate(frames[:3]):
        got, plain = w(f), twin(f)
        slot = w._matte_line.last
        want, _ = host(w, mode="source", strength=0.8, source=slot.source)
        assert got.dtype == np.uint8 and got.shape == (H, W, 3)
        assert np.array_equal(got, egress_ref(want)[0].numpy()), t
        assert not np.array_equal(got, plain)
    # "ema" over a handful of frames, the state followed on the host; as u8, jpeg and pt
    w.set_color_lock("ema", 1.0, 0.3)
    assert w._matte_line is None and w.stream.matte_tap is None
    state = None
    for t, (f, ot) in enumerate(zip(frames, ("u8", "u8", "jpeg", "pt", "u8", "u8"))):
        w.output_type = ot
        got = w(f)
        twin(f)
        want, state = host(w, state=state, mode="ema", rate=0.3, init=t == 0)
        assert np.array_equal(bits(w._lock_dev.state.cpu().numpy()), bits(state)), t
        if ot == "u8":
            assert np.array_equal(got, egress_ref(want)[0].numpy()), t
        elif ot == "jpeg":
            assert got == jpeg.encode_ref(egress_ref(want)[0].numpy(), w.jpeg_quality)
        else:
            assert torch.equal(got, (want / 2 + 0.5).clamp(0, 1)[0])
    w.output_type = "u8"
    # a reference image, under a matte: locked before the composite
    w.set_color_lock(frames[5], 0.6)
    ref = w._lock_ref
    assert ref.shape == (3, 2) and np.all(ref[:, 1] > 0)
    w.set_matte(0.3, 0.7, feather=2)
    for f in frames[:2]:                                                   # (the line starts with the first of them)
        got = w(f)
        twin(f)
        slot = w._matte_line.last
        want, _ = host(w, state=ref, mode="image", strength=0.6)
        assert np.array_equal(got, composite_ref(want, slot.source[None], slot.depth[None], 0.3, 0.7, feather=2)[0])
        assert np.array_equal(bits(w._lock_dev.state.cpu().numpy()), bits(ref))
    # cleared: the outputs of a wrapper that never had a lock
    w.clear_matte()
    w.clear_color_lock()
    assert w.color_lock is None and w._matte_line is None and w.stream.matte_tap is None
    for f in frames[2:4]:
        assert np.array_equal(w(f), twin(f))
