"""-m gpu: L2D_OP_FRAME_MATTE (csrc/matte.hip) against `matte.composite_ref` on every byte, and `set_matte` on the wrapper with small
native components: an all-near matte is the twin wrapper's output, an all-far one the ingested source frame N - 1 calls earlier
(`__call__` and push / pop), a soft one `composite_ref` of the stream's output and the delay line's slot."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (1, 16, 16) smaller than a tile, r = 8 clamps everywhere; (3, 40, 72) a batch, neither axis a whole number of tiles;
# (1, 24, 136) wide and short
SHAPES = [(1, 16, 16), (3, 40, 72), (1, 24, 136)]
RAMPS = {"soft": (0.3, 0.7), "hard": (0.5, 0.5)}


@functools.lru_cache(maxsize=None)
def data(B, H, W):
    """frames N(0, 0.7) with planted -1, +1, 0, values beyond +-1 and fp16 subnormals; depth N(0, 0.6) clipped, with planted values
    at lo_d and hi_d of both ramps (-0.4, 0.4, 0 as fp16), -1 and +1"""
    g = torch.Generator().manual_seed(100 * H + W)
    styled = (torch.randn(B, 3, H, W, generator=g) * 0.7).half()
    source = (torch.randn(B, 3, H, W, generator=g) * 0.7).half()
    depth = (torch.randn(B, H, W, generator=g) * 0.6).clamp(-1, 1).half()
    plant = torch.tensor([-1.0, 1.0, 0.0, 1.5, -2.0, 6e-8, -6e-8, 3e-5, 0.99951171875, -0.0], dtype=torch.float16)
    for t, off in ((styled, 3), (source, 7)):
        for b in range(B):
            for c in range(3):
                t[b, c].view(-1)[off + c:off + c + len(plant)] = plant
                t[b, c].view(-1)[-len(plant):] = plant.flip(0)
    dplant = torch.tensor([-0.4, 0.4, 0.0, -1.0, 1.0, -0.39990234375, 0.400146484375, 6e-8, -6e-8], dtype=torch.float16)
    for b in range(B):
        depth[b].view(-1)[5:5 + len(dplant)] = dplant
        depth[b, -1, -len(dplant):] = dplant                     # the bottom right corner: inside every clamped window there
        depth[b, 0, 0], depth[b, 0, -1], depth[b, -1, 0] = 1.0, -1.0, 0.4
    return styled, source, depth


def launch(styled, source, depth, out, lo, hi, r, keep, show=False, depth_stride=None):
    from live2diff_amd import ops
    from live2diff_amd.matte import matte_params
    B, _, H, W = styled.shape
    lo32, inv32, hard = matte_params(lo, hi)
    ops.run(ops.frame_matte(styled, source, depth, out, B=B, H=H, W=W, lo32=lo32, inv32=inv32, hard=hard, far=keep == "far", show=show,
                            r=r, depth_stride=depth_stride))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def report(tag, got, want):
    n = int((got != want).sum())
    print(f"{tag}: {n} of {want.size} bytes differ" + (f", max |diff| {int(np.abs(got.astype(int) - want.astype(int)).max())}" if n else ""))
    return n


@pytest.mark.parametrize("ramp", list(RAMPS))
@pytest.mark.parametrize("keep", ["near", "far"])
@pytest.mark.parametrize("r", [0, 1, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_composite_ref(shape, r, keep, ramp):
    from live2diff_amd.matte import composite_ref
    styled, source, depth = data(*shape)
    lo, hi = RAMPS[ramp]
    B, H, W = shape
    want = composite_ref(styled, source, depth, lo, hi, feather=r, keep=keep)
    out = torch.full((B, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    got = launch(styled.to(DEV), source.to(DEV), depth.to(DEV), out, lo, hi, r, keep)
    assert report(f"{shape} r {r} {keep} {ramp}", got, want) == 0


@pytest.mark.parametrize("r", [0, 8])
def test_kernel_show_and_depth_in_place(r):
    """`show` writes the matte itself; the depth read as channel 0 of a [B,3,H,W] tensor through the plane stride"""
    from live2diff_amd.matte import composite_ref
    B, H, W = shape = SHAPES[1]
    styled, source, depth = data(*shape)
    dn = torch.full((B, 3, H, W), float("nan"), dtype=torch.float16)
    dn[:, 0] = depth
    dn_dev = dn.to(DEV)
    for show in (True, False):
        want = composite_ref(styled, source, depth, 0.3, 0.7, feather=r, keep="near", show=show)
        out = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
        got = launch(styled.to(DEV), source.to(DEV), dn_dev, out, 0.3, 0.7, r, "near", show=show, depth_stride=3 * H * W)
        assert report(f"r {r} show {show}, depth in place", got, want) == 0
        if show:
            assert len(np.unique(got)) > 2 and np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])


@pytest.mark.parametrize("r", [0, 1, 8])
def test_kernel_identities_and_repeatability(r):
    """m == 1 is the egress op's output for `styled`, m == 0 for `source`; two launches into differently filled outputs agree"""
    from live2diff_amd import ops
    B, H, W = shape = SHAPES[1]
    styled, source, depth = (t.to(DEV) for t in data(*shape))
    eg = torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV)
    ops.run(ops.frame_egress(styled, eg, B=B, H=H, W=W))
    near = launch(styled, source, depth, torch.zeros_like(eg), 0, 0, r, "near")
    assert np.array_equal(near, eg.cpu().numpy())
    ops.run(ops.frame_egress(source, eg, B=B, H=H, W=W))
    far = launch(styled, source, depth, torch.zeros_like(eg), 0, 0, r, "far")
    assert np.array_equal(far, eg.cpu().numpy())
    a = launch(styled, source, depth, torch.zeros_like(eg), 0.3, 0.7, r, "near")
    b = launch(styled, source, depth, torch.full_like(eg, 0xFF), 0.3, 0.7, r, "near")
    assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- the wrapper on the device
def test_wrapper_matte_on_device():
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

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
    frames = u8_frames(N + 3, 96, 128, seed=2)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(matte=None, **more):
        torch.manual_seed(0)                     # `prepare` draws init_noise and the warm-up re-noising from the global generators
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, **kw, **more)
        if matte is not None:
            w.set_matte(*matte[0], **matte[1])
        w.prepare(warm, PROMPT)
        return w

    far = ((0, 0), dict(keep="far"))
    twin, w = wrapper(), wrapper(far)
    warm_last = egress_ref(w.io.ingest(warm)[-1])[0].numpy()     # (a batch ingest: fresh tensors, the slots are not touched)

    # all far: the ingested source frame N - 1 calls earlier, the last warm-up frame before that
    sources = []
    for t, f in enumerate(frames):
        got = w(f)
        sources.append(egress_ref(w.io.last_view)[0].numpy())
        want = sources[t - (N - 1)] if t >= N - 1 else warm_last
        assert got.dtype == np.uint8 and got.shape == (H, W, 3)
        assert report(f"all far, call {t}", got, want) == 0
        twin(f)
    assert len({s.tobytes() for s in sources}) == len(frames) and len(w._matte_line.slots) <= N + 1

    # all near: byte-identical to the twin without a matte, as u8 and as jpeg
    w.set_matte(0, 0)
    for ot in ("u8", "jpeg"):
        w.output_type = twin.output_type = ot
        for t, f in enumerate(frames):
            got, want = w(f), twin(f)
            assert (np.array_equal(got, want) if ot == "u8" else got == want), (ot, t)
    assert isinstance(want, bytes) and want[:2] == b"\xff\xd8"

    # soft, feather 4: composite_ref of the stream's output tensor and the delay line's slot; as jpeg, encode_ref of that frame
    w.set_matte(0.3, 0.7, feather=4)
    for ot in ("u8", "jpeg", "pil"):
        w.output_type = ot
        got = w(frames[0])
        slot = w._matte_line.last
        want = composite_ref(w.stream.prev_image_result, slot.source[None], slot.depth[None], 0.3, 0.7, feather=4)[0]
        assert 0 < np.count_nonzero(want != egress_ref(w.stream.prev_image_result)[0].numpy())       # (the matte does something)
        if ot == "u8":
            assert report("soft matte, u8", got, want) == 0
        elif ot == "jpeg":
            assert got == jpeg.encode_ref(want, w.jpeg_quality)
        else:
            assert np.array_equal(np.array(got), want)
    w.clear_matte()
    w.output_type = twin.output_type = "u8"
    twin(frames[0]), twin(frames[0]), twin(frames[0])
    assert np.array_equal(w(frames[1]), twin(frames[1]))

    # push / pop with one frame in flight: the copies run on the side stream
    wp = wrapper(far, frame_pipelining=True)
    sources, out = [], []
    wp.push(frames[0])
    sources.append(egress_ref(wp.io.last_view)[0].numpy())
    for i in range(len(frames)):
        if i + 1 < len(frames):
            wp.push(frames[i + 1])
            sources.append(egress_ref(wp.io.last_view)[0].numpy())
        out.append(wp.pop())
    torch.cuda.synchronize()
    for t, got in enumerate(out):
        assert report(f"push / pop all far, frame {t}", got, sources[t - (N - 1)] if t >= N - 1 else warm_last) == 0
    assert len(wp._matte_line.slots) <= N + 2
