"""-m gpu: the device-side JPEG encoder (csrc/jpeg.hip, live2diff_amd/jpeg_io.py) against `jpeg.encode_ref`, which
tests/test_jpeg_cpu.py pins to Pillow.  Everything in the format is integer arithmetic, so every comparison here is byte equality
of whole files (or exact equality of coefficient buffers); there is no tolerance anywhere.  Each test is one plain run."""
import functools
import io
import os

import numpy as np
import pytest
import torch

from live2diff_amd import jpeg as J

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((64, 64), (128, 192), (512, 512), (512, 768), (576, 1024))
KINDS = ("noise", "constant", "checker")


@functools.lru_cache(maxsize=None)
def frame(kind, H, W):
    """uniform noise: the longest codes and, at quality 100, many stuffed 0xFF; a constant frame: the shortest rows (one DC
    difference and end-of-block codes); the saturated 0 / 255 checkerboard: 11-bit DC differences"""
    if kind == "noise":
        a = np.random.default_rng(H * 131 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "constant":
        a = np.full((H, W, 3), (200, 30, 90), np.uint8)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.repeat(((((yy >> 3) + (xx >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, 2)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_u8(kind, H, W, q):
    return J.encode_ref(frame(kind, H, W), q)


@functools.lru_cache(maxsize=None)
def fp16_batch(H, W):
    """fp16 [3,3,H,W] well beyond [-1, 1] on both sides (the clamp), with exact 0 / 1 / -1 and rounding ties in it"""
    g = torch.Generator().manual_seed(H + W)
    x = (torch.rand(3, 3, H, W, generator=g) * 2.6 - 1.3).half()
    x[0, :, 0, :4] = torch.tensor([0.0, 1.0, -1.0, 1.0 / 255.0]).half()
    return x


def differing(a: bytes, b: bytes) -> str:
    n = min(len(a), len(b))
    first = next((i for i in range(n) if a[i] != b[i]), n)
    return f"{len(a)} bytes against the reference's {len(b)}, first difference at byte {first}"


@pytest.mark.parametrize("quality", [10, 75, 100])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_files_equal_encode_ref(size, quality):
    from live2diff_amd.frame_io import HipFrameIO
    from live2diff_amd.jpeg_io import HipJpegEncoder
    H, W = size
    enc = HipJpegEncoder(H, W, quality, device=DEV)
    batch = torch.from_numpy(np.stack([frame(k, H, W) for k in KINDS])).to(DEV)
    got = enc.encode(batch)                                                        # uint8, B = 3
    assert isinstance(got, list) and len(got) == 3
    for k, g in zip(KINDS, got):
        want = ref_u8(k, H, W, quality)
        print(f"{H}x{W} q{quality} {k}: {len(g)} bytes")
        assert g == want, f"uint8 batch, {k}: {differing(g, want)}"
        assert len(g) - len(enc.header) <= J.capacity(H, W)
    for i, k in enumerate(KINDS):                                                  # uint8, B = 1: the same file as in the batch
        one = enc.encode(batch[i])
        assert isinstance(one, bytes) and one == got[i], f"uint8 single, {k}: {differing(one, got[i])}"
    x = fp16_batch(H, W).to(DEV)                                                   # fp16: the file of the egress op's bytes
    u8 = HipFrameIO(H, W, device=DEV).egress(x).copy()
    want = [J.encode_ref(u8[i], quality) for i in range(3)]
    got = enc.encode(x)
    for i in range(3):
        assert got[i] == want[i], f"fp16 batch, frame {i}: {differing(got[i], want[i])}"
    one = enc.encode(x[1])
    assert one == want[1], f"fp16 single: {differing(one, want[1])}"


def test_widest_row_the_launcher_accepts():
    """1920 wide: 720 blocks per MCU row, the largest LDS request of the entropy coder"""
    from live2diff_amd import ops
    from live2diff_amd.jpeg_io import HipJpegEncoder
    H, W = 32, ops.JPEG_MAX_W
    enc = HipJpegEncoder(H, W, 100, device=DEV)
    got = enc.encode(torch.from_numpy(frame("noise", H, W).copy()).to(DEV))
    want = ref_u8("noise", H, W, 100)
    assert got == want, differing(got, want)


def test_coefficients_of_the_dct_op_alone():
    from live2diff_amd import ops
    from live2diff_amd.frame_io import egress_ref
    H, W = 128, 192
    for q in (10, 75, 100):
        for k in ("noise", "checker"):
            src = torch.from_numpy(frame(k, H, W)[None].copy()).to(DEV)
            coef = torch.full((H * W * 3 // 2,), 12345, dtype=torch.int16, device=DEV)
            ops.run(ops.jpeg_dct(src, coef, B=1, H=H, W=W, quality=q))
            want = J.coefficients(frame(k, H, W), q)
            got = coef.cpu().numpy().reshape(want.shape)
            assert np.array_equal(got, want), f"uint8 {k} q{q}: {(got != want).sum()} of {want.size} coefficients differ"
    x = fp16_batch(H, W)[:2].contiguous()
    coef = torch.zeros(2 * H * W * 3 // 2, dtype=torch.int16, device=DEV)
    ops.run(ops.jpeg_dct(x.to(DEV), coef, B=2, H=H, W=W, quality=75))
    u8 = egress_ref(x).numpy()
    want = np.stack([J.coefficients(u8[b], 75) for b in range(2)])
    assert np.array_equal(coef.cpu().numpy().reshape(want.shape), want)


def test_entropy_coder_on_crafted_coefficients():
    """Ops 37 + 38 on coefficient buffers no picture would give, against `jpeg.encode_scan`: sparse blocks (zero runs of 16, 32 and 48
    and more: one to three ZRL codes), empty blocks, full blocks, a non-zero coefficient 63 (no end-of-block code), DC differences
    of 11 bits, and in every row a last block that ends in ten 1-bits, so that the padded last byte is 0xFF and must be stuffed."""
    from live2diff_amd import _lib
    from live2diff_amd.jpeg_io import HipJpegEncoder
    H, W, B = 64, 96, 2
    R, M = H // 16, W // 16
    rng = np.random.default_rng(7)
    coef = np.zeros((B, R, M, 6, 64), np.int16)
    dense = rng.integers(-1023, 1024, coef.shape).astype(np.int16)
    keep = rng.random(coef.shape) < rng.choice([0.0, 0.02, 0.1, 0.5, 1.0], size=(B, R, M, 6, 1))
    coef[keep] = dense[keep]
    coef[..., 0] = rng.choice([-1023, -5, 0, 3, 1023], size=(B, R, M, 6))          # differences of up to 2046: 11 bits
    coef[0, 0, 0, 0, 1:] = 0
    coef[0, 0, 0, 0, [17, 50]] = 1, -1                                             # runs of 16 and 32
    coef[0, 0, 1, 4, 1:] = 0
    coef[0, 0, 1, 4, 63] = -700                                                    # a run of 62: three ZRL, no end-of-block
    coef[:, :, M - 1, 5, 63] = 1023                                                # every row ends in 1111111111
    enc = HipJpegEncoder(H, W, 75, device=DEV)
    full = enc.plan(torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV), B)
    bt = enc._batches[B]
    bt.coef.copy_(torch.from_numpy(coef.reshape(-1)))
    tail = _lib.OpList()
    tail.append(full[1])
    tail.append(full[2])
    tail.run()
    torch.cuda.synchronize()
    out = bt.out.cpu().numpy()
    stuffed_padding = 0
    for b in range(B):
        want = enc.header + J.encode_scan(coef[b], 75)
        n = int(out[b, :4].view(np.int32)[0])
        got = out[b, 16:16 + n].tobytes()
        assert got == want, f"frame {b}: {differing(got, want)}"
        stuffed_padding += want.count(b"\xff\x00\xff\xd0") + want.count(b"\xff\x00\xff\xd1") + want.count(b"\xff\x00\xff\xd9")
    assert stuffed_padding >= 3                                                    # the reference itself went through that path


def test_repeatable_with_poisoned_buffers_and_device_result():
    from live2diff_amd.jpeg_io import HipJpegEncoder
    H, W = 128, 192
    enc = HipJpegEncoder(H, W, 100, device=DEV)
    batch = torch.from_numpy(np.stack([frame(k, H, W) for k in KINDS])).to(DEV)
    first = enc.encode(batch)
    bt = enc._batches[3]
    for t in (bt.staging, bt.out, bt.coef):
        t.view(torch.uint8).fill_(0xA5)
    bt.lengths.fill_(0x5A5A5A5A)
    second = enc.encode(batch)
    assert first == second == [ref_u8(k, H, W, 100) for k in KINDS]
    buf, n = enc.encode(batch, to_host=False)
    assert buf.is_cuda and buf.dtype == torch.uint8 and n.dtype == torch.int32 and n.shape == (3,)
    assert [buf[i, :int(n[i])].cpu().numpy().tobytes() for i in range(3)] == first
    buf1, n1 = enc.encode(batch[2], to_host=False)
    assert n1.ndim == 0 and buf1[:int(n1)].cpu().numpy().tobytes() == first[2]


def test_host_copy_is_the_file_not_the_capacity():
    """a frame within the first chunk takes one copy; the first frame that is larger takes a second one for the rest and makes the
    chunk grow, so the frame after it takes one again"""
    from live2diff_amd.jpeg_io import FIRST_CHUNK, HipJpegEncoder
    H = W = 512
    enc = HipJpegEncoder(H, W, 100, device=DEV)
    assert enc.out_stride > 2_000_000
    small = enc.encode(torch.from_numpy(frame("constant", H, W).copy()).to(DEV))
    assert small == ref_u8("constant", H, W, 100) and enc.last_copies == 1 and enc.last_copied_bytes == FIRST_CHUNK
    noisy = torch.from_numpy(frame("noise", H, W).copy()).to(DEV)
    big = enc.encode(noisy)
    assert big == ref_u8("noise", H, W, 100) and len(big) > FIRST_CHUNK
    assert enc.last_copies == 2 and enc.last_copied_bytes == 16 + len(big)
    again = enc.encode(noisy)
    assert again == big and enc.last_copies == 1 and 16 + len(big) <= enc.last_copied_bytes <= 1.26 * len(big) + 4096


def test_encoder_refuses_wrong_inputs():
    from live2diff_amd.jpeg_io import HipJpegEncoder
    enc = HipJpegEncoder(64, 64, 75, device=DEV)
    for bad in (torch.zeros(64, 64, 3, dtype=torch.uint8), torch.zeros(3, 64, 64, device=DEV), torch.zeros(3, 64, 48, dtype=torch.float16, device=DEV),
                torch.zeros(64, 64, 4, dtype=torch.uint8, device=DEV), np.zeros((64, 64, 3), np.uint8)):
        with pytest.raises(ValueError, match="jpeg encode"):
            enc.encode(bad)


# ----------------------------------------------------------------------------- the wrapper
def test_wrapper_jpeg_is_encode_ref_of_its_u8_output():
    """synthetic components as in tests/test_gpu_wrapper.py: a `"jpeg"` wrapper and a `"u8"` wrapper in the same stream state"""
    from PIL import Image
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames

    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    parts = Parts(ucfg, ccfg, H, W, 2)
    warm, frames = u8_frames(8, 96, 128, seed=1), u8_frames(4, 96, 128, seed=2)
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(output_type, **more):
        torch.manual_seed(0)
        w = Wrapper.from_components(parts.pipe(), output_type=output_type, seed=SEED, device=DEV, **kw, **more)
        w.prepare(warm, PROMPT)
        return w

    wj, wu = wrapper("jpeg", jpeg_quality=90), wrapper("u8")
    got = [wj(f) for f in frames]
    raw = [wu(f) for f in frames]
    assert wj.jpeg is not None and wj.jpeg.quality == 90 and len({bytes(g) for g in got}) == 4
    for i in range(4):
        want = J.encode_ref(raw[i], 90)
        assert isinstance(got[i], bytes) and got[i] == want, f"frame {i}: {differing(got[i], want)}"
        im = Image.open(io.BytesIO(got[i]))
        im.load()
        assert im.size == (W, H) and im.mode == "RGB"
    wp = wrapper("jpeg", jpeg_quality=90, frame_pipelining=True)
    out = []
    wp.push(frames[0])
    for i in range(4):
        if i + 1 < 4:
            wp.push(frames[i + 1])
        out.append(wp.pop())
    assert out == got, "push / pop differs from __call__"
