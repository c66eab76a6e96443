"""-m gpu: the two frame I/O kernels (csrc/frame_io.hip) through the C ABI and `HipFrameIO`, against the CPU restatements of
live2diff_amd/frame_io.py (which tests/test_frame_io_cpu.py pins to torch and to the reference's image_utils.py).

Ingest bound, max-abs 5e-4 on the fp16 result, no element excepted: half an fp16 ulp below 1.0 is 2.4e-4; the fp32 reassociation
of <= 25 products of weights <= 1 with values <= 255 is below 1e-5 after the / 255; doubled for margin.
Egress: byte-equal -- the arithmetic is fully specified in fp16 / fp32 IEEE steps."""
import numpy as np
import pytest
import torch

from live2diff_amd import frame_io as FIO

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIX = [((720, 1280), (512, 512)), ((1080, 1920), (512, 768)), ((480, 640), (512, 512)), ((512, 512), (512, 512)),
       ((360, 640), (576, 1024)), ((1280, 720), (512, 512))]
TEN = SIX + [((240, 320), (512, 512)), ((479, 641), (512, 512)), ((2160, 3840), (512, 512)), ((333, 517), (64, 96))]


def frames(B, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, generator=g)


def run_ingest(u8_dev, H, W, out=None):
    from live2diff_amd import ops
    B, Hs, Ws, _ = u8_dev.shape
    nh, nw, top, left = FIO.geometry(Hs, Ws, H, W)
    out = torch.empty(B, 3, H, W, dtype=torch.float16, device=DEV) if out is None else out
    ops.run(ops.frame_ingest(u8_dev, out, B=B, Hs=Hs, Ws=Ws, H=H, W=W, nh=nh, nw=nw, top=top, left=left))
    torch.cuda.synchronize()
    return out


def run_egress(x_dev, out=None):
    from live2diff_amd import ops
    B, _, H, W = x_dev.shape
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV) if out is None else out
    ops.run(ops.frame_egress(x_dev, out, B=B, H=H, W=W))
    torch.cuda.synchronize()
    return out


def ordered(x):
    """fp16 -> integers in value order (adjacent floats differ by one)"""
    b = x.cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("src,dst", TEN)
def test_ingest_matches_reference_arithmetic(src, dst, B):
    (Hs, Ws), (H, W) = src, dst
    u8 = frames(B, Hs, Ws, seed=Hs * 31 + Ws + B)
    got = run_ingest(u8.to(DEV), H, W).cpu()
    ref = FIO.ingest_ref(u8, H, W)
    err = (got.float() - ref).abs().max().item()
    print(f"ingest {Hs}x{Ws} -> {H}x{W} B={B}: max-abs {err:.3e}")
    assert torch.isfinite(got).all()
    assert err <= 5e-4
    if (Hs, Ws) == (H, W):
        want = (2.0 * u8.permute(0, 3, 1, 2).float() / 255.0 - 1.0).to(torch.float16)
        d = (ordered(got) - ordered(want)).abs().max().item()
        print(f"identity geometry: max distance {d} fp16 ulp")
        assert d <= 1


def egress_input(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, 3, H, W, generator=g) * 3.0 - 1.5).to(torch.float16)
    flat = x.view(-1)
    for i, v in enumerate([0.0, -0.0, 1.0, -1.0, float("inf"), float("-inf"), 1.0 - 2.0 ** -11, 1.0 + 2.0 ** -10, -1.0 + 2.0 ** -11]):
        flat[i * 5 + 1] = v
        flat[flat.numel() - 1 - i * 3] = v
    return x


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(16, 24), (512, 512), (576, 1024)])
def test_egress_is_byte_equal(H, W, B):
    x = egress_input(B, H, W, seed=H + W + B)
    got = run_egress(x.to(DEV)).cpu()
    ref = FIO.egress_ref(x)
    n = int((got != ref).sum())
    print(f"egress {H}x{W} B={B}: {n} differing bytes")
    assert n == 0


def test_egress_replays_the_reference_fixture(golden):
    g = golden("frame_io")
    assert np.array_equal(run_egress(torch.from_numpy(g["x"]).to(DEV)).cpu().numpy(), g["pil"])
    sx = torch.from_numpy(g["sweep_x"])
    n = sx.numel() // 16 * 16                                   # H W % 16; the two values cut off are covered by the tail run
    for lo in (0, sx.numel() - n):
        part, want = sx[lo:lo + n], g["sweep_u8"][lo:lo + n]
        got = run_egress(part.reshape(1, 1, n // 16, 16).repeat(1, 3, 1, 1).contiguous().to(DEV)).cpu().numpy()
        assert np.array_equal(got[0, :, :, 0].reshape(-1), want) and np.array_equal(got[..., 0], got[..., 2])


def test_ingest_bit_identity_batch_poison_and_device_input():
    Hs, Ws, H, W = 360, 640, 256, 384
    u8 = frames(8, Hs, Ws, seed=5)
    dev = u8.to(DEV)
    batched = run_ingest(dev, H, W)
    singles = torch.cat([run_ingest(dev[i:i + 1].contiguous(), H, W) for i in range(8)])
    assert torch.equal(batched, singles)
    poisoned = torch.empty_like(batched)
    poisoned.view(torch.uint8).fill_(0xFF)                     # NaN pattern
    assert torch.equal(run_ingest(dev, H, W, out=poisoned), batched)
    out_u8 = torch.empty(8, H, W, 3, dtype=torch.uint8, device=DEV)
    first = run_egress(batched, out=out_u8).clone()
    out_u8.fill_(0xFF)
    assert torch.equal(run_egress(batched, out=out_u8), first)
    io = FIO.HipFrameIO(H, W, device=DEV)
    assert torch.equal(io.ingest(u8), batched)                 # host tensor, batched
    assert torch.equal(io.ingest(u8.numpy()), batched)
    a = io.ingest(u8[3].numpy()).clone()                       # host frame through a slot
    b = io.ingest(dev[3]).clone()                              # device-resident frame: no upload
    torch.cuda.synchronize()
    assert torch.equal(a, batched[3:4]) and torch.equal(b, batched[3:4])
    e = io.egress(batched[3])
    assert isinstance(e, np.ndarray) and e.shape == (H, W, 3) and np.array_equal(e, first[3].cpu().numpy())
    ed = io.egress(batched, to_host=False)
    assert ed.is_cuda and torch.equal(ed, first)


def test_ingest_slots_alternate_and_wait_for_release():
    Hs, Ws, H, W = 96, 128, 64, 64
    A, B_, C = (f.numpy() for f in frames(3, Hs, Ws, seed=9))
    want = FIO.HipFrameIO(H, W, device=DEV).ingest(np.stack([A, B_, C]))
    torch.cuda.synchronize()
    io = FIO.HipFrameIO(H, W, device=DEV)
    a = io.ingest(A)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        copy = a.clone()
        ev = torch.cuda.Event()
        ev.record(side)
    io.release(a, ev)
    b = io.ingest(B_)
    c = io.ingest(C)
    torch.cuda.synchronize()
    assert (copy.cpu().float() - FIO.ingest_ref(A, H, W)).abs().max().item() <= 5e-4
    assert torch.equal(copy, want[0:1])
    assert c.data_ptr() == a.data_ptr() and b.data_ptr() != a.data_ptr()
    assert torch.equal(b, want[1:2]) and torch.equal(c, want[2:3])
    with pytest.raises(ValueError):
        io.release(copy, ev)
