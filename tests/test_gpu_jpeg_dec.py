"""-m gpu: the device-side JPEG decoder (csrc/jpeg_dec.hip, live2diff_amd/jpeg_io.py) against `jpeg.decode_ref` and its stages,
which tests/test_jpeg_dec_cpu.py pins to Pillow.  Everything in the format is integer arithmetic, so every comparison here is exact
equality of coefficient buffers, planes and frames; there is no tolerance anywhere.  All images are fixture-sized; each test is
one plain run."""
import numpy as np
import pytest
import torch

from live2diff_amd import jpeg as J
from test_jpeg_dec_cpu import chunk_values, damaged_interval_case, fixture, with_fill_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda"


def layout_info(mx, my, hs, vs, quant=None, W=None, H=None):
    return J.JpegInfo(H or my * vs * 8, W or mx * hs * 8, hs, vs, np.ones((3, 64), np.int32) if quant is None else quant, (None,) * 4,
                      (0, 1, 1), (0, 1, 1), 0, 0, 0)


# ----------------------------------------------------------------------------- per op
def test_entropy_op_equals_decode_coefficients_ref():
    """op 39 alone, every fixture file, the four chunk sizes (one MCU per lane, chunks that span MCU rows, one chunk per MCU row, one
    lane for the whole scan); the buffer is poisoned first: every coefficient, zeros included, is written"""
    from live2diff_amd import ops
    files, _, _ = fixture()
    n = 0
    for name, f in files.items():
        info = J.parse(f)
        want = J.decode_coefficients_ref(f)
        file = torch.zeros(len(f) + 16, dtype=torch.uint8)
        file[:len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8)
        file, blob = file.to(DEV), torch.from_numpy(J.table_blob(info).copy()).to(DEV)
        params = torch.tensor([info.scan_offset, len(f)], dtype=torch.int32, device=DEV)
        for cm in chunk_values(info):
            off, pred = ops.jpeg_index(info, f, cm)
            coef = torch.full((want.size + 8,), 0x7F7F, dtype=torch.int16, device=DEV)
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.run(ops.jpeg_entropy_dec(file, torch.from_numpy(off).to(DEV), torch.from_numpy(pred).reshape(-1).to(DEV), blob, params, coef, status,
                                         n_mcu=info.n_mcu, ny=info.hs * info.vs, restart_interval=info.restart_interval, chunk_mcus=cm,
                                         C=len(off) - 1, dc_tab=info.dc_tab, ac_tab=info.ac_tab))
            got = coef.cpu().numpy()
            assert int(status.item()) == 0, f"{name}, chunk_mcus {cm}: status {int(status.item())}"
            assert np.array_equal(got[:-8].reshape(want.shape), want), f"{name}, chunk_mcus {cm}"
            assert (got[-8:] == 0x7F7F).all()
            n += 1
    assert n == 4 * len(files)


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (2, 2)])
def test_idct_op_on_random_blocks(hs, vs):
    """op 40 alone: dequantisation, both passes, the range limit and the block's place in its plane.  Dense blocks of +-64 times
    quantisers up to 16 (|dequantised| <= 1024: the largest magnitude for which no intermediate of jidctint can pass 2^31, and far
    into saturation on both sides), sparse blocks, empty blocks, DC-only blocks at the limits.  38 or more blocks: two work-groups."""
    from live2diff_amd import ops
    mx, my = 5, 2 + (hs * vs == 1) * 2
    rng = np.random.default_rng(hs * 10 + vs)
    quant = rng.integers(1, 17, (3, 64)).astype(np.int32)
    info = layout_info(mx, my, hs, vs, quant)
    bpm = info.blocks_per_mcu
    coef = rng.integers(-64, 65, (info.n_mcu, bpm, 64)).astype(np.int16)
    kind = rng.integers(0, 4, (info.n_mcu, bpm))
    coef[kind == 1] *= (rng.random((int((kind == 1).sum()), 64)) < 0.1).astype(np.int16)         # sparse
    coef[kind == 2] = 0                                                                           # empty
    coef[kind == 3, 1:] = 0                                                                       # DC only, up to the limit
    coef[0, 0], coef[0, 1] = 64, -64                                                              # every coefficient at the limit
    assert info.n_mcu * bpm > 32
    want = J.planes_ref(coef, info)
    sat = np.concatenate([p.reshape(-1) for p in want])
    assert (sat == 0).mean() > 0.05 and (sat == 255).mean() > 0.05 and ((sat > 0) & (sat < 255)).mean() > 0.05
    planes = torch.full((coef.size + 16,), 0x7F, dtype=torch.uint8, device=DEV)
    ops.run(ops.jpeg_idct(torch.from_numpy(coef.reshape(-1)).to(DEV), torch.from_numpy(quant.astype(np.uint16).view(np.uint8).reshape(-1).copy()).to(DEV),
                          planes, n_mcu=info.n_mcu, mcus_x=mx, hs=hs, vs=vs))
    got = planes.cpu().numpy()
    at = 0
    for k, p in enumerate(want):
        assert np.array_equal(got[at:at + p.size].reshape(p.shape), p), f"plane {k}"
        at += p.size
    assert at == coef.size and (got[at:] == 0x7F).all()


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (2, 2)])
def test_rgb_op_on_random_planes(hs, vs):
    """op 41 alone: fancy up-sampling (both parities of width and height, partial MCUs, the one- and two-column planes libjpeg
    replicates) and the colour conversion, against `upsample_ref` / `ycc_to_rgb_ref`"""
    from live2diff_amd import ops
    rng = np.random.default_rng(3)
    for W, H in ((8, 8), (16, 16), (23, 17), (17, 23), (100, 75), (3, 5), (2, 40), (6, 4), (1, 1)):
        info = layout_info(-(-W // (8 * hs)), -(-H // (8 * vs)), hs, vs, W=W, H=H)
        shapes = [(info.mcus_y * vs * 8, info.mcus_x * hs * 8)] + [(info.mcus_y * 8, info.mcus_x * 8)] * 2
        y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in shapes)
        cb[:2], cr[-2:] = 0, 255                                                                   # the corners of the colour cube
        rows, cols = info.chroma_size
        want = J.ycc_to_rgb_ref(y[:H, :W], *(J.upsample_ref(p, hs, vs, rows, cols)[:H, :W] for p in (cb, cr)))
        planes = torch.from_numpy(np.concatenate([p.reshape(-1) for p in (y, cb, cr)])).to(DEV)
        out = torch.full((H * W * 3 + 16,), 0x7F, dtype=torch.uint8, device=DEV)
        ops.run(ops.jpeg_rgb(planes, out, H=H, W=W, hs=hs, vs=vs))
        got = out.cpu().numpy()
        assert np.array_equal(got[:-16].reshape(H, W, 3), want), f"{W}x{H}"
        assert (got[-16:] == 0x7F).all()


# ----------------------------------------------------------------------------- the decoder
def test_decoder_equals_decode_ref_byte_for_byte():
    from live2diff_amd.jpeg_io import HipJpegDecoder
    files, pixels, _ = fixture()
    dec = HipJpegDecoder(device=DEV)
    other = HipJpegDecoder(device=DEV, chunk_mcus=1)
    for name, f in files.items():
        out = dec.decode(f)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == pixels[name].shape
        assert np.array_equal(out.cpu().numpy(), pixels[name]), name
        assert np.array_equal(other.decode(memoryview(f)).cpu().numpy(), pixels[name]), f"{name}, chunk_mcus 1"
        dec.check()
        other.check()
    for start in ("23x17_420_blocks", "100x75_422_rows", "17x23_444_none"):        # fill bytes in front of the markers
        name = next(k for k in files if k.startswith(start))
        for d in (dec, other):
            assert np.array_equal(d.decode(with_fill_bytes(files[name])).cpu().numpy(), pixels[name]), f"{name} with fill bytes"
            d.check()
    with pytest.raises(J.JpegUnsupported):
        from test_jpeg_dec_cpu import pillow_file
        dec.decode(pillow_file(pixels["roundtrip"], progressive=True))


def _slot_of(dec, view):
    return next(s for slots, _ in dec._geo.values() for s in slots if s.out.data_ptr() == view.data_ptr())


def test_two_slots_in_turn_and_no_stale_data():
    """A, B, A with different geometries; before the second A every buffer of A's slots is poisoned: a block the entropy op did not
    write, a plane byte or a pixel left from another frame would show"""
    from live2diff_amd.jpeg_io import HipJpegDecoder
    files, pixels, _ = fixture()
    a, b = "noise_q100", next(k for k in files if k.startswith("100x75_422_none"))
    flat = next(k for k in files if k.startswith("100x75") and k.endswith("flat"))
    dec = HipJpegDecoder(device=DEV)
    first = dec.decode(files[a])
    first_host = first.cpu().numpy()
    assert np.array_equal(dec.decode(files[b]).cpu().numpy(), pixels[b])
    for slots, _ in dec._geo.values():
        for s in slots:
            if tuple(s.out.shape) == pixels[a].shape:
                for t in (s.coef_buf, s.planes_buf, s.out_buf):
                    t.view(torch.uint8).fill_(0x7F)
    second = dec.decode(files[a])
    assert second.data_ptr() != first.data_ptr()                                   # the other slot of A's geometry
    assert np.array_equal(second.cpu().numpy(), first_host) and np.array_equal(first_host, pixels[a])
    third = dec.decode(files[a])
    assert third.data_ptr() == first.data_ptr() and np.array_equal(third.cpu().numpy(), pixels[a])
    # a frame of mostly empty blocks into a slot that held noise: same geometry key needs the same tables, so decode it twice
    for _ in range(3):
        assert np.array_equal(dec.decode(files[flat]).cpu().numpy(), pixels[flat])
    dec.check()
    with pytest.raises(ValueError, match="not a view"):
        dec.release(torch.zeros(4, device=DEV), torch.cuda.Event())
    ev = torch.cuda.Event()
    ev.record()
    dec.release(third, ev)
    assert np.array_equal(dec.decode(files[a]).cpu().numpy(), pixels[a]) and np.array_equal(dec.decode(files[a]).cpu().numpy(), pixels[a])


def test_round_trip_through_the_device_encoder():
    from live2diff_amd.jpeg_io import HipJpegDecoder, HipJpegEncoder
    _, _, src = fixture()
    assert src.shape == (48, 64, 3)
    file = HipJpegEncoder(48, 64, 75, device=DEV).encode(torch.from_numpy(src.copy()).to(DEV))
    assert file == J.encode_ref(src, 75)
    got = HipJpegDecoder(device=DEV).decode(file).cpu().numpy()
    assert np.array_equal(got, J.decode_ref(J.encode_ref(src, 75)))
    assert np.abs(got.astype(int) - src.astype(int)).mean() < 8.0                  # it is the picture


def test_damaged_interval_is_reported_and_nothing_else_is_touched():
    """One restart interval of a `restart_marker_blocks=1` file overwritten: the host index is a marker search and does not see it.
    The lanes of the other intervals decode what they decoded before, the damaged one ORs its reason into the status word, `check()`
    raises, and the canaries behind the three buffers are intact.  (tests/test_jpeg_dec_cpu.py runs the same lane code on the same
    file on the host.)"""
    from live2diff_amd.jpeg_io import GUARD, HipJpegDecoder
    f, info, bad, hit = damaged_interval_case()
    dec = HipJpegDecoder(device=DEV, chunk_mcus=1)
    good = dec.decode(f)
    dec.check()
    want = _slot_of(dec, good).coef.cpu().numpy().reshape(info.n_mcu, info.blocks_per_mcu, 64)
    assert np.array_equal(want, J.decode_coefficients_ref(f))
    out = dec.decode(bad)
    slot = _slot_of(dec, out)
    assert slot is not _slot_of(dec, good)
    torch.cuda.synchronize()
    for t in (slot.coef_buf, slot.planes_buf, slot.out_buf):                       # a second run into a slot with canaries in place
        t.view(torch.uint8)[-GUARD:] = 0x5A
    with pytest.raises(ValueError, match="damaged"):
        dec.check()
    dec.decode(f)                                                                  # (takes the first slot)
    out = dec.decode(bad)
    assert _slot_of(dec, out) is slot
    torch.cuda.synchronize()
    assert int(slot.status_host[0]) != 0
    got = slot.coef.cpu().numpy().reshape(want.shape)
    keep = np.ones(info.n_mcu, bool)
    keep[hit] = False
    assert np.array_equal(got[keep], want[keep])
    for t in (slot.coef_buf, slot.planes_buf, slot.out_buf):
        assert (t.view(torch.uint8)[-GUARD:] == 0x5A).all()
    with pytest.raises(ValueError, match="device status"):
        dec.check()
    dec.check()                                                                    # examined once: nothing is pending now
    with pytest.raises(ValueError, match="damaged"):                               # a file the host walks is refused before any launch
        HipJpegDecoder(device=DEV).decode(fixture()[0]["noise_q100"][:5000] + b"\xff\xd9")


def test_ingest_keeps_a_plan_per_static_device_source():
    from live2diff_amd.frame_io import HipFrameIO
    from live2diff_amd.jpeg_io import HipJpegDecoder
    files, pixels, _ = fixture()
    f = files["noise_q100"]
    io, dec = HipFrameIO(64, 64, device=DEV), HipJpegDecoder(device=DEV)
    want = HipFrameIO(64, 64, device=DEV).ingest(pixels["noise_q100"]).clone()     # the same launch on the frame uploaded raw
    for i in range(6):
        assert torch.equal(io.ingest(dec.decode(f)), want)
    assert len(io._device_plans) == 2                                              # two decoder slots meet two ingest slots in step
    for i in range(12):                                                            # fresh tensors every frame: at most four plans are kept
        io.ingest(torch.from_numpy(pixels["noise_q100"].copy()).to(DEV))
    assert len(io._device_plans) <= 4


# ----------------------------------------------------------------------------- the wrapper
def test_wrapper_takes_jpeg_bytes_like_the_decoded_frame():
    """synthetic components as in tests/test_gpu_wrapper.py: `wrapper(bytes)` against `wrapper(decode_ref(bytes))` in the same stream
    state, bit for bit -- JPEG warm-up frames in `prepare`, the direct call, push / pop, an unsupported file through Pillow, and a
    damaged file raising where its output is fetched"""
    from test_gpu_wrapper import PROMPT, SEED, Parts, u8_frames
    from test_jpeg_dec_cpu import pillow, pillow_file

    from live2diff_amd.clip_hip import tiny_clip_config
    from live2diff_amd.config import tiny_config
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    ccfg = tiny_clip_config()
    ucfg = tiny_config(channels=(64, 128, 256, 256), cross_attention_dim=ccfg.hidden_size)
    H = W = 64
    parts = Parts(ucfg, ccfg, H, W, 2)
    warm = [J.encode_ref(f, 90) for f in u8_frames(8, 96, 128, seed=1)]
    frames = [J.encode_ref(f, 90) for f in u8_frames(3, 96, 128, seed=2)]
    frames.append(pillow_file(u8_frames(1, 96, 128, seed=3)[0], quality=85, subsampling=1, optimize=True))        # 4:2:2, no restart markers
    raw_warm, raw = np.stack([J.decode_ref(f) for f in warm]), [J.decode_ref(f) for f in frames]
    kw = dict(num_inference_steps=50, t_index_list=[30, 40], width=W, height=H, warmup_frames=ucfg.sink_size, window_size=ucfg.window_size)

    def wrapper(warmup, **more):
        torch.manual_seed(0)
        w = Wrapper.from_components(parts.pipe(), output_type="u8", seed=SEED, device=DEV, **kw, **more)
        return w, w.prepare(warmup, PROMPT)

    (wj, warm_j), (wu, warm_u) = wrapper(warm), wrapper(raw_warm)
    assert torch.equal(warm_j, warm_u)
    got, want = [wj(f) for f in frames], [wu(f) for f in raw]
    for i in range(4):
        assert np.array_equal(got[i], want[i]), f"frame {i}"
    assert len({g.tobytes() for g in got}) == 4 and wj.jpeg_dec is not None and wj.jpeg_host_decodes == 0 and wu.jpeg_dec is None
    assert np.array_equal(wj(bytearray(frames[1])), wu(raw[1]))
    prog = pillow_file(raw[2], progressive=True)                                   # outside the device's subset: Pillow, and counted
    assert np.array_equal(wj(prog), wu(pillow(prog)))
    assert wj.jpeg_host_decodes == 1
    wh, _ = wrapper(warm, jpeg_decode="host")
    wu2, _ = wrapper(raw_warm)
    assert np.array_equal(wh(frames[0]), wu2(raw[0])) and wh.jpeg_dec is None and wh.jpeg_host_decodes == 9
    wp, _ = wrapper(warm, frame_pipelining=True)
    out = []
    wp.push(frames[0])
    for i in range(4):
        if i + 1 < 4:
            wp.push(frames[i + 1])
        out.append(wp.pop())
    for i in range(4):
        assert np.array_equal(out[i], got[i]), f"push / pop frame {i} differs from __call__"
    # a damaged scan (a restart interval overwritten; the index of such a file is a marker search): ValueError at the output
    f = pillow_file(raw[0], quality=85, restart_marker_blocks=1)
    info = J.parse(f)
    off, _ = J.index_ref(info, f, 1)
    lo, hi = info.scan_offset + (off[1] >> 3), info.scan_offset + (off[2] >> 3) - 2
    with pytest.raises(ValueError, match="damaged"):
        wj(f[:lo] + bytes([0x55] * (hi - lo)) + f[hi:])
    assert np.array_equal(wj(frames[3]).shape, (H, W, 3))                          # the stream goes on
