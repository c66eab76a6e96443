"""CPU tests (-m "not gpu") of the JPEG output path: `live2diff_amd.jpeg.encode_ref` -- the oracle of the kernels in
csrc/jpeg.hip -- pinned byte for byte to Pillow (a committed fixture, and the installed Pillow live), the header / table /
capacity helpers, the op codes and launchers' argument validation in dry-run, the wrapper's `"jpeg"` output type on CPU tensors,
and the MJPEG server's handler on in-memory file objects (no socket)."""
import io
import os
import sys

import numpy as np
import pytest
import torch

from live2diff_amd import jpeg as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = (1, 10, 50, 75, 95, 100)
BASELINE_SIZES = ((256, 256), (512, 512), (512, 768), (576, 1024))


@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def noise(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def smooth(H, W, seed=0):
    yy, xx = np.mgrid[0:H, 0:W]
    s = np.stack([128 + 100 * np.sin(xx / 37.0 + yy / 51.0), 128 + 90 * np.cos(yy / 23.0), xx * 255.0 / W], -1)
    return np.clip(s + np.random.default_rng(seed).normal(0, 6, s.shape), 0, 255).astype(np.uint8)


def checker(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat(((((yy >> 3) + (xx >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, 2)


# ----------------------------------------------------------------------------- pinned to Pillow
def test_encode_ref_equals_pillow_fixture_byte_for_byte(golden):
    g = golden("jpeg_pillow")
    n = 0
    for i in range(4):
        f = g[f"frame_{i}"]
        for q in QUALITIES:
            want = g[f"jpeg_{i}_q{q}"].tobytes()
            got = J.encode_ref(f, q)
            assert got == want, f"frame {i} {f.shape} quality {q}: {len(got)} bytes against Pillow's {len(want)}"
            assert len(got) - len(J.header(f.shape[0], f.shape[1], q)) <= J.capacity(*f.shape[:2])
            n += 1
    assert n == 24 and {g[f"frame_{i}"].shape[:2] for i in range(4)} == {(64, 64), (64, 96), (128, 64), (192, 256)}


def _pillow(u8, q):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(u8).save(b, format="JPEG", quality=q, restart_marker_rows=1)
    return b.getvalue()


def test_encode_ref_equals_installed_pillow_at_stream_sizes():
    if b"\xff\xdd\x00\x04" not in _pillow(np.zeros((16, 16, 3), np.uint8), 75):
        pytest.skip("the installed Pillow ignores restart_marker_rows (no DRI segment in its file)")
    for (H, W), f, q in (((512, 512), smooth(512, 512), 75), ((512, 512), noise(512, 512), 100), ((576, 1024), smooth(576, 1024, 1), 50),
                         ((576, 1024), checker(576, 1024), 95)):
        got, want = J.encode_ref(f, q), _pillow(f, q)
        assert got == want, f"{H}x{W} quality {q}: {len(got)} bytes against Pillow's {len(want)}"
        assert len(got) - len(J.header(H, W, q)) <= J.capacity(H, W)


def test_pillow_decodes_what_encode_ref_writes():
    from PIL import Image
    f = smooth(64, 96)
    im = Image.open(io.BytesIO(J.encode_ref(f, 90)))
    im.load()
    assert im.size == (96, 64) and im.mode == "RGB" and im.format == "JPEG"
    assert [tuple(c[:4]) for c in im.layer] == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]      # (id, h, v, quantisation table): 4:2:0
    err = np.abs(np.asarray(im).astype(int) - f.astype(int)).mean()
    print(f"mean |decoded - source| at quality 90: {err:.2f}")
    assert err < 8.0                                                                 # it is the picture, not merely a valid file


# ----------------------------------------------------------------------------- header, tables, capacity, parts
def test_header_segments_are_in_pillows_order():
    h = J.header(576, 1024, 75)
    assert h[:2] == b"\xff\xd8" and h[2:20] == b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    markers, i = [], 2
    while i < len(h):
        assert h[i] == 0xFF
        markers.append(h[i + 1])
        i += 2 + int.from_bytes(h[i + 2:i + 4], "big")
    assert i == len(h) and markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    sof = h.index(b"\xff\xc0")
    assert h[sof + 4:sof + 19] == bytes([8, 0x02, 0x40, 0x04, 0x00, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert h[h.index(b"\xff\xdd"):][:6] == b"\xff\xdd\x00\x04\x00\x40"                # one MCU row = 64 MCUs
    assert h[-14:] == b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"


def test_tables_follow_the_quality_rule_and_annex_k():
    assert J.BITS_DC_LUMA == (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
    assert J.BITS_AC_LUMA == (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)
    assert J.BITS_DC_CHROMA == (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
    assert J.BITS_AC_CHROMA == (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)
    for _, bits, vals in J.HUFFMAN:
        assert sum(bits) == len(vals) == len(set(vals))
    assert list(J.ZIGZAG[:10]) == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and sorted(J.ZIGZAG) == list(range(64))
    t = J.tables(75)
    assert t.divisors.shape == (2, 64) and t.divisors[0, 0] == 8 * 8 and t.divisors[1, 63] == 8 * 50
    assert np.array_equal(J.tables(50).divisors, 8 * np.stack([J.QUANT_LUMA, J.QUANT_CHROMA]))
    assert (J.tables(100).divisors == 8).all() and J.tables(1).divisors.max() == 8 * 255
    # `length << 16 | code`: EOB and ZRL of both AC tables, the longest code, and the prefix property through Kraft's sum
    assert t.ac[0, 0x00] == (4 << 16 | 0b1010) and t.ac[0, 0xF0] == (11 << 16 | 0b11111111001)
    assert t.ac[1, 0x00] == (2 << 16 | 0b00) and t.ac[1, 0xF0] == (10 << 16 | 0b1111111010)
    assert t.dc[0, 0] == (2 << 16 | 0) and t.dc[1, 11] == (11 << 16 | 0b11111111110)
    for tab, n in ((t.dc[0], 12), (t.dc[1], 12), (t.ac[0], 162), (t.ac[1], 162)):
        lengths = (tab >> 16)[tab != 0]
        assert len(lengths) == n and lengths.max() <= 16 and sum(2.0 ** -int(x) for x in lengths) < 1.0
    packed = t.packed()
    assert packed.dtype == np.int32 and packed.shape == (544,) and packed[32 + 256] == (2 << 16)
    # the header's DQT segments hold the same tables, zigzag order
    h = J.header(64, 64, 75)
    a = h.index(b"\xff\xdb")
    assert list(h[a + 5:a + 69]) == list(t.divisors[0][J.ZIGZAG] // 8)


def test_capacity_bounds_the_worst_frames():
    assert J.BLOCK_BYTES == 216 and J.row_capacity(1024) == 64 * 6 * 432 + 4 and J.capacity(576, 1024) == 36 * J.row_capacity(1024)
    for H, W in ((64, 64), (64, 208)):
        for f in (noise(H, W), noise(H, W, 1) | 0xF0, checker(H, W)):
            scan = len(J.encode_ref(f, 100)) - len(J.header(H, W, 100))
            print(f"{H}x{W}: scan {scan} of capacity {J.capacity(H, W)}")
            assert scan <= J.capacity(H, W)
    for bad in ((60, 64), (64, 72), (0, 64)):
        with pytest.raises(ValueError, match="multiples of 16"):
            J.capacity(*bad)
    with pytest.raises(ValueError, match="multiples of 16"):
        J.encode_ref(np.zeros((64, 40, 3), np.uint8))
    for q in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            J.encode_ref(np.zeros((16, 16, 3), np.uint8), q)


def test_mjpeg_part_is_the_references_layout():
    payload = b"\xff\xd8 not really a jpeg \xff\xd9"
    assert J.mjpeg_part(payload) == (b"--frame\r\n" + b"Content-Type: image/jpeg\r\n" + f"Content-Length: {len(payload)}\r\n\r\n".encode()
                                     + payload + b"\r\n")


def test_restart_intervals_are_independent():
    """what the kernel's decomposition rests on: an MCU row's bytes depend on that row's coefficients alone"""
    f = noise(64, 64, 3)
    g = f.copy()
    g[16:32] = smooth(16, 64)
    a, b = J.encode_ref(f, 75), J.encode_ref(g, 75)
    ra, rb = a.split(b"\xff\xd0")[0], b.split(b"\xff\xd0")[0]
    assert ra == rb and a != b
    assert a.endswith(b"\xff\xd9") and a.count(b"\xff\xd0") >= 1 and b"\xff\xd1" in a and b"\xff\xd2" in a and b"\xff\xd3" not in a[-8:]


# ----------------------------------------------------------------------------- ops in dry-run
def test_op_codes_are_appended_and_abi_unchanged():
    from live2diff_amd import _lib
    assert (_lib.OP_JPEG_DCT, _lib.OP_JPEG_HUFF, _lib.OP_JPEG_PACK) == (36, 37, 38) and _lib.ABI_VERSION == 6
    assert _lib.lib.l2d_abi_version() == 6


@pytest.mark.parametrize("B", [1, 8])
def test_plans_validate_in_dry_run(dry_run, B):
    from live2diff_amd.jpeg_io import HipJpegEncoder
    for H, W in BASELINE_SIZES:
        enc = HipJpegEncoder(H, W, 75, device="cpu")
        assert enc.row_stride >= J.row_capacity(W) and enc.out_stride >= 16 + len(enc.header) + J.capacity(H, W)
        for src in (torch.zeros(B, 3, H, W, dtype=torch.float16), torch.zeros(B, H, W, 3, dtype=torch.uint8)):
            pl = enc.plan(src, B)
            assert len(pl) == 3
            pl.run()


def test_launchers_reject_what_the_kernels_cannot_do(dry_run):
    from live2diff_amd import ops
    from live2diff_amd._lib import L2DError
    H = W = 64
    src = torch.zeros(1, H, W, 3, dtype=torch.uint8)
    big = torch.zeros(1, 16 * 2048 * 3, dtype=torch.uint8)
    coef = torch.zeros(16 * 2048 * 3 // 2 + 8, dtype=torch.int16)
    tab = torch.zeros(544, dtype=torch.int32)
    rs = J.row_capacity(W)
    staging, lengths = torch.zeros(4 * J.row_capacity(2048), dtype=torch.uint8), torch.zeros(64, dtype=torch.int32)
    hdr = torch.zeros(len(J.header(H, W)), dtype=torch.uint8)
    stride = -(-(16 + len(hdr) + 4 * rs) // 4) * 4
    out = torch.zeros(1, stride + 2 * rs, dtype=torch.uint8)
    ops.run(ops.jpeg_dct(src, coef, B=1, H=H, W=W, quality=75))
    ops.run(ops.jpeg_huff(coef, tab, staging, lengths, B=1, H=H, W=W, row_stride=rs))
    ops.run(ops.jpeg_pack(staging, lengths, hdr, out, B=1, H=H, row_stride=rs, out_stride=stride))

    def bad(match, op):
        with pytest.raises(L2DError, match=match):
            ops.run(op)

    bad("multiples of 16", ops.jpeg_dct(big, coef, B=1, H=72, W=W, quality=75))
    bad("multiples of 16", ops.jpeg_dct(big, coef, B=1, H=H, W=72, quality=75))
    bad("limited to 1920", ops.jpeg_dct(big, coef, B=1, H=16, W=2048, quality=75))
    ops.run(ops.jpeg_dct(big, coef, B=1, H=16, W=ops.JPEG_MAX_W, quality=75))
    bad("quality 0", ops.jpeg_dct(src, coef, B=1, H=H, W=W, quality=0))
    bad("quality 101", ops.jpeg_dct(src, coef, B=1, H=H, W=W, quality=101))
    bad("16-byte", ops.jpeg_dct(src, coef[1:], B=1, H=H, W=W, quality=75))
    bad("multiples of 16", ops.jpeg_huff(coef, tab, staging, lengths, B=1, H=H, W=40, row_stride=rs))
    bad("limited to 1920", ops.jpeg_huff(coef, tab, staging, lengths, B=1, H=16, W=2048, row_stride=J.row_capacity(2048)))
    ops.run(ops.jpeg_huff(coef, tab, staging, lengths, B=1, H=16, W=1024, row_stride=J.row_capacity(1024)))
    bad("worst case", ops.jpeg_huff(coef, tab, staging, lengths, B=1, H=H, W=W, row_stride=rs - 1))
    bad("output stride", ops.jpeg_pack(staging, lengths, hdr, out, B=1, H=H, row_stride=rs, out_stride=stride - 4))
    bad("multiple of 16", ops.jpeg_pack(staging, lengths, hdr, out, B=1, H=H + 8, row_stride=rs, out_stride=stride + rs))
    from live2diff_amd.jpeg_io import HipJpegEncoder
    for kw, match in ((dict(height=72, width=64), "multiples of 16"), (dict(height=64, width=2048), "exceeds 1920"),
                      (dict(height=64, width=64, quality=0), "quality"), (dict(height=64, width=64, quality=101), "quality")):
        with pytest.raises(ValueError, match=match):
            HipJpegEncoder(device="cpu", **kw)


# ----------------------------------------------------------------------------- the wrapper on CPU tensors
def test_wrapper_jpeg_on_cpu_is_encode_ref_of_egress_ref(golden):
    from live2diff_amd.frame_io import egress_ref
    from live2diff_amd.wrapper import OUTPUT_TYPES
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    assert OUTPUT_TYPES[:5] == ("pil", "pt", "np", "latent", "u8") and OUTPUT_TYPES[5] == "jpeg" and len(OUTPUT_TYPES) == 6
    x = torch.from_numpy(golden("frame_io")["x"])[:1]
    _, _, h, w = x.shape
    x = x.repeat(1, 1, -(-32 // h), -(-32 // w))
    x = x[:, :, :x.shape[2] // 16 * 16, :x.shape[3] // 16 * 16].contiguous()         # tiled to a multiple of 16
    assert x.shape[2] >= 16 and x.shape[3] >= 16
    wr = Wrapper.__new__(Wrapper)
    wr.io, wr.jpeg, wr.frame_buffer_size = None, None, 1
    for q in (75, 30):
        wr.jpeg_quality = q
        got = wr.postprocess_image(x, "jpeg")
        assert isinstance(got, bytes) and got == J.encode_ref(egress_ref(x)[0].numpy(), q)
    from PIL import Image
    assert Image.open(io.BytesIO(got)).size == (x.shape[3], x.shape[2])


@pytest.mark.parametrize("q", [0, 101, -3, 75.0, "75", True])
def test_wrapper_refuses_jpeg_quality_out_of_range(q):
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    with pytest.raises(ValueError, match="jpeg_quality"):
        Wrapper.from_components(object(), num_inference_steps=50, t_index_list=[1], output_type="jpeg", jpeg_quality=q)
    with pytest.raises(ValueError, match="jpeg_quality"):
        Wrapper(config_path=os.path.join(ROOT, "tests", "golden", "configs", "toonyou.yaml"), few_step_model_type="lcm", num_inference_steps=50, jpeg_quality=q)


def test_wrapper_refuses_jpeg_at_a_size_that_is_no_multiple_of_16():
    from types import SimpleNamespace

    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    with pytest.raises(ValueError, match="multiples of 16"):
        Wrapper.from_components(SimpleNamespace(), num_inference_steps=50, t_index_list=[1], output_type="jpeg", height=72, width=64,
                                device="cpu")


# ----------------------------------------------------------------------------- the MJPEG server's handler, no socket
class _Connection:
    """what `BaseHTTPRequestHandler` asks of a socket, on two in-memory files"""

    def __init__(self, request: bytes):
        self.rfile, self.wfile = io.BytesIO(request), io.BytesIO()
        self.wfile.close = lambda: None                      # (the handler closes its files; the test reads wfile afterwards)

    def makefile(self, mode, *a, **kw):
        return self.rfile if "r" in mode else self.wfile

    def sendall(self, data):
        self.wfile.write(data)


def _serve(handler, path):
    conn = _Connection(f"GET {path} HTTP/1.1\r\nHost: test\r\n\r\n".encode())
    handler(conn, ("127.0.0.1", 0), None)
    return conn.wfile.getvalue()


def test_mjpeg_server_handler_on_memory_files():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    latest = S.Latest()
    handler = S.make_handler(latest)
    page = _serve(handler, "/")
    assert page.startswith(b"HTTP/1.0 200") and b"text/html" in page and b'<img src="/stream"' in page and page.endswith(S.PAGE)
    assert _serve(handler, "/nothing").startswith(b"HTTP/1.0 404")

    class W:                                                 # the producer's wrapper: two frames, then the stream stops
        def __init__(self):
            self.n = 0

        def __call__(self, frame):
            self.n += 1
            if self.n == 2:
                stop.set()
            return J.encode_ref(frame, 50)

    import threading
    stop = threading.Event()
    frames = [noise(16, 16, 1), noise(16, 16, 2)]
    S.produce(W(), frames, latest, stop)                     # (in this thread: `latest` ends up closed, holding frame 2)
    out = _serve(handler, "/stream")
    head, _, body = out.partition(b"\r\n\r\n")
    assert head.startswith(b"HTTP/1.0 200") and b"Content-Type: multipart/x-mixed-replace; boundary=frame" in head
    assert body == J.mjpeg_part(J.encode_ref(frames[1], 50))  # a viewer gets the LATEST part, then the closed stream ends
    assert latest.wait(2) is None and latest.wait(0)[0] == 2
