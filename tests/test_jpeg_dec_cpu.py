"""CPU tests (-m "not gpu") of the JPEG input path: `live2diff_amd.jpeg.decode_ref` and its stages -- the oracle of the kernels in
csrc/jpeg_dec.hip -- pinned byte for byte to Pillow (a committed fixture written by tests/golden/gen_golden_jpeg_dec.py, and the
installed Pillow live); `parse` on what it must refuse; the host index `l2d_jpeg_index` against `index_ref` and on damaged files;
the entropy kernel's lane code run on the host (`l2d_jpeg_entropy_model`: the CPU model of its loop bounds and error reporting);
op codes and the launchers' argument validation in dry-run; the wrapper's bytes input without a device; the MJPEG server's
`--input post` handler on in-memory file objects.  Everything in the format is integer arithmetic: every comparison is equality."""
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

from live2diff_amd import jpeg as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


@functools.lru_cache(maxsize=None)
def fixture():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "jpeg_dec_pillow.npz")))
    files = {k[2:]: g[k].tobytes() for k in g if k.startswith("f_")}
    return files, {k[2:]: g[k] for k in g if k.startswith("p_")}, g["roundtrip_source"]


def chunk_values(info):
    return (1, 3, info.mcus_x, info.n_mcu + 5)


def pillow(f):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))


def pillow_file(u8, mode="RGB", **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(u8).convert(mode).save(b, format="JPEG", **kw)
    return b.getvalue()


# ----------------------------------------------------------------------------- pinned to Pillow
def test_fixture_covers_the_matrix():
    files, pixels, _ = fixture()
    names = [n for n in files if n[0].isdigit()]
    axes = [set(), set(), set(), set(), set(), set()]
    for n in names:
        for a, v in zip(axes, n.split("_")):
            a.add(v)
    assert axes == [{"8x8", "16x16", "23x17", "17x23", "100x75"}, {"444", "422", "420"}, {"none", "blocks", "rows"}, {"std", "opt"},
                    {"q1", "q50", "q95", "q100"}, {"flat", "gradient", "noise"}]
    assert len(names) == 90 and set(files) - set(names) == {"noise_q100", "roundtrip"}
    for n, f in files.items():
        info = J.parse(f)
        assert pixels[n].shape == (info.height, info.width, 3)
        if n[0].isdigit():
            size, ss, rst, tab = n.split("_")[:4]
            assert f"{info.width}x{info.height}" == size and (info.hs, info.vs) == {"444": (1, 1), "422": (2, 1), "420": (2, 2)}[ss]
            assert info.restart_interval == {"none": 0, "blocks": 1, "rows": info.mcus_x}[rst]
            standard = all(t == (h[1], h[2]) for t, h in zip(info.huffman, (J.HUFFMAN[0], J.HUFFMAN[2], J.HUFFMAN[1], J.HUFFMAN[3])))
            assert standard == (tab == "std")


def test_decode_ref_equals_the_fixture_and_the_installed_pillow():
    files, pixels, _ = fixture()
    for n, f in files.items():
        got = J.decode_ref(f)
        assert got.dtype == np.uint8 and np.array_equal(got, pixels[n]), f"{n}: differs from the fixture"
        assert np.array_equal(got, pillow(f)), f"{n}: differs from the installed Pillow"


def test_decode_ref_on_sizes_below_one_block_and_replicated_chroma():
    """libjpeg replicates a chrominance plane of one or two columns instead of filtering it"""
    rng = np.random.default_rng(5)
    for W, H in ((1, 1), (3, 5), (4, 9), (5, 3), (2, 40), (33, 1)):
        for ss in (0, 1, 2):
            f = pillow_file(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), quality=90, subsampling=ss)
            assert np.array_equal(J.decode_ref(f), pillow(f)), (W, H, ss)


def test_stages_compose_to_decode_ref():
    files, pixels, src = fixture()
    for n in ("23x17_420_none_std_q50_noise", "17x23_422_rows_opt_q100_gradient", "100x75_444_blocks_std_q1_flat", "roundtrip"):
        f = next(files[k] for k in files if k == n or k.startswith(n.rsplit("_", 2)[0])) if n not in files else files[n]
        info = J.parse(f)
        coef = J.decode_coefficients_ref(f)
        assert coef.dtype == np.int16 and coef.shape == (info.n_mcu, info.blocks_per_mcu, 64)
        y, cb, cr = J.planes_ref(coef, info)
        assert y.shape == (info.mcus_y * info.vs * 8, info.mcus_x * info.hs * 8) and cb.shape == cr.shape == (info.mcus_y * 8, info.mcus_x * 8)
        # one block by hand: dequantise, IDCT, its place in the plane
        blk = J.idct_ref(coef[0, 0].astype(np.int32) * info.quant[0])
        assert np.array_equal(blk, y[:8, :8])
        rows, cols = info.chroma_size
        up = [J.upsample_ref(p, info.hs, info.vs, rows, cols) for p in (cb, cr)]
        assert up[0].shape == (rows * info.vs, cols * info.hs)
        H, W = info.height, info.width
        assert np.array_equal(J.ycc_to_rgb_ref(y[:H, :W], up[0][:H, :W], up[1][:H, :W]), J.decode_ref(f))
    # the project's own encoder round-trips: its coefficients come back
    f = files["roundtrip"]
    want = J.coefficients(src, 75)                                    # [R][M][6][64], zigzag order
    got = J.decode_coefficients_ref(f).reshape(want.shape)[..., J.ZIGZAG]
    assert np.array_equal(got, want)


def test_upsample_ref_edges_by_hand():
    p = np.array([[10, 20, 40, 80]], np.uint8)
    assert J.upsample_ref(p, 2, 1, 1, 4).tolist() == [[10, (30 + 20 + 2) >> 2, (60 + 10 + 1) >> 2, (60 + 40 + 2) >> 2, (120 + 20 + 1) >> 2,
                                                        (120 + 80 + 2) >> 2, (240 + 40 + 1) >> 2, 80]]
    assert J.upsample_ref(p, 2, 1, 1, 2).tolist() == [[10, 10, 20, 20]]                           # two real columns: replicated
    q = np.array([[0, 16, 32], [64, 64, 64], [255, 255, 255]], np.uint8)                          # the third row is padding
    got = J.upsample_ref(q, 2, 2, 2, 3)
    assert got.shape == (4, 6)
    s0, s1 = 3 * q[0].astype(int) + q[0], 3 * q[0].astype(int) + q[1]                             # above row 0 is row 0
    assert got[0].tolist() == [(4 * s0[0] + 8) >> 4, (3 * s0[0] + s0[1] + 7) >> 4, (3 * s0[1] + s0[0] + 8) >> 4, (3 * s0[1] + s0[2] + 7) >> 4,
                               (3 * s0[2] + s0[1] + 8) >> 4, (4 * s0[2] + 7) >> 4]
    assert got[1, 0] == (4 * s1[0] + 8) >> 4
    assert got[3].tolist() == [64] * 6                                                            # below the last REAL row is that row


def test_idct_ref_saturates():
    dc = np.zeros((3, 64), np.int32)
    dc[0, 0], dc[1, 0], dc[2, 0] = 8 * 200, -8 * 200, 8 * 5
    out = J.idct_ref(dc)
    assert (out[0] == 255).all() and (out[1] == 0).all() and (out[2] == 133).all()


# ----------------------------------------------------------------------------- parse
def test_parse_reads_what_pillow_wrote():
    files, _, _ = fixture()
    info = J.parse(files["noise_q100"])
    assert (info.height, info.width, info.hs, info.vs, info.restart_interval) == (192, 256, 2, 2, 0)
    assert (info.mcus_x, info.mcus_y, info.n_mcu, info.blocks_per_mcu, info.chroma_size) == (16, 12, 192, 6, (96, 128))
    assert info.quant.shape == (3, 64) and (info.quant == 1).all() and info.dc_tab == (0, 1, 1) and info.ac_tab == (0, 1, 1)
    assert files["noise_q100"][info.scan_end:info.scan_end + 2] == b"\xff\xd9" and files["noise_q100"][info.scan_offset - 14:][:2] == b"\xff\xda"
    # fill bytes in front of a marker, a comment, and component ids other than 1, 2, 3 are accepted
    f = files["16x16_420_none_std_q50_flat"] if "16x16_420_none_std_q50_flat" in files else next(v for k, v in files.items() if k.startswith("16x16_420_none"))
    sof, sos = f.index(b"\xff\xc0"), f.index(b"\xff\xda")
    g = bytearray(f[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xff\xff" + f[2:])
    shift = 10
    for at, stride in ((sof + shift + 10, 3), (sos + shift + 5, 2)):
        for c in range(3):
            g[at + c * stride] = (82, 71, 66)[c]
    assert np.array_equal(J.decode_ref(bytes(g)), J.decode_ref(f))


def test_parse_names_what_the_device_does_not_decode():
    rng = np.random.default_rng(1)
    u8 = rng.integers(0, 256, (24, 24, 3), dtype=np.uint8)
    for f, match in ((pillow_file(u8, progressive=True), "progressive"), (pillow_file(u8, "L"), "greyscale"), (pillow_file(u8, "CMYK"), "4 component")):
        with pytest.raises(J.JpegUnsupported, match=match):
            J.parse(f)
        assert issubclass(J.JpegUnsupported, ValueError)
        pillow(f)                                                      # (Pillow itself reads it: the wrapper's host route)
    good = pillow_file(u8, quality=80, subsampling=0)
    sof = good.index(b"\xff\xc0")
    for patch, match in (((sof + 11, 0x41), "sampling factors"), ((sof + 11, 0x12), "sampling factors"), ((sof + 14, 0x21), "sampling factors"),
                         ((sof + 4, 12), "12-bit"), ((sof + 1, 0xC9), "arithmetic"), ((sof + 1, 0xC1), "extended sequential")):
        bad = bytearray(good)
        bad[patch[0]] = patch[1]
        with pytest.raises(J.JpegUnsupported, match=match):
            J.parse(bytes(bad))
    adobe = good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + good[2:]
    with pytest.raises(J.JpegUnsupported, match="Adobe"):
        J.parse(adobe)
    J.parse(adobe[:17] + b"\x01" + adobe[18:])                         # transform 1 (Y Cb Cr) is what the device decodes


def test_parse_refuses_structural_damage():
    files, _, _ = fixture()
    f = files["roundtrip"]
    info = J.parse(f)
    for cut in list(range(0, info.scan_offset, 7)) + [info.scan_offset - 1]:
        with pytest.raises(ValueError) as e:
            J.parse(f[:cut])
        assert not isinstance(e.value, J.JpegUnsupported), cut
    with pytest.raises(ValueError, match="no EOI"):
        J.parse(f[:-2])
    with pytest.raises(ValueError, match="SOI"):
        J.parse(b"\x89PNG" + f)
    dqt, dht = f.index(b"\xff\xdb"), f.index(b"\xff\xc4")
    with pytest.raises(ValueError, match="quantisation table 0 is missing"):
        J.parse(f[:dqt] + f[dqt + 69:])
    with pytest.raises(ValueError, match="Huffman table"):
        J.parse(f[:dht] + f[dht + 33:])
    with pytest.raises(ValueError, match="runs past the file"):
        J.parse(f[:dht + 2] + b"\xff\xff" + f[dht + 4:])


# ----------------------------------------------------------------------------- the host index
def test_index_equals_index_ref():
    from live2diff_amd import ops
    files, _, _ = fixture()
    walked = searched = 0
    for n, f in files.items():
        info = J.parse(f)
        for cm in chunk_values(info):
            want_o, want_p = J.index_ref(info, f, cm)
            got_o, got_p = ops.jpeg_index(info, f, cm)
            interval, chunk, per, C = J.chunk_layout(info.n_mcu, info.restart_interval, cm)
            assert want_o.dtype == np.int32 and want_o.shape == (C + 1,) and want_p.dtype == np.int16 and want_p.shape == (C, 3)
            assert np.array_equal(got_o, want_o) and np.array_equal(got_p, want_p), f"{n}, chunk_mcus {cm}"
            assert want_o[0] == 0 and want_o[-1] == 8 * (info.scan_end - info.scan_offset) and (np.diff(want_o) > 0).all()
            searched += chunk == interval
            walked += chunk != interval
            if info.restart_interval:                                  # behind RSTn: byte-aligned, predictors 0
                starts = np.arange(C) % per == 0
                assert (want_o[:-1][starts] % 8 == 0).all() and (want_p[starts] == 0).all()
                d = f[info.scan_offset:]
                assert all(d[(o >> 3) - 2] == 0xFF and 0xD0 <= d[(o >> 3) - 1] <= 0xD7 for o in want_o[:-1][starts][1:])
    assert walked > 50 and searched > 100


def test_chunk_layout():
    assert J.chunk_layout(10, 0, 3) == (10, 3, 4, 4) and J.chunk_layout(10, 0, 99) == (10, 10, 1, 1)
    assert J.chunk_layout(10, 4, 3) == (4, 3, 2, 5) and J.chunk_layout(10, 4, 4) == (4, 4, 1, 3) and J.chunk_layout(10, 4, 8) == (4, 4, 1, 3)
    assert J.chunk_layout(10, 10, 3) == (10, 3, 4, 4) and J.chunk_layout(10, 12, 3) == (10, 3, 4, 4) and J.chunk_layout(9, 4, 3) == (4, 3, 2, 5)
    with pytest.raises(ValueError, match="chunk_mcus"):
        J.chunk_layout(10, 0, 0)


def test_the_fixture_holds_the_hard_cases_of_the_bit_reader():
    """with one MCU per chunk, a chunk of the noise file begins in the byte directly behind a stuffed FF 00, and one ends inside a
    stuffed FF (so that the next reader starts inside it and has to step over the 00)"""
    files, _, _ = fixture()
    f = files["noise_q100"]
    info = J.parse(f)
    off, _ = J.index_ref(info, f, 1)
    d = f[info.scan_offset:]
    behind = [o for o in off[1:-1] if o >= 16 and d[(o >> 3) - 2] == 0xFF and d[(o >> 3) - 1] == 0x00]
    inside = [o for o in off[1:-1] if o % 8 and d[o >> 3] == 0xFF and d[(o >> 3) + 1] == 0x00]
    print(f"{len(off) - 1} chunks: {len(behind)} begin behind FF 00, {len(inside)} boundaries inside an FF; {d.count(bytes([255, 0]))} stuffed pairs")
    assert len(behind) >= 1 and len(inside) >= 1


def _index_rc(info, data, cm):
    from live2diff_amd import _lib
    C = J.chunk_layout(info.n_mcu, info.restart_interval, max(cm, 1))[3]
    lay = np.array([info.scan_offset, info.n_mcu, info.hs * info.vs, info.restart_interval, cm, *info.dc_tab, *info.ac_tab, C], np.int32)
    blob = J.table_blob(info)
    file = np.frombuffer(data, np.uint8).copy()
    off, pred = np.zeros(C + 1, np.int32), np.zeros((C, 3), np.int16)
    rc = _lib.lib.l2d_jpeg_index(file.ctypes.data, file.size, blob.ctypes.data, lay.ctypes.data, off.ctypes.data, pred.ctypes.data)
    return rc, _lib.lib.l2d_last_error().decode()


def test_index_returns_its_error_code_on_damaged_files():
    files, _, _ = fixture()
    codes = set()
    for n, f in files.items():
        info = J.parse(f)
        for part in (0.25, 0.5, 0.75):
            cut = info.scan_offset + int((info.scan_end - info.scan_offset) * part)
            for cm in (1, info.mcus_x):
                rc, msg = _index_rc(info, f[:cut], cm)
                assert rc in (-2, -3, -4, -5) and "l2d_jpeg_index" in msg, f"{n} cut at {part}: rc {rc} {msg}"
                codes.add(rc)
    f = files["noise_q100"]
    info = J.parse(f)
    assert _index_rc(info, f, 3)[0] == 0
    mid = (info.scan_offset + info.scan_end) // 2
    for fill in (b"\xff" * 16, b"\x00" * 16, bytes(range(16))):
        rc, msg = _index_rc(info, f[:mid] + fill + f[mid + 16:], 3)
        assert rc in (-2, -3, -4, -5), msg
        codes.add(rc)
    assert _index_rc(info, f, 0)[0] == -1 and _index_rc(info._replace(dc_tab=(0, 2, 1)), f, 3)[0] == -1
    print("error codes met:", sorted(codes))
    assert len(codes) >= 2
    from live2diff_amd import ops
    with pytest.raises(ValueError, match="damaged"):
        ops.jpeg_index(info, f[:mid], 3)


# ----------------------------------------------------------------------------- the entropy kernel's lanes, on the host
def _model(info, data, cm, index=None, poison=0x7F7F):
    """(coefficients, status) of `l2d_jpeg_entropy_model`: the op record the decoder would launch, over host arrays"""
    from live2diff_amd import _lib, ops
    C = J.chunk_layout(info.n_mcu, info.restart_interval, cm)[3]
    off, pred = index if index is not None else ops.jpeg_index(info, data, cm)
    file = torch.zeros(len(data) + 16, dtype=torch.uint8)
    file[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    coef = torch.full((info.n_mcu * info.blocks_per_mcu * 64 + 8,), poison, dtype=torch.int16)
    status = torch.zeros(1, dtype=torch.int32)
    op, keep = ops.jpeg_entropy_dec(file, torch.from_numpy(off.copy()), torch.from_numpy(pred.copy()).reshape(-1), torch.from_numpy(J.table_blob(info).copy()),
                                    torch.tensor([info.scan_offset, len(data)], dtype=torch.int32), coef, status, n_mcu=info.n_mcu,
                                    ny=info.hs * info.vs, restart_interval=info.restart_interval, chunk_mcus=cm, C=C, dc_tab=info.dc_tab,
                                    ac_tab=info.ac_tab)
    assert _lib.lib.l2d_jpeg_entropy_model(ctypes.byref(op)) == 0
    assert (coef[-8:] == poison).all()                                 # nothing behind the buffer
    return coef[:-8].numpy().reshape(info.n_mcu, info.blocks_per_mcu, 64), int(status[0])


def test_lane_code_on_the_host_equals_decode_coefficients_ref():
    files, _, _ = fixture()
    for n, f in files.items():
        info = J.parse(f)
        for cm in chunk_values(info):
            got, status = _model(info, f, cm)
            assert status == 0 and np.array_equal(got, J.decode_coefficients_ref(f)), f"{n}, chunk_mcus {cm}"


def with_fill_bytes(f):
    """the same file with two fill bytes (FF) in front of every restart marker and of the EOI, which T.81 B.1.1.2 allows"""
    import re
    info = J.parse(f)
    scan = re.sub(rb"\xff[\xd0-\xd7]", lambda m: b"\xff\xff" + m.group(0), f[info.scan_offset:info.scan_end])
    return f[:info.scan_offset] + scan + b"\xff\xff" + f[info.scan_end:]


def test_fill_bytes_in_front_of_markers_are_accepted():
    from live2diff_amd import ops
    files, pixels, _ = fixture()
    for start in ("23x17_420_blocks", "100x75_422_rows", "17x23_444_none"):
        name = next(k for k in files if k.startswith(start))
        f = with_fill_bytes(files[name])
        info = J.parse(f)
        assert len(f) == len(files[name]) + 2 * (-(-info.n_mcu // info.restart_interval) if info.restart_interval else 1)
        assert np.array_equal(J.decode_ref(f), pixels[name]) and np.array_equal(pillow(f), pixels[name])
        for cm in chunk_values(info):
            want = J.index_ref(info, f, cm)
            got = ops.jpeg_index(info, f, cm)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, cm)
            coef, status = _model(info, f, cm)
            assert status == 0 and np.array_equal(coef, J.decode_coefficients_ref(files[name])), (name, cm)


def damaged_interval_case():
    """(file, info, damaged file, MCUs of the damaged interval): a `restart_marker_blocks=1` file -- indexed by marker search, so the
    host does not walk it -- with the bytes of one interval overwritten (no FF among them: the markers stay where they are)"""
    files, _, _ = fixture()
    name = next(k for k in files if k.startswith("100x75_420_blocks"))
    f = files[name]
    info = J.parse(f)
    off, _ = J.index_ref(info, f, 1)
    k = info.n_mcu // 2
    lo, hi = info.scan_offset + (off[k] >> 3), info.scan_offset + (off[k + 1] >> 3) - 2
    assert hi - lo >= 2 and f[hi:hi + 2] == bytes([0xFF, 0xD0 + (k & 7)])
    bad = f[:lo] + bytes([0x55] * (hi - lo)) + f[hi:]
    return f, info, bad, [k]


def test_lane_code_on_the_host_reports_a_damaged_interval_and_stays_in_bounds():
    """the CPU model of the GPU error-reporting test (tests/test_gpu_jpeg_dec.py), same file, same damage"""
    from live2diff_amd import ops
    f, info, bad, hit = damaged_interval_case()
    index = ops.jpeg_index(info, bad, 1)                               # marker search: the damage goes unseen on the host
    assert np.array_equal(index[0], J.index_ref(info, f, 1)[0])
    got, status = _model(info, bad, 1, index)
    assert status != 0
    keep = np.ones(info.n_mcu, bool)
    keep[hit] = False
    assert np.array_equal(got[keep], J.decode_coefficients_ref(f)[keep])
    # a file cut in the middle with the intact file's index: every lane stops, none reads or writes outside
    cut = f[:(info.scan_offset + info.scan_end) // 2]
    _, status = _model(info, cut, 1, J.index_ref(info, f, 1))
    assert status != 0


# ----------------------------------------------------------------------------- ops in dry-run
def test_op_codes_are_appended_and_abi_unchanged():
    from live2diff_amd import _lib
    assert (_lib.OP_JPEG_ENTROPY_DEC, _lib.OP_JPEG_IDCT, _lib.OP_JPEG_RGB) == (39, 40, 41) and _lib.ABI_VERSION == 6
    assert _lib.lib.l2d_abi_version() == 6 and hasattr(_lib.lib, "l2d_jpeg_index")
    with open(os.path.join(ROOT, "include", "l2d.h")) as h:
        text = h.read()
    for name, v in (("JPEG_ENTROPY_DEC", 39), ("JPEG_IDCT", 40), ("JPEG_RGB", 41)):
        assert f"L2D_OP_{name} = {v}," in text
    assert J.DEC_BLOB_BYTES == 4032 and J.DEC_QUANT_OFF == 3648


def test_plans_validate_in_dry_run(dry_run):
    from live2diff_amd.jpeg_io import HipJpegDecoder
    files, _, _ = fixture()
    for cm in (1, 4, 1000):
        dec = HipJpegDecoder(device="cpu", chunk_mcus=cm)
        for n, f in files.items():
            pl = dec.plan(J.parse(f), len(f))
            assert len(pl) == 3 and [op.kind for op in pl] == [39, 40, 41]
            pl.run()
    with pytest.raises(ValueError, match="chunk_mcus"):
        HipJpegDecoder(device="cpu", chunk_mcus=0)


def test_launchers_reject_what_the_kernels_cannot_do(dry_run):
    from live2diff_amd import ops
    from live2diff_amd._lib import L2DError
    n_mcu, ny, C = 12, 4, 3
    file, blob = torch.zeros(4096, dtype=torch.uint8), torch.zeros(4032, dtype=torch.uint8)
    off, pred, params = torch.zeros(16, dtype=torch.int32), torch.zeros(64, dtype=torch.int16), torch.zeros(4, dtype=torch.int32)
    coef, status = torch.zeros(n_mcu * 6 * 64 + 8, dtype=torch.int16), torch.zeros(4, dtype=torch.int32)
    planes, out = torch.zeros(8192, dtype=torch.uint8), torch.zeros(64 * 48 * 3, dtype=torch.uint8)

    def entropy(**kw):
        a = dict(n_mcu=n_mcu, ny=ny, restart_interval=0, chunk_mcus=4, C=C, dc_tab=(0, 1, 1), ac_tab=(0, 1, 1), coef=coef, off=off)
        a.update(kw)
        c, o = a.pop("coef"), a.pop("off")
        return ops.jpeg_entropy_dec(file, o, pred, blob, params, c, status, **a)

    ops.run(entropy())
    ops.run(entropy(restart_interval=4, chunk_mcus=9))
    ops.run(ops.jpeg_idct(coef, blob[3648:], planes, n_mcu=n_mcu, mcus_x=4, hs=2, vs=2))
    ops.run(ops.jpeg_rgb(planes, out, H=48, W=64, hs=2, vs=2))

    def bad(match, op):
        with pytest.raises(L2DError, match=match):
            ops.run(op)

    bad("chunks do not follow", entropy(C=4))
    bad("chunks do not follow", entropy(restart_interval=5))
    bad("chunks do not follow", entropy(chunk_mcus=0))
    bad("luminance blocks", entropy(ny=3))
    bad("must be positive", entropy(n_mcu=0, C=0))
    bad("table id", entropy(dc_tab=(0, 2, 1)))
    bad("table id", entropy(ac_tab=(0, 1, -1)))
    bad("16-byte aligned", entropy(coef=coef[1:]))
    bad("misaligned", entropy(off=torch.frombuffer(bytearray(80), dtype=torch.int32, offset=2, count=16)))
    bad("not 1 x 1", ops.jpeg_idct(coef, blob[3648:], planes, n_mcu=n_mcu, mcus_x=4, hs=1, vs=2))
    bad("no whole rows", ops.jpeg_idct(coef, blob[3648:], planes, n_mcu=n_mcu, mcus_x=5, hs=2, vs=2))
    bad("16-byte", ops.jpeg_idct(coef[4:], blob[3648:], planes, n_mcu=n_mcu, mcus_x=4, hs=2, vs=2))
    bad("8-byte", ops.jpeg_idct(coef, blob[3648:], planes[4:], n_mcu=n_mcu, mcus_x=4, hs=2, vs=2))
    bad("not 1 x 1", ops.jpeg_rgb(planes, out, H=48, W=64, hs=2, vs=4))
    bad("1 .. 65535", ops.jpeg_rgb(planes, out, H=0, W=64, hs=2, vs=2))
    big = torch.zeros(1, dtype=torch.uint8).expand(65536 * 8 * 192)
    bad("1 .. 65535", ops.jpeg_rgb(big, big, H=8, W=65536, hs=1, vs=1))


# ----------------------------------------------------------------------------- the wrapper without a device
class _Stream:
    """what the wrapper asks of its pipeline, as a pure function of the frame it is handed"""

    def __call__(self, x):
        self.seen = x
        return torch.from_numpy(np.array(x)).permute(2, 0, 1)[None].float() / 127.5 - 1.0

    def update_prompt(self, prompt):
        self.prompt = prompt


def _cpu_wrapper():
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    w = Wrapper.__new__(Wrapper)
    w.io, w.jpeg, w.frame_buffer_size, w.output_type, w.stream = None, None, 1, "pt", _Stream()
    return w


def test_wrapper_without_a_device_takes_bytes_through_pillow():
    files, pixels, _ = fixture()
    w = _cpu_wrapper()
    n = 0
    for name in ("noise_q100", "roundtrip", next(k for k in files if k.startswith("23x17_422"))):
        for data in (files[name], bytearray(files[name]), memoryview(files[name])):
            got = w(data)
            assert np.array_equal(w.stream.seen, J.decode_ref(files[name])) and w.stream.seen.dtype == np.uint8
            assert torch.equal(got, w(J.decode_ref(files[name])))
            n += 1
    assert w.jpeg_host_decodes == n and w.jpeg_dec is None
    prog = pillow_file(pixels["roundtrip"], progressive=True)           # a file the device would not take is the same route
    assert torch.equal(w(prog), w(pillow(prog))) and w.jpeg_host_decodes == n + 1
    for bad in (b"", b"\x89PNG\r\n", bytearray(b"GIF89a")):
        with pytest.raises(ValueError, match="FF D8"):
            w(bad)


def test_wrapper_keyword_jpeg_decode():
    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper as Wrapper
    for v in ("gpu", None, True):
        with pytest.raises(ValueError, match="jpeg_decode"):
            Wrapper.from_components(object(), num_inference_steps=50, t_index_list=[1], jpeg_decode=v)


# ----------------------------------------------------------------------------- the MJPEG server's `--input post`, no socket
class _Connection:
    """what `BaseHTTPRequestHandler` asks of a socket, on two in-memory files"""

    def __init__(self, request: bytes):
        self.rfile, self.wfile = io.BytesIO(request), io.BytesIO()
        self.wfile.close = lambda: None

    def makefile(self, mode, *a, **kw):
        return self.rfile if "r" in mode else self.wfile

    def sendall(self, data):
        self.wfile.write(data)


def _request(handler, method, path, body=b"", length=None):
    head = f"{method} {path} HTTP/1.1\r\nHost: test\r\n"
    if method == "POST":
        head += f"Content-Length: {len(body) if length is None else length}\r\n"
    conn = _Connection(head.encode() + b"\r\n" + body)
    handler(conn, ("127.0.0.1", 0), None)
    return conn.wfile.getvalue()


def test_mjpeg_server_post_input_on_memory_files():
    import threading
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    files, _, _ = fixture()
    frames = [files[k] for k in sorted(files) if k.startswith("16x16")][:6]
    latest, inbox, stop = S.Latest(), S.Inbox(2), threading.Event()
    handler = S.make_handler(latest, inbox)
    page = _request(handler, "GET", "/")
    assert page.startswith(b"HTTP/1.0 200") and page.endswith(S.CAMERA_PAGE) and b"getUserMedia" in page and b"toBlob" in page
    assert b"fetch('/frame'" in page and b'<img src="/stream"' in page
    assert _request(S.make_handler(latest), "GET", "/").endswith(S.PAGE)           # the folder mode's page is what it was
    assert _request(S.make_handler(latest), "POST", "/frame", frames[0]).startswith(b"HTTP/1.0 404")
    assert _request(handler, "POST", "/elsewhere", frames[0]).startswith(b"HTTP/1.0 404")
    assert _request(handler, "POST", "/frame", b"not a jpeg").startswith(b"HTTP/1.0 400")
    assert _request(handler, "POST", "/frame", frames[0], length=S.MAX_POST + 1).startswith(b"HTTP/1.0 413")
    assert _request(handler, "POST", "/frame", frames[0][:10], length=99).startswith(b"HTTP/1.0 400")     # a body cut short
    assert inbox.posted == 0
    for f in frames[:5]:
        assert _request(handler, "POST", "/frame", f).startswith(b"HTTP/1.0 204")
    assert (inbox.posted, inbox.replaced) == (5, 2)                                # two warm-up frames kept, then only the newest

    class W:
        """the producer's wrapper: echoes the frame; the second frame it gets is refused as damaged, the third stops the stream"""

        def __init__(self):
            self.warm, self.seen = None, []

        def prepare(self, warm, prompt):
            self.warm = (list(warm), prompt)

        def __call__(self, frame):
            self.seen.append(frame)
            if len(self.seen) == 1:
                inbox.put(frames[5] + b"damaged")
            elif len(self.seen) == 2:
                inbox.put(frames[0])
                raise ValueError("jpeg: the scan is damaged")
            else:
                stop.set()
            return frame

    w = W()
    S.produce_posted(w, "a prompt", inbox, latest, stop)               # (in this thread; every frame it waits for is there already)
    assert w.warm == (frames[:2], "a prompt") and w.seen == [frames[4], frames[5] + b"damaged", frames[0]]
    assert inbox.failed == 1 and inbox.posted == 7
    out = _request(handler, "GET", "/stream")
    assert out.partition(b"\r\n\r\n")[2] == J.mjpeg_part(frames[0])    # the newest part, then the closed stream ends
    closed = S.Inbox(1)
    closed.close()
    assert closed.warmup_frames() is None and closed.take() is None
