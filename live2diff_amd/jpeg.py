"""Baseline JPEG as this project writes it (csrc/jpeg.hip): the specification in code.

The reference's demo turns every output frame into `image.save(format="JPEG")` plus a multipart header (demo/util.py:27-37).
Here the frame is encoded on the device; this module is the host side of that encoder: `encode_ref` restates the format in
numpy (the oracle of the kernels and the CPU fallback of the wrapper), `header` / `tables` / `capacity` are what the device
side uploads and allocates, `mjpeg_part` is the reference's part layout.

The format is fixed: 8-bit YCbCr 4:2:0, MCU = 16 x 16 pixels = Y00 Y01 Y10 Y11 Cb Cr, libjpeg's accurate integer DCT, the
Annex K quantisation tables scaled by libjpeg's quality rule, the Annex K.3 Huffman tables, one restart interval per MCU row.
Everything is integer arithmetic, so the output is pinned byte for byte: `encode_ref(x, q)` is the file Pillow writes for
`save(format="JPEG", quality=q, restart_marker_rows=1)` (tests/test_jpeg_cpu.py, tests/golden/jpeg_pillow.npz).
"""
import functools
from typing import NamedTuple

import numpy as np

# ----------------------------------------------------------------------------- constant tables (ITU T.81 Annex K; data)
QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)

BITS_DC_LUMA = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
BITS_AC_LUMA = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)
BITS_DC_CHROMA = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
BITS_AC_CHROMA = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)
VALS_DC = bytes(range(12))
VALS_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a34353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
VALS_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536"
    "3738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999a"
    "a2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
# (table class << 4 | table id, BITS, values) in the order the header writes them: DC0, AC0, DC1, AC1
HUFFMAN = ((0x00, BITS_DC_LUMA, VALS_DC), (0x10, BITS_AC_LUMA, VALS_AC_LUMA),
           (0x01, BITS_DC_CHROMA, VALS_DC), (0x11, BITS_AC_CHROMA, VALS_AC_CHROMA))


def _zigzag() -> np.ndarray:
    """ZIGZAG[k] = natural index (row * 8 + column) of the k-th coefficient in zigzag order"""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order, np.int64)


ZIGZAG = _zigzag()

MAX_SYMBOL_BITS = 16 + 11        # the longest Huffman code + the longest magnitude (an 11-bit DC difference)
BLOCK_BYTES = 64 * MAX_SYMBOL_BITS // 8          # 216: the bound on one unstuffed block


def _check(H: int, W: int, quality: int) -> None:
    if H <= 0 or W <= 0 or H % 16 or W % 16:
        raise ValueError(f"jpeg: the frame is {H} x {W}; height and width must be positive multiples of 16 (4:2:0 MCUs, no edge padding)")
    if H > 65535 or W > 65535:
        raise ValueError(f"jpeg: the frame is {H} x {W}; a JPEG dimension is at most 65535")
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"jpeg: quality={quality!r} is outside 1..100")


def quant_tables(quality: int) -> np.ndarray:
    """int64 [2][64], natural order: libjpeg's rule -- s = 5000 // q below 50, 200 - 2 q from 50; Q = clamp((base s + 50) // 100, 1, 255)"""
    _check(16, 16, quality)
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((base * s + 50) // 100, 1, 255) for base in (QUANT_LUMA, QUANT_CHROMA)])


def huffman_codes(bits, vals) -> np.ndarray:
    """uint32 [256]: `length << 16 | code` of every symbol of a table (0 where the table has no such symbol), T.81 Annex C"""
    out = np.zeros(256, np.uint32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (length << 16) | code
            code, k = code + 1, k + 1
        code <<= 1
    assert k == len(vals)
    return out


class Tables(NamedTuple):
    divisors: np.ndarray       # int32 [2][64], natural order: 8 Q (the DCT's output is 8 x the true DCT)
    dc: np.ndarray             # uint32 [2][16]: length << 16 | code of DC size category 0..11, luminance / chrominance
    ac: np.ndarray             # uint32 [2][256]: the same for the AC symbol run << 4 | size (0x00 = EOB, 0xF0 = ZRL)

    def packed(self) -> np.ndarray:
        """the Huffman tables as one int32 array for upload, in the order the kernels index it: dc [2][16], ac [2][256] (the
        kernels derive the divisors from the quality with the same rule and hold the zigzag order as a constant)"""
        return np.concatenate([self.dc.reshape(-1).view(np.int32), self.ac.reshape(-1).view(np.int32)])


@functools.lru_cache(maxsize=None)
def tables(quality: int = 75) -> Tables:
    dc = np.stack([huffman_codes(BITS_DC_LUMA, VALS_DC)[:16], huffman_codes(BITS_DC_CHROMA, VALS_DC)[:16]])
    ac = np.stack([huffman_codes(BITS_AC_LUMA, VALS_AC_LUMA), huffman_codes(BITS_AC_CHROMA, VALS_AC_CHROMA)])
    return Tables((quant_tables(quality) * 8).astype(np.int32), dc, ac)


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(H: int, W: int, quality: int = 75) -> bytes:
    """everything in front of the entropy-coded data, in Pillow's (libjpeg's) order: SOI, APP0 (JFIF 1.01, no density unit,
    1 x 1), DQT 0, DQT 1, SOF0, DHT x 4 (DC0, AC0, DC1, AC1), DRI (W / 16 MCUs = one MCU row), SOS"""
    _check(H, W, quality)
    q = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += _segment(0xDB, bytes([t]) + bytes(int(v) for v in q[t][ZIGZAG]))
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in HUFFMAN:
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + vals)
    out += _segment(0xDD, (W // 16).to_bytes(2, "big"))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0]))


def row_capacity(W: int) -> int:
    """worst-case bytes of one MCU row in the scan, marker included (see `capacity`)"""
    return (W // 16) * 6 * 2 * BLOCK_BYTES + 2 + 2


def capacity(H: int, W: int) -> int:
    """An upper bound on the scan (everything behind `header`, EOI included), in bytes.

    A block is at most 64 symbols (the DC difference and 63 coefficients; an end-of-block or a run of ZRL codes only appears
    where coefficients are zero and costs less than they would) of at most 16 + 11 bits (the longest Huffman code and the longest
    magnitude): 64 x 27 bits = 216 bytes.  An MCU row holds (W / 16) x 6 blocks; padding the last byte with 1-bits adds less than
    one byte; byte stuffing follows every 0xFF with a 0x00 and so at most doubles that (the + 2 is the padded byte, doubled);
    the RSTn / EOI marker behind every row adds 2.  A frame has H / 16 rows."""
    _check(H, W, 75)
    return (H // 16) * row_capacity(W)


def mjpeg_part(jpeg: bytes) -> bytes:
    """one part of a `multipart/x-mixed-replace; boundary=frame` stream, the reference's layout (demo/util.py:27-37)"""
    return b"--frame\r\nContent-Type: image/jpeg\r\nContent-Length: " + str(len(jpeg)).encode() + b"\r\n\r\n" + jpeg + b"\r\n"


# ----------------------------------------------------------------------------- the encoder, stage by stage
def ycc420(u8: np.ndarray):
    """uint8 [H,W,3] -> (Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2]) as int64: 16-bit fixed-point colour conversion per pixel, then
    `(a + b + c + d + bias) >> 2` over each 2 x 2 square with bias 1 in even and 2 in odd output columns"""
    r, g, b = (u8[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16

    def down(p):
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        bias = 1 + (np.arange(s.shape[1]) & 1)
        return (s + bias[None, :]) >> 2

    return y, down(cb), down(cr)


def _ds(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first: bool):
    """one pass of the accurate integer DCT (13 constant bits, 2 extra bits kept after the first pass) along the last axis"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _ds(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _ds(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _ds(z1 + t13 * 6270, n)
    o[6] = _ds(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _ds(t4 + z1 + z3, n), _ds(t5 + z2 + z4, n), _ds(t6 + z2 + z3, n), _ds(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct(blocks: np.ndarray) -> np.ndarray:
    """int64 [..., 8, 8] samples (0..255) -> 8 x their DCT: rows first, then columns, on `sample - 128`"""
    rows = _dct_pass(blocks.astype(np.int64) - 128, True)
    return np.swapaxes(_dct_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantise(c: np.ndarray, divisors: np.ndarray) -> np.ndarray:
    """sign(c) ((|c| + (d >> 1)) // d), d = 8 Q"""
    d = divisors.astype(np.int64)
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def coefficients(u8: np.ndarray, quality: int = 75) -> np.ndarray:
    """uint8 [H,W,3] -> int16 [H/16][W/16][6][64]: the quantised coefficients in scan order, each block in zigzag order (what
    L2D_OP_JPEG_DCT writes)"""
    u8 = np.asarray(u8)
    if u8.dtype != np.uint8 or u8.ndim != 3 or u8.shape[2] != 3:
        raise ValueError(f"jpeg: expected uint8 [H,W,3], got {u8.dtype} {u8.shape}")
    H, W = u8.shape[:2]
    _check(H, W, quality)
    t = tables(quality)
    y, cb, cr = ycc420(u8)
    R, M = H // 16, W // 16
    yb = y.reshape(R, 2, 8, M, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(R, M, 4, 8, 8)          # Y00 Y01 Y10 Y11
    cbb = cb.reshape(R, 8, M, 8).transpose(0, 2, 1, 3)[:, :, None]
    crb = cr.reshape(R, 8, M, 8).transpose(0, 2, 1, 3)[:, :, None]
    div = t.divisors.reshape(2, 8, 8)
    q = np.concatenate([quantise(fdct(yb), div[0]), quantise(fdct(cbb), div[1]), quantise(fdct(crb), div[1])], 2)
    return q.reshape(R, M, 6, 64)[..., ZIGZAG].astype(np.int16)


def _bit_length(a: np.ndarray) -> np.ndarray:
    n = np.zeros(a.shape, np.int64)
    a = a.copy()
    while a.any():
        n += a > 0
        a >>= 1
    return n


def _row_symbols(row: np.ndarray, t: Tables):
    """int [M][6][64] quantised coefficients of one restart interval -> (value, bit count) of every coefficient position, in
    stream order.  Position k of a block carries everything the stream holds because of coefficient k: the ZRL codes of the zero
    run in front of it, its run / size code and its magnitude bits; the last non-zero position (position 0 if the AC part is
    empty) also carries the end-of-block code unless it is position 63.  At most 3 x 11 + 16 + 10 + 4 = 63 bits."""
    M = row.shape[0]
    v = row.astype(np.int64).copy()
    chroma = np.array([0, 0, 0, 0, 1, 1])
    # DC: the difference against the previous block of the same component, 0 in front of the first
    dc = v[:, :, 0]
    prev = np.zeros_like(dc)
    ys = dc[:, :4].reshape(-1)
    prev[:, :4] = np.concatenate([[0], ys[:-1]]).reshape(M, 4)
    prev[1:, 4:] = dc[:-1, 4:]
    v[:, :, 0] = dc - prev
    size = _bit_length(np.abs(v))
    mag = np.where(v < 0, v - 1, v) & ((1 << size) - 1)
    k = np.arange(64)
    nz = (v != 0) & (k > 0)
    last_nz = np.maximum.accumulate(np.where(nz, k, 0), axis=-1)                    # last non-zero position <= k (0: none)
    before = np.concatenate([np.zeros_like(last_nz[..., :1]), last_nz[..., :-1]], -1)
    run = k - before - 1
    tab = chroma[None, :, None]
    code = np.where(k == 0, t.dc[tab, np.minimum(size, 15)], t.ac[tab, ((run & 15) << 4) | np.minimum(size, 15)]).astype(np.int64)
    zrl, eob = t.ac[:, 0xF0].astype(np.int64)[tab], t.ac[:, 0x00].astype(np.int64)[tab]
    val, nbits = np.zeros_like(v), np.zeros_like(v)
    for i in range(3):                                                              # a run of up to 62 zeros: three ZRL at most
        more = nz & (run >= 16 * (i + 1))
        val = np.where(more, (val << (zrl >> 16)) | (zrl & 0xFFFF), val)
        nbits = nbits + np.where(more, zrl >> 16, 0)
    coded = nz | (k == 0)
    val = np.where(coded, (((val << (code >> 16)) | (code & 0xFFFF)) << size) | mag, 0)
    nbits = np.where(coded, nbits + (code >> 16) + size, 0)
    end = last_nz[..., 63:]
    ends = (k == end) & (end != 63)
    val = np.where(ends, (val << (eob >> 16)) | (eob & 0xFFFF), val)
    nbits = nbits + np.where(ends, eob >> 16, 0)
    return val.reshape(-1), nbits.reshape(-1)


def _row_bytes(row: np.ndarray, t: Tables) -> bytes:
    """one restart interval: the bits of its symbols, the last byte filled with 1-bits, 0x00 behind every 0xFF"""
    val, nbits = _row_symbols(row, t)
    keep = nbits > 0
    val, nbits = val[keep], nbits[keep]
    owner = np.repeat(np.arange(len(val)), nbits)                                   # the symbol of every bit of the stream
    pos = np.arange(len(owner)) - np.repeat(np.cumsum(nbits) - nbits, nbits)        # ... and its index in it, MSB first
    bits = ((val[owner] >> (nbits[owner] - 1 - pos)) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-len(bits) % 8, np.uint8)])
    data = np.packbits(bits)
    ff = np.nonzero(data == 0xFF)[0]
    return np.insert(data, ff + 1, 0).tobytes()


def encode_scan(coef: np.ndarray, quality: int = 75) -> bytes:
    """int16 [R][M][6][64] (`coefficients`) -> the entropy-coded data with its restart markers and the EOI"""
    t = tables(quality)
    R = coef.shape[0]
    out = []
    for r in range(R):
        out.append(_row_bytes(coef[r], t))
        out.append(bytes([0xFF, 0xD0 + (r & 7)]) if r + 1 < R else b"\xff\xd9")
    return b"".join(out)


def encode_ref(u8: np.ndarray, quality: int = 75) -> bytes:
    """uint8 [H,W,3] -> the JPEG file.  Readable rather than fast (tenths of a second at 512 x 512)."""
    u8 = np.asarray(u8)
    coef = coefficients(u8, quality)
    return header(u8.shape[0], u8.shape[1], quality) + encode_scan(coef, quality)


# ============================================================================= the decoder (csrc/jpeg_dec.hip)
# What arrives: the reference's demo receives every frame as a JPEG blob from the browser (demo/app.py:81-85, demo/util.py:22), a
# UVC camera delivers MJPEG.  `parse` reads the subset the device decodes (baseline, 8-bit, three components, 4:4:4 / 4:2:2 / 4:2:0,
# any Huffman tables, with or without restart markers), the `*_ref` functions restate libjpeg's decoder in numpy: integer arithmetic
# throughout, `decode_ref` is byte for byte what Pillow returns (tests/test_jpeg_dec_cpu.py).
class JpegUnsupported(ValueError):
    """a valid JPEG file outside the subset the device decodes (the wrapper hands it to Pillow on the host)"""


class JpegInfo(NamedTuple):
    height: int
    width: int
    hs: int                    # luminance sampling factors: (1, 1) 4:4:4, (2, 1) 4:2:2, (2, 2) 4:2:0; chrominance is 1 x 1
    vs: int
    quant: np.ndarray          # int32 [3][64], natural order, per component
    huffman: tuple             # 4 x (BITS tuple [16], values bytes) or None, slot = class * 2 + id: DC0 DC1 AC0 AC1
    dc_tab: tuple              # DC / AC table id of each component
    ac_tab: tuple
    restart_interval: int      # MCUs, 0 = none
    scan_offset: int           # byte offset of the entropy-coded data
    scan_end: int              # byte offset of the EOI marker

    @property
    def mcus_x(self) -> int:
        return -(-self.width // (8 * self.hs))

    @property
    def mcus_y(self) -> int:
        return -(-self.height // (8 * self.vs))

    @property
    def n_mcu(self) -> int:
        return self.mcus_x * self.mcus_y

    @property
    def blocks_per_mcu(self) -> int:
        return self.hs * self.vs + 2

    @property
    def chroma_size(self):
        """(rows, columns) of the real samples of a chrominance plane"""
        return -(-self.height // self.vs), -(-self.width // self.hs)


_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic-coded sequential",
              0xCA: "arithmetic-coded progressive", 0xCB: "arithmetic-coded lossless", 0xCD: "arithmetic-coded differential sequential",
              0xCE: "arithmetic-coded differential progressive", 0xCF: "arithmetic-coded differential lossless"}


def parse(data) -> JpegInfo:
    """The headers of a baseline file: SOI, skipped APPn / COM, DQT, SOF0, DHT, DRI, one interleaved SOS, and the EOI behind the scan.
    `JpegUnsupported` names what the device does not decode; structural damage is a plain ValueError."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise ValueError("jpeg: the data does not begin with SOI (FF D8)")
    quant, huff = {}, [None] * 4
    sof = sos = adobe = None
    ri = 0
    i = 2
    while True:
        if i + 2 > n:
            raise ValueError("jpeg: the headers end before a start of scan")
        if d[i] != 0xFF:
            raise ValueError(f"jpeg: byte {i} is 0x{d[i]:02x} where a marker was expected")
        while d[i + 1] == 0xFF:                                   # fill bytes
            i += 1
            if i + 2 > n:
                raise ValueError("jpeg: the headers end inside fill bytes")
        m = d[i + 1]
        i += 2
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise ValueError("jpeg: EOI before any scan")
        if i + 2 > n:
            raise ValueError(f"jpeg: segment FF {m:02X} has no length")
        L = (d[i] << 8) | d[i + 1]
        if L < 2 or i + L > n:
            raise ValueError(f"jpeg: segment FF {m:02X} at byte {i - 2} runs past the file ({L} bytes, {n - i} left)")
        seg = d[i + 2:i + L]
        i += L
        if m == 0xC0:
            if sof is not None:
                raise ValueError("jpeg: two frame headers")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise ValueError("jpeg: SOF0 has the wrong length")
            if seg[0] != 8:
                raise JpegUnsupported(f"jpeg: {seg[0]}-bit samples")
            H, W, nf = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nf != 3:
                raise JpegUnsupported(f"jpeg: {nf} component(s) ({'greyscale' if nf == 1 else 'CMYK / YCCK' if nf == 4 else 'not Y Cb Cr'})")
            if H == 0 or W == 0:
                raise JpegUnsupported("jpeg: a dimension of 0 (height given by a DNL segment)")
            sof = (H, W, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(3)])
        elif m in _SOF_NAMES:
            raise JpegUnsupported(f"jpeg: {_SOF_NAMES[m]} coding (SOF{m - 0xC0})")
        elif m == 0xCC:
            raise JpegUnsupported("jpeg: arithmetic coding (DAC segment)")
        elif m == 0xDB:
            k = 0
            while k < len(seg):
                pq, tq = seg[k] >> 4, seg[k] & 15
                if pq != 0:
                    raise JpegUnsupported("jpeg: a 16-bit quantisation table")
                if tq > 3 or k + 65 > len(seg):
                    raise ValueError("jpeg: damaged DQT segment")
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(seg, np.uint8, 64, k + 1)
                quant[tq] = t
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                if k + 17 > len(seg):
                    raise ValueError("jpeg: damaged DHT segment")
                tc, th = seg[k] >> 4, seg[k] & 15
                bits = tuple(seg[k + 1:k + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or k + 17 + cnt > len(seg):
                    raise ValueError("jpeg: damaged DHT segment")
                if th > 1:
                    raise JpegUnsupported(f"jpeg: Huffman table id {th} (baseline has 0 and 1)")
                vals = seg[k + 17:k + 17 + cnt]
                code = 0
                for length in range(16):
                    code = (code + bits[length]) << 1
                    if code > (2 << (length + 1)):
                        raise ValueError("jpeg: a DHT segment holds more codes than a prefix code has")
                if tc == 0 and any(v > 11 for v in vals):
                    raise ValueError("jpeg: a DC table names a size category above 11")
                huff[tc * 2 + th] = (bits, vals)
                k += 17 + cnt
        elif m == 0xDD:
            if len(seg) != 2:
                raise ValueError("jpeg: damaged DRI segment")
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if seg[:5] == b"Adobe" and len(seg) >= 12:
                adobe = seg[11]
        elif m == 0xDA:
            if sof is None:
                raise ValueError("jpeg: a scan before the frame header")
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise ValueError("jpeg: SOS has the wrong length")
            if seg[0] != 3:
                raise JpegUnsupported(f"jpeg: a scan of {seg[0]} component(s) (non-interleaved)")
            if [seg[1 + 2 * c] for c in range(3)] != [c[0] for c in sof[2]]:
                raise JpegUnsupported("jpeg: the scan lists the components in another order than the frame")
            if tuple(seg[7:10]) != (0, 63, 0):
                raise ValueError("jpeg: a baseline scan has Ss = 0, Se = 63, Ah = Al = 0")
            sos = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(3)]
            break
    H, W, comps = sof
    if adobe == 0:
        raise JpegUnsupported("jpeg: Adobe APP14 segment with transform 0 (the three components are R G B, not Y Cb Cr)")
    (_, hs, vs, _), c1, c2 = comps
    if (c1[1], c1[2], c2[1], c2[2]) != (1, 1, 1, 1) or (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
        raise JpegUnsupported("jpeg: sampling factors " + ", ".join(f"{c[1]}x{c[2]}" for c in comps) + " (4:4:4, 4:2:2 and 4:2:0 are decoded)")
    for c in range(3):
        if comps[c][3] not in quant:
            raise ValueError(f"jpeg: quantisation table {comps[c][3]} is missing")
        td, ta = sos[c]
        if td > 1 or ta > 1 or huff[td] is None or huff[2 + ta] is None:
            raise ValueError(f"jpeg: Huffman table DC {td} or AC {ta} is missing")
    end = d.rfind(b"\xff\xd9", i)
    if end < 0:
        raise ValueError("jpeg: no EOI behind the scan")
    return JpegInfo(H, W, hs, vs, np.stack([quant[c[3]] for c in comps]), tuple(huff), tuple(s[0] for s in sos),
                    tuple(s[1] for s in sos), ri, i, end)


def _block_component(info: JpegInfo):
    """component of every block of an MCU, in scan order"""
    return [0] * (info.hs * info.vs) + [1, 2]


def _decode_table(bits, vals):
    """uint32 [65536]: `length << 8 | symbol` of the code the next 16 bits begin with, 0 where no code matches"""
    out = np.zeros(65536, np.uint32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            out[lo:lo + (1 << (16 - length))] = (length << 8) | vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return out


class _Walk(NamedTuple):
    entry: np.ndarray          # int64 [n_mcu + 1]: bit offset of every MCU in the stuffed scan; [n_mcu] = 8 x the byte offset of the EOI
    pred: np.ndarray           # int16 [n_mcu][3]: the DC predictors in force in front of every MCU
    coef: np.ndarray           # int16 [n_mcu][blocks][64], absolute DC, natural order


@functools.lru_cache(maxsize=8)
def _walk_cached(d: bytes) -> _Walk:
    info = parse(d)
    scan = np.frombuffer(d, np.uint8, info.scan_end - info.scan_offset, info.scan_offset)
    # markers inside the scan: an FF followed by anything but a stuffed 00 or a further FF (fill bytes in front of a marker)
    ff = np.nonzero((scan[:-1] == 0xFF) & (scan[1:] != 0) & (scan[1:] != 0xFF))[0] if len(scan) > 1 else np.zeros(0, np.int64)
    n_mcu, ri = info.n_mcu, info.restart_interval
    n_int = -(-n_mcu // ri) if ri else 1
    if len(ff) != n_int - 1 or any(scan[p + 1] != 0xD0 + (j & 7) for j, p in enumerate(ff)):
        raise ValueError(f"jpeg: the scan holds {len(ff)} markers where {n_int - 1} restart markers in sequence were expected")
    bounds = [0] + [int(p) + 2 for p in ff], [int(p) for p in ff] + [len(scan)]
    tabs = [_decode_table(*t) if t is not None else None for t in info.huffman]
    comp = _block_component(info)
    entry = np.zeros(n_mcu + 1, np.int64)
    pred_at = np.zeros((n_mcu, 3), np.int16)
    coef = np.zeros((n_mcu, len(comp), 64), np.int16)
    zz = [int(v) for v in ZIGZAG]
    mcu = 0
    for lo, hi in zip(*bounds):
        while hi > lo and scan[hi - 1] == 0xFF:                       # fill bytes belong to the marker, not to the data
            hi -= 1
        raw = scan[lo:hi]
        drop = np.nonzero((raw[:-1] == 0xFF) & (raw[1:] == 0))[0] + 1 if len(raw) > 1 else np.zeros(0, np.int64)
        keep = np.ones(len(raw), bool)
        keep[drop] = False
        where = np.concatenate([np.nonzero(keep)[0] + lo, [hi]])        # raw byte of every unstuffed byte; behind the last: the marker
        u = raw[keep].tobytes() + b"\0\0\0\0"
        nbits = 8 * (len(u) - 4)
        p = 0

        def take(nb):
            nonlocal p
            w = int.from_bytes(u[p >> 3:(p >> 3) + 4], "big")
            v = (w >> (32 - nb - (p & 7))) & ((1 << nb) - 1)
            p += nb
            return v

        def symbol(tab):
            nonlocal p
            e = int(tab[take(16)])
            if e == 0:
                raise ValueError(f"jpeg: invalid Huffman code in MCU {mcu}")
            p -= 16 - (e >> 8)
            return e & 255

        pred = [0, 0, 0]
        count = min(ri, n_mcu - mcu) if ri else n_mcu
        for _ in range(count):
            entry[mcu] = int(where[p >> 3]) * 8 + (p & 7)
            pred_at[mcu] = pred
            for j, c in enumerate(comp):
                s = symbol(tabs[info.dc_tab[c]])
                v = take(s) if s else 0
                if s and v < (1 << (s - 1)):
                    v -= (1 << s) - 1
                pred[c] += v
                if not -32768 <= pred[c] <= 32767:
                    raise ValueError(f"jpeg: DC value out of range in MCU {mcu}")
                coef[mcu, j, 0] = pred[c]
                k = 1
                ac = tabs[2 + info.ac_tab[c]]
                while k < 64:
                    rs = symbol(ac)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16                                   # (a run that reaches the end ends the block, as in libjpeg)
                        continue
                    k += r
                    if k > 63:
                        raise ValueError(f"jpeg: coefficient index past 63 in MCU {mcu}")
                    v = take(s)
                    if v < (1 << (s - 1)):
                        v -= (1 << s) - 1
                    coef[mcu, j, zz[k]] = v
                    k += 1
                if p > nbits:
                    raise ValueError(f"jpeg: the bits run out in MCU {mcu}")
            mcu += 1
        if nbits - p >= 8:
            raise ValueError(f"jpeg: {nbits - p} bits are left behind MCU {mcu - 1}")
    if mcu != n_mcu:
        raise ValueError(f"jpeg: the scan holds {mcu} MCUs, the frame {n_mcu}")
    entry[n_mcu] = info.scan_end * 8 - info.scan_offset * 8
    for a in (entry, pred_at, coef):
        a.setflags(write=False)
    return _Walk(entry, pred_at, coef)


def chunk_layout(n_mcu: int, restart_interval: int, chunk_mcus: int):
    """(interval, chunk, chunks per interval, chunks): a chunk is `chunk` consecutive MCUs in raster order and never spans a restart
    marker -- chunks are counted from the start of every restart interval (without markers the scan is one interval), so a restart
    interval of at most `chunk_mcus` MCUs is a chunk itself.  Chunk c starts at MCU (c // per) * interval + (c % per) * chunk."""
    if chunk_mcus < 1:
        raise ValueError(f"jpeg: chunk_mcus={chunk_mcus!r} must be at least 1")
    interval = restart_interval if 0 < restart_interval < n_mcu else n_mcu
    chunk = min(int(chunk_mcus), interval)
    per = -(-interval // chunk)
    full = (n_mcu - 1) // interval
    return interval, chunk, per, full * per + -(-(n_mcu - full * interval) // chunk)


def index_ref(info: JpegInfo, data, chunk_mcus: int):
    """(bit_offsets int32 [C + 1], dc_pred int16 [C][3]): where every chunk (`chunk_layout`) begins, as a bit offset into the raw,
    still byte-stuffed scan (a position at a byte boundary behind an FF 00 pair counts behind the 00), and the three DC predictors
    in force there.  Behind a restart marker the offset is byte-aligned behind the RSTn and the predictors are 0.  The last offset
    is the EOI marker's."""
    w = _walk_cached(bytes(data))
    interval, chunk, per, C = chunk_layout(info.n_mcu, info.restart_interval, chunk_mcus)
    first = np.array([(c // per) * interval + (c % per) * chunk for c in range(C)], np.int64)
    return np.concatenate([w.entry[first], w.entry[-1:]]).astype(np.int32), w.pred[first].copy()


def decode_coefficients_ref(data) -> np.ndarray:
    """int16 [n_mcu][blocks per MCU][64]: the quantised coefficients, DC absolute, natural (de-zigzagged) order"""
    return _walk_cached(bytes(data)).coef


def _idct_pass(d, shift: int):
    """one pass of jidctint.c along the last axis, int32 arithmetic"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[..., i] for i in range(8))
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 + i6 * -15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)
    return np.stack([(v + (1 << (shift - 1))) >> shift for v in o], -1)


def idct_ref(blocks: np.ndarray) -> np.ndarray:
    """dequantised coefficients int [..., 64] (natural order) -> uint8 [..., 8, 8]: libjpeg's accurate integer IDCT (jidctint.c:
    13 constant bits, 2 extra bits kept after the column pass), `clamp(x + 128, 0, 255)` as its range limit.  int32 arithmetic that
    wraps, as the kernel's: |dequantised| <= 1024 cannot pass 2^31 anywhere, only a damaged file holds more."""
    b = np.asarray(blocks).astype(np.int32).reshape(blocks.shape[:-1] + (8, 8))
    ws = np.swapaxes(_idct_pass(np.swapaxes(b, -1, -2), 11), -1, -2)              # columns first
    return (np.clip(_idct_pass(ws, 18), -128, 127) + 128).astype(np.uint8)


def planes_ref(coef: np.ndarray, info: JpegInfo):
    """coefficients [n_mcu][blocks][64] -> the three uint8 component planes at their padded sizes (what L2D_OP_JPEG_IDCT writes)"""
    my, mx, hs, vs = info.mcus_y, info.mcus_x, info.hs, info.vs
    c = coef.astype(np.int32)
    ny = hs * vs
    y = idct_ref(c[:, :ny] * info.quant[0]).reshape(my, mx, vs, hs, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)
    out = [y]
    for k in (1, 2):
        out.append(idct_ref(c[:, ny + k - 1] * info.quant[k]).reshape(my, mx, 8, 8).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    return out


def upsample_ref(plane: np.ndarray, hs: int, vs: int, rows: int, cols: int) -> np.ndarray:
    """a chrominance plane with `rows` x `cols` real samples -> [rows * vs][cols * hs]: libjpeg's "fancy" triangle filters
    (jdsample.c).  h2v1: `(3 a + b + 1) >> 2` in even, `(3 a + b + 2) >> 2` in odd columns, the first and the last column copied.
    h2v2: `3 near + far` vertically (the row above row 0 is row 0, the row below the last REAL row is that row), then
    `(3 this + last + 8) >> 4` / `(3 this + next + 7) >> 4`, at the ends `(4 this + 8) >> 4` / `(4 this + 7) >> 4`.  A plane of
    one or two columns is replicated instead, as libjpeg does."""
    p = np.asarray(plane)[:rows, :cols].astype(np.int32)
    if hs == 1 and vs == 1:
        return p.astype(np.uint8)
    if cols <= 2:
        return np.repeat(np.repeat(p, vs, 0), hs, 1).astype(np.uint8)
    if vs == 1:
        last, nxt = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
        even, odd = (3 * p + last + 1) >> 2, (3 * p + nxt + 2) >> 2
        even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
        return np.stack([even, odd], -1).reshape(rows, 2 * cols).astype(np.uint8)
    up, down = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    s = np.stack([3 * p + up, 3 * p + down], 1).reshape(2 * rows, cols)           # column sums of output rows 2 r, 2 r + 1
    last, nxt = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    even, odd = (3 * s + last + 8) >> 4, (3 * s + nxt + 7) >> 4
    return np.stack([even, odd], -1).reshape(2 * rows, 2 * cols).astype(np.uint8)


def ycc_to_rgb_ref(y, cb, cr) -> np.ndarray:
    """three uint8 planes -> uint8 [H][W][3] with libjpeg's 16-bit fixed-point tables (jdcolor.c)"""
    y, cb, cr = (np.asarray(a).astype(np.int32) for a in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode_ref(data) -> np.ndarray:
    """the file -> uint8 [H][W][3], byte for byte `np.asarray(Image.open(BytesIO(data)).convert("RGB"))`"""
    d = bytes(data)
    info = parse(d)
    y, cb, cr = planes_ref(decode_coefficients_ref(d), info)
    rows, cols = info.chroma_size
    H, W = info.height, info.width
    cb, cr = (upsample_ref(p, info.hs, info.vs, rows, cols)[:H, :W] for p in (cb, cr))
    return ycc_to_rgb_ref(y[:H, :W], cb, cr)


# ----------------------------------------------------------------------------- what the device side uploads
DEC_LOOK_BITS = 8
DEC_TABLE_BYTES = 2 * 256 + 4 * 18 + 4 * 18 + 256         # lookahead uint16 [256], maxcode int32 [18], valoffset int32 [18], values [256]
DEC_QUANT_OFF = 4 * DEC_TABLE_BYTES
DEC_BLOB_BYTES = DEC_QUANT_OFF + 3 * 64 * 2               # + the quantisation tables, uint16 [3][64], natural order


@functools.lru_cache(maxsize=16)
def _huffman_blob(bits, vals) -> bytes:
    look = np.zeros(256, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        if bits[length - 1]:
            valoff[length] = k - code
            if length <= DEC_LOOK_BITS:
                sym = np.frombuffer(vals, np.uint8, bits[length - 1], k).astype(np.uint16)
                lo = code << (DEC_LOOK_BITS - length)
                n = 1 << (DEC_LOOK_BITS - length)
                look[lo:lo + n * len(sym)] = np.repeat((length << 8) | sym, n)
            code, k = code + bits[length - 1], k + bits[length - 1]
            maxcode[length] = code - 1
        code <<= 1
    return look.tobytes() + maxcode.tobytes() + valoff.tobytes() + bytes(vals) + bytes(256 - len(vals))


def table_blob(info: JpegInfo) -> np.ndarray:
    """uint8 [DEC_BLOB_BYTES]: per Huffman table slot (DC0 DC1 AC0 AC1) the 8-bit lookahead table (`length << 8 | symbol`, 0 = longer
    than 8 bits), libjpeg's maxcode / valoffset arrays for the longer codes and the values; then the quantisation tables"""
    parts = [_huffman_blob(*t) if t is not None else bytes(DEC_TABLE_BYTES) for t in info.huffman]
    return np.frombuffer(b"".join(parts) + info.quant.astype(np.uint16).tobytes(), np.uint8)
