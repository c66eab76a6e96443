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
