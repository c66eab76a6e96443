// The bit reader and Huffman decoder of the baseline JPEG decoder, shared by the host index (l2d_jpeg_index) and the entropy
// kernel (jpeg_dec.hip), and the host index itself.  Plain C++: this header also compiles alone for the CPU (the index was
// developed under -fsanitize=address,undefined on truncated files).  The format and its host restatement: live2diff_amd/jpeg.py.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define JPG_HD __host__ __device__ __forceinline__
#else
#define JPG_HD static inline
#endif

// the table blob (jpeg.table_blob): per Huffman table slot (DC0 DC1 AC0 AC1) the 8-bit lookahead table uint16 [256]
// (`length << 8 | symbol`, 0 = a longer code), maxcode int32 [18], valoffset int32 [18], values uint8 [256]; then the quantisation
// tables uint16 [3][64], natural order
#define JPG_DEC_TABLE 912
#define JPG_DEC_QUANT (4 * JPG_DEC_TABLE)
#define JPG_DEC_BLOB (JPG_DEC_QUANT + 3 * 64 * 2)

// zigzag position -> natural index (row * 8 + column): the one table, as the device's __constant__ array and the host model's
#define JPG_DEC_NAT_TABLE                                                                                                            \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

enum { JPG_ST_CODE = 1, JPG_ST_INDEX63 = 2, JPG_ST_POSITION = 4, JPG_ST_ARGS = 8 };

// MSB-first reader over the byte-stuffed scan `d[0, lim)`: bytes at and behind `lim` read as 0, so nothing outside is touched.
// The 00 behind an FF is skipped as the FF is loaded; `hist` remembers for the last 64 loaded bytes whether one was, which is
// what turns the reader's state back into a position in the stuffed stream.
struct JpgBits {
    const uint8_t *d;
    int bp, lim;                       // next byte to load
    unsigned long long acc, hist;      // unread bits, left-aligned
    int cnt;
};

// at least 32 unread bits afterwards: a code (<= 16) and its magnitude (<= 15).  Four bytes at once where none of them is an FF
// (the usual case), byte by byte otherwise.
JPG_HD void jpg_refill(JpgBits &b) {
    if (b.cnt < 32 && b.bp + 4 <= b.lim) {
        uint32_t w;
        __builtin_memcpy(&w, b.d + b.bp, 4);
        w = __builtin_bswap32(w);
        if ((((~w) - 0x01010101u) & w & 0x80808080u) == 0) {
            b.acc |= (unsigned long long)w << (32 - b.cnt);
            b.cnt += 32;
            b.bp += 4;
            b.hist <<= 4;
            return;
        }
    }
    while (b.cnt < 32) {               // at most 4 rounds
        const unsigned v = b.bp < b.lim ? b.d[b.bp] : 0u;
        ++b.bp;
        unsigned st = 0;
        if (v == 0xFFu && b.bp < b.lim && b.d[b.bp] == 0) {
            ++b.bp;
            st = 1;
        }
        b.acc |= (unsigned long long)v << (56 - b.cnt);
        b.cnt += 8;
        b.hist = (b.hist << 1) | st;
    }
}

JPG_HD void jpg_skip(JpgBits &b, int n) {
    b.acc <<= n;
    b.cnt -= n;
}

JPG_HD void jpg_open(JpgBits &b, const uint8_t *d, int lim, int bit) {
    b.d = d;
    b.lim = lim;
    b.bp = bit >> 3;
    b.acc = 0;
    b.hist = 0;
    b.cnt = 0;
    jpg_refill(b);
    jpg_skip(b, bit & 7);
}

// the position of the next unread bit in the stuffed stream (at a byte boundary behind an FF 00 pair: behind the 00)
JPG_HD int jpg_pos(const JpgBits &b) {
    const int nb = (b.cnt + 7) >> 3;   // (partly) unread bytes: the last nb that were loaded, 0..8 (cnt <= 63)
    const unsigned long long m = b.hist & ((1ull << nb) - 1ull);
    int s = 0;
    for (int i = 0; i < 8; ++i) s += (int)((m >> i) & 1ull);
    return (b.bp - nb - s) * 8 + ((8 - (b.cnt & 7)) & 7);
}

// where the data of an interval ends when its last symbol ends at `p`: the rest of a started byte is padding, and a padded
// byte that came out as FF has its 00 behind it
JPG_HD int jpg_padded_end(const JpgBits &b, int p) {
    if ((p & 7) == 0) return p;
    const int byte = p >> 3;
    const unsigned v = byte < b.lim ? b.d[byte] : 0u;
    return (byte + 1 + (v == 0xFFu ? 1 : 0)) * 8;
}

// the next Huffman symbol, or -1 for a bit pattern that is no code; needs <= 16 bits, leaves >= 16 for the magnitude
JPG_HD int jpg_symbol(JpgBits &b, const uint8_t *tab) {
    jpg_refill(b);
    const unsigned pk = (unsigned)(b.acc >> 48);
    const unsigned e = reinterpret_cast<const uint16_t *>(tab)[pk >> 8];
    if (e) {
        jpg_skip(b, (int)(e >> 8));
        return (int)(e & 255u);
    }
    const int32_t *maxcode = reinterpret_cast<const int32_t *>(tab + 512), *valoff = maxcode + 18;
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(pk >> (16 - l));
        if (code <= maxcode[l]) {
            jpg_skip(b, l);
            return tab[656 + ((code + valoff[l]) & 255)];
        }
    }
    return -1;
}

// `n` magnitude bits (1..15) as the signed value they stand for
JPG_HD int jpg_extend(JpgBits &b, int n) {
    const int v = (int)(b.acc >> (64 - n));
    jpg_skip(b, n);
    return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
}

// jpeg.chunk_layout: chunks never span a restart marker
struct JpgChunks {
    int interval, chunk, per, count;
};
JPG_HD JpgChunks jpg_chunks(int n_mcu, int ri, int chunk_mcus) {
    JpgChunks c;
    c.interval = ri > 0 && ri < n_mcu ? ri : n_mcu;
    c.chunk = chunk_mcus < c.interval ? chunk_mcus : c.interval;
    c.per = (c.interval + c.chunk - 1) / c.chunk;
    const int full = (n_mcu - 1) / c.interval;
    c.count = full * c.per + (n_mcu - full * c.interval + c.chunk - 1) / c.chunk;
    return c;
}

// What one lane of the entropy kernel does with chunk `c` (jpeg_dec.hip; l2d_jpeg_entropy_model runs the same code on the host):
// decode its MCUs from its entry point into `coef`, every coefficient written, and return 0 or the JPG_ST_* reason it stopped for.
// `tab` = the four Huffman tables of the blob, `nat` = zigzag position -> natural index, `tabs` = DC table ids in bits 0..2 and AC
// table ids in bits 4..6.  Every loop is bounded by what the host computed: `count` MCUs x blocks x at most 63 AC symbols, and the
// reader returns zeros behind the chunk's end (+ 16 bytes of look-ahead) instead of reading on.
JPG_HD int jpg_decode_chunk(int c, const uint8_t *file, const int *offsets, const int16_t *dc_pred, const uint8_t *tab,
                            const uint8_t *nat, const int *params, int16_t *coef, int n_mcu, int ny, JpgChunks ck, int cap, int tabs) {
    int scan = params[0], flen = params[1];
    flen = flen < 0 ? 0 : (flen > cap ? cap : flen);
    scan = scan < 0 ? 0 : (scan > flen ? flen : scan);
    const int lim = flen - scan;
    const int lo = offsets[c], hi = offsets[c + 1];
    if (lo < 0 || hi < lo || hi > lim * 8) return JPG_ST_ARGS;
    const int sub = c % ck.per, mcu0 = (c / ck.per) * ck.interval + sub * ck.chunk;
    int count = ck.chunk < ck.interval - sub * ck.chunk ? ck.chunk : ck.interval - sub * ck.chunk;
    count = count < n_mcu - mcu0 ? count : n_mcu - mcu0;
    int p0 = dc_pred[c * 3], p1 = dc_pred[c * 3 + 1], p2 = dc_pred[c * 3 + 2];
    JpgBits b;
    jpg_open(b, file + scan, lim < (hi >> 3) + 16 ? lim : (hi >> 3) + 16, lo);
    const int bpm = ny + 2;
    for (int m = 0; m < count; ++m) {
        for (int j = 0; j < bpm; ++j) {
            int16_t *blk = coef + ((long long)(mcu0 + m) * bpm + j) * 64;
            for (int i = 0; i < 16; ++i) reinterpret_cast<unsigned long long *>(blk)[i] = 0ull;
            const int comp = j < ny ? 0 : j - ny + 1;
            const uint8_t *ac = tab + (2 + ((tabs >> (4 + comp)) & 1)) * JPG_DEC_TABLE;
            int s = jpg_symbol(b, tab + ((tabs >> comp) & 1) * JPG_DEC_TABLE);
            if (s < 0 || s > 11) return JPG_ST_CODE;
            const int diff = s ? jpg_extend(b, s) : 0;
            int v;
            if (comp == 0) v = p0 += diff;
            else if (comp == 1) v = p1 += diff;
            else v = p2 += diff;
            blk[0] = (int16_t)v;
            int k = 1;
            for (int it = 0; it < 63 && k < 64; ++it) {
                const int rs = jpg_symbol(b, ac);
                if (rs < 0) return JPG_ST_CODE;
                s = rs & 15;
                if (s == 0) {                      // end of block, or a run of 16 zeros (one that reaches the end ends the block, as in libjpeg)
                    if (rs != 0xF0) break;
                    k += 16;
                    continue;
                }
                k += rs >> 4;
                if (k > 63) return JPG_ST_INDEX63;
                blk[nat[k++]] = (int16_t)jpg_extend(b, s);
            }
        }
    }
    // a chunk ends where the next begins; in front of a marker the rest of the byte is padding, and RSTn is two bytes
    const int p = jpg_pos(b);
    const bool last = c == ck.count - 1, at_marker = sub == ck.per - 1 || mcu0 + count >= n_mcu;
    if (!at_marker) return p == hi ? 0 : JPG_ST_POSITION;
    // the marker's FF: RSTn lies two bytes in front of the next entry, the last entry is the EOI's own; in front of it, fill bytes (FF) only
    const int first = jpg_padded_end(b, p) >> 3, marker = (hi >> 3) - (last ? 0 : 2);
    if (marker < first) return JPG_ST_POSITION;
    for (int i = first; i <= marker; ++i)
        if (i >= lim || (file + scan)[i] != 0xFFu) return JPG_ST_POSITION;
    return 0;
}

// layout: scan offset, MCUs, luminance blocks per MCU (1 | 2 | 4), restart interval, chunk_mcus, DC table of the three
// components, AC table of the three components, number of chunks the output arrays hold.  Returns 0, or a negative value and a
// message in `err`: -1 arguments, -2 invalid code, -3 coefficient index past 63, -4 the bits run out, -5 markers / MCU count.
static int jpg_index(const uint8_t *file, int64_t len, const uint8_t *blob, const int32_t *lay, int32_t *offsets, int16_t *pred,
                     const char **err) {
    const int scan = lay[0], n_mcu = lay[1], ny = lay[2], ri = lay[3], chunk_mcus = lay[4];
    *err = "";
    if (!file || !blob || !offsets || !pred || len <= 0 || len >= (1ll << 28) || scan < 0 || scan > len || n_mcu <= 0 ||
        (ny != 1 && ny != 2 && ny != 4) || ri < 0 || chunk_mcus <= 0) {
        *err = "invalid arguments";
        return -1;
    }
    for (int k = 5; k < 11; ++k)
        if (lay[k] < 0 || lay[k] > 1) {
            *err = "a Huffman table id is not 0 or 1";
            return -1;
        }
    const JpgChunks ck = jpg_chunks(n_mcu, ri, chunk_mcus);
    if (ck.count != lay[11]) {
        *err = "the number of chunks does not follow from the MCU count, the restart interval and chunk_mcus";
        return -1;
    }
    const uint8_t *d = file + scan;
    const int lim = (int)(len - scan);
    const int n_int = (n_mcu + ck.interval - 1) / ck.interval;
    if (ck.chunk == ck.interval) {                                 // every chunk is a restart interval: a search for the markers
        int c = 0, at = 0;
        memset(pred, 0, sizeof(int16_t) * 3 * (size_t)ck.count);
        offsets[0] = 0;
        while (true) {
            const uint8_t *f = at < lim ? (const uint8_t *)memchr(d + at, 0xFF, (size_t)(lim - at)) : nullptr;
            if (!f || f - d + 1 >= lim) {
                *err = "no EOI behind the scan";
                return -4;
            }
            at = (int)(f - d);
            const unsigned m = d[at + 1];
            if (m == 0) {
                at += 2;
            } else if (m == 0xFF) {                                 // a fill byte in front of a marker
                at += 1;
            } else if (m == 0xD9) {
                if (c != n_int - 1) {
                    *err = "EOI before the last restart interval";
                    return -5;
                }
                offsets[ck.count] = at * 8;
                return 0;
            } else if (m == (0xD0u | (unsigned)(c & 7)) && c + 1 < n_int) {
                at += 2;
                offsets[++c] = at * 8;
            } else {
                *err = "a marker inside the scan that is not the next restart marker";
                return -5;
            }
        }
    }
    int mcu = 0, c = 0, start = 0;
    JpgBits b;
    for (int itv = 0; itv < n_int; ++itv) {
        if (start > lim * 8) {
            *err = "the bits run out";
            return -4;
        }
        jpg_open(b, d, lim, start);
        int p[3] = {0, 0, 0};
        const int count = n_mcu - mcu < ck.interval ? n_mcu - mcu : ck.interval;
        for (int m = 0; m < count; ++m, ++mcu) {
            if (m % ck.chunk == 0) {
                offsets[c] = jpg_pos(b);
                pred[c * 3] = (int16_t)p[0];
                pred[c * 3 + 1] = (int16_t)p[1];
                pred[c * 3 + 2] = (int16_t)p[2];
                ++c;
            }
            for (int j = 0; j < ny + 2; ++j) {
                const int comp = j < ny ? 0 : j - ny + 1;
                const uint8_t *ac = blob + (2 + lay[8 + comp]) * JPG_DEC_TABLE;
                int s = jpg_symbol(b, blob + lay[5 + comp] * JPG_DEC_TABLE);
                if (s < 0 || s > 11) {
                    *err = "invalid Huffman code (DC)";
                    return -2;
                }
                if (s) p[comp] += jpg_extend(b, s);
                if (p[comp] < -32768 || p[comp] > 32767) {
                    *err = "DC value out of range";
                    return -2;
                }
                int k = 1;
                while (k < 64) {                                   // code lengths only: no coefficient is reconstructed
                    const int rs = jpg_symbol(b, ac);
                    if (rs < 0) {
                        *err = "invalid Huffman code (AC)";
                        return -2;
                    }
                    s = rs & 15;
                    if (s == 0) {
                        if (rs != 0xF0) break;
                        k += 16;                                   // (a run that reaches the end ends the block, as in libjpeg)
                        continue;
                    }
                    k += rs >> 4;
                    if (k > 63) {
                        *err = "coefficient index past 63";
                        return -3;
                    }
                    jpg_skip(b, s);
                    ++k;
                }
            }
            if (b.bp > lim + 16) {                                 // (the reader feeds zeros behind the end: the walk would end, only later)
                *err = "the bits run out";
                return -4;
            }
        }
        const int end = jpg_padded_end(b, jpg_pos(b));
        int at = end >> 3;
        while (at + 2 < lim && d[at] == 0xFF && d[at + 1] == 0xFF) ++at;      // fill bytes
        if (at + 2 > lim || d[at] != 0xFF || d[at + 1] != (itv + 1 < n_int ? (0xD0u | (unsigned)(itv & 7)) : 0xD9u)) {
            *err = itv + 1 < n_int ? "no restart marker behind a restart interval" : "no EOI behind the last MCU (the MCU count does not match the frame)";
            return -5;
        }
        start = (at + 2) * 8;
        if (itv + 1 == n_int) offsets[ck.count] = at * 8;
    }
    return 0;
}
