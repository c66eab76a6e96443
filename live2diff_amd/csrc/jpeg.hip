// Baseline JPEG encoder on the device (the format and its host restatement: live2diff_amd/jpeg.py).  The
// reference's demo encodes every output frame on the host (demo/util.py:27-37, `image.save(format="JPEG")`); here the decoder's
// fp16 output becomes the JPEG file in three launches and only the file crosses to the host.
//   jpeg_dct   colour conversion, 2 x 2 chroma down-sampling, libjpeg's accurate integer DCT and quantisation: one wave per MCU
//   jpeg_huff  one work-group per (frame, MCU row = restart interval): Huffman coding, padding, byte stuffing, RSTn / EOI
//   jpeg_pack  the rows copied contiguously behind the header, the file's length in front of it
// All arithmetic is integer: the output is the same file byte for byte as jpeg.encode_ref (tests/test_gpu_jpeg.py).
#include "common.h"

#define JPG_MAX_W 1920                  // 120 MCUs = 720 blocks per row: 155,520 bytes of unstuffed row in LDS (of 160 KB)
#define JPG_BLOCK_WORDS 54              // 64 symbols x (16 + 11) bits = 216 bytes: the bound on one unstuffed block (jpeg.capacity)
#define JPG_TAB 544                     // dc [2][16] + ac [2][256], `length << 16 | code` (jpeg.Tables.packed)
#define JPG_HUFF_NT 1024                // threads of the entropy coder: 16 waves share the <= 720 blocks of a row
#define JPG_HDR_OFF 16                  // the file starts 16 bytes into a frame's output slot; its length is the first word

__constant__ unsigned char jpg_base_q[128] = {
    16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24,  40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
    18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87,  103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99,
    17, 18, 24, 47, 99,  99,  99,  99,  18, 21, 26, 66, 99,  99,  99,  99,  24, 26, 56, 99,  99,  99,  99,  99,  47, 66, 99, 99, 99,  99,  99,  99,
    99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99,  99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99};
// natural index (row * 8 + column) -> position in zigzag order
__constant__ unsigned char jpg_zz_pos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                             41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                             46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// ------------------------------------------------------------------------------------------------------------------ jpeg_dct
__device__ __forceinline__ int jpg_ds(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint.c (13 constant bits, 2 extra bits kept after the first pass) over d[0..7], in place
template <bool FIRST>
__device__ __forceinline__ void jpg_dct8(int (&d)[8]) {
    constexpr int n = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : jpg_ds(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : jpg_ds(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2] = jpg_ds(z1 + t13 * 6270, n);
    d[6] = jpg_ds(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = jpg_ds(u4 + z1 + z3, n);
    d[5] = jpg_ds(u5 + z2 + z4, n);
    d[3] = jpg_ds(u6 + z2 + z3, n);
    d[1] = jpg_ds(u7 + z1 + z4, n);
}

// the egress op's expression (frame_io.hip): rint(255 clamp(fp16(fp16(x / 2) + 0.5), 0, 1)), half to even
__device__ __forceinline__ int jpg_u8(h16 x) {
    const h16 t = (h16)((float)x * 0.5f);
    float v = (float)(h16)((float)t + 0.5f);
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return (int)rintf(255.0f * v);
}

// One wave = one MCU (16 x 16 pixels -> Y00 Y01 Y10 Y11 Cb Cr), four MCUs per work-group.  A lane converts one 2 x 2 square of
// pixels (four Y samples, one Cb and one Cr sample); then 48 lanes take one row of one block each, and after a transposition
// through LDS one column each; the quantised block leaves in zigzag order as 16-byte stores.
template <bool U8>
__global__ __launch_bounds__(256) void jpeg_dct_kernel(const void *__restrict__ src, int16_t *__restrict__ coef, int B, int H, int W,
                                                       int quality) {
    __shared__ int s_div[128];
    __shared__ int s_ws[4][6][8][9];                                  // (a row of 9: lanes 8 words apart would share banks)
    __shared__ __attribute__((aligned(16))) short s_blk[4][384];      // the MCU's samples, later its quantised coefficients
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < 128) {
        const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        int q = ((int)jpg_base_q[tid] * s + 50) / 100;
        q = q < 1 ? 1 : (q > 255 ? 255 : q);
        s_div[tid] = q * 8;                                           // the DCT's output is 8 x the true DCT
    }
    const int M = W >> 4, R = H >> 4;
    const long long mcu = (long long)blockIdx.x * 4 + wave;
    const bool active = mcu < (long long)B * R * M;
    short *blk_s = s_blk[wave];
    if (active) {
        const int mx = (int)(mcu % M), r = (int)((mcu / M) % R), b = (int)(mcu / ((long long)M * R));
        const int cy = lane >> 3, cx = lane & 7;
        const int y0 = r * 16 + 2 * cy, x0 = mx * 16 + 2 * cx;
        int cbs = 0, crs = 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            int rgb[2][3];
            if (U8) {
                const uint8_t *p = (const uint8_t *)src + (((long long)b * H + y0 + dy) * W + x0) * 3;
#pragma unroll
                for (int e = 0; e < 6; ++e) rgb[e / 3][e % 3] = p[e];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const h16x2 v = *reinterpret_cast<const h16x2 *>((const h16 *)src + (((long long)b * 3 + c) * H + y0 + dy) * W + x0);
                    rgb[0][c] = jpg_u8(v[0]);
                    rgb[1][c] = jpg_u8(v[1]);
                }
            }
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int rr = rgb[dx][0], gg = rgb[dx][1], bb = rgb[dx][2];
                const int py = 2 * cy + dy, px = 2 * cx + dx;
                blk_s[((py >> 3) * 2 + (px >> 3)) * 64 + (py & 7) * 8 + (px & 7)] = (short)((19595 * rr + 38470 * gg + 7471 * bb + 32768) >> 16);
                cbs += (-11059 * rr - 21709 * gg + 32768 * bb + (128 << 16) + 32767) >> 16;
                crs += (32768 * rr - 27439 * gg - 5329 * bb + (128 << 16) + 32767) >> 16;
            }
        }
        const int bias = 1 + (cx & 1);                                // (the MCU starts at an even chroma column)
        blk_s[256 + lane] = (short)((cbs + bias) >> 2);
        blk_s[320 + lane] = (short)((crs + bias) >> 2);
    }
    __syncthreads();
    const int blk = lane >> 3, k = lane & 7;
    int d[8];
    if (active && lane < 48) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (int)blk_s[blk * 64 + k * 8 + i] - 128;
        jpg_dct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) s_ws[wave][blk][k][i] = d[i];
    }
    __syncthreads();
    if (active && lane < 48) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s_ws[wave][blk][i][k];
        jpg_dct8<false>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int nat = i * 8 + k;
            const int dv = s_div[(blk >= 4 ? 64 : 0) + nat];
            const int a = d[i] < 0 ? -d[i] : d[i];
            const int q = (int)((unsigned)(a + (dv >> 1)) / (unsigned)dv);
            blk_s[blk * 64 + jpg_zz_pos[nat]] = (short)(d[i] < 0 ? -q : q);
        }
    }
    __syncthreads();
    if (active && lane < 48) reinterpret_cast<uint4 *>(coef + mcu * 384)[lane] = reinterpret_cast<const uint4 *>(blk_s)[lane];
}

static int jpg_check_size(const char *what, const l2d_op *op, int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) {
        l2d_set_error("%s(tag %d): invalid arguments (non-positive size)", what, op->tag);
        return L2D_EINVAL;
    }
    if (H % 16 || W % 16) {
        l2d_set_error("%s(tag %d): %d x %d: height and width must be multiples of 16 (4:2:0 MCUs, no edge padding)", what, op->tag, H, W);
        return L2D_EINVAL;
    }
    if (W > JPG_MAX_W || H > 65520) {
        l2d_set_error("%s(tag %d): %d x %d: the width is limited to %d (an MCU row is entropy-coded in LDS), the height to 65520", what,
                      op->tag, H, W, JPG_MAX_W);
        return L2D_EINVAL;
    }
    if ((long long)B * H * W * 3 >= (1ll << 31)) {
        l2d_set_error("%s(tag %d): B H W 3 must stay below 2^31", what, op->tag);
        return L2D_EINVAL;
    }
    return L2D_OK;
}

int l2d_launch_jpeg_dct(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], H = op->i[1], W = op->i[2], u8 = op->i[3], quality = op->i[4];
    if (!op->p[0] || !op->p[1]) {
        l2d_set_error("jpeg_dct(tag %d): invalid arguments (null pointer)", op->tag);
        return L2D_EINVAL;
    }
    const int rc = jpg_check_size("jpeg_dct", op, B, H, W);
    if (rc != L2D_OK) return rc;
    if (quality < 1 || quality > 100) {
        l2d_set_error("jpeg_dct(tag %d): quality %d is outside 1..100", op->tag, quality);
        return L2D_EINVAL;
    }
    if ((u8 != 0 && u8 != 1) || (((uintptr_t)op->p[1]) & 15) || (!u8 && (((uintptr_t)op->p[0]) & 3))) {
        l2d_set_error("jpeg_dct(tag %d): source kind %d is not 0 (fp16 NCHW) or 1 (uint8 NHWC), or the coefficient buffer is not "
                      "16-byte / the fp16 source not 4-byte aligned", op->tag, u8);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const long long total = (long long)B * (H / 16) * (W / 16);
    const dim3 grid((unsigned)((total + 3) / 4));
    if (u8)
        hipLaunchKernelGGL(jpeg_dct_kernel<true>, grid, dim3(256), 0, s, op->p[0], (int16_t *)op->p[1], B, H, W, quality);
    else
        hipLaunchKernelGGL(jpeg_dct_kernel<false>, grid, dim3(256), 0, s, op->p[0], (int16_t *)op->p[1], B, H, W, quality);
    return l2d_check_launch("jpeg_dct", op->tag);
}

// ------------------------------------------------------------------------------------------------------------------ jpeg_huff
// What the stream holds because of coefficient `lane` of block `blk`: the ZRL codes of the zero run in front of it, its run / size
// code and its magnitude bits, and behind the last non-zero coefficient (the DC difference if the AC part is empty) the
// end-of-block code unless that is coefficient 63 -- at most 3 x 11 + 16 + 10 + 4 = 63 bits, right-aligned in `v`.  Nothing in it
// depends on another block's code: the DC predictor is the quantised DC of the previous block of the component, in `row`.
// `c` = jpg_coef(row, blk, lane): the caller loads the next block's while this one is coded.  Called by all 64 lanes of a wave (ballot).
__device__ __forceinline__ int jpg_coef(const int16_t *__restrict__ row, int blk, int lane) {
    int c = row[blk * 64 + lane];
    if (lane == 0) {
        const int j = blk % 6;
        const int prev = j == 0 ? blk - 3 : (j < 4 ? blk - 1 : blk - 6);      // Y00 follows the previous MCU's Y11
        if (prev >= 0) c -= row[prev * 64];
    }
    return c;
}

__device__ __forceinline__ int jpg_symbol(int c, int blk, int lane, const unsigned *s_tab, unsigned long long &v) {
    const int chroma = blk % 6 >= 4;
    const bool nz = lane > 0 && c != 0;
    const unsigned long long mask = __ballot(nz);
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int before = below ? 63 - __clzll((long long)below) : 0;
    const int last = mask ? 63 - __clzll((long long)mask) : 0;
    v = 0;
    if (!nz && lane != 0) return 0;
    const int run = lane == 0 ? 0 : lane - before - 1;
    const int a = c < 0 ? -c : c;
    int size = 32 - __clz(a);
    size = size > 15 ? 15 : size;
    const unsigned mag = (unsigned)(c < 0 ? c - 1 : c) & ((1u << size) - 1u);
    const unsigned *ac = s_tab + 32 + chroma * 256;
    const unsigned code = lane == 0 ? s_tab[chroma * 16 + size] : ac[((run & 15) << 4) | size];
    const unsigned zrl = ac[0xF0], eob = ac[0x00];
    int n = 0;
    for (int i = 0; i < (run >> 4); ++i) {
        v = (v << (zrl >> 16)) | (zrl & 0xFFFFu);
        n += (int)(zrl >> 16);
    }
    v = (((v << (code >> 16)) | (code & 0xFFFFu)) << size) | mag;
    n += (int)(code >> 16) + size;
    if (lane == last && last != 63) {
        v = (v << (eob >> 16)) | (eob & 0xFFFFu);
        n += (int)(eob >> 16);
    }
    return n;
}

__device__ __forceinline__ int jpg_wave_incl_scan(int x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// OR the low `n` bits of `v` (1 <= n <= 63) into the MSB-first bit stream `w` (big-endian 32-bit words) at bit `p`.  OR commutes,
// so the stream does not depend on the order in which lanes arrive.  Only non-zero words are touched: they lie inside the stream.
__device__ __forceinline__ void jpg_emit(unsigned *w, int p, unsigned long long v, int n) {
    const unsigned long long a = v << (64 - n);
    const int i = p >> 5, sh = p & 31;
    const unsigned long long hi = a >> sh;
    const unsigned w0 = (unsigned)(hi >> 32), w1 = (unsigned)hi, w2 = (unsigned)(a << (32 - sh));
    if (w0) atomicOr(&w[i], w0);
    if (w1) atomicOr(&w[i + 1], w1);
    if (w2) atomicOr(&w[i + 2], w2);
}

// One work-group per (MCU row, frame).  Pass 1: the bit length of every block; a scan gives every block its place.  Pass 2: the
// same symbols again, OR-ed into the zeroed row in LDS.  Then the last byte is filled with 1-bits and the row goes to its slot of
// the staging buffer with a 0x00 behind every 0xFF (a ballot per 1024 bytes gives each byte its shift), the marker behind it.
__global__ __launch_bounds__(JPG_HUFF_NT) void jpeg_huff_kernel(const int16_t *__restrict__ coef, const unsigned *__restrict__ tab,
                                                        uint8_t *__restrict__ staging, int *__restrict__ len, int R, int nblk,
                                                        int row_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jpg_smem[];
    unsigned *s_tab = reinterpret_cast<unsigned *>(jpg_smem);                  // [544]
    int *s_misc = reinterpret_cast<int *>(s_tab + JPG_TAB);                    // [48]: ballot counts [2][16], [32] the row's bits
    int *s_off = s_misc + 48;                                                  // [nblk rounded up to 4]
    unsigned *s_bits = reinterpret_cast<unsigned *>(s_off + ((nblk + 3) & ~3)); // [nblk * 54 + 4]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = blockIdx.x, b = blockIdx.y;
    const int16_t *row = coef + ((long long)b * R + r) * nblk * 64;
    constexpr int NT = JPG_HUFF_NT, NW = JPG_HUFF_NT / 64;
    for (int i = tid; i < JPG_TAB; i += NT) s_tab[i] = tab[i];
    __syncthreads();

    unsigned long long v;
    int c = wave < nblk ? jpg_coef(row, wave, lane) : 0;
    for (int blk = wave; blk < nblk; blk += NW) {
        const int cn = blk + NW < nblk ? jpg_coef(row, blk + NW, lane) : 0;
        int n = jpg_symbol(c, blk, lane, s_tab, v);
        c = cn;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) s_off[blk] = n;
    }
    __syncthreads();
    if (wave == 0) {                                                           // exclusive scan of <= 720 lengths, a chunk per lane
        const int per = (nblk + 63) >> 6;
        const int lo = min(lane * per, nblk), hi = min(lo + per, nblk);
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += s_off[i];
        const int incl = jpg_wave_incl_scan(sum, lane);
        int run = incl - sum;
        for (int i = lo; i < hi; ++i) {
            const int t = s_off[i];
            s_off[i] = run;
            run += t;
        }
        if (lane == 63) s_misc[32] = incl;
    }
    __syncthreads();
    const int limit = nblk * JPG_BLOCK_WORDS * 32;                              // (only tables that are no Huffman tables could exceed it)
    const int nbits = min(s_misc[32], limit);
    const int nbytes = (nbits + 7) >> 3;
    for (int i = tid; i < ((nbytes + 3) >> 2); i += NT) s_bits[i] = 0u;
    __syncthreads();

    c = wave < nblk ? jpg_coef(row, wave, lane) : 0;
    for (int blk = wave; blk < nblk; blk += NW) {
        const int cn = blk + NW < nblk ? jpg_coef(row, blk + NW, lane) : 0;
        const int n = jpg_symbol(c, blk, lane, s_tab, v);
        c = cn;
        const int incl = jpg_wave_incl_scan(n, lane);
        const int p = s_off[blk] + incl - n;
        if (n > 0 && p + n <= limit) jpg_emit(s_bits, p, v, n);
    }
    if (tid == 0 && (nbits & 7)) jpg_emit(s_bits, nbits, (1ull << (8 - (nbits & 7))) - 1ull, 8 - (nbits & 7));
    __syncthreads();

    uint8_t *dst = staging + ((long long)b * R + r) * row_stride;
    int base = 0;                                                              // the 0x00 bytes inserted so far
    for (int j0 = 0, it = 0; j0 < nbytes; j0 += NT, it ^= 1) {
        const int j = j0 + tid;
        const unsigned byte = j < nbytes ? (s_bits[j >> 2] >> (24 - 8 * (j & 3))) & 255u : 0u;
        const bool ff = byte == 255u;
        const unsigned long long m = __ballot(ff);
        if (lane == 0) s_misc[it * NW + wave] = __popcll(m);
        __syncthreads();
        int pre = __popcll(m & ((1ull << lane) - 1ull)), tot = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int cnt = s_misc[it * NW + w];
            pre += w < wave ? cnt : 0;
            tot += cnt;
        }
        if (j < nbytes) {
            dst[base + j + pre] = (uint8_t)byte;
            if (ff) dst[base + j + pre + 1] = 0;
        }
        base += tot;
    }
    if (tid == 0) {
        dst[nbytes + base] = 0xFF;
        dst[nbytes + base + 1] = (uint8_t)(r + 1 < R ? 0xD0 + (r & 7) : 0xD9);
        len[b * R + r] = nbytes + base + 2;
    }
}

static size_t jpg_huff_lds(int nblk) { return 4 * (size_t)(JPG_TAB + 48 + ((nblk + 3) & ~3) + nblk * JPG_BLOCK_WORDS + 4); }
static int jpg_row_capacity(int W) { return (W / 16) * 6 * 2 * JPG_BLOCK_WORDS * 4 + 4; }        // jpeg.row_capacity

int l2d_launch_jpeg_huff(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], H = op->i[1], W = op->i[2], row_stride = op->i[3];
    if (!op->p[0] || !op->p[1] || !op->p[2] || !op->p[3]) {
        l2d_set_error("jpeg_huff(tag %d): invalid arguments (null pointer)", op->tag);
        return L2D_EINVAL;
    }
    const int rc = jpg_check_size("jpeg_huff", op, B, H, W);
    if (rc != L2D_OK) return rc;
    if (row_stride < jpg_row_capacity(W) || (long long)B * (H / 16) * row_stride >= (1ll << 31)) {
        l2d_set_error("jpeg_huff(tag %d): row stride %d is below the worst case of a %d-wide MCU row (%d bytes), or the staging buffer "
                      "reaches 2^31 bytes", op->tag, row_stride, W, jpg_row_capacity(W));
        return L2D_EINVAL;
    }
    if ((((uintptr_t)op->p[0]) & 1) || (((uintptr_t)op->p[1]) & 3) || (((uintptr_t)op->p[3]) & 3)) {
        l2d_set_error("jpeg_huff(tag %d): coefficient / table / length buffer is misaligned", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const int nblk = (W / 16) * 6;
    const size_t lds = jpg_huff_lds(nblk);
    static size_t attr_dev[L2D_MAX_DEV] = {0};
    size_t &have = attr_dev[l2d_dev_ordinal()];
    if (lds > 64 * 1024 && have < lds) {
        if (hipFuncSetAttribute((const void *)jpeg_huff_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)jpg_huff_lds(JPG_MAX_W / 16 * 6)) ==
            hipSuccess)
            have = jpg_huff_lds(JPG_MAX_W / 16 * 6);
        else
            (void)hipGetLastError();
    }
    hipLaunchKernelGGL(jpeg_huff_kernel, dim3(H / 16, B), dim3(JPG_HUFF_NT), lds, s, (const int16_t *)op->p[0], (const unsigned *)op->p[1],
                       (uint8_t *)op->p[2], (int *)op->p[3], H / 16, nblk, row_stride);
    return l2d_check_launch("jpeg_huff", op->tag);
}

// ------------------------------------------------------------------------------------------------------------------ jpeg_pack
// One work-group per (MCU row, frame): the row's place is the sum of the lengths in front of it (at most a few hundred words, read
// by every lane alike); row 0 also writes the header, the last row the file's length.  A length outside [0, row_stride] cannot
// come out of jpeg_huff; it is clamped so that a stale buffer can never turn into a write outside the frame's slot.
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint8_t *__restrict__ staging, const int *__restrict__ len,
                                                        const uint8_t *__restrict__ hdr, uint8_t *__restrict__ out, int R, int row_stride,
                                                        int hdr_len, long long out_stride) {
    const int tid = threadIdx.x, r = blockIdx.x, b = blockIdx.y;
    const int *ln = len + b * R;
    long long off = 0;
    for (int i = 0; i < r; ++i) off += min(max(ln[i], 0), row_stride);
    const int n = min(max(ln[r], 0), row_stride);
    const uint8_t *src = staging + ((long long)b * R + r) * row_stride;
    uint8_t *frame = out + b * out_stride;
    uint8_t *dst = frame + JPG_HDR_OFF + hdr_len + off;
    for (int i = tid; i < n; i += 256) dst[i] = src[i];
    if (r == 0)
        for (int i = tid; i < hdr_len; i += 256) frame[JPG_HDR_OFF + i] = hdr[i];
    if (r == R - 1 && tid == 0) *reinterpret_cast<int *>(frame) = (int)(hdr_len + off + n);
}

int l2d_launch_jpeg_pack(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], H = op->i[1], row_stride = op->i[2], hdr_len = op->i[3];
    const long long out_stride = op->l[0];
    if (!op->p[0] || !op->p[1] || !op->p[2] || !op->p[3] || B <= 0 || H <= 0 || H % 16 || row_stride <= 0 || hdr_len <= 0) {
        l2d_set_error("jpeg_pack(tag %d): invalid arguments (null pointer, non-positive size, or H = %d is no multiple of 16)", op->tag, H);
        return L2D_EINVAL;
    }
    const long long need = JPG_HDR_OFF + (long long)hdr_len + (long long)(H / 16) * row_stride;
    if (out_stride < need || out_stride % 4 || need >= (1ll << 31) || (((uintptr_t)op->p[3]) & 3) || (((uintptr_t)op->p[1]) & 3)) {
        l2d_set_error("jpeg_pack(tag %d): output stride %lld is below 16 + header + rows x row stride = %lld, the file reaches 2^31 "
                      "bytes, or the output / length buffer is not 4-byte aligned", op->tag, out_stride, need);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(H / 16, B), dim3(256), 0, s, (const uint8_t *)op->p[0], (const int *)op->p[1],
                       (const uint8_t *)op->p[2], (uint8_t *)op->p[3], H / 16, row_stride, hdr_len, out_stride);
    return l2d_check_launch("jpeg_pack", op->tag);
}
