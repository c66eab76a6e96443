// Baseline JPEG decoder on the device (the format and its host restatement: live2diff_amd/jpeg.py).  The
// reference's demo receives every frame as a JPEG blob and decodes it on the host (demo/app.py:81-85, demo/util.py:22,
// `Image.open`); here the compressed file is uploaded and becomes the uint8 frame the ingest op reads in three launches.
//   l2d_jpeg_index    host: where every chunk of MCUs begins in the scan and the DC predictors there -- the only serial part of
//                     a baseline scan: one walk over code lengths, or a byte search when restart markers give the entries
//   jpeg_entropy_dec  one lane per chunk: Huffman decoding from its entry point, absolute DC, every coefficient written
//   jpeg_idct         dequantisation and libjpeg's accurate integer IDCT, 8 blocks per wave -> uint8 component planes
//   jpeg_rgb          libjpeg's "fancy" chroma up-sampling and the colour conversion -> uint8 [H][W][3]
// All arithmetic is integer: the frame equals jpeg.decode_ref (and Pillow's) byte for byte (tests/test_gpu_jpeg_dec.py).
#include "common.h"
#include "jpeg_index.h"

__constant__ unsigned char jpg_dec_nat[64] = JPG_DEC_NAT_TABLE;

// ------------------------------------------------------------------------------------------------------------ jpeg_entropy_dec
// One lane per chunk (jpg_decode_chunk, jpeg_index.h), one wave per work-group (the kernel is latency-bound: small groups spread
// the chunks over the CUs); the Huffman tables are in LDS.  A lane that meets an invalid code, a coefficient index past 63, or
// does not end where the next chunk begins ORs its reason into the status word and stops; it waits for nobody.
__global__ __launch_bounds__(64) void jpeg_entropy_dec_kernel(const uint8_t *__restrict__ file, const int *__restrict__ offsets,
                                                              const int16_t *__restrict__ dc_pred, const uint8_t *__restrict__ blob,
                                                              const int *__restrict__ params, int16_t *__restrict__ coef,
                                                              int *__restrict__ status, int n_mcu, int ny, JpgChunks ck, int cap,
                                                              int tabs) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tab[JPG_DEC_QUANT];
    __shared__ uint8_t s_nat[64];
    const int lane = threadIdx.x;
    for (int i = lane; i < JPG_DEC_QUANT / 4; i += 64) reinterpret_cast<uint32_t *>(s_tab)[i] = reinterpret_cast<const uint32_t *>(blob)[i];
    s_nat[lane] = jpg_dec_nat[lane];
    __syncthreads();
    const int c = blockIdx.x * 64 + lane;
    if (c >= ck.count) return;
    const int err = jpg_decode_chunk(c, file, offsets, dc_pred, s_tab, s_nat, params, coef, n_mcu, ny, ck, cap, tabs);
    if (err) atomicOr(status, err);
}

static int jpg_dec_layout(const char *what, const l2d_op *op, int n_mcu, int ny) {
    if (n_mcu <= 0 || (ny != 1 && ny != 2 && ny != 4)) {
        l2d_set_error("%s(tag %d): %d MCUs of %d luminance blocks: the count must be positive, the blocks 1 (4:4:4), 2 (4:2:2) or 4 (4:2:0)",
                      what, op->tag, n_mcu, ny);
        return L2D_EINVAL;
    }
    if ((long long)n_mcu * (ny + 2) * 64 >= (1ll << 31)) {
        l2d_set_error("%s(tag %d): the coefficient buffer reaches 2^31 elements", what, op->tag);
        return L2D_EINVAL;
    }
    return L2D_OK;
}

int l2d_launch_jpeg_entropy_dec(const l2d_op *op, hipStream_t s) {
    const int n_mcu = op->i[0], ny = op->i[1], ri = op->i[2], chunk_mcus = op->i[3], C = op->i[4], cap = op->i[5];
    for (int k = 0; k < 7; ++k)
        if (!op->p[k]) {
            l2d_set_error("jpeg_entropy_dec(tag %d): invalid arguments (null pointer)", op->tag);
            return L2D_EINVAL;
        }
    const int rc = jpg_dec_layout("jpeg_entropy_dec", op, n_mcu, ny);
    if (rc != L2D_OK) return rc;
    if (ri < 0 || chunk_mcus <= 0 || jpg_chunks(n_mcu, ri, chunk_mcus).count != C) {
        l2d_set_error("jpeg_entropy_dec(tag %d): %d chunks do not follow from %d MCUs, restart interval %d and chunk_mcus %d", op->tag, C,
                      n_mcu, ri, chunk_mcus);
        return L2D_EINVAL;
    }
    if (cap <= 0 || cap >= (1 << 28)) {
        l2d_set_error("jpeg_entropy_dec(tag %d): file capacity %d is outside 1 .. 2^28 - 1 (bit offsets are int32)", op->tag, cap);
        return L2D_EINVAL;
    }
    int tabs = 0;
    for (int k = 0; k < 3; ++k) {
        if ((op->i[6 + k] | op->i[9 + k]) & ~1) {
            l2d_set_error("jpeg_entropy_dec(tag %d): a Huffman table id is not 0 or 1", op->tag);
            return L2D_EINVAL;
        }
        tabs |= (op->i[6 + k] << k) | (op->i[9 + k] << (4 + k));
    }
    if ((((uintptr_t)op->p[1]) & 3) || (((uintptr_t)op->p[2]) & 1) || (((uintptr_t)op->p[3]) & 3) || (((uintptr_t)op->p[4]) & 3) ||
        (((uintptr_t)op->p[5]) & 15) || (((uintptr_t)op->p[6]) & 3)) {
        l2d_set_error("jpeg_entropy_dec(tag %d): index / table / parameter / status buffer is misaligned, or the coefficient buffer is not "
                      "16-byte aligned", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    hipLaunchKernelGGL(jpeg_entropy_dec_kernel, dim3((C + 63) / 64), dim3(64), 0, s, (const uint8_t *)op->p[0], (const int *)op->p[1],
                       (const int16_t *)op->p[2], (const uint8_t *)op->p[3], (const int *)op->p[4], (int16_t *)op->p[5], (int *)op->p[6], n_mcu,
                       ny, jpg_chunks(n_mcu, ri, chunk_mcus), cap, tabs);
    return l2d_check_launch("jpeg_entropy_dec", op->tag);
}

// ------------------------------------------------------------------------------------------------------------------ jpeg_idct
// one pass of jidctint.c (13 constant bits) over d[0..7], in place; SHIFT = 11 behind the column pass (2 extra bits kept), 18
// behind the row pass.  32-bit two's-complement arithmetic that WRAPS (unsigned operations, an arithmetic shift at the end), as
// jpeg.idct_ref does: no picture comes near the range (|dequantised| <= 1024 cannot pass 2^31 anywhere), and coefficients only
// a damaged file holds give a defined, repeatable result instead of undefined behaviour.
template <int SHIFT>
__device__ __forceinline__ void jpg_idct8(unsigned (&d)[8]) {
    typedef unsigned U;
    U z1 = (d[2] + d[6]) * 4433u;
    U t2 = z1 + d[6] * (U)-15137, t3 = z1 + d[2] * 6270u;
    U t0 = (d[0] + d[4]) * 8192u, t1 = (d[0] - d[4]) * 8192u;
    const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7];
    t1 = d[5];
    t2 = d[3];
    t3 = d[1];
    z1 = t0 + t3;
    U z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const U z5 = (z3 + z4) * 9633u;
    t0 *= 2446u;
    t1 *= 16819u;
    t2 *= 25172u;
    t3 *= 12299u;
    z1 *= (U)-7373;
    z2 *= (U)-20995;
    z3 = z3 * (U)-16069 + z5;
    z4 = z4 * (U)-3196 + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    constexpr U r = 1u << (SHIFT - 1);
    d[0] = (U)((int)(t10 + t3 + r) >> SHIFT);
    d[7] = (U)((int)(t10 - t3 + r) >> SHIFT);
    d[1] = (U)((int)(t11 + t2 + r) >> SHIFT);
    d[6] = (U)((int)(t11 - t2 + r) >> SHIFT);
    d[2] = (U)((int)(t12 + t1 + r) >> SHIFT);
    d[5] = (U)((int)(t12 - t1 + r) >> SHIFT);
    d[3] = (U)((int)(t13 + t0 + r) >> SHIFT);
    d[4] = (U)((int)(t13 - t0 + r) >> SHIFT);
}

// 8 lanes per block, 32 blocks per work-group.  A lane loads one row of its block (16 bytes) and dequantises it; through LDS it
// takes a column for the first pass (libjpeg's order: columns, then rows), and through LDS again a row for the second; the row
// leaves as one 8-byte store into its component's plane.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t *__restrict__ coef, const uint16_t *__restrict__ quant,
                                                        uint8_t *__restrict__ planes, int n_mcu, int mx, int hs, int vs) {
    __shared__ int s_q[192];
    __shared__ unsigned s_ws[32][8][9];                                  // (a row of 9: lanes 8 words apart would share banks)
    const int tid = threadIdx.x, slot = tid >> 3, k = tid & 7;
    if (tid < 192) s_q[tid] = quant[tid];
    __syncthreads();
    const int ny = hs * vs, bpm = ny + 2;
    const long long g = (long long)blockIdx.x * 32 + slot;
    const bool active = g < (long long)n_mcu * bpm;
    unsigned d[8];
    int comp = 0;
    if (active) {
        const int j = (int)(g % bpm);
        comp = j < ny ? 0 : j - ny + 1;
        const uint4 raw = reinterpret_cast<const uint4 *>(coef + g * 64)[k];
        const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int v = (int)(short)(w[i >> 1] >> (16 * (i & 1)));
            s_ws[slot][k][i] = (unsigned)v * (unsigned)s_q[comp * 64 + k * 8 + i];
        }
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s_ws[slot][i][k];
        jpg_idct8<11>(d);
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s_ws[slot][i][k] = d[i];
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s_ws[slot][k][i];
        jpg_idct8<18>(d);
        unsigned out[2] = {0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int v = min(max((int)d[i], -128), 127) + 128;
            out[i >> 2] |= (unsigned)v << (8 * (i & 3));
        }
        const int mcu = (int)(g / bpm), j = (int)(g % bpm);
        const int my = n_mcu / mx, mcx = mcu % mx, mcy = mcu / mx;
        const long long ysize = (long long)my * vs * 8 * mx * hs * 8, csize = (long long)my * 8 * mx * 8;
        long long at;
        if (comp == 0) {
            const int bx = mcx * hs + j % hs, by = mcy * vs + j / hs;
            at = ((long long)by * 8 + k) * (mx * hs * 8) + bx * 8;
        } else {
            at = ysize + (comp - 1) * csize + ((long long)mcy * 8 + k) * (mx * 8) + mcx * 8;
        }
        *reinterpret_cast<uint2 *>(planes + at) = make_uint2(out[0], out[1]);
    }
}

static int jpg_dec_sampling(const char *what, const l2d_op *op, int hs, int vs) {
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) {
        l2d_set_error("%s(tag %d): luminance sampling %d x %d is not 1 x 1 (4:4:4), 2 x 1 (4:2:2) or 2 x 2 (4:2:0)", what, op->tag, hs, vs);
        return L2D_EINVAL;
    }
    return L2D_OK;
}

int l2d_launch_jpeg_idct(const l2d_op *op, hipStream_t s) {
    const int n_mcu = op->i[0], mx = op->i[1], hs = op->i[2], vs = op->i[3];
    if (!op->p[0] || !op->p[1] || !op->p[2]) {
        l2d_set_error("jpeg_idct(tag %d): invalid arguments (null pointer)", op->tag);
        return L2D_EINVAL;
    }
    int rc = jpg_dec_sampling("jpeg_idct", op, hs, vs);
    if (rc != L2D_OK) return rc;
    rc = jpg_dec_layout("jpeg_idct", op, n_mcu, hs * vs);
    if (rc != L2D_OK) return rc;
    if (mx <= 0 || n_mcu % mx) {
        l2d_set_error("jpeg_idct(tag %d): %d MCUs are no whole rows of %d", op->tag, n_mcu, mx);
        return L2D_EINVAL;
    }
    if ((((uintptr_t)op->p[0]) & 15) || (((uintptr_t)op->p[1]) & 1) || (((uintptr_t)op->p[2]) & 7)) {
        l2d_set_error("jpeg_idct(tag %d): the coefficient buffer is not 16-byte, the planes are not 8-byte or the tables not 2-byte aligned",
                      op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const long long blocks = (long long)n_mcu * (hs * vs + 2);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + 31) / 32)), dim3(256), 0, s, (const int16_t *)op->p[0],
                       (const uint16_t *)op->p[1], (uint8_t *)op->p[2], n_mcu, mx, hs, vs);
    return l2d_check_launch("jpeg_idct", op->tag);
}

// ------------------------------------------------------------------------------------------------------------------- jpeg_rgb
// libjpeg's "fancy" up-sampling (jdsample.c) as a gather: the chrominance sample of pixel (x, y) from its up to four neighbours in
// the down-sampled plane.  `cw` x `ch` are the REAL samples of the plane (the bottom edge repeats the last real row, the last
// column is copied), `pw` its padded row length.  A plane of one or two columns is replicated, as libjpeg does.
__device__ __forceinline__ int jpg_chroma(const uint8_t *__restrict__ p, int x, int y, int hs, int vs, int cw, int ch, int pw) {
    if (hs == 1) return p[(long long)y * pw + x];
    const int cx = x >> 1;
    if (cw <= 2) return p[(long long)(vs == 2 ? y >> 1 : y) * pw + cx];
    const int side = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
    if (vs == 1) {
        const uint8_t *r = p + (long long)y * pw;
        return side == cx ? r[cx] : (3 * r[cx] + r[side] + 1 + (x & 1)) >> 2;
    }
    const int cy = y >> 1, far = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    const uint8_t *n = p + (long long)cy * pw, *f = p + (long long)far * pw;
    const int here = 3 * n[cx] + f[cx], there = 3 * n[side] + f[side];
    return (3 * here + there + 8 - (x & 1)) >> 4;
}

// one thread per pixel pair (x even, x + 1)
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const uint8_t *__restrict__ planes, uint8_t *__restrict__ out, int H, int W, int hs,
                                                       int vs, int mx, int my) {
    const int pairs = (W + 1) >> 1;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)pairs * H) return;
    const int y = (int)(t / pairs), x0 = (int)(t % pairs) * 2;
    const int yw = mx * hs * 8, pw = mx * 8;
    const long long ysize = (long long)my * vs * 8 * yw, csize = (long long)my * 8 * pw;
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    const uint8_t *cbp = planes + ysize, *crp = cbp + csize;
    for (int x = x0; x < min(x0 + 2, W); ++x) {
        const int yy = planes[(long long)y * yw + x];
        const int cb = jpg_chroma(cbp, x, y, hs, vs, cw, ch, pw) - 128, cr = jpg_chroma(crp, x, y, hs, vs, cw, ch, pw) - 128;
        const int r = yy + ((91881 * cr + 32768) >> 16);
        const int g = yy + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        const int b = yy + ((116130 * cb + 32768) >> 16);
        uint8_t *o = out + ((long long)y * W + x) * 3;
        o[0] = (uint8_t)min(max(r, 0), 255);
        o[1] = (uint8_t)min(max(g, 0), 255);
        o[2] = (uint8_t)min(max(b, 0), 255);
    }
}

int l2d_launch_jpeg_rgb(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], hs = op->i[2], vs = op->i[3];
    if (!op->p[0] || !op->p[1]) {
        l2d_set_error("jpeg_rgb(tag %d): invalid arguments (null pointer)", op->tag);
        return L2D_EINVAL;
    }
    const int rc = jpg_dec_sampling("jpeg_rgb", op, hs, vs);
    if (rc != L2D_OK) return rc;
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (long long)H * W * 3 >= (1ll << 31)) {
        l2d_set_error("jpeg_rgb(tag %d): %d x %d: a JPEG dimension is 1 .. 65535 and H W 3 must stay below 2^31", op->tag, H, W);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const int mx = (W + 8 * hs - 1) / (8 * hs), my = (H + 8 * vs - 1) / (8 * vs);
    const long long threads = (long long)((W + 1) >> 1) * H;
    hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, (const uint8_t *)op->p[0], (uint8_t *)op->p[1],
                       H, W, hs, vs, mx, my);
    return l2d_check_launch("jpeg_rgb", op->tag);
}

// ------------------------------------------------------------------------------------------------------------ l2d_jpeg_index
static const unsigned char jpg_dec_nat_host[64] = JPG_DEC_NAT_TABLE;

// the entropy kernel's lanes, one after the other on the host, from the op record the kernel would be launched with (HOST
// pointers): the CPU model of its loop bounds and its error reporting (tests/test_jpeg_dec_cpu.py)
extern "C" int l2d_jpeg_entropy_model(const l2d_op *op) {
    const int n_mcu = op->i[0], ny = op->i[1];
    if (!op->p[0] || !op->p[6] || jpg_dec_layout("jpeg_entropy_model", op, n_mcu, ny) != L2D_OK || op->i[3] <= 0) return L2D_EINVAL;
    const JpgChunks ck = jpg_chunks(n_mcu, op->i[2], op->i[3]);
    int tabs = 0;
    for (int k = 0; k < 3; ++k) tabs |= ((op->i[6 + k] & 1) << k) | ((op->i[9 + k] & 1) << (4 + k));
    if (ck.count != op->i[4]) return L2D_EINVAL;
    for (int c = 0; c < ck.count; ++c)
        *(int *)op->p[6] |= jpg_decode_chunk(c, (const uint8_t *)op->p[0], (const int *)op->p[1], (const int16_t *)op->p[2], (const uint8_t *)op->p[3],
                                             jpg_dec_nat_host, (const int *)op->p[4], (int16_t *)op->p[5], n_mcu, ny, ck, op->i[5], tabs);
    return L2D_OK;
}

extern "C" int l2d_jpeg_index(const uint8_t *file, int64_t len, const uint8_t *blob, const int32_t *layout, int32_t *bit_offsets,
                              int16_t *dc_pred) {
    const char *err = "";
    const int rc = jpg_index(file, len, blob, layout, bit_offsets, dc_pred, &err);
    if (rc != 0) l2d_set_error("l2d_jpeg_index: %s (code %d)", err, rc);
    return rc;
}
