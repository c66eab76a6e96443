// The matte from the caller: a mask of a person segmenter, a keyer or a hand-drawn region -- uint8,
// uint16 or fp32, any size -- becomes the raw matte plane of the output chain, fp32 [H][W] in [0, 1] at the stream's size, in
// place of (or combined with) the smoothstep ramp over the frame's depth.  Everything behind the raw matte -- edge refit, hold,
// feather, backdrop, both composites, `show` -- reads this plane under its plane flag.  The reference has no counterpart.
//
//   v = float(s) / 255 (uint8), float(s) / 65535 (uint16), min(max(x, 0), 1) with NaN -> 0 (fp32)
//   r = sum_y wy (sum_x wx v)               the antialiased triangle weights of the frame ingest (the tables of depth_io.tables,
//                                           which the oracle reads too), the horizontal pass first, taps ascending
//   P = rint(255 min(max(r, 0), 1))         half to even; L2D_MASK_INVERT: 255 - P
//   mu = float(P) / 255
//   m0 = mu (replace), min(m_r, mu) (L2D_MASK_AND), max(m_r, mu) (L2D_MASK_OR)      m_r: px_ramp of the depth plane
//
// The mask is quantised to byte levels at the stream's size: a constant mask comes back exactly 0 or 1 whatever the weights'
// rounding, and the integers the edge refit and the backdrop form of the plane (rint(255 m0)) are P itself.  Every product, sum
// and quotient is one fp32 operation with one rounding (the file is built with -ffp-contract=off, see the Makefile), min and
// max are exact, so numpy restates the plane bit for bit (live2diff_amd/mask_io.py mask_ref, front_ref).  The shape is
// L2D_OP_DEPTH_INGEST's with one resampled plane in place of two: one work-group per MI_TH x MI_TW output tile, the horizontal
// sums of the source rows the tile's taps reach staged in LDS, then the vertical pass and the epilogue.  Every element of the
// plane is written by a plain store on every launch: nothing is zeroed, there is no atomic.
#include "frame_px.h"

#define MI_THREADS 256
#define MI_TH L2D_DEPTH_TILE_H
#define MI_TW L2D_DEPTH_TILE_W
#define MI_MAX_K L2D_DEPTH_MAX_TAPS                   // 2 * 8 + 1 taps per axis at scale 8
#define MI_ROWS ((MI_TH - 1) * 8 + MI_MAX_K + 7)      // source rows under one tile at scale 8: 137, rounded up to a multiple of 8
#define MI_U8 0
#define MI_U16 1
#define MI_F32 2

#define MI_LDS_BYTES (MI_ROWS * MI_TW * 4 + MI_TW * MI_MAX_K * 4 + MI_TW * 4)
static_assert(MI_LDS_BYTES == 20736, "the LDS of the mask ingest as DESIGN.md section 8.z16 and the resource test state it");
static_assert(MI_TH * MI_TW % MI_THREADS == 0 && MI_TW == 32, "a half-wave is one row of the tile: conflict-free LDS rows");

struct mi_params {
    int Hm, Wm, H, W, Kx, Ky, flags;
    float lo, inv;
};

// v of one source sample
template <int TYPE>
__device__ __forceinline__ float mi_unit(const void *__restrict__ src, long long idx) {
    if (TYPE == MI_U8) return __fdiv_rn((float)((const uint8_t *)src)[idx], 255.0f);
    if (TYPE == MI_U16) return __fdiv_rn((float)((const uint16_t *)src)[idx], 65535.0f);
    const float x = ((const float *)src)[idx];
    return x != x ? 0.0f : fminf(fmaxf(x, 0.0f), 1.0f);
}

// grid (tiles x, tiles y).  What is read from a table is clamped to the image and to the staged rows.
template <int TYPE>
__device__ __forceinline__ void mi_body(const void *__restrict__ src, float *__restrict__ out, const h16 *__restrict__ depth,
                                        const int *__restrict__ xmin, const float *__restrict__ wx, const int *__restrict__ ymin,
                                        const float *__restrict__ wy, const mi_params &p) {
    __shared__ float hs[MI_ROWS][MI_TW];
    __shared__ float swx[MI_TW][MI_MAX_K];
    __shared__ int sxlo[MI_TW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * MI_TW, y0 = blockIdx.y * MI_TH;
    const int tw = min(MI_TW, p.W - x0), th = min(MI_TH, p.H - y0);

    for (int i = tid; i < MI_TW * MI_MAX_K; i += MI_THREADS) {
        const int c = i / MI_MAX_K, j = i % MI_MAX_K;
        swx[c][j] = (c < tw && j < p.Kx) ? wx[(long long)(x0 + c) * p.Kx + j] : 0.0f;
    }
    if (tid < MI_TW) sxlo[tid] = tid < tw ? xmin[x0 + tid] : 0;
    const int r0 = min(max(ymin[y0], 0), p.Hm - 1);
    const int r1 = min(max(ymin[y0 + th - 1] + p.Ky, r0 + 1), p.Hm);
    const int nrows = min(r1 - r0, MI_ROWS);
    __syncthreads();

    // horizontal pass: one lane per (source row, tile column)
    for (int i = tid; i < nrows * MI_TW; i += MI_THREADS) {
        const int r = i / MI_TW, c = i % MI_TW;
        float n = 0.0f;
        if (c < tw) {
            const long long row = (long long)(r0 + r) * p.Wm;
            const int lo = sxlo[c];
            for (int j = 0; j < p.Kx; ++j) {
                const int xi = min(max(lo + j, 0), p.Wm - 1);          // (a tap past the row's own count has weight 0)
                n = __fadd_rn(n, __fmul_rn(swx[c][j], mi_unit<TYPE>(src, row + xi)));
            }
        }
        hs[r][c] = n;
    }
    __syncthreads();

    // vertical pass and the epilogue: MI_TH x MI_TW outputs, two per lane; consecutive lanes consecutive floats of a row
    const int ramp = ((p.flags & L2D_MASK_RAMP_HARD) ? L2D_MATTE_HARD : 0) | ((p.flags & L2D_MASK_RAMP_FAR) ? L2D_MATTE_FAR : 0);
#pragma unroll
    for (int it = 0; it < MI_TH * MI_TW / MI_THREADS; ++it) {
        const int o = it * MI_THREADS + tid;
        const int yy = o / MI_TW, c = o % MI_TW;
        if (yy < th && c < tw) {
            const int y = y0 + yy;
            const int lo = ymin[y] - r0;
            float n = 0.0f;
            for (int k = 0; k < p.Ky; ++k) {
                const int rr = min(max(lo + k, 0), nrows - 1);
                n = __fadd_rn(n, __fmul_rn(wy[(long long)y * p.Ky + k], hs[rr][c]));
            }
            float P = rintf(__fmul_rn(255.0f, fminf(fmaxf(n, 0.0f), 1.0f)));
            if (p.flags & L2D_MASK_INVERT) P = __fsub_rn(255.0f, P);
            float m = __fdiv_rn(P, 255.0f);
            const long long e = (long long)y * p.W + x0 + c;
            if (p.flags & (L2D_MASK_AND | L2D_MASK_OR)) {
                const float mr = px_ramp(depth[e], p.lo, p.inv, ramp);
                m = (p.flags & L2D_MASK_AND) ? fminf(mr, m) : fmaxf(mr, m);
            }
            out[e] = m;
        }
    }
}

#define MI_KERNEL(name, TYPE)                                                                                                       \
    __global__ __launch_bounds__(MI_THREADS) void name(const void *__restrict__ src, float *__restrict__ out,                        \
                                                       const h16 *__restrict__ depth, const int *__restrict__ xmin,                  \
                                                       const float *__restrict__ wx, const int *__restrict__ ymin,                   \
                                                       const float *__restrict__ wy, mi_params p) {                                  \
        mi_body<TYPE>(src, out, depth, xmin, wx, ymin, wy, p);                                                                      \
    }
MI_KERNEL(mask_ingest_u8_kernel, MI_U8)
MI_KERNEL(mask_ingest_u16_kernel, MI_U16)
MI_KERNEL(mask_ingest_f32_kernel, MI_F32)

int l2d_launch_mask_ingest(const l2d_op *op, hipStream_t s) {
    const int Hm = op->i[0], Wm = op->i[1], H = op->i[2], W = op->i[3];
    const int nh = op->i[4], nw = op->i[5], top = op->i[6], left = op->i[7], Kx = op->i[8], Ky = op->i[9], flags = op->i[10];
    const int known = L2D_MASK_U16 | L2D_MASK_F32 | L2D_MASK_INVERT | L2D_MASK_AND | L2D_MASK_OR | L2D_MASK_RAMP_HARD | L2D_MASK_RAMP_FAR;
    if (flags & ~known) {
        l2d_set_error("mask_ingest(tag %d): unknown flag bits 0x%x (1 uint16, 2 fp32, 4 invert, 8 and, 16 or, 64 hard ramp, 128 far)",
                      op->tag, flags);
        return L2D_EINVAL;
    }
    if (((flags & L2D_MASK_U16) && (flags & L2D_MASK_F32)) || ((flags & L2D_MASK_AND) && (flags & L2D_MASK_OR))) {
        l2d_set_error("mask_ingest(tag %d): flags 0x%x name two sample types or two ways to combine", op->tag, flags);
        return L2D_EINVAL;
    }
    const bool ramp = (flags & (L2D_MASK_AND | L2D_MASK_OR)) != 0;
    if (!ramp && (flags & (L2D_MASK_RAMP_HARD | L2D_MASK_RAMP_FAR))) {
        l2d_set_error("mask_ingest(tag %d): ramp flags without L2D_MASK_AND / _OR (a replacing mask reads no depth)", op->tag);
        return L2D_EINVAL;
    }
    for (int k = 0; k < 7; ++k) {
        if (!op->p[k] && (k != 2 || ramp)) {
            l2d_set_error("mask_ingest(tag %d): invalid arguments (pointer %d is null)", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if (Hm <= 0 || Wm <= 0 || H <= 0 || W <= 0 || nh <= 0 || nw <= 0) {
        l2d_set_error("mask_ingest(tag %d): invalid arguments (non-positive size: mask %d x %d, output %d x %d, resized %d x %d)", op->tag,
                      Hm, Wm, H, W, nh, nw);
        return L2D_EINVAL;
    }
    const int elem = (flags & L2D_MASK_F32) ? 4 : ((flags & L2D_MASK_U16) ? 2 : 1);
    if ((((uintptr_t)op->p[0]) & (elem - 1)) || (((uintptr_t)op->p[1]) & 15) || (((uintptr_t)op->p[2]) & 1)) {
        l2d_set_error("mask_ingest(tag %d): the mask is not aligned to its element, the plane not to 16 bytes or the depth not to 2", op->tag);
        return L2D_EINVAL;
    }
    for (int k = 3; k < 7; ++k) {
        if (((uintptr_t)op->p[k]) & 3) {
            l2d_set_error("mask_ingest(tag %d): pointer %d is not 4-byte aligned", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if ((long long)Hm * Wm >= (1ll << 31) || (long long)H * W >= (1ll << 31)) {
        l2d_set_error("mask_ingest(tag %d): Hm Wm and H W must stay below 2^31", op->tag);
        return L2D_EINVAL;
    }
    if (top < 0 || left < 0 || (long long)top + H > nh || (long long)left + W > nw) {
        l2d_set_error("mask_ingest(tag %d): crop window (top %d, left %d, %d x %d) lies outside the resized image %d x %d", op->tag, top,
                      left, H, W, nh, nw);
        return L2D_EINVAL;
    }
    const float sy = (float)Hm / (float)nh, sx = (float)Wm / (float)nw;
    if (sy > 8.0f || sx > 8.0f) {
        l2d_set_error("mask_ingest(tag %d): scale %.3f x %.3f exceeds 8 (17 taps per axis)", op->tag, sy, sx);
        return L2D_EINVAL;
    }
    if (Kx < 1 || Ky < 1 || Kx > MI_MAX_K || Ky > MI_MAX_K) {
        l2d_set_error("mask_ingest(tag %d): %d x %d taps, need 1..%d per axis", op->tag, Ky, Kx, MI_MAX_K);
        return L2D_EINVAL;
    }
    const float lo = op->f[0], inv = op->f[1];
    if (ramp && !px_check_ramp("mask_ingest", op->tag, lo, inv, (flags & L2D_MASK_RAMP_HARD) != 0)) return L2D_EINVAL;
    if (px_overlap(op->p[1], 4ll * H * W, op->p[0], (long long)elem * Hm * Wm) || px_overlap(op->p[1], 4ll * H * W, op->p[2], 2ll * H * W)) {
        l2d_set_error("mask_ingest(tag %d): the plane overlaps the mask or the depth plane", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    mi_params p;
    p.Hm = Hm, p.Wm = Wm, p.H = H, p.W = W, p.Kx = Kx, p.Ky = Ky, p.flags = flags, p.lo = lo, p.inv = inv;
    const dim3 grid((unsigned)((W + MI_TW - 1) / MI_TW), (unsigned)((H + MI_TH - 1) / MI_TH));
    auto kernel = (flags & L2D_MASK_F32) ? mask_ingest_f32_kernel : ((flags & L2D_MASK_U16) ? mask_ingest_u16_kernel : mask_ingest_u8_kernel);
    hipLaunchKernelGGL(kernel, grid, dim3(MI_THREADS), 0, s, (const void *)op->p[0], (float *)op->p[1], (const h16 *)op->p[2],
                       (const int *)op->p[3], (const float *)op->p[4], (const int *)op->p[5], (const float *)op->p[6], p);
    return l2d_check_launch("mask_ingest", op->tag);
}
