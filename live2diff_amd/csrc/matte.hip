// Depth matte: the stream's output composited over its own source frame by a matte made of the frame's
// own depth map, written as the uint8 HWC frame the egress op writes -- one launch in place of L2D_OP_FRAME_EGRESS.  The reference
// has no counterpart: its depth map is encoded as the UNet's conditioning and dropped (pipeline_stream_animation_depth.py:544-571).
//
//   d = float(depth)                          fp16 in [-1, 1], 1 = nearest
//   t = clamp((d - lo) * inv, 0, 1)           (hard: t = d >= lo ? 1 : 0)
//   m = (t * t) * (3 - 2 * t)                 (far: m = 1 - m)
//   r > 0: m = box_(2r+1)(m) as a horizontal, then a vertical pass; coordinates clamped to the image; the taps added in
//          increasing coordinate order; each pass divided (a correctly rounded division) by float(2r + 1)
//   o = v_c + m * (v_s - v_c)                 v = clamp(fp16(fp16(x / 2) + 0.5), 0, 1), the egress op's chain, on styled / source
//   byte = rint(o * 255)                      (show: rint(m * 255) in all three channels)
//
// Every step is one fp32 operation with one rounding (the file is built with -ffp-contract=off, see the Makefile), so that numpy
// restates it bit for bit (live2diff_amd/matte.py `composite_ref`).  A bandwidth kernel: 16-byte loads of fp16 rows, no MFMA.
#include "frame_px.h"

#define MT_MAX_R L2D_MATTE_MAX_R
#define MT_TW 64                              // tile width in pixels: 8 lanes of 8 pixels
#define MT_TH 16                              // tile height
#define MT_THREADS (MT_TH * MT_TW / 8)        // 128: one lane = 8 consecutive pixels of one row in the blend stage
#define MT_MW (MT_TW + 16)                    // the tile's row of m: one 8-pixel group of halo on either side (r <= 8)
#define MT_MH (MT_TH + 2 * MT_MAX_R)

#define MT_HARD L2D_MATTE_HARD
#define MT_FAR L2D_MATTE_FAR
#define MT_SHOW L2D_MATTE_SHOW
#define MT_PLANE L2D_MATTE_PLANE
static_assert(MT_HARD == 1 && MT_FAR == 2, "px_ramp reads the hard and far bits of the flags");

struct mt_params {
    float lo, inv;
    int flags, r;
};

// L2D_MATTE_PLANE: the `depth` operand is an fp32 plane of ready matte values (L2D_OP_FRAME_MATTE_EDGE
// writes one) and the ramp is skipped.  PLANE is a template parameter of the three kernel bodies, so the kernels of the flag-clear
// path (frame_matte_point_kernel, frame_matte_box_kernel, frame_matte_up_kernel) hold no trace of it; frame_plane_* are its.
template <bool PLANE>
__device__ __forceinline__ float mt_value(const void *depth, long long i, const mt_params &p) {
    if constexpr (PLANE) return reinterpret_cast<const float *>(depth)[i];
    else return px_ramp(reinterpret_cast<const h16 *>(depth)[i], p.lo, p.inv, p.flags);
}

// eight consecutive values from element i (a multiple of 8) on
template <bool PLANE>
__device__ __forceinline__ void mt_value8(const void *depth, long long i, const mt_params &p, float *v) {
    if constexpr (PLANE) {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(depth) + i);
        const f32x4 a = src[0], b = src[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[e + 4] = b[e]; }
    } else {
        const h16x8 d = l2d_ld8(reinterpret_cast<const h16 *>(depth) + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = px_ramp(d[e], p.lo, p.inv, p.flags);
    }
}

__device__ __forceinline__ unsigned mt_byte(float vs, float vc, float m) {
    const float o = __fadd_rn(vc, __fmul_rn(m, __fsub_rn(vs, vc)));
    return (unsigned)rintf(__fmul_rn(o, 255.0f));
}

// N pixels (N = 8 or 16) of three planes each of styled / source + their matte -> 3 N packed bytes in N * 3 / 4 words
template <int N>
__device__ __forceinline__ void mt_blend(const h16 (&s)[3][N], const h16 (&c)[3][N], const float (&m)[N], int show, unsigned (&wd)[N * 3 / 4]) {
    unsigned char q[N * 3];
#pragma unroll
    for (int e = 0; e < N; ++e) {
        if (show) {
            q[e * 3] = q[e * 3 + 1] = q[e * 3 + 2] = (unsigned char)(unsigned)rintf(__fmul_rn(m[e], 255.0f));
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) q[e * 3 + ch] = (unsigned char)mt_byte(px_unit(s[ch][e]), px_unit(c[ch][e]), m[e]);
        }
    }
#pragma unroll
    for (int u = 0; u < N * 3 / 4; ++u)
        wd[u] = (unsigned)q[u * 4] | ((unsigned)q[u * 4 + 1] << 8) | ((unsigned)q[u * 4 + 2] << 16) | ((unsigned)q[u * 4 + 3] << 24);
}

// r = 0: every pixel on its own.  One lane = 16 consecutive pixels of the [H W] plane = 48 bytes, three 16-byte stores (the
// egress kernel's shape).
template <bool PLANE>
__device__ __forceinline__ void mt_point_body(const h16 *__restrict__ styled, const h16 *__restrict__ source, const void *__restrict__ depth,
                                              uint8_t *__restrict__ dst, int B, int HW, long long dstride, const mt_params &p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int per = HW >> 4;
    if (idx >= (long long)B * per) return;
    const int b = (int)(idx / per);
    const int p0 = (int)(idx % per) * 16;
    const int show = p.flags & MT_SHOW;
    h16 s[3][16], c[3][16];
    float m[16];
    mt_value8<PLANE>(depth, (long long)b * dstride + p0, p, m);
    mt_value8<PLANE>(depth, (long long)b * dstride + p0 + 8, p, m + 8);
    if (!show) {
        const long long off = (long long)b * 3 * HW + p0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const h16x8 s0 = l2d_ld8(styled + off + (long long)ch * HW), s1 = l2d_ld8(styled + off + (long long)ch * HW + 8);
            const h16x8 c0 = l2d_ld8(source + off + (long long)ch * HW), c1 = l2d_ld8(source + off + (long long)ch * HW + 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s[ch][e] = s0[e]; s[ch][e + 8] = s1[e];
                c[ch][e] = c0[e]; c[ch][e + 8] = c1[e];
            }
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int e = 0; e < 16; ++e) s[ch][e] = c[ch][e] = (h16)0.0f;
    }
    unsigned wd[12];
    mt_blend<16>(s, c, m, show, wd);
    uint4 *out = reinterpret_cast<uint4 *>(dst + ((long long)b * HW + p0) * 3);
#pragma unroll
    for (int v = 0; v < 3; ++v) out[v] = make_uint4(wd[v * 4], wd[v * 4 + 1], wd[v * 4 + 2], wd[v * 4 + 3]);
}

__global__ __launch_bounds__(256) void frame_matte_point_kernel(const h16 *__restrict__ styled, const h16 *__restrict__ source,
                                                                const h16 *__restrict__ depth, uint8_t *__restrict__ dst, int B, int HW,
                                                                long long dstride, mt_params p) {
    mt_point_body<false>(styled, source, depth, dst, B, HW, dstride, p);
}

__global__ __launch_bounds__(256) void frame_plane_point_kernel(const h16 *__restrict__ styled, const h16 *__restrict__ source,
                                                                const float *__restrict__ plane, uint8_t *__restrict__ dst, int B, int HW,
                                                                long long dstride, mt_params p) {
    mt_point_body<true>(styled, source, plane, dst, B, HW, dstride, p);
}

// r > 0: one work-group per MT_TH x MT_TW tile.  Stage 1 writes m of the tile and its halo into LDS (rows clamped to the image;
// an 8-pixel group lies wholly inside or wholly outside it because W % 8 == 0, and one outside holds the edge pixel's value);
// stage 2 is the horizontal pass, one lane per column (conflict-free 4-byte reads); stage 3 the vertical pass in the blend
// stage's layout (16-byte reads), then the blend and 8 pixels = 24 bytes per lane as three 8-byte stores.
template <bool PLANE>
__device__ __forceinline__ void mt_box_body(const h16 *__restrict__ styled, const h16 *__restrict__ source, const void *__restrict__ depth,
                                            uint8_t *__restrict__ dst, int H, int W, long long dstride, const mt_params &p) {
    __shared__ __attribute__((aligned(16))) float mm[MT_MH][MT_MW];
    __shared__ __attribute__((aligned(16))) float hh[MT_MH][MT_TW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * MT_TW, y0 = blockIdx.y * MT_TH, b = blockIdx.z;
    const int r = p.r, taps = 2 * r + 1, rows = MT_TH + 2 * r;
    const int show = p.flags & MT_SHOW;
    const float n = (float)taps;
    const long long HW = (long long)H * W;

    // this lane's 8 pixels of the blend stage: their loads are issued first, the box passes run under them
    const int by = tid >> 3, bx = (tid & 7) * 8;
    const int y = y0 + by, x = x0 + bx;
    const bool live = y < H && x < W;           // (x + 8 <= W then: W % 8 == 0)
    h16 s[3][8], c[3][8];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        h16x8 sv = l2d_zero8(), cv = l2d_zero8();
        if (live && !show) {
            const long long off = ((long long)b * 3 + ch) * HW + (long long)y * W + x;
            sv = l2d_ld8(styled + off);
            cv = l2d_ld8(source + off);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[ch][e] = sv[e]; c[ch][e] = cv[e]; }
    }

    const long long dp = (long long)b * dstride;
    for (int g = tid; g < rows * (MT_MW / 8); g += MT_THREADS) {
        const int j = g / (MT_MW / 8), cg = g % (MT_MW / 8);
        int yy = y0 - r + j;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
        const int gx = x0 - 8 + cg * 8;
        const long long row = dp + (long long)yy * W;
        float v[8];
        if (gx < 0 || gx >= W) {
            const float edge = mt_value<PLANE>(depth, row + (gx < 0 ? 0 : W - 1), p);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = edge;
        } else {
            mt_value8<PLANE>(depth, row + gx, p, v);
        }
        f32x4 *o = reinterpret_cast<f32x4 *>(&mm[j][cg * 8]);
        o[0] = f32x4{v[0], v[1], v[2], v[3]};
        o[1] = f32x4{v[4], v[5], v[6], v[7]};
    }
    __syncthreads();

    // horizontal: hh[j][c] = (mm[j][8 + c - r] + ... + mm[j][8 + c + r]) / n
    for (int i = tid; i < rows * MT_TW; i += MT_THREADS) {
        const int j = i / MT_TW, cc = i % MT_TW;
        const float *src = &mm[j][8 + cc - r];
        float acc = src[0];
        for (int k = 1; k < taps; ++k) acc = __fadd_rn(acc, src[k]);
        hh[j][cc] = __fdiv_rn(acc, n);
    }
    __syncthreads();

    // vertical: m[e] = (hh[by][bx + e] + ... + hh[by + 2 r][bx + e]) / n
    float m[8];
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(&hh[by][bx]);
        f32x4 a0 = src[0], a1 = src[1];
        for (int k = 1; k < taps; ++k) {
            const f32x4 *nx = reinterpret_cast<const f32x4 *>(&hh[by + k][bx]);
            const f32x4 b0 = nx[0], b1 = nx[1];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0[e] = __fadd_rn(a0[e], b0[e]);
                a1[e] = __fadd_rn(a1[e], b1[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m[e] = __fdiv_rn(a0[e], n);
            m[e + 4] = __fdiv_rn(a1[e], n);
        }
    }
    if (!live) return;
    unsigned wd[6];
    mt_blend<8>(s, c, m, show, wd);
    uint2 *out = reinterpret_cast<uint2 *>(dst + (((long long)b * H + y) * W + x) * 3);      // 24 (...) is a multiple of 8
#pragma unroll
    for (int v = 0; v < 3; ++v) out[v] = make_uint2(wd[v * 2], wd[v * 2 + 1]);
}

__global__ __launch_bounds__(MT_THREADS) void frame_matte_box_kernel(const h16 *__restrict__ styled, const h16 *__restrict__ source,
                                                                     const h16 *__restrict__ depth, uint8_t *__restrict__ dst, int H, int W,
                                                                     long long dstride, mt_params p) {
    mt_box_body<false>(styled, source, depth, dst, H, W, dstride, p);
}

__global__ __launch_bounds__(MT_THREADS) void frame_plane_box_kernel(const h16 *__restrict__ styled, const h16 *__restrict__ source,
                                                                     const float *__restrict__ plane, uint8_t *__restrict__ dst, int H, int W,
                                                                     long long dstride, mt_params p) {
    mt_box_body<true>(styled, source, plane, dst, H, W, dstride, p);
}

int l2d_launch_frame_matte(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], H = op->i[1], W = op->i[2], r = op->i[3], flags = op->i[4];
    const long long dstride = op->l[0];
    if (!op->p[0] || !op->p[1] || !op->p[2] || !op->p[3] || B <= 0 || H <= 0 || W <= 0) {
        l2d_set_error("frame_matte(tag %d): invalid arguments (null pointer or non-positive size)", op->tag);
        return L2D_EINVAL;
    }
    const long long HW = (long long)H * W;
    if (W % 8 || HW % 16) {
        l2d_set_error("frame_matte(tag %d): W = %d must be a multiple of 8 and H W = %lld a multiple of 16", op->tag, W, HW);
        return L2D_EINVAL;
    }
    if (r < 0 || r > MT_MAX_R) {
        l2d_set_error("frame_matte(tag %d): feather radius %d, need 0..%d", op->tag, r, MT_MAX_R);
        return L2D_EINVAL;
    }
    if (flags & ~(MT_HARD | MT_FAR | MT_SHOW | MT_PLANE)) {
        l2d_set_error("frame_matte(tag %d): unknown flag bits 0x%x (1 hard, 2 far, 4 show, 16 plane)", op->tag, flags);
        return L2D_EINVAL;
    }
    const bool plane = (flags & MT_PLANE) != 0;
    if (dstride < HW || dstride % 8) {
        l2d_set_error("frame_matte(tag %d): depth plane stride %lld, need a multiple of 8 that is at least H W = %lld", op->tag, dstride, HW);
        return L2D_EINVAL;
    }
    for (int k = 0; k < 4; ++k) {
        if (((uintptr_t)op->p[k]) & 15) {
            l2d_set_error("frame_matte(tag %d): pointer %d is not 16-byte aligned", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if ((long long)B * HW * 3 >= (1ll << 31) || B > 65535) {
        l2d_set_error("frame_matte(tag %d): B H W 3 must stay below 2^31 and B below 65536", op->tag);
        return L2D_EINVAL;
    }
    const float lo = plane ? 0.0f : op->f[0], inv = plane ? 0.0f : op->f[1];          // (a plane: the ramp is not read)
    if (!plane && !px_check_ramp("frame_matte", op->tag, lo, inv, (flags & MT_HARD) != 0)) return L2D_EINVAL;
    L2D_DRY_RETURN();
    mt_params p;
    p.lo = lo; p.inv = inv; p.flags = flags; p.r = r;
    const h16 *styled = (const h16 *)op->p[0], *source = (const h16 *)op->p[1], *depth = (const h16 *)op->p[2];
    const float *mplane = (const float *)op->p[2];
    uint8_t *dst = (uint8_t *)op->p[3];
    const dim3 tiles((W + MT_TW - 1) / MT_TW, (H + MT_TH - 1) / MT_TH, B);
    const long long total = (long long)B * (HW / 16);
    if (plane && r == 0) {
        hipLaunchKernelGGL(frame_plane_point_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, styled, source, mplane, dst, B,
                           (int)HW, dstride, p);
    } else if (plane) {
        hipLaunchKernelGGL(frame_plane_box_kernel, tiles, dim3(MT_THREADS), 0, s, styled, source, mplane, dst, H, W, dstride, p);
    } else if (r == 0) {
        hipLaunchKernelGGL(frame_matte_point_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, styled, source, depth, dst, B,
                           (int)HW, dstride, p);
    } else {
        hipLaunchKernelGGL(frame_matte_box_kernel, tiles, dim3(MT_THREADS), 0, s, styled, source, depth, dst, H, W, dstride, p);
    }
    return l2d_check_launch("frame_matte", op->tag);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Matte at the output size: the styled frame, already resampled to the output size by
// L2D_OP_FRAME_RESIZE, composited over the CAMERA's own pixels at that size by the matte of the stream-sized depth plane, sampled
// bilinearly (half-pixel centres).  live2diff_amd/matte.py `composite_up_ref` restates it bit for bit:
//
//   m        the matte of L2D_OP_FRAME_MATTE at the stream's size, feather applied there (px_ramp + the two box passes)
//   a_top = m[y0][x0] + fx (m[y0][x1] - m[y0][x0])     a_bot likewise on row y1     M = a_top + fy (a_bot - a_top)
//   o = C + M (S - C) on the bytes as fp32             byte = rint(o)               (show: rint(255 M) in all three channels)
//
// each subtraction, multiplication and addition rounded once.  One work-group per MU_T x MU_T output tile and frame: the depth
// patch the tile's taps reach plus the feather halo becomes m in LDS (coordinates clamped to the image: edge replication), the
// box filter runs as a horizontal and a vertical pass there, the tile's M is formed from the four taps, then the bytes.
#define MU_T 32                                   // output tile, pixels (both axes)
#define MU_THREADS 256
#define MU_SPAN (2 * MU_T)                        // source pixels a tile's taps reach along an axis at the 1/2 limit: see below
#define MU_PATCH (MU_SPAN + 2 * MT_MAX_R)         // ... plus the halo: 80
#define MU_STRIDE MU_PATCH                        // floats per LDS row; 80 % 32 == 16 keeps two short rows of one half-wave apart
#define MU_ITEMS 32                               // stores per output row of a tile: <= 3 head bytes + 24 dwords + 3 tail bytes
// The taps of output o lie at k = floor((o + 0.5) s - 0.5) and k + 1 with s = n_in / n_out <= 2.  Over a tile the first k and
// the last differ by at most ceil((T - 1) s) <= 2 T - 2, so first k .. last k + 1 are at most 2 T source pixels.
static_assert(MU_SPAN >= 2 * (MU_T - 1) + 2, "a tile's taps fit the span at a ratio of 1/2");
static_assert(MU_T * 3 / 4 + 6 <= MU_ITEMS, "a tile row is stored by MU_ITEMS lanes");
#define MU_LDS_BYTES (2 * MU_PATCH * MU_STRIDE * 4 + MU_T * MU_T * 4 + MU_T * MU_T * 3 + 6 * MU_T * 4)
static_assert(MU_LDS_BYTES == 59136, "the LDS size DESIGN.md section 8.z7 states");
static_assert(2 * MU_LDS_BYTES <= 160 * 1024, "two work-groups per CU");

template <bool PLANE>
__device__ __forceinline__ void mu_body(const uint8_t *__restrict__ styled, const uint8_t *__restrict__ camera, const void *__restrict__ depth,
                                        uint8_t *__restrict__ dst, const int *__restrict__ tx, const int *__restrict__ ty, int H, int W, int Ho,
                                        int Wo, long long dstride, const mt_params &p) {
    __shared__ __attribute__((aligned(16))) float mm[MU_PATCH * MU_STRIDE];       // m of the patch; later the filtered m
    __shared__ __attribute__((aligned(16))) float hh[MU_PATCH * MU_STRIDE];       // the horizontal pass' rows
    __shared__ float mt[MU_T * MU_T];                                             // M of the tile
    __shared__ __attribute__((aligned(16))) unsigned char ob[MU_T * MU_T * 3];    // the tile's bytes
    __shared__ int x0s[MU_T], x1s[MU_T], y0s[MU_T], y1s[MU_T];
    __shared__ float fxs[MU_T], fys[MU_T];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * MU_T, oy0 = blockIdx.y * MU_T, b = blockIdx.z;
    const int tw = Wo - ox0 < MU_T ? Wo - ox0 : MU_T, th = Ho - oy0 < MU_T ? Ho - oy0 : MU_T;
    const int r = p.r, taps = 2 * r + 1;
    int sx0, nx, sy0, ny;
    px_span<MU_SPAN>(tx, Wo, W, ox0, tw, sx0, nx);
    px_span<MU_SPAN>(ty, Ho, H, oy0, th, sy0, ny);
    if (tid < MU_T) {
        px_stage(tx, Wo, W, ox0, tw, sx0, nx, tid, x0s, x1s, fxs);
    } else if (tid >= 64 && tid < 64 + MU_T) {
        px_stage(ty, Ho, H, oy0, th, sy0, ny, tid - 64, y0s, y1s, fys);
    }

    // m of the patch and its halo: mm[j][c] = m(clamp(sy0 - r + j), clamp(sx0 - r + c))
    const int rows = ny + 2 * r, cols = nx + 2 * r;
    const long long dp = (long long)b * dstride;
    for (int i = tid; i < rows * cols; i += MU_THREADS) {
        const int j = i / cols, c = i - j * cols;
        const int yy = px_clampi(sy0 - r + j, 0, H - 1), xx = px_clampi(sx0 - r + c, 0, W - 1);
        mm[j * MU_STRIDE + c] = mt_value<PLANE>(depth, dp + (long long)yy * W + xx, p);
    }
    __syncthreads();

    if (r > 0) {
        const float n = (float)taps;
        // horizontal: hh[j][c] = (mm[j][c] + ... + mm[j][c + 2 r]) / n
        for (int i = tid; i < rows * nx; i += MU_THREADS) {
            const int j = i / nx, c = i - j * nx;
            const float *src = mm + j * MU_STRIDE + c;
            float acc = src[0];
            for (int k = 1; k < taps; ++k) acc = __fadd_rn(acc, src[k]);
            hh[j * MU_STRIDE + c] = __fdiv_rn(acc, n);
        }
        __syncthreads();
        // vertical, into the patch buffer (nobody reads the patch any more): mm[y][c] = (hh[y][c] + ... + hh[y + 2 r][c]) / n
        for (int i = tid; i < ny * nx; i += MU_THREADS) {
            const int y = i / nx, c = i - y * nx;
            const float *src = hh + y * MU_STRIDE + c;
            float acc = src[0];
            for (int k = 1; k < taps; ++k) acc = __fadd_rn(acc, src[k * MU_STRIDE]);
            mm[y * MU_STRIDE + c] = __fdiv_rn(acc, n);
        }
        __syncthreads();
    }

    // M of the tile from the four taps
    for (int i = tid; i < th * tw; i += MU_THREADS) {
        const int yy = i / tw, xx = i - yy * tw;
        const float *t0 = mm + y0s[yy] * MU_STRIDE, *t1 = mm + y1s[yy] * MU_STRIDE;
        const int a = x0s[xx], c = x1s[xx];
        const float fx = fxs[xx], fy = fys[yy];
        const float top = __fadd_rn(t0[a], __fmul_rn(fx, __fsub_rn(t0[c], t0[a])));
        const float bot = __fadd_rn(t1[a], __fmul_rn(fx, __fsub_rn(t1[c], t1[a])));
        mt[yy * MU_T + xx] = __fadd_rn(top, __fmul_rn(fy, __fsub_rn(bot, top)));
    }
    __syncthreads();

    // the bytes: one lane per byte of a tile row, consecutive lanes consecutive addresses of both frames
    const int nb = tw * 3;
    const int show = p.flags & MT_SHOW;
    for (int i = tid; i < th * nb; i += MU_THREADS) {
        const int yy = i / nb, e = i - yy * nb;
        const float M = mt[yy * MU_T + e / 3];
        float o;
        if (show) {
            o = __fmul_rn(M, 255.0f);
        } else {
            const long long g = (((long long)b * Ho + oy0 + yy) * Wo + ox0) * 3 + e;
            const float S = (float)styled[g], C = (float)camera[g];
            o = __fadd_rn(C, __fmul_rn(M, __fsub_rn(S, C)));
        }
        ob[yy * MU_T * 3 + e] = (unsigned char)(unsigned)rintf(o);
    }
    __syncthreads();

    // the tile's rows: tw * 3 bytes each at an address of any alignment, MU_ITEMS lanes per row, one store each (px_store_row).
    // Every byte lies inside row oy0 + yy < Ho, columns ox0 .. ox0 + tw - 1 < Wo.
    for (int i = tid; i < th * MU_ITEMS; i += MU_THREADS) {
        const int yy = i / MU_ITEMS, it = i % MU_ITEMS;
        uint8_t *g = dst + (((long long)b * Ho + oy0 + yy) * Wo + ox0) * 3;
        const unsigned char *o = ob + yy * MU_T * 3;
        px_store_row(g, o, nb, it);
    }
}

__global__ __launch_bounds__(MU_THREADS) void frame_matte_up_kernel(const uint8_t *__restrict__ styled, const uint8_t *__restrict__ camera,
                                                                    const h16 *__restrict__ depth, uint8_t *__restrict__ dst,
                                                                    const int *__restrict__ tx, const int *__restrict__ ty, int H, int W,
                                                                    int Ho, int Wo, long long dstride, mt_params p) {
    mu_body<false>(styled, camera, depth, dst, tx, ty, H, W, Ho, Wo, dstride, p);
}

// (its name must not contain the name above: tests/test_matte_up_resources.py finds that kernel by it)
__global__ __launch_bounds__(MU_THREADS) void frame_plane_up_kernel(const uint8_t *__restrict__ styled, const uint8_t *__restrict__ camera,
                                                                    const float *__restrict__ plane, uint8_t *__restrict__ dst,
                                                                    const int *__restrict__ tx, const int *__restrict__ ty, int H, int W,
                                                                    int Ho, int Wo, long long dstride, mt_params p) {
    mu_body<true>(styled, camera, plane, dst, tx, ty, H, W, Ho, Wo, dstride, p);
}

int l2d_launch_frame_matte_up(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], H = op->i[1], W = op->i[2], Ho = op->i[3], Wo = op->i[4], r = op->i[5], flags = op->i[6];
    const long long dstride = op->l[0];
    for (int k = 0; k < 6; ++k) {
        if (!op->p[k]) {
            l2d_set_error("frame_matte_up(tag %d): pointer %d is null", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if (B <= 0 || H <= 0 || W <= 0) {
        l2d_set_error("frame_matte_up(tag %d): non-positive size (B %d, H %d, W %d)", op->tag, B, H, W);
        return L2D_EINVAL;
    }
    if (!px_axis_ok(H, Ho) || !px_axis_ok(W, Wo)) {
        l2d_set_error("frame_matte_up(tag %d): %d x %d -> %d x %d: an output size must lie in 1..%d and between half and 8 times the "
                      "matte's size", op->tag, H, W, Ho, Wo, L2D_RESIZE_MAX_SIZE);
        return L2D_EINVAL;
    }
    if ((long long)B * Ho * Wo * 3 >= (1ll << 31) || B > 65535) {
        l2d_set_error("frame_matte_up(tag %d): B Ho Wo 3 must stay below 2^31 and B below 65536", op->tag);
        return L2D_EINVAL;
    }
    if (r < 0 || r > MT_MAX_R) {
        l2d_set_error("frame_matte_up(tag %d): feather radius %d, need 0..%d", op->tag, r, MT_MAX_R);
        return L2D_EINVAL;
    }
    if (flags & ~(MT_HARD | MT_FAR | MT_SHOW | MT_PLANE)) {
        l2d_set_error("frame_matte_up(tag %d): unknown flag bits 0x%x (1 hard, 2 far, 4 show, 16 plane)", op->tag, flags);
        return L2D_EINVAL;
    }
    const bool plane = (flags & MT_PLANE) != 0;
    const long long HW = (long long)H * W;
    if (dstride < HW || (((uintptr_t)op->p[2]) & (plane ? 3 : 1))) {
        l2d_set_error("frame_matte_up(tag %d): depth plane stride %lld, need at least H W = %lld, and a 2-byte aligned plane (4-byte: a "
                      "float plane)", op->tag, dstride, HW);
        return L2D_EINVAL;
    }
    for (int k = 4; k < 6; ++k) {
        if (((uintptr_t)op->p[k]) & 3) {
            l2d_set_error("frame_matte_up(tag %d): table pointer %d is not 4-byte aligned", op->tag, k);
            return L2D_EINVAL;
        }
    }
    const float lo = plane ? 0.0f : op->f[0], inv = plane ? 0.0f : op->f[1];          // (a plane: the ramp is not read)
    if (!plane && !px_check_ramp("frame_matte_up", op->tag, lo, inv, (flags & MT_HARD) != 0)) return L2D_EINVAL;
    L2D_DRY_RETURN();
    mt_params p;
    p.lo = lo; p.inv = inv; p.flags = flags; p.r = r;
    const dim3 tiles((Wo + MU_T - 1) / MU_T, (Ho + MU_T - 1) / MU_T, B);
    if (plane) {
        hipLaunchKernelGGL(frame_plane_up_kernel, tiles, dim3(MU_THREADS), 0, s, (const uint8_t *)op->p[0], (const uint8_t *)op->p[1],
                           (const float *)op->p[2], (uint8_t *)op->p[3], (const int *)op->p[4], (const int *)op->p[5], H, W, Ho, Wo, dstride,
                           p);
    } else {
        hipLaunchKernelGGL(frame_matte_up_kernel, tiles, dim3(MU_THREADS), 0, s, (const uint8_t *)op->p[0], (const uint8_t *)op->p[1],
                           (const h16 *)op->p[2], (uint8_t *)op->p[3], (const int *)op->p[4], (const int *)op->p[5], H, W, Ho, Wo, dstride,
                           p);
    }
    return l2d_check_launch("frame_matte_up", op->tag);
}
