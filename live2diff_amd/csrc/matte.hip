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
#include "common.h"

#define MT_MAX_R L2D_MATTE_MAX_R
#define MT_TW 64                              // tile width in pixels: 8 lanes of 8 pixels
#define MT_TH 16                              // tile height
#define MT_THREADS (MT_TH * MT_TW / 8)        // 128: one lane = 8 consecutive pixels of one row in the blend stage
#define MT_MW (MT_TW + 16)                    // the tile's row of m: one 8-pixel group of halo on either side (r <= 8)
#define MT_MH (MT_TH + 2 * MT_MAX_R)

#define MT_HARD L2D_MATTE_HARD
#define MT_FAR L2D_MATTE_FAR
#define MT_SHOW L2D_MATTE_SHOW

struct mt_params {
    float lo, inv;
    int flags, r;
};

__device__ __forceinline__ float mt_matte(h16 depth, const mt_params &p) {
    const float d = (float)depth;
    float t;
    if (p.flags & MT_HARD) {
        t = d >= p.lo ? 1.0f : 0.0f;
    } else {
        t = __fmul_rn(__fsub_rn(d, p.lo), p.inv);
        t = fminf(fmaxf(t, 0.0f), 1.0f);
    }
    const float m = __fmul_rn(__fmul_rn(t, t), __fsub_rn(3.0f, __fmul_rn(2.0f, t)));
    return (p.flags & MT_FAR) ? __fsub_rn(1.0f, m) : m;
}

// the egress op's fp16 chain (frame_io.hip fio_u8), widened to fp32
__device__ __forceinline__ float mt_unit(h16 x) {
    const h16 t = (h16)((float)x * 0.5f);
    const float v = (float)(h16)((float)t + 0.5f);
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
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
            for (int ch = 0; ch < 3; ++ch) q[e * 3 + ch] = (unsigned char)mt_byte(mt_unit(s[ch][e]), mt_unit(c[ch][e]), m[e]);
        }
    }
#pragma unroll
    for (int u = 0; u < N * 3 / 4; ++u)
        wd[u] = (unsigned)q[u * 4] | ((unsigned)q[u * 4 + 1] << 8) | ((unsigned)q[u * 4 + 2] << 16) | ((unsigned)q[u * 4 + 3] << 24);
}

// r = 0: every pixel on its own.  One lane = 16 consecutive pixels of the [H W] plane = 48 bytes, three 16-byte stores (the
// egress kernel's shape).
__global__ __launch_bounds__(256) void frame_matte_point_kernel(const h16 *__restrict__ styled, const h16 *__restrict__ source,
                                                                const h16 *__restrict__ depth, uint8_t *__restrict__ dst, int B, int HW,
                                                                long long dstride, mt_params p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int per = HW >> 4;
    if (idx >= (long long)B * per) return;
    const int b = (int)(idx / per);
    const int p0 = (int)(idx % per) * 16;
    const int show = p.flags & MT_SHOW;
    h16 s[3][16], c[3][16];
    float m[16];
    const h16 *dp = depth + (long long)b * dstride + p0;
    const h16x8 d0 = l2d_ld8(dp), d1 = l2d_ld8(dp + 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        m[e] = mt_matte(d0[e], p);
        m[e + 8] = mt_matte(d1[e], p);
    }
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

// r > 0: one work-group per MT_TH x MT_TW tile.  Stage 1 writes m of the tile and its halo into LDS (rows clamped to the image;
// an 8-pixel group lies wholly inside or wholly outside it because W % 8 == 0, and one outside holds the edge pixel's value);
// stage 2 is the horizontal pass, one lane per column (conflict-free 4-byte reads); stage 3 the vertical pass in the blend
// stage's layout (16-byte reads), then the blend and 8 pixels = 24 bytes per lane as three 8-byte stores.
__global__ __launch_bounds__(MT_THREADS) void frame_matte_box_kernel(const h16 *__restrict__ styled, const h16 *__restrict__ source,
                                                                     const h16 *__restrict__ depth, uint8_t *__restrict__ dst, int H, int W,
                                                                     long long dstride, mt_params p) {
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

    const h16 *dp = depth + (long long)b * dstride;
    for (int g = tid; g < rows * (MT_MW / 8); g += MT_THREADS) {
        const int j = g / (MT_MW / 8), cg = g % (MT_MW / 8);
        int yy = y0 - r + j;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
        const int gx = x0 - 8 + cg * 8;
        const h16 *row = dp + (long long)yy * W;
        float v[8];
        if (gx < 0 || gx >= W) {
            const float edge = mt_matte(row[gx < 0 ? 0 : W - 1], p);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = edge;
        } else {
            const h16x8 d = l2d_ld8(row + gx);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = mt_matte(d[e], p);
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
    if (flags & ~(MT_HARD | MT_FAR | MT_SHOW)) {
        l2d_set_error("frame_matte(tag %d): unknown flag bits 0x%x (1 hard, 2 far, 4 show)", op->tag, flags);
        return L2D_EINVAL;
    }
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
    const float lo = op->f[0], inv = op->f[1];
    if (!(lo >= -1.0f && lo <= 1.0f) || !(inv >= 0.0f) || inv > 3.0e38f || ((flags & MT_HARD) != 0) != (inv == 0.0f)) {
        l2d_set_error("frame_matte(tag %d): lo = %g must lie in [-1, 1], inv = %g be finite, and 0 exactly when the hard flag is set", op->tag,
                      lo, inv);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    mt_params p;
    p.lo = lo; p.inv = inv; p.flags = flags; p.r = r;
    const h16 *styled = (const h16 *)op->p[0], *source = (const h16 *)op->p[1], *depth = (const h16 *)op->p[2];
    uint8_t *dst = (uint8_t *)op->p[3];
    if (r == 0) {
        const long long total = (long long)B * (HW / 16);
        hipLaunchKernelGGL(frame_matte_point_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, styled, source, depth, dst, B,
                           (int)HW, dstride, p);
    } else {
        hipLaunchKernelGGL(frame_matte_box_kernel, dim3((W + MT_TW - 1) / MT_TW, (H + MT_TH - 1) / MT_TH, B), dim3(MT_THREADS), 0, s, styled,
                           source, depth, dst, H, W, dstride, p);
    }
    return l2d_check_launch("frame_matte", op->tag);
}
