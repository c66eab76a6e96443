// Steady: hold still what the camera holds still.  The temporal attention keeps the stream's structure
// coherent and the colour lock its global colour statistics; nothing holds a pixel, so a wall that does not move in the camera
// shimmers in the styled output.  This launch measures, in exact integers on the BYTES a viewer would see, where the frame's
// source moved since the source of the output before, holds the previous output pixel where it did not (a per-pixel EMA) and
// lets the new styled pixel through untouched where it did.  The reference has no counterpart.
//
//   b = rint(255 clamp(fp16(fp16(x / 2) + 0.5), 0, 1))      the egress op's byte of the source frame (frame_px.h px_byte)
//   d = max_c |b_c - bp_c|                                   bp: the bytes of the previous output's source; an integer in 0..255
//   D = sum of d over the (2r+1) x (2r+1) window             coordinates clamped to the image; an integer: any order
//   dbar = float(D) / float((2r+1)^2)                        one correctly rounded division (r = 0: float(d))
//   t = clamp((dbar - lo) inv, 0, 1)                         (hard: t = dbar >= lo ? 1 : 0)
//   w = (t t) (3 - 2 t)                                      1 = moving, 0 = still
//   a = 1 - s (1 - w)
//   o = half(P + a (S - P))                                  where a == 1: S's own bits
//   show: picture = half(2 w - 1) in all three channels, beside o
//   init: o = S, and nothing of the previous state is read
//
// Every floating-point step is one fp32 operation with one rounding (the file is built with -ffp-contract=off, see the
// Makefile), so that numpy restates it bit for bit (live2diff_amd/steady.py `steady_ref`).  The new state (o, b) goes to a
// second pair of buffers: the tile form's halo reads neighbours' previous bytes, so no block may read what another writes.
// A bandwidth kernel: 16-byte accesses to the fp16 rows, 8-byte accesses to the planar bytes, plain stores, no MFMA.
#include "steady_px.h"                        // the helpers steady_follow.hip shares: sd_params, sd_bytes8 .. sd_alpha8

#define SD_POINT_THREADS 256

// r = 0, and every init frame: each pixel on its own.  One lane = 8 consecutive pixels of the [H W] plane: per channel three
// 16-byte loads, one 8-byte load, one 16-byte and one 8-byte store.
__global__ __launch_bounds__(SD_POINT_THREADS) void frame_steady_point_kernel(const h16 *__restrict__ styled, const h16 *__restrict__ source,
                                                                              const h16 *__restrict__ prev_out,
                                                                              const uint8_t *__restrict__ prev_bytes, h16 *__restrict__ out,
                                                                              uint8_t *__restrict__ next_bytes, h16 *__restrict__ picture,
                                                                              int HW, sd_params p) {
    const long long px = ((long long)blockIdx.x * SD_POINT_THREADS + threadIdx.x) * 8;
    if (px >= HW) return;                          // (px + 8 <= H W then: W % 8 == 0)
    const bool init = (p.flags & SD_INIT) != 0, show = (p.flags & SD_SHOW) != 0;
    h16x8 S[3], P[3];
    uint2 now[3];
    unsigned d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const long long off = (long long)ch * HW + px;
        S[ch] = l2d_ld8(styled + off);
        P[ch] = init ? S[ch] : l2d_ld8(prev_out + off);
        now[ch] = sd_bytes8(l2d_ld8(source + off));
        if (!init) sd_motion8(now[ch], *reinterpret_cast<const uint2 *>(prev_bytes + off), d);
    }
    float w[8], a[8];
    h16x8 pic;
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = sd_weight((float)d[e], p);
    sd_alpha8(w, p.s, a, pic);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const long long off = (long long)ch * HW + px;
        const h16x8 o = init ? S[ch] : sd_blend8(S[ch], P[ch], a);
        l2d_st8(out + off, o);
        if (show) l2d_st8(picture + off, init ? S[ch] : pic);
        *reinterpret_cast<uint2 *>(next_bytes + off) = now[ch];
    }
}

// r > 0: one work-group per SD_TH x SD_TW tile (frame_matte_box_kernel's plan).  Stage 1 writes d of the tile and its halo
// into LDS (rows clamped to the image; an 8-pixel group lies wholly inside or wholly outside it because W % 8 == 0, and one
// outside holds the edge pixel's value) and, for the groups of the tile itself, the new bytes; stage 2 is the horizontal
// sum, one lane per column; stage 3 the vertical sum in the blend stage's layout (16-byte reads), then the blend.
__global__ __launch_bounds__(SD_THREADS) void frame_steady_box_kernel(const h16 *__restrict__ styled, const h16 *__restrict__ source,
                                                                      const h16 *__restrict__ prev_out,
                                                                      const uint8_t *__restrict__ prev_bytes, h16 *__restrict__ out,
                                                                      uint8_t *__restrict__ next_bytes, h16 *__restrict__ picture, int H,
                                                                      int W, sd_params p) {
    __shared__ __attribute__((aligned(16))) unsigned char dd[SD_DH][SD_DW];       // d of the tile and its halo
    __shared__ __attribute__((aligned(16))) unsigned short hh[SD_DH][SD_TW];      // the horizontal sums
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SD_TW, y0 = blockIdx.y * SD_TH;
    const int r = p.r, taps = 2 * r + 1, rows = SD_TH + 2 * r;
    const bool show = (p.flags & SD_SHOW) != 0;
    const long long HW = (long long)H * W;

    // this lane's 8 pixels of the blend stage: their loads are issued first, the sums run under them
    const int by = tid >> 3, bx = (tid & 7) * 8;
    const int y = y0 + by, x = x0 + bx;
    const bool live = y < H && x < W;           // (x + 8 <= W then: W % 8 == 0)
    const long long px = (long long)y * W + x;
    h16x8 S[3], P[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        S[ch] = live ? l2d_ld8(styled + ch * HW + px) : l2d_zero8();
        P[ch] = live ? l2d_ld8(prev_out + ch * HW + px) : l2d_zero8();
    }

    for (int g = tid; g < rows * (SD_DW / 8); g += SD_THREADS) {
        const int j = g / (SD_DW / 8), cg = g % (SD_DW / 8);
        const int yu = y0 - r + j;
        const int yy = yu < 0 ? 0 : (yu > H - 1 ? H - 1 : yu);
        const int gx = x0 - 8 + cg * 8;
        unsigned d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (gx < 0 || gx >= W) {
            const long long e0 = (long long)yy * W + (gx < 0 ? 0 : W - 1);
            unsigned m = 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const unsigned a = sd_absdiff(px_byte(source[ch * HW + e0]), (unsigned)prev_bytes[ch * HW + e0]);
                m = a > m ? a : m;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = m;
        } else {
            const long long g0 = (long long)yy * W + gx;
            const bool own = yu == yy && j >= r && j < r + SD_TH && cg >= 1 && cg <= SD_TW / 8;     // a group of the tile itself
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const uint2 now = sd_bytes8(l2d_ld8(source + ch * HW + g0));
                sd_motion8(now, *reinterpret_cast<const uint2 *>(prev_bytes + ch * HW + g0), d);
                if (own) *reinterpret_cast<uint2 *>(next_bytes + ch * HW + g0) = now;
            }
        }
        *reinterpret_cast<uint2 *>(&dd[j][cg * 8]) = px_pack8(d);
    }
    __syncthreads();

    // horizontal: hh[j][c] = dd[j][8 + c - r] + ... + dd[j][8 + c + r]
    for (int i = tid; i < rows * SD_TW; i += SD_THREADS) {
        const int j = i / SD_TW, cc = i % SD_TW;
        const unsigned char *src = &dd[j][8 + cc - r];
        unsigned acc = 0u;
        for (int k = 0; k < taps; ++k) acc += src[k];
        hh[j][cc] = (unsigned short)acc;
    }
    __syncthreads();
    if (!live) return;

    // vertical: D[e] = hh[by][bx + e] + ... + hh[by + 2 r][bx + e]
    unsigned D[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (int k = 0; k < taps; ++k) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&hh[by + k][bx]);
        D[0] += v.x & 65535u; D[1] += v.x >> 16;
        D[2] += v.y & 65535u; D[3] += v.y >> 16;
        D[4] += v.z & 65535u; D[5] += v.z >> 16;
        D[6] += v.w & 65535u; D[7] += v.w >> 16;
    }
    const float n = (float)(taps * taps);
    float w[8], a[8];
    h16x8 pic;
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = sd_weight(__fdiv_rn((float)D[e], n), p);
    sd_alpha8(w, p.s, a, pic);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        l2d_st8(out + ch * HW + px, sd_blend8(S[ch], P[ch], a));
        if (show) l2d_st8(picture + ch * HW + px, pic);
    }
}

int l2d_launch_frame_steady(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], r = op->i[2], flags = op->i[3];
    if (flags & ~(SD_HARD | SD_SHOW | SD_INIT)) {
        l2d_set_error("frame_steady(tag %d): unknown flag bits 0x%x (1 hard, 2 show, 4 init)", op->tag, flags);
        return L2D_EINVAL;
    }
    const bool init = (flags & SD_INIT) != 0, show = (flags & SD_SHOW) != 0;
    for (int k = 0; k < 7; ++k) {
        const bool optional = (init && (k == 2 || k == 3)) || (!show && k == 6);
        if (!op->p[k] && !optional) {
            l2d_set_error("frame_steady(tag %d): pointer %d is null (2 and 3 may be with the init flag, 6 without the show flag)", op->tag, k);
            return L2D_EINVAL;
        }
        if (((uintptr_t)op->p[k]) & ((k == 3 || k == 5) ? 7 : 15)) {
            l2d_set_error("frame_steady(tag %d): pointer %d is not aligned (fp16 frames 16 bytes, byte planes 8)", op->tag, k);
            return L2D_EINVAL;
        }
    }
    const long long HW = px_check_frame("frame_steady", op->tag, H, W);
    if (HW < 0) return L2D_EINVAL;
    if (r < 0 || r > SD_MAX_R) {
        l2d_set_error("frame_steady(tag %d): radius %d, need 0..%d", op->tag, r, SD_MAX_R);
        return L2D_EINVAL;
    }
    // the new state never lies where this launch reads: other blocks' halos read the previous bytes, every block its styled
    // and previous pixels (an exact alias is refused by the same test)
    const void *const hread[3] = {op->p[0], op->p[1], op->p[2]};
    const void *const hwrite[2] = {op->p[4], show ? op->p[6] : nullptr};
    for (int a = 0; a < 2; ++a) {
        for (int b = 0; b < 3; ++b) {
            if (px_overlap(hwrite[a], HW * 6, hread[b], HW * 6)) {
                l2d_set_error("frame_steady(tag %d): output frame %d overlaps input frame %d (out / the picture against styled, source, "
                              "prev_out)", op->tag, a ? 6 : 4, b);
                return L2D_EINVAL;
            }
        }
    }
    if (show && px_overlap(op->p[4], HW * 6, op->p[6], HW * 6)) {
        l2d_set_error("frame_steady(tag %d): the picture overlaps the output frame", op->tag);
        return L2D_EINVAL;
    }
    if (px_overlap(op->p[5], HW * 3, op->p[3], HW * 3)) {
        l2d_set_error("frame_steady(tag %d): next_bytes overlaps prev_bytes (a tile's halo reads what its neighbour would write)", op->tag);
        return L2D_EINVAL;
    }
    const float lo = op->f[0], inv = op->f[1], st = op->f[2];
    if (!sd_check_floats("frame_steady", op->tag, lo, inv, st)) return L2D_EINVAL;
    L2D_DRY_RETURN();
    sd_params p;
    p.lo = lo; p.inv = inv; p.s = st; p.flags = flags; p.r = r;
    const h16 *styled = (const h16 *)op->p[0], *source = (const h16 *)op->p[1], *prev_out = (const h16 *)op->p[2];
    const uint8_t *prev_bytes = (const uint8_t *)op->p[3];
    h16 *out = (h16 *)op->p[4], *picture = (h16 *)op->p[6];
    uint8_t *next_bytes = (uint8_t *)op->p[5];
    if (r == 0 || init) {
        const long long lanes = HW / 8;
        hipLaunchKernelGGL(frame_steady_point_kernel, dim3((unsigned)((lanes + SD_POINT_THREADS - 1) / SD_POINT_THREADS)),
                           dim3(SD_POINT_THREADS), 0, s, styled, source, prev_out, prev_bytes, out, next_bytes, picture, (int)HW, p);
    } else {
        hipLaunchKernelGGL(frame_steady_box_kernel, dim3((W + SD_TW - 1) / SD_TW, (H + SD_TH - 1) / SD_TH), dim3(SD_THREADS), 0, s, styled,
                           source, prev_out, prev_bytes, out, next_bytes, picture, H, W, p);
    }
    return l2d_check_launch("frame_steady", op->tag);
}
