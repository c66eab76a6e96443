// Matte hold: keep the matte still where the camera is still.  The depth matte is a fresh draw in every
// frame -- a smoothstep over that frame's depth map, normalised on that frame alone -- so the silhouette between the real and the
// styled part crawls by a few pixels while nothing in front of the camera moves.  This launch filters the matte in time with
// steady's measure of where the source moved (steady.hip), in front of the feather and the composite, which then read the held
// plane under L2D_MATTE_PLANE.  The reference has no counterpart.
//
//   m0 = the matte in front of the feather          px_ramp of the fp16 depth plane, or (PLANE) an fp32 plane as L2D_OP_FRAME_MATTE_EDGE writes it
//   b, d, D, dbar, t, w                             L2D_OP_FRAME_STEADY's, on the source's bytes against the previous record's
//   a = 1 - s (1 - w)
//   h = P + a (m0 - P)                              P: the previous held plane; three fp32 operations
//   h = min(max(h, min(m0, P)), max(m0, P))         the fp32 blend may leave [min, max] by an ulp: the clamp is part of the arithmetic
//   where a == 1: m0's own bits
//   FOLLOW: P and the previous bytes are fetched at (cl(y + dy), cl(x + dx)), (dy, dx) the vector of the pixel's own 8 x 8 block
//   INIT: h = m0, and neither the previous record nor the field is read
//
// Every floating-point step is one fp32 operation with one rounding (the file is built with -ffp-contract=off, see the Makefile),
// so that numpy restates it bit for bit (live2diff_amd/matte.py `hold_ref`).  The new record (h, b) goes to a second pair of
// buffers: a tile's halo, and a displaced fetch, read what a neighbour would write.  A bandwidth kernel in L2D_OP_FRAME_STEADY's
// tile form: 16-byte accesses to the planes and the fp16 rows, 8-byte accesses to the planar bytes, plain stores, no MFMA.
#include <string.h>

#include "steady_px.h"                        // sd_bytes8 .. sd_alpha8, fl_bytes8, the tile's sizes; frame_px.h: px_ramp, px_byte, the checks

#define MH_HARD L2D_MATTE_HOLD_HARD
#define MH_INIT L2D_MATTE_HOLD_INIT
#define MH_PLANE L2D_MATTE_HOLD_PLANE
#define MH_FOLLOW L2D_MATTE_HOLD_FOLLOW
#define MH_RAMP_HARD L2D_MATTE_HOLD_RAMP_HARD
#define MH_RAMP_FAR L2D_MATTE_HOLD_RAMP_FAR
static_assert(MH_HARD == SD_HARD, "sd_weight reads the hard bit of the flags");

#define MH_LDS_BYTES (SD_DH * SD_DW + 2 * SD_DH * SD_TW)
static_assert(MH_LDS_BYTES == 6656, "DESIGN.md section 8.z15 and tests/test_matte_hold_resources.py state this size");

struct mh_params {
    sd_params sd;                             // lo, inv, s of the motion ramp; flags: SD_HARD; r
    float rlo, rinv;                          // the depth ramp (not read with PLANE)
    int rflags;                               // L2D_MATTE_HARD | L2D_MATTE_FAR of the depth ramp
    int init;
};

// d of the 8-pixel group at row yy (clamped by the caller), column gx (a multiple of 8, inside the image or one group beside it):
// a group beside the image holds the edge pixel's value.  FOLLOW: the previous bytes along the vector of the group's own block.
template <bool FOLLOW>
__device__ __forceinline__ void mh_halo_d(const h16 *__restrict__ source, const uint8_t *__restrict__ prev_bytes,
                                          const signed char *__restrict__ field, int H, int W, long long HW, int yy, int gx, unsigned (&d)[8]) {
    const int Wb = W >> 3;
    if (gx < 0 || gx >= W) {
        const int ex = gx < 0 ? 0 : W - 1;
        const long long e0 = (long long)yy * W + ex;
        long long q0 = e0;
        if constexpr (FOLLOW) {
            const signed char *v = field + 2 * ((long long)(yy >> 3) * Wb + (ex >> 3));
            q0 = (long long)px_clampi(yy + v[0], 0, H - 1) * W + px_clampi(ex + v[1], 0, W - 1);
        }
        unsigned m = 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const unsigned a = sd_absdiff(px_byte(source[ch * HW + e0]), (unsigned)prev_bytes[ch * HW + q0]);
            m = a > m ? a : m;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = m;
    } else {
        const long long g0 = (long long)yy * W + gx;
        int dx = 0;
        long long prow = (long long)yy * W;
        if constexpr (FOLLOW) {
            const signed char *v = field + 2 * ((long long)(yy >> 3) * Wb + (gx >> 3));
            dx = v[1];
            prow = (long long)px_clampi(yy + v[0], 0, H - 1) * W;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint2 now = sd_bytes8(l2d_ld8(source + ch * HW + g0));
            uint2 before;
            if constexpr (FOLLOW) before = fl_bytes8(prev_bytes + ch * HW + prow, gx + dx, W);
            else before = *reinterpret_cast<const uint2 *>(prev_bytes + ch * HW + g0);
            sd_motion8(now, before, d);
        }
    }
}

// One work-group per SD_TH x SD_TW tile (frame_steady_box_kernel's plan; r = 0 takes it too).  A lane owns 8 consecutive pixels
// of one row: it loads their source, matte input and previous record first, writes their new bytes and their d into LDS; the
// groups of the halo (and of tile positions outside the image, which hold clamped values) follow; then the horizontal sums, one
// lane per column, the vertical sums in the owner's layout (16-byte reads), and the blend.
template <bool PLANE, bool FOLLOW>
__device__ __forceinline__ void mh_body(const h16 *__restrict__ source, const void *__restrict__ min, const float *__restrict__ prev_plane,
                                        const uint8_t *__restrict__ prev_bytes, float *__restrict__ out_plane,
                                        uint8_t *__restrict__ next_bytes, const signed char *__restrict__ field, int H, int W,
                                        const mh_params &p) {
    __shared__ __attribute__((aligned(16))) unsigned char dd[SD_DH][SD_DW];       // d of the tile and its halo
    __shared__ __attribute__((aligned(16))) unsigned short hh[SD_DH][SD_TW];      // the horizontal sums
    static_assert(sizeof(dd) + sizeof(hh) == MH_LDS_BYTES, "the LDS size the file states");
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SD_TW, y0 = blockIdx.y * SD_TH;
    const int r = p.sd.r, taps = 2 * r + 1, rows = SD_TH + 2 * r;
    const bool init = p.init != 0;
    const long long HW = (long long)H * W;

    const int by = tid >> 3, bx = (tid & 7) * 8;
    const int y = y0 + by, x = x0 + bx;
    const bool live = y < H && x < W;           // (x + 8 <= W then: W % 8 == 0)
    const long long px = (long long)y * W + x;
    h16x8 src[3];
    uint2 before[3];
    float m0[8], P[8];
    if (live) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) src[ch] = l2d_ld8(source + ch * HW + px);
        if constexpr (PLANE) {
            const f32x4 *mp = reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(min) + px);
            const f32x4 a = mp[0], b = mp[1];
#pragma unroll
            for (int e = 0; e < 4; ++e) { m0[e] = a[e]; m0[e + 4] = b[e]; }
        } else {
            const h16x8 dv = l2d_ld8(reinterpret_cast<const h16 *>(min) + px);
#pragma unroll
            for (int e = 0; e < 8; ++e) m0[e] = px_ramp(dv[e], p.rlo, p.rinv, p.rflags);
        }
        if (!init) {
            if constexpr (FOLLOW) {
                const signed char *v = field + 2 * ((long long)(y >> 3) * (W >> 3) + (x >> 3));
                const int dy = v[0], dx = v[1];
                const long long prow = (long long)px_clampi(y + dy, 0, H - 1) * W;
#pragma unroll
                for (int e = 0; e < 8; ++e) P[e] = prev_plane[prow + px_clampi(x + dx + e, 0, W - 1)];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) before[ch] = fl_bytes8(prev_bytes + ch * HW + prow, x + dx, W);
            } else {
                const f32x4 *pp = reinterpret_cast<const f32x4 *>(prev_plane + px);
                const f32x4 a = pp[0], b = pp[1];
#pragma unroll
                for (int e = 0; e < 4; ++e) { P[e] = a[e]; P[e + 4] = b[e]; }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) before[ch] = *reinterpret_cast<const uint2 *>(prev_bytes + ch * HW + px);
            }
        }
        unsigned d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint2 now = sd_bytes8(src[ch]);
            if (!init) sd_motion8(now, before[ch], d);
            *reinterpret_cast<uint2 *>(next_bytes + ch * HW + px) = now;
        }
        if (init) {
            f32x4 *op = reinterpret_cast<f32x4 *>(out_plane + px);
            op[0] = f32x4{m0[0], m0[1], m0[2], m0[3]};
            op[1] = f32x4{m0[4], m0[5], m0[6], m0[7]};
        } else {
            *reinterpret_cast<uint2 *>(&dd[r + by][8 + bx]) = px_pack8(d);
        }
    }
    if (init) return;                            // (uniform: no barrier has been passed)

    for (int g = tid; g < rows * (SD_DW / 8); g += SD_THREADS) {
        const int j = g / (SD_DW / 8), cg = g % (SD_DW / 8);
        const int yu = y0 - r + j;
        const int gx = x0 - 8 + cg * 8;
        if (j >= r && j < r + SD_TH && cg >= 1 && cg <= SD_TW / 8 && yu < H && gx < W) continue;      // its owner wrote it
        if (r == 0 && (cg == 0 || cg == SD_DW / 8 - 1)) continue;                                      // no tap reaches the side halo
        const int yy = yu < 0 ? 0 : (yu > H - 1 ? H - 1 : yu);
        unsigned d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        mh_halo_d<FOLLOW>(source, prev_bytes, field, H, W, HW, yy, gx, d);
        *reinterpret_cast<uint2 *>(&dd[j][cg * 8]) = px_pack8(d);
    }
    __syncthreads();

    // horizontal: hh[j][c] = dd[j][8 + c - r] + ... + dd[j][8 + c + r]
    for (int i = tid; i < rows * SD_TW; i += SD_THREADS) {
        const int j = i / SD_TW, cc = i % SD_TW;
        const unsigned char *s = &dd[j][8 + cc - r];
        unsigned acc = 0u;
        for (int k = 0; k < taps; ++k) acc += s[k];
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
    float w[8], a[8], h[8];
    h16x8 pic;
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = sd_weight(__fdiv_rn((float)D[e], n), p.sd);
    sd_alpha8(w, p.sd.s, a, pic);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = __fadd_rn(P[e], __fmul_rn(a[e], __fsub_rn(m0[e], P[e])));
        const float c = fminf(fmaxf(v, fminf(m0[e], P[e])), fmaxf(m0[e], P[e]));
        h[e] = a[e] == 1.0f ? m0[e] : c;
    }
    f32x4 *op = reinterpret_cast<f32x4 *>(out_plane + px);
    op[0] = f32x4{h[0], h[1], h[2], h[3]};
    op[1] = f32x4{h[4], h[5], h[6], h[7]};
}

__global__ __launch_bounds__(SD_THREADS) void frame_hold_depth_kernel(const h16 *__restrict__ source, const h16 *__restrict__ depth,
                                                                      const float *__restrict__ prev_plane,
                                                                      const uint8_t *__restrict__ prev_bytes, float *__restrict__ out_plane,
                                                                      uint8_t *__restrict__ next_bytes, int H, int W, mh_params p) {
    mh_body<false, false>(source, depth, prev_plane, prev_bytes, out_plane, next_bytes, nullptr, H, W, p);
}

__global__ __launch_bounds__(SD_THREADS) void frame_hold_plane_kernel(const h16 *__restrict__ source, const float *__restrict__ plane,
                                                                      const float *__restrict__ prev_plane,
                                                                      const uint8_t *__restrict__ prev_bytes, float *__restrict__ out_plane,
                                                                      uint8_t *__restrict__ next_bytes, int H, int W, mh_params p) {
    mh_body<true, false>(source, plane, prev_plane, prev_bytes, out_plane, next_bytes, nullptr, H, W, p);
}

__global__ __launch_bounds__(SD_THREADS) void frame_hold_depth_follow_kernel(const h16 *__restrict__ source, const h16 *__restrict__ depth,
                                                                             const float *__restrict__ prev_plane,
                                                                             const uint8_t *__restrict__ prev_bytes,
                                                                             float *__restrict__ out_plane, uint8_t *__restrict__ next_bytes,
                                                                             const signed char *__restrict__ field, int H, int W, mh_params p) {
    mh_body<false, true>(source, depth, prev_plane, prev_bytes, out_plane, next_bytes, field, H, W, p);
}

__global__ __launch_bounds__(SD_THREADS) void frame_hold_plane_follow_kernel(const h16 *__restrict__ source, const float *__restrict__ plane,
                                                                             const float *__restrict__ prev_plane,
                                                                             const uint8_t *__restrict__ prev_bytes,
                                                                             float *__restrict__ out_plane, uint8_t *__restrict__ next_bytes,
                                                                             const signed char *__restrict__ field, int H, int W, mh_params p) {
    mh_body<true, true>(source, plane, prev_plane, prev_bytes, out_plane, next_bytes, field, H, W, p);
}

int l2d_launch_frame_matte_hold(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], r = op->i[2], flags = op->i[3];
    if (flags & ~(MH_HARD | MH_INIT | MH_PLANE | MH_FOLLOW | MH_RAMP_HARD | MH_RAMP_FAR)) {
        l2d_set_error("frame_matte_hold(tag %d): unknown flag bits 0x%x (1 hard, 4 init, 16 plane, 32 follow, 64 ramp hard, 128 ramp far)",
                      op->tag, flags);
        return L2D_EINVAL;
    }
    const bool init = (flags & MH_INIT) != 0, plane = (flags & MH_PLANE) != 0, follow = (flags & MH_FOLLOW) != 0;
    for (int k = 0; k < 7; ++k) {
        const bool optional = (init && (k == 2 || k == 3 || k == 6)) || (!follow && k == 6);
        if (!op->p[k] && !optional) {
            l2d_set_error("frame_matte_hold(tag %d): pointer %d is null (2, 3 and 6 may be with the init flag, 6 without the follow flag)",
                          op->tag, k);
            return L2D_EINVAL;
        }
        if (k < 6 && (((uintptr_t)op->p[k]) & ((k == 3 || k == 5) ? 7 : 15))) {
            l2d_set_error("frame_matte_hold(tag %d): pointer %d is not aligned (planes and frames 16 bytes, byte planes 8)", op->tag, k);
            return L2D_EINVAL;
        }
    }
    const long long HW = px_check_frame("frame_matte_hold", op->tag, H, W);
    if (HW < 0) return L2D_EINVAL;
    if (r < 0 || r > SD_MAX_R) {
        l2d_set_error("frame_matte_hold(tag %d): radius %d, need 0..%d", op->tag, r, SD_MAX_R);
        return L2D_EINVAL;
    }
    const float lo = op->f[0], inv = op->f[1], st = op->f[2];
    if (!sd_check_floats("frame_matte_hold", op->tag, lo, inv, st)) return L2D_EINVAL;
    float rlo = 0.0f, rinv = 0.0f;
    if (!plane) {
        memcpy(&rlo, &op->i[4], sizeof(float));
        memcpy(&rinv, &op->i[5], sizeof(float));
        if (!px_check_ramp("frame_matte_hold", op->tag, rlo, rinv, (flags & MH_RAMP_HARD) != 0)) return L2D_EINVAL;
    } else if (flags & (MH_RAMP_HARD | MH_RAMP_FAR)) {
        l2d_set_error("frame_matte_hold(tag %d): the ramp's flags do not go with a plane (it carries them)", op->tag);
        return L2D_EINVAL;
    }
    // the new record never lies where this launch reads (a tile's halo and a displaced fetch read what a neighbour would write),
    // nor do its two parts share a byte
    const void *const rd[4] = {op->p[0], op->p[1], op->p[2], op->p[3]};
    const long long rdn[4] = {HW * 6, plane ? HW * 4 : HW * 2, HW * 4, HW * 3};
    const void *const wr[2] = {op->p[4], op->p[5]};
    const long long wrn[2] = {HW * 4, HW * 3};
    for (int a = 0; a < 2; ++a) {
        for (int b = 0; b < 4; ++b) {
            if (px_overlap(wr[a], wrn[a], rd[b], rdn[b])) {
                l2d_set_error("frame_matte_hold(tag %d): output %d overlaps input %d (the out plane / next_bytes against the source, the "
                              "matte input, prev_plane, prev_bytes)", op->tag, 4 + a, b);
                return L2D_EINVAL;
            }
        }
    }
    if (px_overlap(wr[0], wrn[0], wr[1], wrn[1])) {
        l2d_set_error("frame_matte_hold(tag %d): the out plane overlaps next_bytes", op->tag);
        return L2D_EINVAL;
    }
    const long long fb = 2ll * ((H + 7) / 8) * (W / 8);
    if (follow && (px_overlap(op->p[6], fb, wr[0], wrn[0]) || px_overlap(op->p[6], fb, wr[1], wrn[1]))) {
        l2d_set_error("frame_matte_hold(tag %d): the field overlaps an output (the out plane or next_bytes)", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    mh_params p;
    p.sd.lo = lo; p.sd.inv = inv; p.sd.s = st; p.sd.flags = (flags & MH_HARD) ? SD_HARD : 0; p.sd.r = r;
    p.rlo = rlo; p.rinv = rinv;
    p.rflags = ((flags & MH_RAMP_HARD) ? L2D_MATTE_HARD : 0) | ((flags & MH_RAMP_FAR) ? L2D_MATTE_FAR : 0);
    p.init = init ? 1 : 0;
    const h16 *source = (const h16 *)op->p[0];
    const float *prev_plane = (const float *)op->p[2];
    const uint8_t *prev_bytes = (const uint8_t *)op->p[3];
    float *out_plane = (float *)op->p[4];
    uint8_t *next_bytes = (uint8_t *)op->p[5];
    const signed char *field = (const signed char *)op->p[6];
    const dim3 tiles((W + SD_TW - 1) / SD_TW, (H + SD_TH - 1) / SD_TH), threads(SD_THREADS);
    if (follow && !init) {                         // (an init frame looks nowhere: the variant without the field)
        if (plane)
            hipLaunchKernelGGL(frame_hold_plane_follow_kernel, tiles, threads, 0, s, source, (const float *)op->p[1], prev_plane, prev_bytes,
                               out_plane, next_bytes, field, H, W, p);
        else
            hipLaunchKernelGGL(frame_hold_depth_follow_kernel, tiles, threads, 0, s, source, (const h16 *)op->p[1], prev_plane, prev_bytes,
                               out_plane, next_bytes, field, H, W, p);
    } else if (plane) {
        hipLaunchKernelGGL(frame_hold_plane_kernel, tiles, threads, 0, s, source, (const float *)op->p[1], prev_plane, prev_bytes, out_plane,
                           next_bytes, H, W, p);
    } else {
        hipLaunchKernelGGL(frame_hold_depth_kernel, tiles, threads, 0, s, source, (const h16 *)op->p[1], prev_plane, prev_bytes, out_plane,
                           next_bytes, H, W, p);
    }
    return l2d_check_launch("frame_matte_hold", op->tag);
}
