// The steady mode's pixel helpers (DESIGN.md sections 8.z8, 8.z14 and 8.z15): the byte motion, the weight, the alpha and the blend,
// shared by steady.hip (L2D_OP_FRAME_STEADY), steady_follow.hip (L2D_OP_FRAME_STEADY_FOLLOW) and matte_hold.hip
// (L2D_OP_FRAME_MATTE_HOLD), so that all give the same bits.
// Everything written with __f*_rn is bit-exact only in a file built with -ffp-contract=off (frame_px.h's second rule): all are.
#pragma once
#include "frame_px.h"

#define SD_MAX_R L2D_STEADY_MAX_R
#define SD_TW 64                              // tile width in pixels: 8 lanes of 8 pixels
#define SD_TH 16                              // tile height
#define SD_THREADS (SD_TH * SD_TW / 8)        // 128: one lane = 8 consecutive pixels of one row in the blend stage
#define SD_DW (SD_TW + 16)                    // the tile's row of d: one 8-pixel group of halo on either side (r <= 8)
#define SD_DH (SD_TH + 2 * SD_MAX_R)

#define SD_HARD L2D_STEADY_HARD
#define SD_SHOW L2D_STEADY_SHOW
#define SD_INIT L2D_STEADY_INIT

static_assert(SD_MAX_R <= 8, "the halo is one 8-pixel group on either side");
static_assert(255 * (2 * SD_MAX_R + 1) < 65536, "a row sum of d fits 16 bits");

struct sd_params {
    float lo, inv, s;
    int flags, r;
};

#ifdef __HIPCC__
__device__ __forceinline__ unsigned sd_absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

// 8 pixels of one source plane -> their 8 bytes, packed lowest pixel first
__device__ __forceinline__ uint2 sd_bytes8(h16x8 c) {
    unsigned lo = 0u, hi = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        lo |= px_byte(c[e]) << (8 * e);
        hi |= px_byte(c[e + 4]) << (8 * e);
    }
    return make_uint2(lo, hi);
}

// d[e] = max(d[e], |now_e - before_e|) over the 8 packed bytes of one channel
__device__ __forceinline__ void sd_motion8(uint2 now, uint2 before, unsigned (&d)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned a = sd_absdiff((now.x >> (8 * e)) & 255u, (before.x >> (8 * e)) & 255u);
        const unsigned b = sd_absdiff((now.y >> (8 * e)) & 255u, (before.y >> (8 * e)) & 255u);
        d[e] = a > d[e] ? a : d[e];
        d[e + 4] = b > d[e + 4] ? b : d[e + 4];
    }
}

// 8 consecutive pixels of a byte row from column x on, each column clamped to the image on its own
__device__ __forceinline__ uint2 fl_bytes8(const uint8_t *__restrict__ row, int x, int W) {
    unsigned q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = row[px_clampi(x + e, 0, W - 1)];
    return px_pack8(q);
}

// dbar -> w
__device__ __forceinline__ float sd_weight(float dbar, const sd_params &p) {
    float t;
    if (p.flags & SD_HARD) {
        t = dbar >= p.lo ? 1.0f : 0.0f;
    } else {
        t = __fmul_rn(__fsub_rn(dbar, p.lo), p.inv);
        t = fminf(fmaxf(t, 0.0f), 1.0f);
    }
    return __fmul_rn(__fmul_rn(t, t), __fsub_rn(3.0f, __fmul_rn(2.0f, t)));
}

// 8 pixels of one channel: o = half(P + a (S - P)), S's own bits where a == 1
__device__ __forceinline__ h16x8 sd_blend8(h16x8 S, h16x8 P, const float (&a)[8]) {
    h16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float s = (float)S[e], q = (float)P[e];
        const h16 v = (h16)__fadd_rn(q, __fmul_rn(a[e], __fsub_rn(s, q)));
        o[e] = a[e] == 1.0f ? S[e] : v;
    }
    return o;
}

// w of 8 pixels -> a, and with show the picture half(2 w - 1)
__device__ __forceinline__ void sd_alpha8(const float (&w)[8], float s, float (&a)[8], h16x8 &pic) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        a[e] = __fsub_rn(1.0f, __fmul_rn(s, __fsub_rn(1.0f, w[e])));
        pic[e] = (h16)__fsub_rn(__fmul_rn(2.0f, w[e]), 1.0f);
    }
}
#endif

// the checks L2D_OP_FRAME_STEADY and L2D_OP_FRAME_STEADY_FOLLOW share on their floats: false, with the error set, where they refuse
static inline bool sd_check_floats(const char *name, int tag, float lo, float inv, float st) {
    if (!(lo >= 0.0f && lo <= 3.0e38f) || !(inv >= 0.0f && inv <= 3.0e38f)) {
        l2d_set_error("%s(tag %d): lo = %g and inv = %g must be finite and not negative", name, tag, lo, inv);
        return false;
    }
    if (!(st >= 0.0f && st <= 1.0f)) {
        l2d_set_error("%s(tag %d): strength = %g must lie in [0, 1]", name, tag, st);
        return false;
    }
    return true;
}
