// The output chain's pixel arithmetic: the one definition of what its stages must agree on bit for bit
// -- the egress op's byte, the depth ramp, the integer luma, the bilinear tap staging of `matte.up_table`, the store of a tile row
// at any alignment -- and of the argument checks their launchers share.  Two rules go with it:
//   * px_unit and px_byte hold no contractable expression (every multiplication and addition is rounded to fp16 or feeds a
//     comparison before the next one), so they give the same bits in frame_io.hip and resize.hip, which are built with
//     -ffp-contract=fast, as in the files built without contraction.
//   * px_ramp, like everything written with __f*_rn, is bit-exact only in a file built with -ffp-contract=off: with contraction
//     the backend fuses the intrinsics whatever the source says (the Makefile's comment on wblend).  All of its users are.
#pragma once
#include "common.h"

#ifdef __HIPCC__
// v = clamp(fp16(fp16(x / 2) + 0.5), 0, 1): the reference's expression on an fp16 tensor with its rounding points
// (image_utils.py:13,30), widened to fp32
__device__ __forceinline__ float px_unit(h16 x) {
    const h16 t = (h16)((float)x * 0.5f);
    const float v = (float)(h16)((float)t + 0.5f);
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}

// the egress op's byte
__device__ __forceinline__ unsigned px_byte(h16 x) {
    return (unsigned)rintf(255.0f * px_unit(x));        // 255 v is exact in fp32 (11 x 8 bits); rint rounds half to even
}

// the depth matte's ramp: t = clamp((d - lo) inv, 0, 1) (hard: d >= lo), m = t t (3 - 2 t) (far: 1 - m); `flags` are L2D_MATTE_*
__device__ __forceinline__ float px_ramp(h16 depth, float lo, float inv, int flags) {
    const float d = (float)depth;
    float t;
    if (flags & L2D_MATTE_HARD) {
        t = d >= lo ? 1.0f : 0.0f;
    } else {
        t = __fmul_rn(__fsub_rn(d, lo), inv);
        t = fminf(fmaxf(t, 0.0f), 1.0f);
    }
    const float m = __fmul_rn(__fmul_rn(t, t), __fsub_rn(3.0f, __fmul_rn(2.0f, t)));
    return (flags & L2D_MATTE_FAR) ? __fsub_rn(1.0f, m) : m;
}

__device__ __forceinline__ unsigned px_luma(unsigned r, unsigned g, unsigned b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

__device__ __forceinline__ int px_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// eight values below 256 -> their bytes, lowest first
__device__ __forceinline__ uint2 px_pack8(const unsigned *v) {
    return make_uint2(v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24), v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24));
}

// One axis of an output tile under a bilinear table (matte.up_table: first tap, second tap, weight): the span [s0, s0 + n) of
// source coordinates the taps of outputs o0 .. o0 + t - 1 reach, at most SPAN.  Everything read from a table is clamped to the
// image and to the span, so a wrong table gives a wrong picture and never an access outside a buffer.
template <int SPAN>
__device__ __forceinline__ void px_span(const int *__restrict__ tab, int n_out, int n_in, int o0, int t, int &s0, int &n) {
    s0 = px_clampi(tab[o0], 0, n_in - 1);
    const int s1 = px_clampi(tab[n_out + o0 + t - 1], s0, n_in - 1);
    n = s1 - s0 + 1 > SPAN ? SPAN : s1 - s0 + 1;
}

// ... and output o0 + lane's two taps relative to s0 and its weight
__device__ __forceinline__ void px_stage(const int *__restrict__ tab, int n_out, int n_in, int o0, int t, int s0, int n, int lane,
                                         int *i0, int *i1, float *f) {
    int a = 0, b = 0;
    float w = 0.0f;
    if (lane < t) {
        a = px_clampi(px_clampi(tab[o0 + lane], 0, n_in - 1) - s0, 0, n - 1);
        b = px_clampi(px_clampi(tab[n_out + o0 + lane], 0, n_in - 1) - s0, 0, n - 1);
        w = __int_as_float(tab[2 * n_out + o0 + lane]);
        w = fminf(fmaxf(w, 0.0f), 1.0f);          // (a weight of `up_table` lies in [0, 1]: this changes none of them)
    }
    i0[lane] = a;
    i1[lane] = b;
    f[lane] = w;
}

// A tile row of nb bytes `o` to an address `g` of any alignment: bytes up to the first dword boundary, whole dwords, bytes behind
// the last one.  Lane `it` of the row does one store (or none): nb / 4 + 6 lanes cover a row.  Only g[0 .. nb) is written.
__device__ __forceinline__ void px_store_row(uint8_t *g, const unsigned char *o, int nb, int it) {
    int head = (int)((0 - (uintptr_t)g) & 3);
    head = head > nb ? nb : head;
    const int ndw = (nb - head) >> 2;
    const int tail = nb - head - ndw * 4;
    if (it < head) {
        g[it] = o[it];
    } else if (it < head + ndw) {
        const int e = head + (it - head) * 4;
        *reinterpret_cast<unsigned *>(g + e) =
            (unsigned)o[e] | ((unsigned)o[e + 1] << 8) | ((unsigned)o[e + 2] << 16) | ((unsigned)o[e + 3] << 24);
    } else if (it < head + ndw + tail) {
        const int e = head + ndw * 4 + (it - head - ndw);
        g[e] = o[e];
    }
}
#endif

// ------------------------------------------------------------------------------------------------------------------------------
// the launchers' checks; each sets the error and returns false (px_check_frame: -1) where it refuses

// do [a, a + na) and [b, b + nb) share a byte?  (a null pointer overlaps nothing)
static inline bool px_overlap(const void *a, long long na, const void *b, long long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// an output size along one axis: 1..L2D_RESIZE_MAX_SIZE and between half and 8 times its source size
static inline bool px_axis_ok(int n_in, int n_out) {
    return n_out >= 1 && n_out <= L2D_RESIZE_MAX_SIZE && 2ll * n_out >= n_in && n_out <= 8ll * n_in;
}

// the geometry of a tiled stream-size launch: returns H W
static inline long long px_check_frame(const char *name, int tag, int H, int W) {
    if (H <= 0 || W <= 0) {
        l2d_set_error("%s(tag %d): invalid arguments (non-positive size %d x %d)", name, tag, H, W);
        return -1;
    }
    if (W % 8) {
        l2d_set_error("%s(tag %d): W = %d must be a multiple of 8", name, tag, W);
        return -1;
    }
    const long long HW = (long long)H * W;
    if (3 * HW >= (1ll << 31)) {
        l2d_set_error("%s(tag %d): 3 H W = %lld must stay below 2^31", name, tag, 3 * HW);
        return -1;
    }
    return HW;
}

static inline bool px_check_ramp(const char *name, int tag, float lo, float inv, bool hard) {
    if (!(lo >= -1.0f && lo <= 1.0f) || !(inv >= 0.0f) || inv > 3.0e38f || hard != (inv == 0.0f)) {
        l2d_set_error("%s(tag %d): lo = %g must lie in [-1, 1], inv = %g be finite, and 0 exactly when the hard flag is set", name, tag, lo,
                      inv);
        return false;
    }
    return true;
}

// the first n pointers of the op: none null, all 16-byte aligned
static inline bool px_check_pointers16(const char *name, const l2d_op *op, int n) {
    for (int k = 0; k < n; ++k) {
        if (!op->p[k]) {
            l2d_set_error("%s(tag %d): pointer %d is null", name, op->tag, k);
            return false;
        }
        if (((uintptr_t)op->p[k]) & 15) {
            l2d_set_error("%s(tag %d): pointer %d is not 16-byte aligned", name, op->tag, k);
            return false;
        }
    }
    return true;
}
