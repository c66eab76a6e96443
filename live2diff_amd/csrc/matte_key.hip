// Matte key: cut the frame by a colour or by a clean plate.  Every pixel of the frame's source is
// compared, on the bytes a viewer would see, against a key colour (a green or blue screen) or against a picture of the empty room
// taken by a camera that does not move; where it differs is the subject.  The launch writes the raw matte plane of the output
// chain, fp32 [H][W] in [0, 1], exactly as L2D_OP_MASK_INGEST writes it, so everything behind the raw matte -- edge refit, hold,
// feather, backdrop, both composites, `show` -- reads it under its plane flag.  The reference has no counterpart.
//
//   b = px_byte of the fp16 source (3 channels)      k = the key: three bytes of the record, or (PLATE) planar uint8 [3][H][W]
//   dR, dG, dB = b - k                               integers in -255 .. 255
//   dy = (77 dR + 150 dG + 29 dB + 128) >> 8         arithmetic shift; formed as px_luma(d + 255) - 255, which is the same integer
//   cb = dB - dy, cr = dR - dy
//   D = cb^2 + cr^2 + ((L dy^2 + 128) >> 8)          L = rint(256 luma) in 0 .. 256
//   S = the sum of D over the (2 r + 1)^2 window, coordinates clamped to the image, r in 0 .. 4
//   mean = float(S) / float((2 r + 1)^2)             one correctly rounded conversion, one correctly rounded division
//   t = clamp((mean - lo2) inv, 0, 1)  (HARD: mean >= lo2), m = t t (3 - 2 t)            sd_weight of steady_px.h
//   P = rint(255 m), half to even; INVERT: 255 - P;  mu = float(P) / 255
//   out = mu (replace), min(m_r, mu) (AND), max(m_r, mu) (OR)                            m_r: px_ramp of the depth plane
//
// Bounds: |cb|, |cr| <= 510 and dy^2 <= 255^2, so D <= 2 * 510^2 + 255^2 = 585,225 < 2^20, and a window sum <= 81 D < 2^26 < 2^31:
// 32-bit integers hold everything (the static_asserts below).  The integers are exact and every floating-point step is one fp32
// operation with one rounding (the file is built with -ffp-contract=off, see the Makefile), so numpy restates the plane bit for
// bit (live2diff_amd/matte_key.py key_ref, mask_io.front_ref).  L2D_OP_FRAME_MATTE_HOLD's tile form: one work-group per SD_TH x
// SD_TW tile, 8 pixels per lane; D of the tile and of one 8-pixel group of halo on either side goes to LDS as 32-bit integers,
// then the row sums, then the column sums in the owner's layout.  Every element of the plane is written by a plain store on every
// launch: nothing is zeroed, there is no atomic.
//
// L2D_OP_FRAME_PLANAR_BYTES is the plate capture: the fp16 source -> its planar egress bytes, one lane per 8 pixels.
//
// L2D_OP_MATTE_KEY_ADAPT is the plate key over a plate that follows drifting light.  The plate is a
// state record, planar uint16 [3][H][W] in 8.8 fixed point (0 .. 65280); the byte the key compares against is k = (s + 128) >> 8,
// and the plane is formed and written exactly as above.  Behind the plane's stores every lane moves the three channels of its 8
// pixels towards the source's bytes and writes them to the NEXT record:
//   P0 = P in front of INVERT, an integer 0 .. 255       a = (a_bg (255 - P0) + a_fg P0 + 127) / 255     a_bg, a_fg in 0 .. 32768
//   e = 256 b - s                                        s' = s + ((a e + 32768) >> 16)                  arithmetic shift
// |e| <= 65280 and a <= 32768, so |a e| + 32768 <= 2,139,127,808 < 2^31, and s' stays in 0 .. 65280 because a / 65536 <= 1 / 2
// (the static_asserts below).  INIT reads the plate's bytes instead of a record: s = 256 k.  The record read is never the record
// written, because a tile's halo reads what a neighbour would write: the two ping-pong (live2diff_amd/matte_key.py adapt_ref).
//
// The plate gain follows a sudden exposure or white-balance step: one gain per channel between the plate
// and the frame's source, measured on every keyed frame, by which the plate's bytes are multiplied in front of mk_D.
//   L2D_OP_MATTE_KEY_GAIN_HIST: per pixel and channel, valid when 16 <= k <= 239 and 4 <= b <= 251, q = min(511, (128 b + (k >> 1))
//   / k), the ratio in units of 1 / 128; every block of MKG_BLOCK pixels counts its valid samples per (channel, q) in LDS and
//   writes the 3 x 512 counts to its partial.  L2D_OP_MATTE_KEY_GAIN: the partials' sum, then per channel n and the lower median
//   g (the smallest q with 2 cum(q) >= n; 128 if n < min_count), clamped to [ceil(16384 / lim), lim] -> the record int32 {g_r,
//   g_g, g_b, n_r, n_g, n_b, 0, 0}.  L2D_MATTE_KEY_GAIN on ops 59 and 61: k' = min(255, (g k + 64) >> 7) takes k's place in the
//   key; the state's update does not read it.  g k + 64 <= 511 * 255 + 64 < 2^17 and a count <= H W < 2^31 / 3, so 2 cum fits 32
//   bits (the static_asserts below).  g = 128 gives k' = k: the unflagged kernels' bits.
#include "steady_px.h"                        // the tile's sizes, sd_weight; frame_px.h: px_byte, px_luma, px_pack8, px_ramp, the checks

#define MK_MAX_R L2D_MATTE_KEY_MAX_R
#define MK_PLATE L2D_MATTE_KEY_PLATE
#define MK_HARD L2D_MATTE_KEY_HARD
#define MK_INVERT L2D_MATTE_KEY_INVERT
#define MK_AND L2D_MATTE_KEY_AND
#define MK_OR L2D_MATTE_KEY_OR
#define MK_RAMP_HARD L2D_MATTE_KEY_RAMP_HARD
#define MK_RAMP_FAR L2D_MATTE_KEY_RAMP_FAR
#define MK_ADAPT_INIT L2D_MATTE_KEY_ADAPT_INIT
#define MK_MAX_RATE L2D_MATTE_KEY_MAX_RATE
#define MK_GAIN L2D_MATTE_KEY_GAIN
#define MKG_STATE L2D_MATTE_KEY_GAIN_STATE
#define MKG_UNITY L2D_MATTE_KEY_GAIN_UNITY
#define MKG_BINS L2D_MATTE_KEY_GAIN_BINS
#define MKG_BLOCK L2D_MATTE_KEY_GAIN_BLOCK
#define MKG_THREADS 512                       // L2D_OP_MATTE_KEY_GAIN_HIST: one 8-pixel group per lane
#define MKG_MEDIAN_THREADS (2 * MKG_BINS)     // L2D_OP_MATTE_KEY_GAIN: two lanes per bin
#define MKG_LDS_BYTES (3 * MKG_BINS * 4)
#define MK_MAX_STATE (255 * 256)              // a plate byte in 8.8 fixed point
#define MK_DH (SD_TH + 2 * MK_MAX_R)          // the rows of D under one tile: 24
#define MK_MAX_L 256
#define MK_MAX_D (2 * 510 * 510 + ((MK_MAX_L * 255 * 255 + 128) >> 8))

#define MK_LDS_BYTES (MK_DH * SD_DW * 4 + MK_DH * SD_TW * 4)
static_assert(MK_LDS_BYTES == 13824, "DESIGN.md section 8.z17, l2d.h and tests/test_matte_key_resources.py state this size");
static_assert(MK_MAX_R <= 8, "the halo is one 8-pixel group on either side");
static_assert(MK_MAX_D == 585225 && MK_MAX_D < (1 << 20), "D stays below 2^20");
static_assert((long long)MK_MAX_D * (2 * MK_MAX_R + 1) * (2 * MK_MAX_R + 1) < (1ll << 31), "a window sum of D fits 32 bits");
static_assert((long long)MK_MAX_RATE * MK_MAX_STATE + 32768 == 2139127808ll && (long long)MK_MAX_RATE * MK_MAX_STATE + 32768 < (1ll << 31),
              "|a e| + 32768 fits 32 bits");
static_assert(2 * MK_MAX_RATE <= 65536, "a / 65536 <= 1 / 2: the state moves no further than half way, so it stays in 0 .. 65280");

static_assert(MKG_LDS_BYTES == 6144, "DESIGN.md section 8.z19, l2d.h and tests/test_matte_key_gain_resources.py state this size");
static_assert((MKG_BINS - 1) * 255 + 64 < (1 << 17), "g k + 64 stays below 2^17");
static_assert(3ll * ((1ll << 31) / 3) < (1ll << 31) && 2ll * ((1ll << 31) / 3) < (1ll << 32),
              "a count is at most H W < 2^31 / 3: the sum over a channel and 2 cum fit 32 bits");
static_assert(128 * 251 + (239 >> 1) < (1 << 15), "128 b + (k >> 1) of a valid sample is exact in fp32, and so is the correction step");
static_assert(MKG_BLOCK % (8 * MKG_THREADS) == 0, "a block is whole steps of 8 pixels per lane");

// where the key's bytes come from
enum { MK_KEY_COLOR = 0, MK_KEY_PLATE = 1, MK_KEY_STATE = 2 };

struct mk_params {
    sd_params th;                             // lo2, inv of the key's ramp; flags: SD_HARD; r
    int L, kr, kg, kb;                        // the luma weight; the key colour (not read with PLATE)
    int flags;                                // MK_INVERT | MK_AND | MK_OR
    float rlo, rinv;                          // the depth ramp (read only with AND / OR)
    int rflags;                               // L2D_MATTE_HARD | L2D_MATTE_FAR of the depth ramp
};

struct mk_adapt {                             // L2D_OP_MATTE_KEY_ADAPT beside mk_params
    const uint16_t *state;                    // the record read (null under INIT)
    uint16_t *next;                           // the record written
    int a_bg, a_fg;                           // rint(65536 rate), rint(65536 absorb)
};

// the plate byte of a state word
__device__ __forceinline__ int mk_state_byte(unsigned s) { return (int)((s + 128u) >> 8); }

// one channel of 8 pixels: the state moves towards the source's bytes by a[e] / 65536 of the way, packed lowest pixel first
__device__ __forceinline__ uint4 mk_adapt8(h16x8 c, const unsigned (&s)[8], const int (&a)[8]) {
    unsigned n[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int d = 256 * (int)px_byte(c[e]) - (int)s[e];
        n[e] = (unsigned)((int)s[e] + ((a[e] * d + 32768) >> 16));
    }
    return make_uint4(n[0] | (n[1] << 16), n[2] | (n[3] << 16), n[4] | (n[5] << 16), n[6] | (n[7] << 16));
}

// 8 state words as one 16-byte load, lowest pixel first
__device__ __forceinline__ void mk_state8(const uint16_t *__restrict__ p, unsigned (&s)[8]) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    s[0] = v.x & 65535u; s[1] = v.x >> 16; s[2] = v.y & 65535u; s[3] = v.y >> 16;
    s[4] = v.z & 65535u; s[5] = v.z >> 16; s[6] = v.w & 65535u; s[7] = v.w >> 16;
}

// the plate's byte under a gain: k' = min(255, (g k + 64) >> 7); g = 128: k
__device__ __forceinline__ int mk_gain_byte(int g, int k) { return min(255, (g * k + 64) >> 7); }

// D of one pixel: its bytes against the key's
__device__ __forceinline__ unsigned mk_D(unsigned r, unsigned g, unsigned b, int kr, int kg, int kb, int L) {
    const int dR = (int)r - kr, dG = (int)g - kg, dB = (int)b - kb;
    // 77 + 150 + 29 = 256: the luma of the differences raised by 255 is dy + 255, and every argument is non-negative
    const int dy = (int)px_luma((unsigned)(dR + 255), (unsigned)(dG + 255), (unsigned)(dB + 255)) - 255;
    const int cb = dB - dy, cr = dR - dy;
    return (unsigned)(cb * cb + cr * cr + ((L * dy * dy + 128) >> 8));
}

// D of the 8-pixel group at row yy (clamped by the caller), column gx (a multiple of 8, inside the image or one group beside it):
// a group beside the image holds the edge pixel's value, which is what a clamped coordinate reads
template <int KEY, bool GAIN>
__device__ __forceinline__ void mk_group(const h16 *__restrict__ source, const uint8_t *__restrict__ plate,
                                         const uint16_t *__restrict__ state, int W, long long HW, int yy, int gx, const mk_params &p,
                                         const int (&gn)[3], unsigned (&D)[8]) {
    constexpr bool PLATE = KEY == MK_KEY_PLATE;
    if (gx < 0 || gx >= W) {
        const long long e0 = (long long)yy * W + (gx < 0 ? 0 : W - 1);
        int kr = p.kr, kg = p.kg, kb = p.kb;
        if constexpr (PLATE) {
            kr = plate[e0];
            kg = plate[HW + e0];
            kb = plate[2 * HW + e0];
        }
        if constexpr (KEY == MK_KEY_STATE) {
            kr = mk_state_byte(state[e0]);
            kg = mk_state_byte(state[HW + e0]);
            kb = mk_state_byte(state[2 * HW + e0]);
        }
        if constexpr (GAIN) {
            kr = mk_gain_byte(gn[0], kr);
            kg = mk_gain_byte(gn[1], kg);
            kb = mk_gain_byte(gn[2], kb);
        }
        const unsigned d = mk_D(px_byte(source[e0]), px_byte(source[HW + e0]), px_byte(source[2 * HW + e0]), kr, kg, kb, p.L);
#pragma unroll
        for (int e = 0; e < 8; ++e) D[e] = d;
    } else {
        const long long g0 = (long long)yy * W + gx;
        const h16x8 R = l2d_ld8(source + g0), G = l2d_ld8(source + HW + g0), B = l2d_ld8(source + 2 * HW + g0);
        uint2 k[3] = {make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u)};
        if constexpr (PLATE) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) k[ch] = *reinterpret_cast<const uint2 *>(plate + ch * HW + g0);
        }
        unsigned sr[8] = {}, sg[8] = {}, sb[8] = {};
        if constexpr (KEY == MK_KEY_STATE) {
            mk_state8(state + g0, sr);
            mk_state8(state + HW + g0, sg);
            mk_state8(state + 2 * HW + g0, sb);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int kr = p.kr, kg = p.kg, kb = p.kb;
            if constexpr (PLATE) {
                const int sh = 8 * (e & 3);
                kr = (int)(((e < 4 ? k[0].x : k[0].y) >> sh) & 255u);
                kg = (int)(((e < 4 ? k[1].x : k[1].y) >> sh) & 255u);
                kb = (int)(((e < 4 ? k[2].x : k[2].y) >> sh) & 255u);
            }
            if constexpr (KEY == MK_KEY_STATE) {
                kr = mk_state_byte(sr[e]);
                kg = mk_state_byte(sg[e]);
                kb = mk_state_byte(sb[e]);
            }
            if constexpr (GAIN) {
                kr = mk_gain_byte(gn[0], kr);
                kg = mk_gain_byte(gn[1], kg);
                kb = mk_gain_byte(gn[2], kb);
            }
            D[e] = mk_D(px_byte(R[e]), px_byte(G[e]), px_byte(B[e]), kr, kg, kb, p.L);
        }
    }
}

// grid (tiles x, tiles y), SD_THREADS lanes.  Every index into the frame is formed of a row clamped to [0, H - 1] and a column
// group inside [0, W - 8] (or the edge pixel): nothing outside the source, the plate (or the state record) and the depth plane is
// read.  ADAPT: the lane's 8 pixels of the next record are written behind the plane's; KEY says what the record is made of
// (MK_KEY_PLATE: INIT).  GAIN: the key's bytes are multiplied by the record's three gains first (ordinary loads; the launcher's
// L2D_OP_MATTE_KEY_GAIN in front of this launch wrote them).
template <int KEY, bool ADAPT = false, bool GAIN = false>
__device__ __forceinline__ void mk_body(const h16 *__restrict__ source, float *__restrict__ out, const h16 *__restrict__ depth,
                                        const uint8_t *__restrict__ plate, int H, int W, const mk_params &p,
                                        const mk_adapt &ad = mk_adapt{nullptr, nullptr, 0, 0}, const int *__restrict__ gain = nullptr) {
    __shared__ __attribute__((aligned(16))) unsigned dd[MK_DH][SD_DW];            // D of the tile and its halo
    __shared__ __attribute__((aligned(16))) unsigned hh[MK_DH][SD_TW];            // the row sums
    static_assert(sizeof(dd) + sizeof(hh) == MK_LDS_BYTES, "the LDS size the file states");
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SD_TW, y0 = blockIdx.y * SD_TH;
    const int r = p.th.r, taps = 2 * r + 1, rows = SD_TH + 2 * r;
    const long long HW = (long long)H * W;
    int gn[3] = {MKG_UNITY, MKG_UNITY, MKG_UNITY};
    if constexpr (GAIN) {
        static_assert(KEY != MK_KEY_COLOR, "a gain corrects a plate");
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) gn[ch] = px_clampi(gain[ch], 0, MKG_BINS - 1);
    }

    for (int g = tid; g < rows * (SD_DW / 8); g += SD_THREADS) {
        const int j = g / (SD_DW / 8), cg = g % (SD_DW / 8);
        if (r == 0 && (cg == 0 || cg == SD_DW / 8 - 1)) continue;                 // no tap reaches the side halo
        const int yy = px_clampi(y0 - r + j, 0, H - 1);
        unsigned D[8];
        mk_group<KEY, GAIN>(source, plate, ad.state, W, HW, yy, x0 - 8 + cg * 8, p, gn, D);
        uint4 *d4 = reinterpret_cast<uint4 *>(&dd[j][cg * 8]);
        d4[0] = make_uint4(D[0], D[1], D[2], D[3]);
        d4[1] = make_uint4(D[4], D[5], D[6], D[7]);
    }
    __syncthreads();

    // rows: hh[j][c] = dd[j][8 + c - r] + ... + dd[j][8 + c + r]
    for (int i = tid; i < rows * SD_TW; i += SD_THREADS) {
        const int j = i / SD_TW, cc = i % SD_TW;
        const unsigned *s = &dd[j][8 + cc - r];
        unsigned acc = 0u;
        for (int k = 0; k < taps; ++k) acc += s[k];
        hh[j][cc] = acc;
    }
    __syncthreads();

    const int by = tid >> 3, bx = (tid & 7) * 8;
    const int y = y0 + by, x = x0 + bx;
    if (y >= H || x >= W) return;                // (x + 8 <= W otherwise: W % 8 == 0)
    // columns: S[e] = hh[by][bx + e] + ... + hh[by + 2 r][bx + e]
    unsigned S[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (int k = 0; k < taps; ++k) {
        const uint4 a = *reinterpret_cast<const uint4 *>(&hh[by + k][bx]);
        const uint4 b = *reinterpret_cast<const uint4 *>(&hh[by + k][bx + 4]);
        S[0] += a.x; S[1] += a.y; S[2] += a.z; S[3] += a.w;
        S[4] += b.x; S[5] += b.y; S[6] += b.z; S[7] += b.w;
    }
    const float n = (float)(taps * taps);
    const long long px = (long long)y * W + x;
    float m[8];
    int a[8];                                    // (ADAPT only) the rate of each pixel
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float P = rintf(__fmul_rn(255.0f, sd_weight(__fdiv_rn((float)S[e], n), p.th)));
        if constexpr (ADAPT) {
            const int P0 = (int)P;
            a[e] = (ad.a_bg * (255 - P0) + ad.a_fg * P0 + 127) / 255;
        }
        if (p.flags & MK_INVERT) P = __fsub_rn(255.0f, P);
        m[e] = __fdiv_rn(P, 255.0f);
    }
    if (p.flags & (MK_AND | MK_OR)) {
        const h16x8 dv = l2d_ld8(depth + px);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float mr = px_ramp(dv[e], p.rlo, p.rinv, p.rflags);
            m[e] = (p.flags & MK_AND) ? fminf(mr, m[e]) : fmaxf(mr, m[e]);
        }
    }
    f32x4 *op = reinterpret_cast<f32x4 *>(out + px);
    op[0] = f32x4{m[0], m[1], m[2], m[3]};
    op[1] = f32x4{m[4], m[5], m[6], m[7]};
    if constexpr (ADAPT) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            unsigned sv[8];
            if constexpr (KEY == MK_KEY_STATE) {
                mk_state8(ad.state + ch * HW + px, sv);
            } else {
                const uint2 k = *reinterpret_cast<const uint2 *>(plate + ch * HW + px);
#pragma unroll
                for (int e = 0; e < 8; ++e) sv[e] = (((e < 4 ? k.x : k.y) >> (8 * (e & 3))) & 255u) << 8;
            }
            *reinterpret_cast<uint4 *>(ad.next + ch * HW + px) = mk_adapt8(l2d_ld8(source + ch * HW + px), sv, a);
        }
    }
}

__global__ __launch_bounds__(SD_THREADS) void matte_key_color_kernel(const h16 *__restrict__ source, float *__restrict__ out,
                                                                     const h16 *__restrict__ depth, int H, int W, mk_params p) {
    mk_body<MK_KEY_COLOR>(source, out, depth, nullptr, H, W, p);
}

__global__ __launch_bounds__(SD_THREADS) void matte_key_plate_kernel(const h16 *__restrict__ source, float *__restrict__ out,
                                                                     const h16 *__restrict__ depth, const uint8_t *__restrict__ plate,
                                                                     int H, int W, mk_params p) {
    mk_body<MK_KEY_PLATE>(source, out, depth, plate, H, W, p);
}

__global__ __launch_bounds__(SD_THREADS) void matte_key_adapt_init_kernel(const h16 *__restrict__ source, float *__restrict__ out,
                                                                          const h16 *__restrict__ depth,
                                                                          const uint8_t *__restrict__ plate, int H, int W, mk_params p,
                                                                          mk_adapt ad) {
    mk_body<MK_KEY_PLATE, true>(source, out, depth, plate, H, W, p, ad);
}

__global__ __launch_bounds__(SD_THREADS) void matte_key_adapt_state_kernel(const h16 *__restrict__ source, float *__restrict__ out,
                                                                           const h16 *__restrict__ depth, int H, int W, mk_params p,
                                                                           mk_adapt ad) {
    mk_body<MK_KEY_STATE, true>(source, out, depth, nullptr, H, W, p, ad);
}

// the three gained forms: the same bodies with the record's pointer
__global__ __launch_bounds__(SD_THREADS) void matte_gain_key_plate_kernel(const h16 *__restrict__ source, float *__restrict__ out,
                                                                          const h16 *__restrict__ depth,
                                                                          const uint8_t *__restrict__ plate, int H, int W, mk_params p,
                                                                          const int *__restrict__ gain) {
    mk_body<MK_KEY_PLATE, false, true>(source, out, depth, plate, H, W, p, mk_adapt{nullptr, nullptr, 0, 0}, gain);
}

__global__ __launch_bounds__(SD_THREADS) void matte_gain_key_init_kernel(const h16 *__restrict__ source, float *__restrict__ out,
                                                                         const h16 *__restrict__ depth,
                                                                         const uint8_t *__restrict__ plate, int H, int W, mk_params p,
                                                                         mk_adapt ad, const int *__restrict__ gain) {
    mk_body<MK_KEY_PLATE, true, true>(source, out, depth, plate, H, W, p, ad, gain);
}

__global__ __launch_bounds__(SD_THREADS) void matte_gain_key_state_kernel(const h16 *__restrict__ source, float *__restrict__ out,
                                                                          const h16 *__restrict__ depth, int H, int W, mk_params p,
                                                                          mk_adapt ad, const int *__restrict__ gain) {
    mk_body<MK_KEY_STATE, true, true>(source, out, depth, nullptr, H, W, p, ad, gain);
}

// one channel of 8 pixels into the block's histogram: bytes b against plate bytes k.  The quotient is a reciprocal's, corrected to
// the floor: num < 2^15 and k < 2^8 are exact in fp32 and the product is off by less than one, so one step either way suffices.
// Equal neighbours (a flat wall) go in as one atomic.
__device__ __forceinline__ void mkg_count8(unsigned *__restrict__ hist, h16x8 v, const unsigned (&k)[8]) {
    unsigned run = MKG_BINS, cnt = 0u;           // (MKG_BINS: no run yet)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const unsigned b = px_byte(v[e]), kk = k[e];
        if (kk < 16u || kk > 239u || b < 4u || b > 251u) continue;
        const unsigned num = 128u * b + (kk >> 1);
        unsigned q = (unsigned)__fmul_rn((float)num, __frcp_rn((float)kk));
        const int rem = (int)num - (int)(q * kk);
        if (rem < 0) --q;
        else if (rem >= (int)kk) ++q;
        q = min(q, (unsigned)(MKG_BINS - 1));
        if (q == run) {
            ++cnt;
        } else {
            if (cnt) atomicAdd(&hist[run], cnt);
            run = q;
            cnt = 1u;
        }
    }
    if (cnt) atomicAdd(&hist[run], cnt);
}

// grid nblk, MKG_THREADS lanes: block i counts the pixels [i MKG_BLOCK, min(HW, (i + 1) MKG_BLOCK)), 8 per lane (HW % 8 == 0: a group
// lies inside the frame or outside it), and writes all 3 x 512 counts of its partial
template <bool STATE>
__device__ __forceinline__ void mkg_hist_body(const h16 *__restrict__ source, const void *__restrict__ key, unsigned *__restrict__ partials,
                                              long long HW) {
    __shared__ unsigned hist[3][MKG_BINS];
    static_assert(sizeof(hist) == MKG_LDS_BYTES, "the LDS size the file states");
    const int tid = threadIdx.x;
    for (int j = tid; j < 3 * MKG_BINS; j += MKG_THREADS) (&hist[0][0])[j] = 0u;
    __syncthreads();
    const long long first = (long long)blockIdx.x * MKG_BLOCK;
    for (int g = tid * 8; g < MKG_BLOCK; g += 8 * MKG_THREADS) {
        const long long px = first + g;
        if (px >= HW) break;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            unsigned k[8];
            if constexpr (STATE) {
                unsigned sv[8];
                mk_state8((const uint16_t *)key + ch * HW + px, sv);
#pragma unroll
                for (int e = 0; e < 8; ++e) k[e] = (unsigned)mk_state_byte(sv[e]);
            } else {
                const uint2 kv = *reinterpret_cast<const uint2 *>((const uint8_t *)key + ch * HW + px);
#pragma unroll
                for (int e = 0; e < 8; ++e) k[e] = ((e < 4 ? kv.x : kv.y) >> (8 * (e & 3))) & 255u;
            }
            mkg_count8(hist[ch], l2d_ld8(source + ch * HW + px), k);
        }
    }
    __syncthreads();
    unsigned *out = partials + (long long)blockIdx.x * 3 * MKG_BINS;
    for (int j = tid; j < 3 * MKG_BINS; j += MKG_THREADS) out[j] = (&hist[0][0])[j];
}

__global__ __launch_bounds__(MKG_THREADS) void matte_gain_hist_plate_kernel(const h16 *__restrict__ source, const uint8_t *__restrict__ plate,
                                                                            unsigned *__restrict__ partials, long long HW) {
    mkg_hist_body<false>(source, plate, partials, HW);
}

__global__ __launch_bounds__(MKG_THREADS) void matte_gain_hist_state_kernel(const h16 *__restrict__ source, const uint16_t *__restrict__ state,
                                                                            unsigned *__restrict__ partials, long long HW) {
    mkg_hist_body<true>(source, state, partials, HW);
}

// one work-group of 2 x MKG_BINS lanes: lanes j and MKG_BINS + j sum bin j of the three channels over the even and the odd partials
// (the loads of 8 partials are in flight at once), the upper half hands its sums over through LDS, and the lower half owns the bins
__global__ __launch_bounds__(MKG_MEDIAN_THREADS) void matte_gain_median_kernel(const unsigned *__restrict__ partials, int *__restrict__ record,
                                                                               int nblk, int lim, int min_count) {
    __shared__ unsigned cum[3][MKG_BINS];
    static_assert(sizeof(cum) == MKG_LDS_BYTES, "the LDS size the file states");
    const int j = threadIdx.x & (MKG_BINS - 1);
    const bool upper = threadIdx.x >= MKG_BINS;
    unsigned h[3] = {0u, 0u, 0u};
#pragma unroll 8
    for (int b = upper ? 1 : 0; b < nblk; b += 2) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) h[ch] += partials[((long long)b * 3 + ch) * MKG_BINS + j];
    }
    if (upper) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) cum[ch][j] = h[ch];
    }
    __syncthreads();
    if (!upper) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) cum[ch][j] += h[ch];
    }
    __syncthreads();
    // an inclusive scan, in place: every owner reads, all wait, every owner writes
    for (int d = 1; d < MKG_BINS; d <<= 1) {
        unsigned a[3] = {0u, 0u, 0u};
        if (!upper && j >= d) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) a[ch] = cum[ch][j - d];
        }
        __syncthreads();
        if (!upper) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) cum[ch][j] += a[ch];
        }
        __syncthreads();
    }
    if (upper) return;
    const int lo = (MKG_UNITY * MKG_UNITY + lim - 1) / lim;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned n = cum[ch][MKG_BINS - 1], c = cum[ch][j], below = j ? cum[ch][j - 1] : 0u;
        const bool few = n < (unsigned)min_count;
        // the smallest q with 2 cum(q) >= n: exactly one lane (bin 0's takes n = 0)
        const bool mine = few ? j == 0 : (2u * c >= n && (j == 0 || 2u * below < n));
        if (mine) record[ch] = few ? MKG_UNITY : px_clampi(j, lo, lim);
        if (j == 0) record[3 + ch] = (int)n;
    }
    if (j == 0) record[6] = record[7] = 0;
}

// one lane per 8 consecutive elements of the [3][H][W] frame: n8 = 3 H W / 8 groups
__global__ __launch_bounds__(256) void frame_planar_bytes_kernel(const h16 *__restrict__ source, uint8_t *__restrict__ out, int n8) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n8) return;
    const h16x8 v = l2d_ld8(source + 8ll * g);
    unsigned b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = px_byte(v[e]);
    *reinterpret_cast<uint2 *>(out + 8ll * g) = px_pack8(b);
}

// what L2D_OP_MATTE_KEY and L2D_OP_MATTE_KEY_ADAPT refuse alike (`plate`: p3 is read; `colour`: i5 i6 i7 are): the frame's H W, or
// -1 with the error set.  `known` are the flag bits of the op.
static long long mk_check(const char *name, const l2d_op *op, int known, bool plate, bool colour) {
    // (the gain's own checks are mk_check_gain's, behind these)
    const int H = op->i[0], W = op->i[1], r = op->i[2], flags = op->i[3], L = op->i[4];
    if (flags & ~known) {
        l2d_set_error("%s(tag %d): unknown flag bits 0x%x (1 plate, 2 hard, 4 invert, 8 and, 16 or, 64 hard ramp, 128 far)", name, op->tag,
                      flags);
        return -1;
    }
    if ((flags & MK_AND) && (flags & MK_OR)) {
        l2d_set_error("%s(tag %d): flags 0x%x name two ways to combine", name, op->tag, flags);
        return -1;
    }
    const bool ramp = (flags & (MK_AND | MK_OR)) != 0;
    if (!ramp && (flags & (MK_RAMP_HARD | MK_RAMP_FAR))) {
        l2d_set_error("%s(tag %d): ramp flags without L2D_MATTE_KEY_AND / _OR (a replacing key reads no depth)", name, op->tag);
        return -1;
    }
    if (!px_check_pointers16(name, op, 2)) return -1;
    if (ramp && (!op->p[2] || (((uintptr_t)op->p[2]) & 15))) {
        l2d_set_error("%s(tag %d): pointer 2 (the depth plane of AND / OR) is null or not 16-byte aligned", name, op->tag);
        return -1;
    }
    if (plate && (!op->p[3] || (((uintptr_t)op->p[3]) & 7))) {
        l2d_set_error("%s(tag %d): pointer 3 (the plate) is null or not 8-byte aligned", name, op->tag);
        return -1;
    }
    const long long HW = px_check_frame(name, op->tag, H, W);
    if (HW < 0) return -1;
    if (r < 0 || r > MK_MAX_R) {
        l2d_set_error("%s(tag %d): radius %d, need 0..%d", name, op->tag, r, MK_MAX_R);
        return -1;
    }
    if (L < 0 || L > MK_MAX_L) {
        l2d_set_error("%s(tag %d): luma weight L = %d, need 0..%d", name, op->tag, L, MK_MAX_L);
        return -1;
    }
    if (colour) {
        for (int k = 5; k < 8; ++k) {
            if (op->i[k] < 0 || op->i[k] > 255) {
                l2d_set_error("%s(tag %d): key colour (%d, %d, %d): need bytes", name, op->tag, op->i[5], op->i[6], op->i[7]);
                return -1;
            }
        }
    }
    const float lo2 = op->f[0], inv = op->f[1], rlo = op->f[2], rinv = op->f[3];
    if (!(lo2 >= 0.0f && lo2 <= 3.0e38f) || !(inv >= 0.0f && inv <= 3.0e38f) || ((flags & MK_HARD) != 0) != (inv == 0.0f)) {
        l2d_set_error("%s(tag %d): lo2 = %g and inv = %g must be finite and not negative, inv 0 exactly when the hard flag is set", name,
                      op->tag, lo2, inv);
        return -1;
    }
    if (ramp && !px_check_ramp(name, op->tag, rlo, rinv, (flags & MK_RAMP_HARD) != 0)) return -1;
    if (px_overlap(op->p[1], 4 * HW, op->p[0], 6 * HW) || (ramp && px_overlap(op->p[1], 4 * HW, op->p[2], 2 * HW))
        || (plate && px_overlap(op->p[1], 4 * HW, op->p[3], 3 * HW))) {
        l2d_set_error("%s(tag %d): the plane overlaps the source, the depth plane or the plate", name, op->tag);
        return -1;
    }
    return HW;
}

// the kernels' parameters of a checked record
static mk_params mk_params_of(const l2d_op *op) {
    const int flags = op->i[3];
    mk_params p;
    p.th.lo = op->f[0]; p.th.inv = op->f[1]; p.th.s = 0.0f; p.th.flags = (flags & MK_HARD) ? SD_HARD : 0; p.th.r = op->i[2];
    p.L = op->i[4]; p.kr = op->i[5]; p.kg = op->i[6]; p.kb = op->i[7];
    p.flags = flags & (MK_INVERT | MK_AND | MK_OR);
    p.rlo = op->f[2]; p.rinv = op->f[3];
    p.rflags = ((flags & MK_RAMP_HARD) ? L2D_MATTE_HARD : 0) | ((flags & MK_RAMP_FAR) ? L2D_MATTE_FAR : 0);
    return p;
}

// L2D_MATTE_KEY_GAIN on a checked record: the gain record p6 against the plane (and `also`, op 61's state written)
static bool mk_check_gain(const char *name, const l2d_op *op, long long HW, const void *also, long long also_bytes) {
    if (!op->p[6]) {                             // (a record from before the gain: the bit meant nothing then)
        l2d_set_error("%s(tag %d): unknown flag bits 0x%x for a record without pointer 6: L2D_MATTE_KEY_GAIN needs the gain record", name,
                      op->tag, MK_GAIN);
        return false;
    }
    if (((uintptr_t)op->p[6]) & 15) {
        l2d_set_error("%s(tag %d): pointer 6 (the gain record of L2D_MATTE_KEY_GAIN) is not 16-byte aligned", name, op->tag);
        return false;
    }
    if (px_overlap(op->p[1], 4 * HW, op->p[6], 32) || px_overlap(also, also_bytes, op->p[6], 32)) {
        l2d_set_error("%s(tag %d): the plane or the state written overlaps the gain record", name, op->tag);
        return false;
    }
    return true;
}

int l2d_launch_matte_key(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1];
    const bool plate = (op->i[3] & MK_PLATE) != 0, gain = (op->i[3] & MK_GAIN) != 0;
    if (gain && !plate) {
        l2d_set_error("matte_key(tag %d): L2D_MATTE_KEY_GAIN with a colour key (a gain corrects a plate)", op->tag);
        return L2D_EINVAL;
    }
    const long long HW = mk_check("matte_key", op, MK_PLATE | MK_HARD | MK_INVERT | MK_AND | MK_OR | MK_RAMP_HARD | MK_RAMP_FAR | MK_GAIN,
                                  plate, !plate);
    if (HW < 0) return L2D_EINVAL;
    if (gain && !mk_check_gain("matte_key", op, HW, nullptr, 0)) return L2D_EINVAL;
    L2D_DRY_RETURN();
    const mk_params p = mk_params_of(op);
    const dim3 tiles((W + SD_TW - 1) / SD_TW, (H + SD_TH - 1) / SD_TH), threads(SD_THREADS);
    if (gain)
        hipLaunchKernelGGL(matte_gain_key_plate_kernel, tiles, threads, 0, s, (const h16 *)op->p[0], (float *)op->p[1],
                           (const h16 *)op->p[2], (const uint8_t *)op->p[3], H, W, p, (const int *)op->p[6]);
    else if (plate)
        hipLaunchKernelGGL(matte_key_plate_kernel, tiles, threads, 0, s, (const h16 *)op->p[0], (float *)op->p[1], (const h16 *)op->p[2],
                           (const uint8_t *)op->p[3], H, W, p);
    else
        hipLaunchKernelGGL(matte_key_color_kernel, tiles, threads, 0, s, (const h16 *)op->p[0], (float *)op->p[1], (const h16 *)op->p[2], H,
                           W, p);
    return l2d_check_launch("matte_key", op->tag);
}

int l2d_launch_matte_key_adapt(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], flags = op->i[3], a_bg = op->i[5], a_fg = op->i[6];
    const bool init = (flags & MK_ADAPT_INIT) != 0, gain = (flags & MK_GAIN) != 0;
    const long long HW = mk_check("matte_key_adapt", op,
                                  MK_PLATE | MK_HARD | MK_INVERT | MK_AND | MK_OR | MK_RAMP_HARD | MK_RAMP_FAR | MK_ADAPT_INIT | MK_GAIN, init, false);
    if (HW < 0) return L2D_EINVAL;
    if (a_bg < 0 || a_bg > MK_MAX_RATE || a_fg < 0 || a_fg > MK_MAX_RATE) {
        l2d_set_error("matte_key_adapt(tag %d): rates a_bg = %d, a_fg = %d, need 0..%d (65536 times a rate of at most 1 / 2)", op->tag, a_bg,
                      a_fg, MK_MAX_RATE);
        return L2D_EINVAL;
    }
    if (!op->p[5] || (((uintptr_t)op->p[5]) & 15) || (!init && (!op->p[4] || (((uintptr_t)op->p[4]) & 15)))) {
        l2d_set_error("matte_key_adapt(tag %d): pointer 5 (the state written) or, without INIT, pointer 4 (the state read) is null or not "
                      "16-byte aligned", op->tag);
        return L2D_EINVAL;
    }
    const bool ramp = (flags & (MK_AND | MK_OR)) != 0;
    if ((!init && px_overlap(op->p[5], 6 * HW, op->p[4], 6 * HW)) || px_overlap(op->p[5], 6 * HW, op->p[0], 6 * HW)
        || px_overlap(op->p[5], 6 * HW, op->p[1], 4 * HW) || (ramp && px_overlap(op->p[5], 6 * HW, op->p[2], 2 * HW))
        || (init && px_overlap(op->p[5], 6 * HW, op->p[3], 3 * HW))) {
        l2d_set_error("matte_key_adapt(tag %d): the state written overlaps the state read, the source, the plane, the depth plane or the "
                      "plate", op->tag);
        return L2D_EINVAL;
    }
    // (the plane against the state read, which takes the plate's place)
    if (!init && px_overlap(op->p[1], 4 * HW, op->p[4], 6 * HW)) {
        l2d_set_error("matte_key_adapt(tag %d): the plane overlaps the state read", op->tag);
        return L2D_EINVAL;
    }
    if (gain && !mk_check_gain("matte_key_adapt", op, HW, op->p[5], 6 * HW)) return L2D_EINVAL;
    L2D_DRY_RETURN();
    const mk_params p = mk_params_of(op);
    const mk_adapt ad = {init ? nullptr : (const uint16_t *)op->p[4], (uint16_t *)op->p[5], a_bg, a_fg};
    const dim3 tiles((W + SD_TW - 1) / SD_TW, (H + SD_TH - 1) / SD_TH), threads(SD_THREADS);
    if (gain && init)
        hipLaunchKernelGGL(matte_gain_key_init_kernel, tiles, threads, 0, s, (const h16 *)op->p[0], (float *)op->p[1],
                           (const h16 *)op->p[2], (const uint8_t *)op->p[3], H, W, p, ad, (const int *)op->p[6]);
    else if (gain)
        hipLaunchKernelGGL(matte_gain_key_state_kernel, tiles, threads, 0, s, (const h16 *)op->p[0], (float *)op->p[1],
                           (const h16 *)op->p[2], H, W, p, ad, (const int *)op->p[6]);
    else if (init)
        hipLaunchKernelGGL(matte_key_adapt_init_kernel, tiles, threads, 0, s, (const h16 *)op->p[0], (float *)op->p[1],
                           (const h16 *)op->p[2], (const uint8_t *)op->p[3], H, W, p, ad);
    else
        hipLaunchKernelGGL(matte_key_adapt_state_kernel, tiles, threads, 0, s, (const h16 *)op->p[0], (float *)op->p[1],
                           (const h16 *)op->p[2], H, W, p, ad);
    return l2d_check_launch("matte_key_adapt", op->tag);
}

// the geometry ops 62 and 63 share: H W, or -1 with the error set (`nblk` must be the blocks of H W)
static long long mkg_check_frame(const char *name, const l2d_op *op, int nblk) {
    const long long HW = px_check_frame(name, op->tag, op->i[0], op->i[1]);
    if (HW < 0) return -1;
    if (nblk != (int)((HW + MKG_BLOCK - 1) / MKG_BLOCK)) {
        l2d_set_error("%s(tag %d): nblk = %d, but %d x %d is %lld blocks of %d pixels", name, op->tag, nblk, op->i[0], op->i[1],
                      (HW + MKG_BLOCK - 1) / MKG_BLOCK, MKG_BLOCK);
        return -1;
    }
    return HW;
}

int l2d_launch_matte_key_gain_hist(const l2d_op *op, hipStream_t s) {
    const int flags = op->i[2], nblk = op->i[3];
    const bool state = (flags & MKG_STATE) != 0;
    if (flags & ~MKG_STATE) {
        l2d_set_error("matte_key_gain_hist(tag %d): unknown flag bits 0x%x (1 state)", op->tag, flags);
        return L2D_EINVAL;
    }
    if (!op->p[0] || !op->p[1] || !op->p[2] || (((uintptr_t)op->p[0]) & 15) || (((uintptr_t)op->p[2]) & 15)
        || (((uintptr_t)op->p[1]) & (state ? 15 : 7))) {
        l2d_set_error("matte_key_gain_hist(tag %d): a pointer is null or misaligned (the source, the state and the partials 16 bytes, the "
                      "plate 8)", op->tag);
        return L2D_EINVAL;
    }
    const long long HW = mkg_check_frame("matte_key_gain_hist", op, nblk);
    if (HW < 0) return L2D_EINVAL;
    const long long pbytes = (long long)nblk * MKG_LDS_BYTES;
    if (px_overlap(op->p[2], pbytes, op->p[0], 6 * HW) || px_overlap(op->p[2], pbytes, op->p[1], (state ? 6 : 3) * HW)) {
        l2d_set_error("matte_key_gain_hist(tag %d): the partials overlap the source or the plate", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    if (state)
        hipLaunchKernelGGL(matte_gain_hist_state_kernel, dim3((unsigned)nblk), dim3(MKG_THREADS), 0, s, (const h16 *)op->p[0],
                           (const uint16_t *)op->p[1], (unsigned *)op->p[2], HW);
    else
        hipLaunchKernelGGL(matte_gain_hist_plate_kernel, dim3((unsigned)nblk), dim3(MKG_THREADS), 0, s, (const h16 *)op->p[0],
                           (const uint8_t *)op->p[1], (unsigned *)op->p[2], HW);
    return l2d_check_launch("matte_key_gain_hist", op->tag);
}

int l2d_launch_matte_key_gain(const l2d_op *op, hipStream_t s) {
    const int nblk = op->i[2], lim = op->i[3], min_count = op->i[4];
    if (!px_check_pointers16("matte_key_gain", op, 2)) return L2D_EINVAL;
    const long long HW = mkg_check_frame("matte_key_gain", op, nblk);
    if (HW < 0) return L2D_EINVAL;
    if (lim < MKG_UNITY || lim > MKG_BINS - 1 || min_count < 0 || min_count > HW) {
        l2d_set_error("matte_key_gain(tag %d): lim = %d (need %d..%d) or min_count = %d (need 0..%lld)", op->tag, lim, MKG_UNITY, MKG_BINS - 1,
                      min_count, HW);
        return L2D_EINVAL;
    }
    if (px_overlap(op->p[1], 32, op->p[0], (long long)nblk * MKG_LDS_BYTES)) {
        l2d_set_error("matte_key_gain(tag %d): the record overlaps the partials", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    hipLaunchKernelGGL(matte_gain_median_kernel, dim3(1), dim3(MKG_MEDIAN_THREADS), 0, s, (const unsigned *)op->p[0], (int *)op->p[1], nblk, lim,
                       min_count);
    return l2d_check_launch("matte_key_gain", op->tag);
}

int l2d_launch_frame_planar_bytes(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1];
    if (!px_check_pointers16("frame_planar_bytes", op, 2)) return L2D_EINVAL;
    const long long HW = px_check_frame("frame_planar_bytes", op->tag, H, W);
    if (HW < 0) return L2D_EINVAL;
    if (px_overlap(op->p[1], 3 * HW, op->p[0], 6 * HW)) {
        l2d_set_error("frame_planar_bytes(tag %d): the bytes overlap the frame", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const int n8 = (int)(3 * HW / 8);
    hipLaunchKernelGGL(frame_planar_bytes_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, (const h16 *)op->p[0],
                       (uint8_t *)op->p[1], n8);
    return l2d_check_launch("frame_planar_bytes", op->tag);
}
