// Edge-aware matte: the depth matte re-fitted locally as a linear function of the frame it cuts -- a
// guided filter (He et al.) with the source frame's luma as the guide -- so that the matte's edges land where the frame's own
// edges are instead of a few pixels beside them.  One launch in front of the composite (L2D_OP_FRAME_MATTE / _UP with
// L2D_MATTE_PLANE), which reads the fp32 plane this one writes.  The reference has no counterpart.
//
//   P = rint(255 m)                                          m: px_ramp of the depth plane (ramp, hard, far)
//   b = rint(255 clamp(fp16(fp16(x / 2) + 0.5), 0, 1))       the egress op's bytes of the source frame
//   Y = (77 R + 150 G + 29 B + 128) >> 8                     the guide, 0..255
//   S_I, S_P, S_II, S_IP                                     sums of Y, P, Y Y, Y P over the (2r+1)^2 window, coordinates clamped
//   cov = n S_IP - S_I S_P,  var = n S_II - S_I S_I          int64, n = (2r+1)^2; both below 2^33
//   a = double(cov) / (double(var) + E)                      E = double(n n) eps eps, from the host
//   A = rint(4096 a)
//   bc = (double(S_P) - a double(S_I)) / double(n)           one multiplication, one subtraction, one division
//   B = rint(4096 bc)
//   Q = window_sum(A) Y + window_sum(B)                      int64; A and B at clamped coordinates
//   out = float(min(max(double(Q) / double(n 4096 255), 0), 1))
//
// Integers are exact in any order; every fp64 step is one correctly rounded operation (the file is built with
// -ffp-contract=off, see the Makefile; the intrinsics are colorlock.hip's), so numpy restates the plane bit for bit
// (live2diff_amd/matte.py `edge_ref`).  One work-group per 16 x 64 tile: Y and P of the tile and a halo of 2r as bytes in LDS,
// the four sums as a horizontal and a vertical pass, A and B on the tile and a halo of r, their sums the same way.
#include <string.h>

#include "frame_px.h"

#define ME_MAX_R L2D_MATTE_EDGE_MAX_R
#define ME_TW 64                              // the tile: L2D_OP_FRAME_MATTE's
#define ME_TH 16
#define ME_THREADS 256
#define ME_PAD (2 * ME_MAX_R)                 // columns of halo kept on either side of the tile: two 8-pixel groups
#define ME_YW (ME_TW + 2 * ME_PAD)            // 96: a row of Y / P
#define ME_YH (ME_TH + 4 * ME_MAX_R)          // 48
#define ME_AW (ME_TW + 2 * ME_MAX_R)          // 80: a row of A / B, and of the first horizontal sums
#define ME_AH (ME_TH + 2 * ME_MAX_R)          // 32
#define ME_TAPS (2 * ME_MAX_R + 1)

// LDS: the bytes, the first pass' row sums (S_I and S_P packed into one word, S_II, S_IP; the second pass' row sums of A and B
// take their place), A and B
#define ME_BYTES_Y (ME_YH * ME_YW)                        // 4608, twice
#define ME_WORDS_H (3 * ME_YH * ME_AW)                    // 11520 words
#define ME_WORDS_AB (2 * ME_AH * ME_AW)                   // 5120 words
#define ME_LDS_BYTES (2 * ME_BYTES_Y + 4 * ME_WORDS_H + 4 * ME_WORDS_AB)
static_assert(ME_PAD % 8 == 0 && ME_PAD >= 2 * ME_MAX_R, "the halo of 2r is whole 8-pixel groups");
static_assert(255 * ME_TAPS < 65536, "a row sum of Y or P fits 16 bits");
static_assert(255ll * 255 * ME_TAPS * ME_TAPS < (1ll << 32), "a window sum of Y Y or Y P fits 32 bits");
static_assert(2 * ME_AH * ME_TW <= ME_WORDS_H, "the row sums of A and B fit where the first pass' row sums were");
// |a| <= 127.5 / (2 eps) <= 63.75: |A| <= 261120; |bc| <= 255 + 63.75 * 255: |B| <= 67629056
static_assert(261120ll * ME_TAPS * ME_TAPS < (1ll << 31), "the window sum of A fits 32 bits");
static_assert(67629056ll * ME_TAPS < (1ll << 31), "a row sum of B fits 32 bits (the window sum does not: 64 bits)");
static_assert(ME_LDS_BYTES == 75776, "the LDS size DESIGN.md section 8.z9 states");
static_assert(2 * ME_LDS_BYTES <= 160 * 1024, "two work-groups per CU");

struct me_params {
    float lo, inv;
    int flags, r;
    double E;
};

__device__ __forceinline__ unsigned me_p(h16 depth, const me_params &p) {
    return (unsigned)rintf(__fmul_rn(px_ramp(depth, p.lo, p.inv, p.flags), 255.0f));
}

// L2D_MATTE_EDGE_PLANE: P of a ready matte value (clamped: whatever the plane holds, P fits its byte)
__device__ __forceinline__ unsigned me_pm(float m) { return (unsigned)rintf(__fmul_rn(fminf(fmaxf(m, 0.0f), 1.0f), 255.0f)); }


// PLANE (L2D_MATTE_EDGE_PLANE): `depth` is the fp32 plane of ready matte values.  A template parameter, not a branch: the
// instance without it is the kernel as it was (a branch that is uniform over the launch cost the flag-clear form 0.4 - 0.65 us
// of 12.1 at 512 x 512).
template <bool PLANE>
__global__ __launch_bounds__(ME_THREADS) void frame_matte_edge_kernel(const h16 *__restrict__ source, const h16 *__restrict__ depth,
                                                                      float *__restrict__ out, int H, int W, me_params p) {
    __shared__ __attribute__((aligned(16))) unsigned char yb[ME_YH][ME_YW];       // Y at (y0 - 2r + j, x0 - ME_PAD + c), clamped
    __shared__ __attribute__((aligned(16))) unsigned char pb[ME_YH][ME_YW];       // P likewise
    __shared__ __attribute__((aligned(16))) unsigned hbuf[ME_WORDS_H];
    __shared__ int Aa[ME_AH][ME_AW];                                               // A at (y0 - r + v, x0 - r + u), clamped
    __shared__ int Bb[ME_AH][ME_AW];
    unsigned (*hSS)[ME_AW] = reinterpret_cast<unsigned (*)[ME_AW]>(hbuf);                                   // S_I | S_P << 16 of a row
    unsigned (*hII)[ME_AW] = reinterpret_cast<unsigned (*)[ME_AW]>(hbuf + ME_YH * ME_AW);
    unsigned (*hIP)[ME_AW] = reinterpret_cast<unsigned (*)[ME_AW]>(hbuf + 2 * ME_YH * ME_AW);
    int (*hA)[ME_TW] = reinterpret_cast<int (*)[ME_TW]>(hbuf);                                              // behind the first pass
    int (*hB)[ME_TW] = reinterpret_cast<int (*)[ME_TW]>(hbuf + ME_AH * ME_TW);

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ME_TW, y0 = blockIdx.y * ME_TH;
    const int r = p.r, taps = 2 * r + 1, n = taps * taps;
    const int rows2 = ME_TH + 4 * r, rows1 = ME_TH + 2 * r, cols1 = ME_TW + 2 * r;
    const long long HW = (long long)H * W;
    constexpr bool from_plane = PLANE;
    const float *__restrict__ mplane = reinterpret_cast<const float *>(depth);

    // Y and P of the tile and its halo of 2r.  An 8-pixel group lies wholly inside or wholly outside the image (W % 8 == 0);
    // one outside holds the edge pixel's values; a group no window reaches is skipped.
    for (int g = tid; g < rows2 * (ME_YW / 8); g += ME_THREADS) {
        const int j = g / (ME_YW / 8), cg = g % (ME_YW / 8);
        if (cg * 8 + 8 <= ME_PAD - 2 * r || cg * 8 >= ME_PAD + ME_TW + 2 * r) continue;
        const int yy = px_clampi(y0 - 2 * r + j, 0, H - 1);
        const int gx = x0 - ME_PAD + cg * 8;
        unsigned yv[8], pv[8];
        if (gx < 0 || gx >= W) {
            const long long e0 = (long long)yy * W + (gx < 0 ? 0 : W - 1);
            const unsigned ye = px_luma(px_byte(source[e0]), px_byte(source[HW + e0]), px_byte(source[2 * HW + e0]));
            const unsigned pe = from_plane ? me_pm(mplane[e0]) : me_p(depth[e0], p);
#pragma unroll
            for (int e = 0; e < 8; ++e) { yv[e] = ye; pv[e] = pe; }
        } else {
            const long long g0 = (long long)yy * W + gx;
            const h16x8 cr = l2d_ld8(source + g0), cgn = l2d_ld8(source + HW + g0), cb = l2d_ld8(source + 2 * HW + g0);
            // (either form issues the matte input's loads beside the frame's, in front of the arithmetic)
            if (from_plane) {
                const f32x4 m0 = *reinterpret_cast<const f32x4 *>(mplane + g0), m1 = *reinterpret_cast<const f32x4 *>(mplane + g0 + 4);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    yv[e] = px_luma(px_byte(cr[e]), px_byte(cgn[e]), px_byte(cb[e]));
                    pv[e] = me_pm(e < 4 ? m0[e & 3] : m1[e & 3]);
                }
            } else {
                const h16x8 d = l2d_ld8(depth + g0);
#pragma unroll
                for (int e = 0; e < 8; ++e) { yv[e] = px_luma(px_byte(cr[e]), px_byte(cgn[e]), px_byte(cb[e])); pv[e] = me_p(d[e], p); }
            }
        }
        *reinterpret_cast<uint2 *>(&yb[j][cg * 8]) = px_pack8(yv);
        *reinterpret_cast<uint2 *>(&pb[j][cg * 8]) = px_pack8(pv);
    }
    __syncthreads();

    // first horizontal pass: row sums at columns u = 0 .. cols1 - 1 (x = x0 - r + u), eight consecutive columns per lane as a
    // sliding window.  The leftmost tap of column u is byte column ME_PAD - 2r + u, the rightmost ME_PAD + u <= 95: the
    // columns at or behind cols1 that a group of eight also forms read inside the row and are never used.
    {
        const int groups = (cols1 + 7) / 8;                       // <= ME_AW / 8
        for (int i = tid; i < rows2 * groups; i += ME_THREADS) {
            const int j = i / groups, u0 = (i % groups) * 8;
            const unsigned char *ys = &yb[j][ME_PAD - 2 * r + u0], *ps = &pb[j][ME_PAD - 2 * r + u0];
            unsigned sI = 0u, sP = 0u, sII = 0u, sIP = 0u;
            for (int k = 0; k < taps; ++k) {
                const unsigned y = ys[k], q = ps[k];
                sI += y; sP += q; sII += y * y; sIP += y * q;
            }
            hSS[j][u0] = sI | (sP << 16); hII[j][u0] = sII; hIP[j][u0] = sIP;
#pragma unroll
            for (int e = 1; e < 8; ++e) {
                const unsigned y1 = ys[taps - 1 + e], q1 = ps[taps - 1 + e], y0b = ys[e - 1], q0b = ps[e - 1];
                sI += y1 - y0b; sP += q1 - q0b; sII += y1 * y1 - y0b * y0b; sIP += y1 * q1 - y0b * q0b;
                hSS[j][u0 + e] = sI | (sP << 16); hII[j][u0 + e] = sII; hIP[j][u0 + e] = sIP;
            }
        }
    }
    __syncthreads();

    // first vertical pass and the coefficients, on the tile and a halo of r.  A position outside the image holds the
    // coefficients of the clamped position (the window sums of A and B clamp their coordinates); that position lies nearer
    // to the tile, so its window is in LDS as well.
    {
        const double dn = (double)n;
        for (int i = tid; i < rows1 * cols1; i += ME_THREADS) {
            const int v = i / cols1, u = i - v * cols1;
            const int xc = px_clampi(x0 - r + u, 0, W - 1), yc = px_clampi(y0 - r + v, 0, H - 1);
            const int uc = px_clampi(xc - (x0 - r), 0, cols1 - 1), j0 = px_clampi(yc - y0 + r, 0, rows1 - 1);       // the window's first row
            unsigned sI = 0u, sP = 0u, sII = 0u, sIP = 0u;
            for (int k = 0; k < taps; ++k) {
                const unsigned w = hSS[j0 + k][uc];
                sI += w & 65535u; sP += w >> 16; sII += hII[j0 + k][uc]; sIP += hIP[j0 + k][uc];
            }
            const long long cov = (long long)n * sIP - (long long)sI * sP;
            const long long var = (long long)n * sII - (long long)sI * sI;
            const double a = __ddiv_rn((double)cov, __dadd_rn((double)var, p.E));
            const double bc = __ddiv_rn(__dsub_rn((double)sP, __dmul_rn(a, (double)sI)), dn);
            Aa[v][u] = (int)rint(__dmul_rn(a, 4096.0));
            Bb[v][u] = (int)rint(__dmul_rn(bc, 4096.0));
        }
    }
    __syncthreads();

    // second horizontal pass: hA[v][c] = Aa[v][c] + ... + Aa[v][c + 2r] (x = x0 + c), hB likewise
    for (int i = tid; i < rows1 * ME_TW; i += ME_THREADS) {
        const int v = i / ME_TW, c = i % ME_TW;
        int sa = 0, sb = 0;
        for (int k = 0; k < taps; ++k) { sa += Aa[v][c + k]; sb += Bb[v][c + k]; }
        hA[v][c] = sa;
        hB[v][c] = sb;
    }
    __syncthreads();

    // second vertical pass and the plane: consecutive lanes consecutive floats of a row
    const double den = (double)((long long)n * 4096 * 255);
    for (int i = tid; i < ME_TH * ME_TW; i += ME_THREADS) {
        const int ty = i / ME_TW, c = i % ME_TW;
        const int y = y0 + ty, x = x0 + c;
        if (y >= H || x >= W) continue;
        int SA = 0;
        long long SB = 0;
        for (int k = 0; k < taps; ++k) { SA += hA[ty + k][c]; SB += hB[ty + k][c]; }
        const long long Q = (long long)SA * (int)yb[ty + 2 * r][ME_PAD + c] + SB;
        double q = __ddiv_rn((double)Q, den);
        q = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
        out[(long long)y * W + x] = (float)q;
    }
}

int l2d_launch_frame_matte_edge(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], r = op->i[2], flags = op->i[3];
    if (!px_check_pointers16("frame_matte_edge", op, 3)) return L2D_EINVAL;
    if (px_check_frame("frame_matte_edge", op->tag, H, W) < 0) return L2D_EINVAL;
    if (r < 1 || r > ME_MAX_R) {
        l2d_set_error("frame_matte_edge(tag %d): radius %d, need 1..%d", op->tag, r, ME_MAX_R);
        return L2D_EINVAL;
    }
    if (flags & ~(L2D_MATTE_HARD | L2D_MATTE_FAR | L2D_MATTE_EDGE_PLANE)) {
        l2d_set_error("frame_matte_edge(tag %d): unknown flag bits 0x%x (1 hard, 2 far, 32 plane)", op->tag, flags);
        return L2D_EINVAL;
    }
    if ((flags & L2D_MATTE_EDGE_PLANE) && (flags & (L2D_MATTE_HARD | L2D_MATTE_FAR))) {
        l2d_set_error("frame_matte_edge(tag %d): ramp flags beside L2D_MATTE_EDGE_PLANE (the plane carries them)", op->tag);
        return L2D_EINVAL;
    }
    me_params p;
    static_assert(sizeof(double) == sizeof(op->l[0]), "E travels as the bits of a double");
    memcpy(&p.E, &op->l[0], sizeof(double));
    const double nn = (double)((2 * r + 1) * (2 * r + 1)) * (double)((2 * r + 1) * (2 * r + 1));
    if (!(p.E >= nn && p.E <= 1.0e300)) {
        l2d_set_error("frame_matte_edge(tag %d): E = %g must be finite and at least n n = %g (eps >= 1: the coefficients fit 32 bits)",
                      op->tag, p.E, nn);
        return L2D_EINVAL;
    }
    const float lo = op->f[0], inv = op->f[1];
    if (!(flags & L2D_MATTE_EDGE_PLANE) && !px_check_ramp("frame_matte_edge", op->tag, lo, inv, (flags & L2D_MATTE_HARD) != 0))
        return L2D_EINVAL;
    if ((flags & L2D_MATTE_EDGE_PLANE) && px_overlap(op->p[2], 4ll * H * W, op->p[1], 4ll * H * W)) {
        l2d_set_error("frame_matte_edge(tag %d): the output overlaps the input plane (a tile's halo reads its neighbours' pixels)", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    p.lo = lo; p.inv = inv; p.flags = flags; p.r = r;
    auto kernel = (flags & L2D_MATTE_EDGE_PLANE) ? frame_matte_edge_kernel<true> : frame_matte_edge_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((W + ME_TW - 1) / ME_TW, (H + ME_TH - 1) / ME_TH), dim3(ME_THREADS), 0, s,
                       (const h16 *)op->p[0], (const h16 *)op->p[1], (float *)op->p[2], H, W, p);
    return l2d_check_launch("frame_matte_edge", op->tag);
}
