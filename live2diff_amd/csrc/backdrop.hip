// Backdrop blur: the delayed source frame blurred with the subject left out, as the kept part of the
// matte composite (L2D_OP_FRAME_MATTE's p1, or through a resize L2D_OP_FRAME_MATTE_UP's p1).  A plain blur drags the subject's
// colours into the room around the silhouette, exactly where the matte shows the room; here every pixel carries a weight that
// falls to 1/256 on the subject, and the blur is an iterated normalised box filter of the weighted frame.  The reference has no
// counterpart.
//
//   P0[c] = rint(255 clamp(fp16(fp16(x / 2) + 0.5), 0, 1))   the egress op's bytes of the source frame
//   M  = rint(255 m)                                         m: px_ramp of the depth plane (ramp, hard, far)
//   W0 = 256 - M                                             1..256: never 0, so nothing divides by 0
//   per pass, n = (2r+1)^2, window sums with clamped coordinates:
//     D = window_sum(W);  N[c] = window_sum(W P[c]);  P[c] <- (2 N[c] + D) / (2 D);  W <- (D + n - 1) / n      (both floor)
//   out[c] = half(float(P[c]) float(2 / 255) - 1)            two fp32 operations and one rounding
//
// Exact integers in any order, so numpy restates the frame bit for bit (live2diff_amd/backdrop.py `blur_ref`, `frame_of`).  One
// work-group per 16 x 64 tile: the three byte planes and W - 1 as a byte, over a halo of passes * r, in LDS; every pass there, on
// a region that shrinks by r, as a horizontal pass (row sums of W as 16 bits, of W P[c] as 32, channel by channel through one
// buffer) and a vertical pass that writes the bytes back in place.  A position outside the image holds the value of the clamped
// position (the next pass' window sums clamp their coordinates); that position lies nearer to the tile, so its window is in
// LDS as well.  LDS banks: in the horizontal pass a lane slides over eight consecutive columns, so consecutive lanes read bytes 8
// apart -- lanes l and l + 16 of a 32-lane group share a bank, 2-way -- and keep their eight sums in registers, which leave as
// 16-byte stores; the vertical pass and the frame's rows read consecutive entries of a row with consecutive lanes, conflict-free
// inside a row.  One column per lane is conflict-free throughout and was slower: see the horizontal pass.
#include "frame_px.h"

#define BD_MAX_R L2D_BACKDROP_MAX_R
#define BD_MAX_PASSES L2D_BACKDROP_MAX_PASSES
#define BD_TW 64                              // the tile: L2D_OP_FRAME_MATTE's
#define BD_TH 16
#define BD_THREADS 1024                       // 4 waves per SIMD: the tap loops are chains of LDS reads, and at 512 x 512 a CU has one tile
#define BD_PAD (BD_MAX_R * BD_MAX_PASSES)     // 24: rows and columns of halo kept on every side of the tile
#define BD_BW (BD_TW + 2 * BD_PAD + 8)        // 120: a row of bytes, and one group that the last eight row sums of a lane may read into
#define BD_BH (BD_TH + 2 * BD_PAD)            // 64
#define BD_HW (BD_TW + 2 * (BD_PAD - BD_MAX_R))   // 96: a row of row sums (the widest region a pass writes, rounded up to 8)
#define BD_TAPS (2 * BD_MAX_R + 1)

#define BD_LDS_BYTES (4 * BD_BH * BD_BW + 2 * BD_BH * BD_HW + 4 * BD_BH * BD_HW)
static_assert(BD_PAD % 8 == 0, "the halo is whole 8-pixel groups");
// the last tap of the last column a lane forms: BD_PAD - h_in + (cols_out + 5) + 2r = BD_TW + BD_PAD + 5 + h_in
static_assert(BD_HW % 8 == 0 && BD_TW + 2 * BD_PAD + 6 <= BD_BW, "the columns a group of eight row sums reads lie inside the byte row");
static_assert(256 * BD_TAPS < 65536, "a row sum of W fits 16 bits");
static_assert(2ll * 256 * 255 * BD_TAPS * BD_TAPS + 256ll * BD_TAPS * BD_TAPS < (1ll << 32), "2 N + D fits 32 bits");
static_assert(BD_LDS_BYTES == 67584, "the LDS size DESIGN.md section 8.z13 states");
static_assert(2 * BD_LDS_BYTES <= 160 * 1024 && BD_LDS_BYTES <= 80 * 1024, "two work-groups per CU");

struct bd_params {
    float lo, inv;
    int flags, r, passes;
};

// W0 - 1 = 255 - rint(255 m)
__device__ __forceinline__ unsigned bd_w(h16 depth, const bd_params &p) {
    return 255u - (unsigned)rintf(__fmul_rn(px_ramp(depth, p.lo, p.inv, p.flags), 255.0f));
}

// L2D_BACKDROP_PLANE: W0 - 1 of a ready matte value (clamped: whatever the plane holds, the weight fits its byte)
__device__ __forceinline__ unsigned bd_wm(float m) { return 255u - (unsigned)rintf(__fmul_rn(fminf(fmaxf(m, 0.0f), 1.0f), 255.0f)); }

__global__ __launch_bounds__(BD_THREADS) void frame_backdrop_blur_kernel(const h16 *__restrict__ source, const h16 *__restrict__ depth,
                                                                         h16 *__restrict__ out, int H, int W, bd_params p) {
    // plane c at (y0 - BD_PAD + j, x0 - BD_PAD + cb), clamped: P[0..2] and W - 1
    __shared__ __attribute__((aligned(16))) unsigned char pl[4][BD_BH][BD_BW];
    __shared__ __attribute__((aligned(16))) unsigned short hD[BD_BH][BD_HW];                 // row sums of W, at byte row j and column u of the pass' region
    __shared__ __attribute__((aligned(16))) unsigned hN[BD_BH][BD_HW];                       // row sums of W P[c], one channel at a time

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * BD_TW, y0 = blockIdx.y * BD_TH;
    const int r = p.r, taps = 2 * r + 1;
    const unsigned n = (unsigned)(taps * taps);
    const int halo = p.passes * r;                              // <= BD_PAD
    const long long HW = (long long)H * W;
    const bool from_plane = (p.flags & L2D_BACKDROP_PLANE) != 0;                   // uniform over the launch
    const float *__restrict__ mplane = reinterpret_cast<const float *>(depth);

    // the bytes of the tile and its halo.  An 8-pixel group lies wholly inside or wholly outside the image (W % 8 == 0); one
    // outside holds the edge pixel's values; a group no window reaches is skipped.
    {
        const int rows = BD_TH + 2 * halo;
        for (int g = tid; g < rows * (BD_BW / 8); g += BD_THREADS) {
            const int j = BD_PAD - halo + g / (BD_BW / 8), cg = g % (BD_BW / 8);
            if (cg * 8 + 8 <= BD_PAD - halo || cg * 8 >= BD_PAD + BD_TW + halo) continue;
            const int yy = px_clampi(y0 - BD_PAD + j, 0, H - 1);
            const int gx = x0 - BD_PAD + cg * 8;
            unsigned v[4][8];
            if (gx < 0 || gx >= W) {
                const long long e0 = (long long)yy * W + (gx < 0 ? 0 : W - 1);
                const unsigned b0 = px_byte(source[e0]), b1 = px_byte(source[HW + e0]), b2 = px_byte(source[2 * HW + e0]);
                const unsigned w = from_plane ? bd_wm(mplane[e0]) : bd_w(depth[e0], p);
#pragma unroll
                for (int e = 0; e < 8; ++e) { v[0][e] = b0; v[1][e] = b1; v[2][e] = b2; v[3][e] = w; }
            } else {
                const long long g0 = (long long)yy * W + gx;
                const h16x8 c0 = l2d_ld8(source + g0), c1 = l2d_ld8(source + HW + g0), c2 = l2d_ld8(source + 2 * HW + g0);
#pragma unroll
                for (int e = 0; e < 8; ++e) { v[0][e] = px_byte(c0[e]); v[1][e] = px_byte(c1[e]); v[2][e] = px_byte(c2[e]); }
                if (from_plane) {
                    const f32x4 m0 = *reinterpret_cast<const f32x4 *>(mplane + g0), m1 = *reinterpret_cast<const f32x4 *>(mplane + g0 + 4);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[3][e] = bd_wm(e < 4 ? m0[e & 3] : m1[e & 3]);
                } else {
                    const h16x8 d = l2d_ld8(depth + g0);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[3][e] = bd_w(d[e], p);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) *reinterpret_cast<uint2 *>(&pl[c][j][cg * 8]) = px_pack8(v[c]);
        }
    }
    __syncthreads();

    for (int k = 1; k <= p.passes; ++k) {
        const int h_out = (p.passes - k) * r, h_in = h_out + r;           // the halo this pass writes / reads
        const int rows_in = BD_TH + 2 * h_in, rows_out = BD_TH + 2 * h_out, cols_out = BD_TW + 2 * h_out;
        const int groups = (cols_out + 7) / 8;                            // <= BD_HW / 8
        for (int c = 0; c < 3; ++c) {
            // horizontal pass: row sums at columns u = 0 .. cols_out - 1 (x = x0 - h_out + u), eight consecutive columns per
            // lane as a sliding window.  The leftmost tap of column u is byte column BD_PAD - h_in + u; the columns at or
            // behind cols_out that a group of eight also forms read inside the byte row and are never used.  Measured at
            // 512 x 512, r 6, 3 passes: this form 36.1 us (36.8 with the sums stored one by one as they are formed, an 8-way
            // conflict on the words); one column per lane -- no conflict anywhere, four times the byte reads -- 44.6 us.
            for (int i = tid; i < rows_in * groups; i += BD_THREADS) {
                const int j = BD_PAD - h_in + i / groups, u0 = (i % groups) * 8;
                const unsigned char *ps = &pl[c][j][BD_PAD - h_in + u0], *ws = &pl[3][j][BD_PAD - h_in + u0];
                unsigned sD = 0u, sN = 0u;
                for (int t = 0; t < taps; ++t) {
                    const unsigned w = ws[t] + 1u;
                    sD += w; sN += w * ps[t];
                }
                unsigned vN[8], vD[8];
                vN[0] = sN; vD[0] = sD;
#pragma unroll
                for (int e = 1; e < 8; ++e) {
                    const unsigned w1 = ws[taps - 1 + e] + 1u, w0 = ws[e - 1] + 1u;
                    sD += w1 - w0; sN += w1 * ps[taps - 1 + e] - w0 * ps[e - 1];
                    vN[e] = sN; vD[e] = sD;
                }
                // the eight sums leave as 16-byte stores: two for the words, one for the half-words
                *reinterpret_cast<uint4 *>(&hN[j][u0]) = make_uint4(vN[0], vN[1], vN[2], vN[3]);
                *reinterpret_cast<uint4 *>(&hN[j][u0 + 4]) = make_uint4(vN[4], vN[5], vN[6], vN[7]);
                if (c == 0)
                    *reinterpret_cast<uint4 *>(&hD[j][u0]) = make_uint4(vD[0] | (vD[1] << 16), vD[2] | (vD[3] << 16), vD[4] | (vD[5] << 16),
                                                                        vD[6] | (vD[7] << 16));
            }
            __syncthreads();

            // vertical pass, the division, and the byte back in place: nothing reads plane c again in this pass, and W - 1
            // is replaced behind the third channel's row sums.  (One position per lane: a lane that slides a window down
            // eight rows reads a quarter of the words and was slower, 40.9 against 36.7 us at 512 x 512 -- fewer lanes, longer
            // chains.)
            for (int i = tid; i < rows_out * cols_out; i += BD_THREADS) {
                const int v = i / cols_out, u = i - v * cols_out;
                const int yc = px_clampi(y0 - h_out + v, 0, H - 1), xc = px_clampi(x0 - h_out + u, 0, W - 1);
                const int jc = yc - y0 + BD_PAD, uc = xc - x0 + h_out;   // inside the region: the clamped position lies nearer to the tile
                unsigned D = 0u, N = 0u;
                for (int t = 0; t < taps; ++t) { D += hD[jc - r + t][uc]; N += hN[jc - r + t][uc]; }
                const int j = BD_PAD - h_out + v, cb = BD_PAD - h_out + u;
                pl[c][j][cb] = (unsigned char)((2u * N + D) / (2u * D));
                if (c == 2) pl[3][j][cb] = (unsigned char)((D + n - 1u) / n - 1u);
            }
            __syncthreads();
        }
    }

    // the frame: eight halves, 16 bytes, per lane
    const float scale = (float)(2.0 / 255.0);                     // numpy's float32(2 / 255)
    for (int i = tid; i < 3 * BD_TH * (BD_TW / 8); i += BD_THREADS) {
        const int c = i / (BD_TH * (BD_TW / 8)), ty = (i / (BD_TW / 8)) % BD_TH, cg = i % (BD_TW / 8);
        const int y = y0 + ty, x = x0 + cg * 8;
        if (y >= H || x >= W) continue;
        const uint2 b = *reinterpret_cast<const uint2 *>(&pl[c][BD_PAD + ty][BD_PAD + cg * 8]);
        h16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned q = ((e < 4 ? b.x : b.y) >> (8 * (e & 3))) & 255u;
            o[e] = (h16)__fsub_rn(__fmul_rn((float)q, scale), 1.0f);
        }
        l2d_st8(out + c * HW + (long long)y * W + x, o);
    }
}

int l2d_launch_frame_backdrop_blur(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], r = op->i[2], passes = op->i[3], flags = op->i[4];
    if (!px_check_pointers16("frame_backdrop_blur", op, 3)) return L2D_EINVAL;
    const long long HW = px_check_frame("frame_backdrop_blur", op->tag, H, W);
    if (HW < 0) return L2D_EINVAL;
    if (r < 1 || r > BD_MAX_R) {
        l2d_set_error("frame_backdrop_blur(tag %d): radius %d, need 1..%d", op->tag, r, BD_MAX_R);
        return L2D_EINVAL;
    }
    if (passes < 1 || passes > BD_MAX_PASSES) {
        l2d_set_error("frame_backdrop_blur(tag %d): %d passes, need 1..%d", op->tag, passes, BD_MAX_PASSES);
        return L2D_EINVAL;
    }
    if (flags & ~(L2D_MATTE_HARD | L2D_MATTE_FAR | L2D_BACKDROP_PLANE)) {
        l2d_set_error("frame_backdrop_blur(tag %d): unknown flag bits 0x%x (1 hard, 2 far, 32 plane)", op->tag, flags);
        return L2D_EINVAL;
    }
    const bool plane = (flags & L2D_BACKDROP_PLANE) != 0;
    if (plane && (flags & (L2D_MATTE_HARD | L2D_MATTE_FAR))) {
        l2d_set_error("frame_backdrop_blur(tag %d): ramp flags beside L2D_BACKDROP_PLANE (the plane carries them)", op->tag);
        return L2D_EINVAL;
    }
    const float lo = op->f[0], inv = op->f[1];
    if (!plane && !px_check_ramp("frame_backdrop_blur", op->tag, lo, inv, (flags & L2D_MATTE_HARD) != 0)) return L2D_EINVAL;
    for (int k = 0; k < 2; ++k) {
        if (px_overlap(op->p[2], 6 * HW, op->p[k], (k == 0 ? 6 : (plane ? 4 : 2)) * HW)) {
            l2d_set_error("frame_backdrop_blur(tag %d): the output overlaps pointer %d (a tile's halo reads its neighbours' pixels)", op->tag, k);
            return L2D_EINVAL;
        }
    }
    L2D_DRY_RETURN();
    bd_params p;
    p.lo = lo; p.inv = inv; p.flags = flags; p.r = r; p.passes = passes;
    hipLaunchKernelGGL(frame_backdrop_blur_kernel, dim3((W + BD_TW - 1) / BD_TW, (H + BD_TH - 1) / BD_TH), dim3(BD_THREADS), 0, s,
                       (const h16 *)op->p[0], (const h16 *)op->p[1], (h16 *)op->p[2], H, W, p);
    return l2d_check_launch("frame_backdrop_blur", op->tag);
}
