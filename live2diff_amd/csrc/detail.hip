// Detail mode: the camera's fine detail in the upscaled frame.  The styled frame resampled to the
// output size (L2D_OP_FRAME_RESIZE) holds the stream's lines of information and no more; the camera frame at the output size
// (resize.CameraTap) holds what the stream-size bottleneck lost.  The regression-based detail injection of pan-sharpening puts
// it back: the styled frame is the low-resolution colour image, the camera's luma at the output size the high-resolution band,
// and the injection gain the local regression slope of each styled channel on the source frame's luma -- stage 1 of the guided
// filter of matte_edge.hip.  The reference has no counterpart.  Two launches:
//
// L2D_OP_FRAME_DETAIL_GAIN, at the stream's size:
//   P[c]                                                     the bytes the resize reads: the egress op's bytes of the fp16 frame,
//                                                            or the uint8 HWC frame of the matte (L2D_DETAIL_U8)
//   Y = (77 R + 150 G + 29 B + 128) >> 8                     the guide: luma of the egress op's bytes of the source frame
//   S_I, S_II (once), S_P, S_IP (per channel)                sums of Y, Y Y, P, Y P over the (2r+1)^2 window, coordinates clamped
//   cov = n S_IP - S_I S_P,  var = n S_II - S_I S_I          int64, n = (2r+1)^2
//   a = double(cov) / (double(var) + E),  A = rint(4096 a)   E = double(n n) eps eps, from the host; |A| <= 261120
//   G[c] = window_sum(A)                                     int32: n 4096 times the mean gain
//
// L2D_OP_FRAME_DETAIL, at the output size:
//   d = luma(C) - luma(L)                                    C the camera's bytes, L the source frame through the same filter as S
//   g = the bilinear taps (matte.up_table) of float(G[c])    a_y = g[y][x0] + fx (g[y][x1] - g[y][x0]); top + fy (bot - top)
//   t = g float(d);  u = t k;  u = min(max(u, -limit), limit);  o = min(max(float(S) + u, 0), 255);  byte = rint(o)
//   SHOW: byte = rint(min(max(128 + u, 0), 255))
//
// Integers are exact in any order; every floating-point step is one correctly rounded operation (the file is built with
// -ffp-contract=off, see the Makefile), so numpy restates both bit for bit (live2diff_amd/detail.py `gains_ref`, `inject_ref`).
#include <math.h>
#include <string.h>

#include "frame_px.h"

// ------------------------------------------------------------------------------------------------------------------------------
// the gains
#define DG_MAX_R L2D_MATTE_EDGE_MAX_R
#define DG_TW 64                              // the tile: L2D_OP_FRAME_MATTE_EDGE's
#define DG_TH 16
#define DG_THREADS 256
#define DG_PAD (2 * DG_MAX_R)                 // columns of halo kept on either side of the tile: two 8-pixel groups
#define DG_YW (DG_TW + 2 * DG_PAD)            // 96: a row of Y / P
#define DG_YH (DG_TH + 4 * DG_MAX_R)          // 48
#define DG_AW (DG_TW + 2 * DG_MAX_R)          // 80: a row of A, and of the first horizontal sums
#define DG_AH (DG_TH + 2 * DG_MAX_R)          // 32
#define DG_TAPS (2 * DG_MAX_R + 1)

// LDS: the bytes of Y and the three P planes; ONE set of row sums (two words per position: Y and Y Y first, then channel by
// channel P and Y P, then the row sums of A); the window sums S_I and S_II, formed once; A of one channel
#define DG_BYTES_Y (DG_YH * DG_YW)                        // 4608, four times
#define DG_WORDS_H (2 * DG_YH * DG_AW)                    // 7680 words
#define DG_WORDS_S (2 * DG_AH * DG_AW)                    // 5120 words
#define DG_WORDS_A (DG_AH * DG_AW)                        // 2560 words
#define DG_LDS_BYTES (4 * DG_BYTES_Y + 4 * DG_WORDS_H + 4 * DG_WORDS_S + 4 * DG_WORDS_A)
static_assert(DG_PAD % 8 == 0 && DG_PAD >= 2 * DG_MAX_R, "the halo of 2r is whole 8-pixel groups");
static_assert(255 * DG_TAPS < 65536, "a row sum of Y or P fits 16 bits");
static_assert(255ll * 255 * DG_TAPS * DG_TAPS < (1ll << 32), "a window sum of Y Y or Y P fits 32 bits");
static_assert(DG_AH * DG_TW <= DG_WORDS_H, "the row sums of A fit where the first pass' row sums were");
// |a| <= 127.5 / (2 eps) <= 63.75: |A| <= 261120
static_assert(261120ll * DG_TAPS * DG_TAPS < (1ll << 31), "the window sum of A fits 32 bits");
static_assert(DG_LDS_BYTES == 79872, "the LDS size DESIGN.md section 8.z10 states");
static_assert(DG_LDS_BYTES <= 80 * 1024 && 2 * DG_LDS_BYTES <= 160 * 1024, "two work-groups per CU");

// the three bytes of pixel `e` of an 8-pixel group of a uint8 HWC frame, held as six dwords
__device__ __forceinline__ unsigned dg_hwc(const unsigned *w, int e, int c) {
    const int k = e * 3 + c;
    return (w[k >> 2] >> ((k & 3) * 8)) & 255u;
}

__global__ __launch_bounds__(DG_THREADS) void frame_detail_gain_kernel(const void *__restrict__ frame, const h16 *__restrict__ source,
                                                                       int *__restrict__ out, int H, int W, int r, int u8, double E) {
    __shared__ __attribute__((aligned(16))) unsigned char yb[DG_YH][DG_YW];       // Y at (y0 - 2r + j, x0 - DG_PAD + c), clamped
    __shared__ __attribute__((aligned(16))) unsigned char pb[3][DG_YH][DG_YW];    // P[c] likewise
    __shared__ __attribute__((aligned(16))) unsigned hbuf[DG_WORDS_H];
    __shared__ unsigned sI[DG_AH][DG_AW];                                          // S_I at (y0 - r + v, x0 - r + u), clamped
    __shared__ unsigned sII[DG_AH][DG_AW];
    __shared__ int Aa[DG_AH][DG_AW];                                               // A of the channel in hand, likewise
    unsigned (*h1)[DG_AW] = reinterpret_cast<unsigned (*)[DG_AW]>(hbuf);                                    // row sums of Y, then of P
    unsigned (*h2)[DG_AW] = reinterpret_cast<unsigned (*)[DG_AW]>(hbuf + DG_YH * DG_AW);                    // of Y Y, then of Y P
    int (*hA)[DG_TW] = reinterpret_cast<int (*)[DG_TW]>(hbuf);                                              // behind them, of A

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * DG_TW, y0 = blockIdx.y * DG_TH;
    const int taps = 2 * r + 1, n = taps * taps;
    const int rows2 = DG_TH + 4 * r, rows1 = DG_TH + 2 * r, cols1 = DG_TW + 2 * r;
    const long long HW = (long long)H * W;
    const h16 *fh = (const h16 *)frame;
    const unsigned char *fb = (const unsigned char *)frame;

    // Y and P of the tile and its halo of 2r.  An 8-pixel group lies wholly inside or wholly outside the image (W % 8 == 0, so
    // W >= 8); one outside holds the edge pixel's values; a group no window reaches is skipped.
    for (int g = tid; g < rows2 * (DG_YW / 8); g += DG_THREADS) {
        const int j = g / (DG_YW / 8), cg = g % (DG_YW / 8);
        if (cg * 8 + 8 <= DG_PAD - 2 * r || cg * 8 >= DG_PAD + DG_TW + 2 * r) continue;
        const int yy = px_clampi(y0 - 2 * r + j, 0, H - 1);
        const int gx = x0 - DG_PAD + cg * 8;
        // (a group outside the image: the nearest group of the row is loaded and its edge pixel takes all eight places)
        const int edge = gx < 0 ? 0 : (gx >= W ? 7 : -1);
        const long long g0 = (long long)yy * W + (gx < 0 ? 0 : (gx >= W ? W - 8 : gx));
        unsigned yv[8], pv[3][8];
        {
            const h16x8 cr = l2d_ld8(source + g0), cgn = l2d_ld8(source + HW + g0), cb = l2d_ld8(source + 2 * HW + g0);
#pragma unroll
            for (int e = 0; e < 8; ++e) yv[e] = px_luma(px_byte(cr[e]), px_byte(cgn[e]), px_byte(cb[e]));
        }
        if (u8) {
            // 24 bytes at a multiple of 24 from a 16-byte aligned frame: three 8-byte loads
            const uint2 *q = reinterpret_cast<const uint2 *>(fb + g0 * 3);
            const uint2 q0 = q[0], q1 = q[1], q2 = q[2];
            const unsigned w[6] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y};
#pragma unroll
            for (int e = 0; e < 8; ++e) { pv[0][e] = dg_hwc(w, e, 0); pv[1][e] = dg_hwc(w, e, 1); pv[2][e] = dg_hwc(w, e, 2); }
        } else {
            const h16x8 fr = l2d_ld8(fh + g0), fg = l2d_ld8(fh + HW + g0), fbl = l2d_ld8(fh + 2 * HW + g0);
#pragma unroll
            for (int e = 0; e < 8; ++e) { pv[0][e] = px_byte(fr[e]); pv[1][e] = px_byte(fg[e]); pv[2][e] = px_byte(fbl[e]); }
        }
        if (edge >= 0) {
            const int k = edge;                                   // 0 or 7
            const unsigned ye = k ? yv[7] : yv[0], p0 = k ? pv[0][7] : pv[0][0], p1 = k ? pv[1][7] : pv[1][0], p2 = k ? pv[2][7] : pv[2][0];
#pragma unroll
            for (int e = 0; e < 8; ++e) { yv[e] = ye; pv[0][e] = p0; pv[1][e] = p1; pv[2][e] = p2; }
        }
        *reinterpret_cast<uint2 *>(&yb[j][cg * 8]) = px_pack8(yv);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint2 *>(&pb[c][j][cg * 8]) = px_pack8(pv[c]);
    }
    __syncthreads();

    // The horizontal pass of the guide: row sums of Y and Y Y at columns u = 0 .. cols1 - 1 (x = x0 - r + u), eight consecutive
    // columns per lane as a sliding window.  The leftmost tap of column u is byte column DG_PAD - 2r + u, the rightmost
    // DG_PAD + u <= 95: the columns at or behind cols1 that a group of eight also forms read inside the row and are never used.
    const int groups = (cols1 + 7) / 8;                           // <= DG_AW / 8
    for (int i = tid; i < rows2 * groups; i += DG_THREADS) {
        const int j = i / groups, u0 = (i % groups) * 8;
        const unsigned char *ys = &yb[j][DG_PAD - 2 * r + u0];
        unsigned a = 0u, b = 0u;
        for (int k = 0; k < taps; ++k) {
            const unsigned y = ys[k];
            a += y; b += y * y;
        }
        h1[j][u0] = a; h2[j][u0] = b;
#pragma unroll
        for (int e = 1; e < 8; ++e) {
            const unsigned y1 = ys[taps - 1 + e], yl = ys[e - 1];
            a += y1 - yl; b += y1 * y1 - yl * yl;
            h1[j][u0 + e] = a; h2[j][u0 + e] = b;
        }
    }
    __syncthreads();

    // its vertical pass, on the tile and a halo of r: S_I and S_II, formed once for the three channels.  A position outside the
    // image holds the sums of the clamped position (the window sum of A clamps its coordinates); that position lies nearer to
    // the tile, so its window is in LDS as well.
    for (int i = tid; i < rows1 * cols1; i += DG_THREADS) {
        const int v = i / cols1, u = i - v * cols1;
        const int xc = px_clampi(x0 - r + u, 0, W - 1), yc = px_clampi(y0 - r + v, 0, H - 1);
        const int uc = px_clampi(xc - (x0 - r), 0, cols1 - 1), j0 = px_clampi(yc - y0 + r, 0, rows1 - 1);           // the window's first row
        unsigned a = 0u, b = 0u;
        for (int k = 0; k < taps; ++k) { a += h1[j0 + k][uc]; b += h2[j0 + k][uc]; }
        sI[v][u] = a; sII[v][u] = b;
    }
    __syncthreads();

    for (int c = 0; c < 3; ++c) {
        // the horizontal pass of the channel: row sums of P and Y P, through the same buffers
        for (int i = tid; i < rows2 * groups; i += DG_THREADS) {
            const int j = i / groups, u0 = (i % groups) * 8;
            const unsigned char *ys = &yb[j][DG_PAD - 2 * r + u0], *ps = &pb[c][j][DG_PAD - 2 * r + u0];
            unsigned a = 0u, b = 0u;
            for (int k = 0; k < taps; ++k) {
                const unsigned q = ps[k];
                a += q; b += ys[k] * q;
            }
            h1[j][u0] = a; h2[j][u0] = b;
#pragma unroll
            for (int e = 1; e < 8; ++e) {
                const unsigned y1 = ys[taps - 1 + e], q1 = ps[taps - 1 + e], yl = ys[e - 1], ql = ps[e - 1];
                a += q1 - ql; b += y1 * q1 - yl * ql;
                h1[j][u0 + e] = a; h2[j][u0 + e] = b;
            }
        }
        __syncthreads();

        // its vertical pass and the coefficient
        for (int i = tid; i < rows1 * cols1; i += DG_THREADS) {
            const int v = i / cols1, u = i - v * cols1;
            const int xc = px_clampi(x0 - r + u, 0, W - 1), yc = px_clampi(y0 - r + v, 0, H - 1);
            const int uc = px_clampi(xc - (x0 - r), 0, cols1 - 1), j0 = px_clampi(yc - y0 + r, 0, rows1 - 1);
            unsigned sP = 0u, sIP = 0u;
            for (int k = 0; k < taps; ++k) { sP += h1[j0 + k][uc]; sIP += h2[j0 + k][uc]; }
            const unsigned si = sI[v][u];
            const long long cov = (long long)n * sIP - (long long)si * sP;
            const long long var = (long long)n * sII[v][u] - (long long)si * si;
            const double a = __ddiv_rn((double)cov, __dadd_rn((double)var, E));
            Aa[v][u] = (int)rint(__dmul_rn(a, 4096.0));
        }
        __syncthreads();

        // the horizontal pass of A: hA[v][x] = Aa[v][x] + ... + Aa[v][x + 2r] (column x0 + x)
        for (int i = tid; i < rows1 * DG_TW; i += DG_THREADS) {
            const int v = i / DG_TW, x = i % DG_TW;
            int sa = 0;
            for (int k = 0; k < taps; ++k) sa += Aa[v][x + k];
            hA[v][x] = sa;
        }
        __syncthreads();

        // its vertical pass and the plane: consecutive lanes consecutive words of a row
        for (int i = tid; i < DG_TH * DG_TW; i += DG_THREADS) {
            const int ty = i / DG_TW, x = i % DG_TW;
            const int gy = y0 + ty, gx = x0 + x;
            if (gy >= H || gx >= W) continue;
            int SA = 0;
            for (int k = 0; k < taps; ++k) SA += hA[ty + k][x];
            out[c * HW + (long long)gy * W + gx] = SA;
        }
        __syncthreads();                                          // (the next channel's row sums overwrite hA)
    }
}

int l2d_launch_frame_detail_gain(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], r = op->i[2], flags = op->i[3];
    if (!px_check_pointers16("frame_detail_gain", op, 3)) return L2D_EINVAL;
    if (px_check_frame("frame_detail_gain", op->tag, H, W) < 0) return L2D_EINVAL;
    if (r < 1 || r > DG_MAX_R) {
        l2d_set_error("frame_detail_gain(tag %d): radius %d, need 1..%d", op->tag, r, DG_MAX_R);
        return L2D_EINVAL;
    }
    if (flags & ~L2D_DETAIL_U8) {
        l2d_set_error("frame_detail_gain(tag %d): unknown flag bits 0x%x (1 uint8 frame)", op->tag, flags);
        return L2D_EINVAL;
    }
    double E;
    static_assert(sizeof(double) == sizeof(op->l[0]), "E travels as the bits of a double");
    memcpy(&E, &op->l[0], sizeof(double));
    const double nn = (double)((2 * r + 1) * (2 * r + 1)) * (double)((2 * r + 1) * (2 * r + 1));
    if (!(E >= nn && E <= 1.0e300)) {
        l2d_set_error("frame_detail_gain(tag %d): E = %g must be finite and at least n n = %g (eps >= 1: the gains fit 32 bits)", op->tag,
                      E, nn);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    hipLaunchKernelGGL(frame_detail_gain_kernel, dim3((W + DG_TW - 1) / DG_TW, (H + DG_TH - 1) / DG_TH), dim3(DG_THREADS), 0, s, op->p[0],
                       (const h16 *)op->p[1], (int *)op->p[2], H, W, r, (flags & L2D_DETAIL_U8) ? 1 : 0, E);
    return l2d_check_launch("frame_detail_gain", op->tag);
}

// ------------------------------------------------------------------------------------------------------------------------------
// the injection
#define DT_T 32                                   // output tile, pixels (both axes): L2D_OP_FRAME_MATTE_UP's
#define DT_THREADS 256
#define DT_SPAN (2 * DT_T)                        // source pixels a tile's taps reach along an axis at the 1/2 limit (matte.hip MU_SPAN)
#define DT_STRIDE (DT_SPAN + 1)                   // floats per LDS row of a gain plane
#define DT_ITEMS 32                               // stores per output row of a tile: <= 3 head bytes + 24 dwords + 3 tail bytes
static_assert(DT_SPAN >= 2 * (DT_T - 1) + 2, "a tile's taps fit the span at a ratio of 1/2");
static_assert(DT_T * 3 / 4 + 6 <= DT_ITEMS, "a tile row is stored by DT_ITEMS lanes");
#define DT_LDS_BYTES (3 * DT_SPAN * DT_STRIDE * 4 + DT_T * DT_T * 3 + 6 * DT_T * 4)
static_assert(DT_LDS_BYTES == 53760, "the LDS size DESIGN.md section 8.z10 states");
static_assert(2 * DT_LDS_BYTES <= 160 * 1024, "two work-groups per CU");

__global__ __launch_bounds__(DT_THREADS) void frame_detail_kernel(const uint8_t *__restrict__ styled, const uint8_t *__restrict__ camera,
                                                                  const uint8_t *__restrict__ low, const int *__restrict__ gains,
                                                                  const int *__restrict__ tx, const int *__restrict__ ty,
                                                                  uint8_t *__restrict__ dst, int H, int W, int Ho, int Wo, int show, float k,
                                                                  float limit) {
    __shared__ float gg[3][DT_SPAN * DT_STRIDE];                                  // float(G[c]) of the patch the tile's taps reach
    __shared__ __attribute__((aligned(16))) unsigned char ob[DT_T * DT_T * 3];    // the tile's bytes
    __shared__ int x0s[DT_T], x1s[DT_T], y0s[DT_T], y1s[DT_T];
    __shared__ float fxs[DT_T], fys[DT_T];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * DT_T, oy0 = blockIdx.y * DT_T;
    const int tw = Wo - ox0 < DT_T ? Wo - ox0 : DT_T, th = Ho - oy0 < DT_T ? Ho - oy0 : DT_T;
    int sx0, nx, sy0, ny;
    px_span<DT_SPAN>(tx, Wo, W, ox0, tw, sx0, nx);
    px_span<DT_SPAN>(ty, Ho, H, oy0, th, sy0, ny);
    if (tid < DT_T) {
        px_stage(tx, Wo, W, ox0, tw, sx0, nx, tid, x0s, x1s, fxs);
    } else if (tid >= 64 && tid < 64 + DT_T) {
        px_stage(ty, Ho, H, oy0, th, sy0, ny, tid - 64, y0s, y1s, fys);
    }

    // the gains of the patch: sy0 + j <= H - 1 and sx0 + c <= W - 1 by px_span
    const long long HW = (long long)H * W;
    for (int i = tid; i < 3 * ny * nx; i += DT_THREADS) {
        const int ch = i / (ny * nx), q = i - ch * (ny * nx);
        const int j = q / nx, c = q - j * nx;
        gg[ch][j * DT_STRIDE + c] = (float)gains[ch * HW + (long long)(sy0 + j) * W + (sx0 + c)];
    }
    __syncthreads();

    // the bytes: one lane per pixel
    for (int i = tid; i < th * tw; i += DT_THREADS) {
        const int yy = i / tw, xx = i - yy * tw;
        const long long g = ((long long)(oy0 + yy) * Wo + ox0 + xx) * 3;
        const int lc = (int)px_luma(camera[g], camera[g + 1], camera[g + 2]);
        const int ll = (int)px_luma(low[g], low[g + 1], low[g + 2]);
        const float d = (float)(lc - ll);
        const int r0 = y0s[yy] * DT_STRIDE, r1 = y1s[yy] * DT_STRIDE;
        const int a = x0s[xx], c = x1s[xx];
        const float fx = fxs[xx], fy = fys[yy];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float *t0 = gg[ch] + r0, *t1 = gg[ch] + r1;
            const float top = __fadd_rn(t0[a], __fmul_rn(fx, __fsub_rn(t0[c], t0[a])));
            const float bot = __fadd_rn(t1[a], __fmul_rn(fx, __fsub_rn(t1[c], t1[a])));
            const float gv = __fadd_rn(top, __fmul_rn(fy, __fsub_rn(bot, top)));
            float u = __fmul_rn(__fmul_rn(gv, d), k);
            u = fminf(fmaxf(u, -limit), limit);
            float o = __fadd_rn(show ? 128.0f : (float)styled[g + ch], u);
            o = fminf(fmaxf(o, 0.0f), 255.0f);
            ob[(yy * DT_T + xx) * 3 + ch] = (unsigned char)(unsigned)rintf(o);
        }
    }
    __syncthreads();

    // the tile's rows: tw * 3 bytes each at an address of any alignment, DT_ITEMS lanes per row, one store each (px_store_row).
    // Every byte lies inside row oy0 + yy < Ho, columns ox0 .. ox0 + tw - 1 < Wo.
    const int nb = tw * 3;
    for (int i = tid; i < th * DT_ITEMS; i += DT_THREADS) {
        const int yy = i / DT_ITEMS, it = i % DT_ITEMS;
        uint8_t *g = dst + ((long long)(oy0 + yy) * Wo + ox0) * 3;
        const unsigned char *o = ob + yy * DT_T * 3;
        px_store_row(g, o, nb, it);
    }
}

int l2d_launch_frame_detail(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], Ho = op->i[2], Wo = op->i[3], flags = op->i[4];
    const float k = op->f[0], limit = op->f[1];
    for (int j = 0; j < 7; ++j) {
        if (!op->p[j]) {
            l2d_set_error("frame_detail(tag %d): pointer %d is null", op->tag, j);
            return L2D_EINVAL;
        }
    }
    if (H <= 0 || W <= 0) {
        l2d_set_error("frame_detail(tag %d): non-positive size (H %d, W %d)", op->tag, H, W);
        return L2D_EINVAL;
    }
    if (!px_axis_ok(H, Ho) || !px_axis_ok(W, Wo)) {
        l2d_set_error("frame_detail(tag %d): %d x %d -> %d x %d: an output size must lie in 1..%d and between half and 8 times the "
                      "gains' size", op->tag, H, W, Ho, Wo, L2D_RESIZE_MAX_SIZE);
        return L2D_EINVAL;
    }
    const long long nbytes = (long long)Ho * Wo * 3;
    if (nbytes >= (1ll << 31) || 3ll * H * W >= (1ll << 31)) {
        l2d_set_error("frame_detail(tag %d): Ho Wo 3 and 3 H W must stay below 2^31", op->tag);
        return L2D_EINVAL;
    }
    for (int j = 3; j < 6; ++j) {
        if (((uintptr_t)op->p[j]) & 3) {
            l2d_set_error("frame_detail(tag %d): pointer %d (the gains, the x table, the y table) is not 4-byte aligned", op->tag, j);
            return L2D_EINVAL;
        }
    }
    if (flags & ~L2D_DETAIL_SHOW) {
        l2d_set_error("frame_detail(tag %d): unknown flag bits 0x%x (2 show)", op->tag, flags);
        return L2D_EINVAL;
    }
    if (!(limit >= 0.0f) || limit > 3.0e38f || !(k >= 0.0f) || k > 3.0e38f) {
        l2d_set_error("frame_detail(tag %d): limit = %g and k = %g must be finite and not negative", op->tag, limit, k);
        return L2D_EINVAL;
    }
    for (int j = 0; j < 3; ++j) {
        if (px_overlap(op->p[6], nbytes, op->p[j], nbytes)) {
            l2d_set_error("frame_detail(tag %d): dst overlaps input %d (a tile reads what another may have written)", op->tag, j);
            return L2D_EINVAL;
        }
    }
    L2D_DRY_RETURN();
    hipLaunchKernelGGL(frame_detail_kernel, dim3((Wo + DT_T - 1) / DT_T, (Ho + DT_T - 1) / DT_T), dim3(DT_THREADS), 0, s,
                       (const uint8_t *)op->p[0], (const uint8_t *)op->p[1], (const uint8_t *)op->p[2], (const int *)op->p[3],
                       (const int *)op->p[4], (const int *)op->p[5], (uint8_t *)op->p[6], H, W, Ho, Wo, (flags & L2D_DETAIL_SHOW) ? 1 : 0, k,
                       limit);
    return l2d_check_launch("frame_detail", op->tag);
}
