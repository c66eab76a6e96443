// Output size: the uint8 frame resampled to a size of the caller's choice with Pillow's `Image.resize`
// arithmetic, one launch behind the colour lock and the matte and in front of the JPEG encoder or the copy to the host.  The
// reference has no counterpart: its callers resize the PIL image they get on the host.
//
//   tables (per axis, built on the host in fp64: live2diff_amd/resize.py `coefficients`)
//       xmin[n_out], count[n_out], k[n_out][KS]: output index xx reads input xmin[xx] .. xmin[xx] + count[xx] - 1 with the
//       22-bit fixed-point weights k[xx][0 .. count[xx])
//   one pass    out = clip((2^21 + sum_x in[xmin + x] k[xx][x]) >> 22, 0, 255), arithmetic shift, 32-bit integers
//   the frame   bytes (fp16 source: the egress op's chain first) -> horizontal pass -> uint8 -> vertical pass -> uint8
//
// Integer arithmetic throughout, so the frame equals `resize_ref` (and Pillow) byte for byte; the only floating point is the
// egress chain of the fp16 source.  One work-group per RS_TH x RS_TW output tile and frame: the source patch the tile needs lies
// in LDS as bytes, the horizontally resampled rows of the patch in a second LDS buffer, the vertical pass reads that one.
#include "frame_px.h"

#define RS_TW 32                                  // output tile, pixels
#define RS_TH 32
#define RS_THREADS 256
#define RS_MAX_KS L2D_RESIZE_MAX_KS               // 13 taps: Lanczos at a 2x down-scale
#define RS_BITS 22
// Source pixels one tile needs along an axis: last centre - first centre = (T - 1) scale, plus the support on either side, plus
// one for the two truncations.  With scale <= 2 and support <= 3 max(scale, 1) <= 6: at most 2 (T - 1) + 13 = 2 T + 11.
#define RS_SPAN (2 * RS_TW + RS_MAX_KS)           // 77 (>= 2 T + 11, both tile sizes are equal)
#define RS_PSTRIDE (RS_SPAN * 3 + 1)              // bytes per patch row
#define RS_ITEMS 32                               // stores per output row of a tile: <= 3 head bytes + 24 dwords + 3 tail bytes

static_assert(RS_TW == RS_TH, "RS_SPAN is sized for both axes");
static_assert(RS_TW * 3 / 4 + 6 <= RS_ITEMS, "a tile row is stored by RS_ITEMS lanes");
static_assert(RS_TH * RS_TW * 3 <= RS_SPAN * RS_PSTRIDE, "the output tile reuses the patch buffer");
#define RS_LDS_BYTES (RS_SPAN * RS_PSTRIDE + RS_SPAN * RS_TW * 3 + (RS_TW + RS_TH) * (RS_MAX_KS + 2) * 4)
static_assert(2 * RS_LDS_BYTES <= 160 * 1024, "two work-groups per CU");

__device__ __forceinline__ unsigned char rs_clip(int acc) {
    const int v = acc >> RS_BITS;                 // (arithmetic: acc may be negative, Lanczos and bicubic undershoot)
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One axis of the tile: the span [s0, s0 + n) of source coordinates it reads, and per output its first tap relative to s0, its
// count and its weights, copied to LDS.  Everything read from the tables is clamped to the image, to the KS the launcher was
// given and to the LDS buffers, so a wrong table gives a wrong picture and never an access outside a buffer.
struct rs_axis {
    int s0, n;
};

__device__ __forceinline__ rs_axis rs_span(const int *__restrict__ tab, int n_out, int n_in, int o0, int t) {
    const int *tmin = tab, *tcnt = tab + n_out;
    rs_axis a;
    a.s0 = px_clampi(tmin[o0], 0, n_in);
    const int last = o0 + t - 1;
    const int s1 = px_clampi(tmin[last] + tcnt[last], a.s0, n_in);
    a.n = s1 - a.s0 > RS_SPAN ? RS_SPAN : s1 - a.s0;
    return a;
}

__device__ __forceinline__ void rs_stage(const int *__restrict__ tab, int n_out, int ks, int o0, int t, const rs_axis &a, int lane,
                                         int *first, int *count, int *k) {
    const int *tmin = tab, *tcnt = tab + n_out, *tk = tab + 2 * n_out;
    if (lane < RS_TW) {
        int lo = 0, n = 0;
        if (lane < t) {
            lo = px_clampi(tmin[o0 + lane] - a.s0, 0, a.n);
            n = px_clampi(tcnt[o0 + lane], 0, ks);
            n = n > a.n - lo ? a.n - lo : n;
        }
        first[lane] = lo;
        count[lane] = n;
    }
    for (int i = lane; i < t * ks; i += RS_THREADS / 2) k[(i / ks) * RS_MAX_KS + i % ks] = tk[o0 * ks + i];
}

template <bool U8>
__global__ __launch_bounds__(RS_THREADS) void frame_resize_kernel(const void *__restrict__ src, uint8_t *__restrict__ dst,
                                                                  const int *__restrict__ tx, const int *__restrict__ ty, int H, int W,
                                                                  int Ho, int Wo, int ksx, int ksy, int pitch) {
    __shared__ __attribute__((aligned(16))) unsigned char patch[RS_SPAN * RS_PSTRIDE];      // source bytes; later the output tile
    __shared__ __attribute__((aligned(16))) unsigned char hbuf[RS_SPAN * RS_TW * 3];        // the horizontal pass' rows
    __shared__ int kx[RS_TW * RS_MAX_KS], ky[RS_TH * RS_MAX_KS];
    __shared__ int fx[RS_TW], cx[RS_TW], fy[RS_TH], cy[RS_TH];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * RS_TW, oy0 = blockIdx.y * RS_TH, b = blockIdx.z;
    const int tw = Wo - ox0 < RS_TW ? Wo - ox0 : RS_TW, th = Ho - oy0 < RS_TH ? Ho - oy0 : RS_TH;
    const rs_axis ax = rs_span(tx, Wo, W, ox0, tw), ay = rs_span(ty, Ho, H, oy0, th);

    // the tables of the tile: the first half of the block takes x, the second y
    if (tid < RS_THREADS / 2) {
        rs_stage(tx, Wo, ksx, ox0, tw, ax, tid, fx, cx, kx);
    } else {
        rs_stage(ty, Ho, ksy, oy0, th, ay, tid - RS_THREADS / 2, fy, cy, ky);
    }

    // the source patch as bytes, pixel-interleaved: patch[j][x * 3 + c]
    if (U8) {
        const int rowb = ax.n * 3;
        // (`pitch`: the source's row pitch in pixels, W unless the source is a window of a wider frame)
        const uint8_t *s8 = (const uint8_t *)src + (((long long)b * H + ay.s0) * pitch + ax.s0) * 3;
        for (int i = tid; i < ay.n * rowb; i += RS_THREADS) {
            const int j = i / rowb, e = i - j * rowb;
            patch[j * RS_PSTRIDE + e] = s8[(long long)j * pitch * 3 + e];
        }
    } else {
        const int plane = ay.n * ax.n;
        const h16 *s16 = (const h16 *)src + ((long long)b * 3 * H + ay.s0) * W + ax.s0;
        for (int i = tid; i < 3 * plane; i += RS_THREADS) {
            const int c = i / plane, r = i - c * plane;
            const int j = r / ax.n, x = r - j * ax.n;
            patch[j * RS_PSTRIDE + x * 3 + c] = (unsigned char)px_byte(s16[((long long)c * H + j) * W + x]);
        }
    }
    __syncthreads();

    // horizontal: every row of the patch, the tile's columns
    for (int i = tid; i < ay.n * tw; i += RS_THREADS) {
        const int j = i / tw, xx = i - j * tw;
        const int n = cx[xx];
        const unsigned char *p = patch + j * RS_PSTRIDE + fx[xx] * 3;
        const int *k = kx + xx * RS_MAX_KS;
        int a0 = 1 << (RS_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t) {
            const int kk = k[t];
            a0 += (int)p[t * 3] * kk;
            a1 += (int)p[t * 3 + 1] * kk;
            a2 += (int)p[t * 3 + 2] * kk;
        }
        unsigned char *o = hbuf + (j * RS_TW + xx) * 3;
        o[0] = rs_clip(a0);
        o[1] = rs_clip(a1);
        o[2] = rs_clip(a2);
    }
    __syncthreads();

    // vertical: the tile, into the patch buffer (nobody reads the patch any more)
    for (int i = tid; i < th * tw; i += RS_THREADS) {
        const int yy = i / tw, xx = i - yy * tw;
        const int n = cy[yy];
        const unsigned char *p = hbuf + (fy[yy] * RS_TW + xx) * 3;
        const int *k = ky + yy * RS_MAX_KS;
        int a0 = 1 << (RS_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t) {
            const int kk = k[t];
            a0 += (int)p[t * RS_TW * 3] * kk;
            a1 += (int)p[t * RS_TW * 3 + 1] * kk;
            a2 += (int)p[t * RS_TW * 3 + 2] * kk;
        }
        unsigned char *o = patch + (yy * RS_TW + xx) * 3;
        o[0] = rs_clip(a0);
        o[1] = rs_clip(a1);
        o[2] = rs_clip(a2);
    }
    __syncthreads();

    // the tile's rows: tw * 3 bytes each at an address of any alignment, RS_ITEMS lanes per row, one store each (px_store_row).
    // Every byte lies inside row oy0 + yy < Ho, columns ox0 .. ox0 + tw - 1 < Wo.
    const int nb = tw * 3;
    for (int i = tid; i < th * RS_ITEMS; i += RS_THREADS) {
        const int yy = i / RS_ITEMS, it = i % RS_ITEMS;
        uint8_t *g = dst + (((long long)b * Ho + oy0 + yy) * Wo + ox0) * 3;
        const unsigned char *o = patch + yy * RS_TW * 3;
        px_store_row(g, o, nb, it);
    }
}

int l2d_launch_frame_resize(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], H = op->i[1], W = op->i[2], Ho = op->i[3], Wo = op->i[4], kind = op->i[5], ksx = op->i[6], ksy = op->i[7];
    if (!op->p[0] || !op->p[1] || B <= 0 || H <= 0 || W <= 0 || (kind != 0 && kind != 1)) {
        l2d_set_error("frame_resize(tag %d): invalid arguments (null pointer, non-positive size or source kind %d)", op->tag, kind);
        return L2D_EINVAL;
    }
    if (!px_axis_ok(H, Ho) || !px_axis_ok(W, Wo)) {
        l2d_set_error("frame_resize(tag %d): %d x %d -> %d x %d: an output size must lie in 1..%d and between half and 8 times its "
                      "source size", op->tag, H, W, Ho, Wo, L2D_RESIZE_MAX_SIZE);
        return L2D_EINVAL;
    }
    if (ksx < 1 || ksx > RS_MAX_KS || ksy < 1 || ksy > RS_MAX_KS) {
        l2d_set_error("frame_resize(tag %d): KS = %d (x), %d (y) taps, need 1..%d", op->tag, ksx, ksy, RS_MAX_KS);
        return L2D_EINVAL;
    }
    if ((long long)B * Ho * Wo * 3 >= (1ll << 31) || B > 65535) {
        l2d_set_error("frame_resize(tag %d): B Ho Wo 3 must stay below 2^31 and B below 65536", op->tag);
        return L2D_EINVAL;
    }
    for (int k = 2; k < 4; ++k) {
        if (!op->p[k] || (((uintptr_t)op->p[k]) & 3)) {
            l2d_set_error("frame_resize(tag %d): table pointer %d is null or not 4-byte aligned", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if (kind == 0 && (((uintptr_t)op->p[0]) & 3)) {
        l2d_set_error("frame_resize(tag %d): the fp16 source is not 4-byte aligned", op->tag);
        return L2D_EINVAL;
    }
    const int pitch = op->i[8];                   // 0: W
    if (pitch != 0 && (pitch < W || kind != 1 || B != 1)) {
        l2d_set_error("frame_resize(tag %d): a source row pitch (%d pixels) must be at least W = %d and goes with a uint8 source and "
                      "B = 1 only", op->tag, pitch, W);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const dim3 grid((Wo + RS_TW - 1) / RS_TW, (Ho + RS_TH - 1) / RS_TH, B);
    uint8_t *dst = (uint8_t *)op->p[1];
    const int *tx = (const int *)op->p[2], *ty = (const int *)op->p[3];
    if (kind == 1) {
        hipLaunchKernelGGL(frame_resize_kernel<true>, grid, dim3(RS_THREADS), 0, s, op->p[0], dst, tx, ty, H, W, Ho, Wo, ksx, ksy,
                           pitch ? pitch : W);
    } else {
        hipLaunchKernelGGL(frame_resize_kernel<false>, grid, dim3(RS_THREADS), 0, s, op->p[0], dst, tx, ty, H, W, Ho, Wo, ksx, ksy, W);
    }
    return l2d_check_launch("frame_resize", op->tag);
}
