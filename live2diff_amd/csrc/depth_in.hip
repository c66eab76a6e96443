// Depth from the caller: a depth frame of an RGB-D camera or of the caller's own estimator -- uint16 or
// fp32, any size -- becomes the stream's conditioning map, fp16 [B][3][H][W] in [-1, 1], in place of the detector path
// (glue.hip resize + midas_hip + depth_norm_resize).  The reference has no counterpart.  Two launches:
//
//   L2D_OP_DEPTH_INGEST     per source sample z: v = 1 where it is valid (uint16: z != invalid; fp32: finite and != invalid; both:
//                           u finite and not negative), u = float(z) ("inverse") or 1 / float(z) ("distance"), u = 0 where
//                           v = 0.  Per output pixel, with the antialiased triangle weights of the frame ingest (tables the host
//                           builds with frame_io.aa_weights and uploads: the oracle reads the same numbers), taps ascending:
//                             num = sum_y wy (sum_x wx u),  den = sum_y wy (sum_x wx v),  R = num / den where den > 0, else -1
//                           -- a normalised convolution: holes smaller than the filter's footprint are filled by their valid
//                           neighbours, larger ones stay holes.  One work-group per DI_TH x DI_TW output tile and frame: the
//                           horizontal sums of the source rows the tile's taps reach are staged in LDS (never the raw patch:
//                           at scale 8 an fp32 patch of 137 x 265 samples would not fit), then the vertical pass.  R goes out
//                           as an fp32 plane, and the tile's {min, max, any} over its valued pixels as three plain stores:
//                           nothing is zeroed between frames and there is no atomic (the pattern of colorlock.hip).
//   L2D_OP_DEPTH_NORMALIZE  every block takes min and max over all partials of the call -- all B frames jointly -- or the
//                           fixed range of its record, then n = clamp((R - mn) / (mx - mn), 0, 1), out = fp16(2 n - 1) on all
//                           three planes; -1 for a pixel with no value, and everywhere where nothing has a value or the map is
//                           flat: mx - mn <= 2^-14 mx, which holds mx <= mn and the rounding noise of the resampling -- R of
//                           a constant frame moves by up to 2 x (2 x 2 x 34 + 1) roundings of 2^-24, below 2^-15.9 of its value,
//                           and stretching that to [-1, 1] would condition the stream on noise.  The margin belongs to the
//                           range the frames give; a fixed range is flat only where mx <= mn.
//
// Every product, sum and quotient is one fp32 operation with one rounding (the file is built with -ffp-contract=off, see the
// Makefile; fp32 division is the correctly rounded one), min and max are exact, so numpy restates both ops bit for bit
// (live2diff_amd/depth_io.py resample_ref, normalize_ref).  Launch-bound like the frame ingest: no MFMA.
#include "common.h"

#define DI_THREADS 256
#define DI_WAVES (DI_THREADS / L2D_WAVE)
#define DI_TH L2D_DEPTH_TILE_H
#define DI_TW L2D_DEPTH_TILE_W
#define DI_MAX_K L2D_DEPTH_MAX_TAPS                   // 2 * 8 + 1 taps per axis at scale 8
#define DI_ROWS ((DI_TH - 1) * 8 + DI_MAX_K + 7)      // source rows under one tile at scale 8: 15 x 8 between the first and the
                                                      // last centre + 17 taps = 137, rounded up to a multiple of 8
#define DI_F32 L2D_DEPTH_F32
#define DI_DISTANCE L2D_DEPTH_DISTANCE
#define DI_HAS_INVALID L2D_DEPTH_HAS_INVALID
#define DI_FIXED L2D_DEPTH_FIXED_RANGE
#define DI_FLAT 6.103515625e-05f                      // 2^-14: the relative range at or below which a map counts as flat

#define DI_LDS_BYTES (2 * DI_ROWS * DI_TW * 4 + DI_TW * DI_MAX_K * 4 + DI_TW * 4 + DI_WAVES * 3 * 4)
static_assert(DI_LDS_BYTES == 39216, "the LDS of the ingest kernel as DESIGN.md section 8.z12 and the resource test state it");
#define DN_LDS_BYTES (DI_WAVES * 3 * 4 + 3 * 4)
static_assert(DN_LDS_BYTES == 60, "the LDS of the normalise kernel as DESIGN.md section 8.z12 and the resource test state it");
static_assert(DI_LDS_BYTES <= 80 * 1024, "two work-groups per CU");
static_assert(DI_TH * DI_TW % DI_THREADS == 0 && DI_TW == 32, "a half-wave is one row of the tile: conflict-free LDS rows");

struct di_params {
    int B, Hd, Wd, H, W, Kx, Ky, flags, invalid_u16;
    float invalid_f32;
};

// (u, v) of one source sample
__device__ __forceinline__ void di_sample(const void *__restrict__ src, long long idx, const di_params &p, float &u, float &v) {
    float zf;
    bool ok;
    if (p.flags & DI_F32) {
        zf = ((const float *)src)[idx];
        ok = (__float_as_uint(zf) & 0x7f800000u) != 0x7f800000u;
        if (p.flags & DI_HAS_INVALID) ok = ok && zf != p.invalid_f32;
    } else {
        const int z = ((const uint16_t *)src)[idx];
        zf = (float)z;
        ok = !(p.flags & DI_HAS_INVALID) || z != p.invalid_u16;
    }
    const float q = (p.flags & DI_DISTANCE) ? __fdiv_rn(1.0f, zf) : zf;
    ok = ok && (__float_as_uint(q) & 0x7f800000u) != 0x7f800000u && q >= 0.0f;
    u = ok ? q : 0.0f;
    v = ok ? 1.0f : 0.0f;
}

// grid (tiles x, tiles y, B); partials[((b tiles_y + ty) tiles_x + tx)][3] = min, max, any of the tile's valued pixels
// (+inf, -1, 0 where it has none).  What is read from a table is clamped to the image and to the staged rows.
__global__ __launch_bounds__(DI_THREADS) void depth_ingest_kernel(const void *__restrict__ src, float *__restrict__ R,
                                                                  float *__restrict__ partials, const int *__restrict__ xmin,
                                                                  const float *__restrict__ wx, const int *__restrict__ ymin,
                                                                  const float *__restrict__ wy, di_params p) {
    __shared__ float hn[DI_ROWS][DI_TW];
    __shared__ float hd[DI_ROWS][DI_TW];
    __shared__ float swx[DI_TW][DI_MAX_K];
    __shared__ int sxlo[DI_TW];
    __shared__ float red[DI_WAVES][3];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * DI_TW, y0 = blockIdx.y * DI_TH, b = blockIdx.z;
    const int tw = min(DI_TW, p.W - x0), th = min(DI_TH, p.H - y0);

    for (int i = tid; i < DI_TW * DI_MAX_K; i += DI_THREADS) {
        const int c = i / DI_MAX_K, j = i % DI_MAX_K;
        swx[c][j] = (c < tw && j < p.Kx) ? wx[(long long)(x0 + c) * p.Kx + j] : 0.0f;
    }
    if (tid < DI_TW) sxlo[tid] = tid < tw ? xmin[x0 + tid] : 0;
    const int r0 = min(max(ymin[y0], 0), p.Hd - 1);
    const int r1 = min(max(ymin[y0 + th - 1] + p.Ky, r0 + 1), p.Hd);
    const int nrows = min(r1 - r0, DI_ROWS);
    __syncthreads();

    // horizontal pass: one lane per (source row, tile column)
    for (int i = tid; i < nrows * DI_TW; i += DI_THREADS) {
        const int r = i / DI_TW, c = i % DI_TW;
        float n = 0.0f, d = 0.0f;
        if (c < tw) {
            const long long row = ((long long)b * p.Hd + r0 + r) * p.Wd;
            const int lo = sxlo[c];
            for (int j = 0; j < p.Kx; ++j) {
                const int xi = min(max(lo + j, 0), p.Wd - 1);          // (a tap past the row's own count has weight 0)
                const float w = swx[c][j];
                float u, v;
                di_sample(src, row + xi, p, u, v);
                n = __fadd_rn(n, __fmul_rn(w, u));
                d = __fadd_rn(d, __fmul_rn(w, v));
            }
        }
        hn[r][c] = n;
        hd[r][c] = d;
    }
    __syncthreads();

    // vertical pass: DI_TH x DI_TW outputs, two per lane
    float mn = __builtin_inff(), mx = -1.0f, any = 0.0f;
#pragma unroll
    for (int it = 0; it < DI_TH * DI_TW / DI_THREADS; ++it) {
        const int o = it * DI_THREADS + tid;
        const int yy = o / DI_TW, c = o % DI_TW;
        if (yy < th && c < tw) {
            const int y = y0 + yy;
            const int lo = ymin[y] - r0;
            float n = 0.0f, d = 0.0f;
            for (int k = 0; k < p.Ky; ++k) {
                const int rr = min(max(lo + k, 0), nrows - 1);
                const float w = wy[(long long)y * p.Ky + k];
                n = __fadd_rn(n, __fmul_rn(w, hn[rr][c]));
                d = __fadd_rn(d, __fmul_rn(w, hd[rr][c]));
            }
            const bool has = d > 0.0f;
            const float r = has ? __fdiv_rn(n, d) : -1.0f;
            R[((long long)b * p.H + y) * p.W + x0 + c] = r;
            if (has) {
                mn = fminf(mn, r);
                mx = fmaxf(mx, r);
                any = 1.0f;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        any = fmaxf(any, __shfl_xor(any, o, 64));
    }
    if ((tid & (L2D_WAVE - 1)) == 0) {
        red[tid / L2D_WAVE][0] = mn;
        red[tid / L2D_WAVE][1] = mx;
        red[tid / L2D_WAVE][2] = any;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < DI_WAVES; ++w) {
            mn = fminf(mn, red[w][0]);
            mx = fmaxf(mx, red[w][1]);
            any = fmaxf(any, red[w][2]);
        }
        float *q = partials + (((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 3;
        q[0] = mn;
        q[1] = mx;
        q[2] = any;
    }
}

// one lane = 8 consecutive pixels of one frame: two 16-byte loads of R, three 16-byte stores
__global__ __launch_bounds__(DI_THREADS) void depth_normalize_kernel(const float *__restrict__ R, const float *__restrict__ partials,
                                                                     h16 *__restrict__ out, int B, int HW, int npart, int flags,
                                                                     float fmn, float fmx) {
    __shared__ float red[DI_WAVES][3];
    __shared__ float rng[3];
    const int tid = threadIdx.x;
    const long long g = (long long)blockIdx.x * DI_THREADS + tid;
    const int per = HW >> 3;
    const bool live = g < (long long)B * per;
    const int b = live ? (int)(g / per) : 0;
    const int px = live ? (int)(g % per) * 8 : 0;

    // this lane's pixels: the loads are issued first, the reduction runs under them
    f32x4 r0 = {-1.0f, -1.0f, -1.0f, -1.0f}, r1 = r0;
    if (live) {
        const f32x4 *q = reinterpret_cast<const f32x4 *>(R + (long long)b * HW + px);
        r0 = q[0];
        r1 = q[1];
    }

    float mn = __builtin_inff(), mx = -1.0f, any = 0.0f;
    if (!(flags & DI_FIXED)) {
        for (int i = tid; i < npart; i += DI_THREADS) {
            mn = fminf(mn, partials[(long long)i * 3]);
            mx = fmaxf(mx, partials[(long long)i * 3 + 1]);
            any = fmaxf(any, partials[(long long)i * 3 + 2]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o, 64));
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            any = fmaxf(any, __shfl_xor(any, o, 64));
        }
        if ((tid & (L2D_WAVE - 1)) == 0) {
            red[tid / L2D_WAVE][0] = mn;
            red[tid / L2D_WAVE][1] = mx;
            red[tid / L2D_WAVE][2] = any;
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (flags & DI_FIXED) {
            mn = fmn;
            mx = fmx;
            any = 1.0f;
        } else {
#pragma unroll
            for (int w = 1; w < DI_WAVES; ++w) {
                mn = fminf(mn, red[w][0]);
                mx = fmaxf(mx, red[w][1]);
                any = fmaxf(any, red[w][2]);
            }
        }
        const float span = __fsub_rn(mx, mn);
        // (the margin is for the range the frame itself gives: a caller's fixed range, however narrow, is taken at its word)
        const bool ok = (flags & DI_FIXED) ? mx > mn : (any > 0.0f && span > __fmul_rn(mx, DI_FLAT));
        rng[0] = mn;
        rng[1] = span;
        rng[2] = ok ? 1.0f : 0.0f;
    }
    __syncthreads();
    if (!live) return;
    const float lo = rng[0], span = rng[1];
    const bool ok = rng[2] != 0.0f;
    h16x8 y;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = e < 4 ? r0[e & 3] : r1[e & 3];
        float n = 0.0f;
        if (ok && v >= 0.0f) {
            n = __fdiv_rn(__fsub_rn(v, lo), span);
            n = fminf(fmaxf(n, 0.0f), 1.0f);
        }
        y[e] = (h16)__fsub_rn(__fmul_rn(2.0f, n), 1.0f);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) l2d_st8(out + ((long long)b * 3 + ch) * HW + px, y);
}

int l2d_launch_depth_ingest(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], Hd = op->i[1], Wd = op->i[2], H = op->i[3], W = op->i[4];
    const int nh = op->i[5], nw = op->i[6], top = op->i[7], left = op->i[8], Kx = op->i[9], Ky = op->i[10], flags = op->i[11];
    for (int k = 0; k < 7; ++k) {
        if (!op->p[k]) {
            l2d_set_error("depth_ingest(tag %d): invalid arguments (pointer %d is null)", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if (B <= 0 || Hd <= 0 || Wd <= 0 || H <= 0 || W <= 0 || nh <= 0 || nw <= 0) {
        l2d_set_error("depth_ingest(tag %d): invalid arguments (non-positive size: B = %d, source %d x %d, output %d x %d, resized %d x %d)",
                      op->tag, B, Hd, Wd, H, W, nh, nw);
        return L2D_EINVAL;
    }
    if (flags & ~(DI_F32 | DI_DISTANCE | DI_HAS_INVALID)) {
        l2d_set_error("depth_ingest(tag %d): unknown flag bits 0x%x (1 fp32, 2 distance, 4 invalid value)", op->tag, flags);
        return L2D_EINVAL;
    }
    if ((((uintptr_t)op->p[0]) & ((flags & DI_F32) ? 3 : 1)) || (((uintptr_t)op->p[1]) & 15)) {
        l2d_set_error("depth_ingest(tag %d): the source is not aligned to its element, or R not to 16 bytes", op->tag);
        return L2D_EINVAL;
    }
    for (int k = 2; k < 7; ++k) {
        if (((uintptr_t)op->p[k]) & 3) {
            l2d_set_error("depth_ingest(tag %d): pointer %d is not 4-byte aligned", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if ((long long)B * Hd * Wd >= (1ll << 31) || (long long)B * H * W >= (1ll << 31) || B > 65535) {
        l2d_set_error("depth_ingest(tag %d): B Hd Wd and B H W must stay below 2^31, B below 65536", op->tag);
        return L2D_EINVAL;
    }
    if (top < 0 || left < 0 || (long long)top + H > nh || (long long)left + W > nw) {
        l2d_set_error("depth_ingest(tag %d): crop window (top %d, left %d, %d x %d) lies outside the resized image %d x %d", op->tag, top,
                      left, H, W, nh, nw);
        return L2D_EINVAL;
    }
    const float sy = (float)Hd / (float)nh, sx = (float)Wd / (float)nw;
    if (sy > 8.0f || sx > 8.0f) {
        l2d_set_error("depth_ingest(tag %d): scale %.3f x %.3f exceeds 8 (17 taps per axis)", op->tag, sy, sx);
        return L2D_EINVAL;
    }
    if (Kx < 1 || Ky < 1 || Kx > DI_MAX_K || Ky > DI_MAX_K) {
        l2d_set_error("depth_ingest(tag %d): %d x %d taps, need 1..%d per axis", op->tag, Ky, Kx, DI_MAX_K);
        return L2D_EINVAL;
    }
    if ((flags & DI_HAS_INVALID) && !(flags & DI_F32) && (op->i[12] < 0 || op->i[12] > 65535)) {
        l2d_set_error("depth_ingest(tag %d): invalid = %d is no uint16 value", op->tag, op->i[12]);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    di_params p;
    p.B = B, p.Hd = Hd, p.Wd = Wd, p.H = H, p.W = W, p.Kx = Kx, p.Ky = Ky, p.flags = flags;
    p.invalid_u16 = op->i[12];
    p.invalid_f32 = op->f[0];
    const dim3 grid((unsigned)((W + DI_TW - 1) / DI_TW), (unsigned)((H + DI_TH - 1) / DI_TH), (unsigned)B);
    hipLaunchKernelGGL(depth_ingest_kernel, grid, dim3(DI_THREADS), 0, s, (const void *)op->p[0], (float *)op->p[1], (float *)op->p[2],
                       (const int *)op->p[3], (const float *)op->p[4], (const int *)op->p[5], (const float *)op->p[6], p);
    return l2d_check_launch("depth_ingest", op->tag);
}

int l2d_launch_depth_normalize(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], H = op->i[1], W = op->i[2], npart = op->i[3], flags = op->i[4];
    for (int k = 0; k < 3; ++k) {
        if (!op->p[k]) {
            l2d_set_error("depth_normalize(tag %d): invalid arguments (pointer %d is null)", op->tag, k);
            return L2D_EINVAL;
        }
        if (((uintptr_t)op->p[k]) & (k == 1 ? 3 : 15)) {
            l2d_set_error("depth_normalize(tag %d): pointer %d is not aligned (R and the output 16 bytes, the partials 4)", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if (B <= 0 || H <= 0 || W <= 0) {
        l2d_set_error("depth_normalize(tag %d): invalid arguments (non-positive size: B = %d, %d x %d)", op->tag, B, H, W);
        return L2D_EINVAL;
    }
    const long long HW = (long long)H * W;
    if (HW % 8) {
        l2d_set_error("depth_normalize(tag %d): H W = %lld is not a multiple of 8 (a lane stores 8 pixels)", op->tag, HW);
        return L2D_EINVAL;
    }
    if ((long long)B * HW * 3 >= (1ll << 31)) {
        l2d_set_error("depth_normalize(tag %d): B H W 3 must stay below 2^31", op->tag);
        return L2D_EINVAL;
    }
    if (flags & ~DI_FIXED) {
        l2d_set_error("depth_normalize(tag %d): unknown flag bits 0x%x (8 fixed range)", op->tag, flags);
        return L2D_EINVAL;
    }
    const long long want = (long long)B * ((H + DI_TH - 1) / DI_TH) * ((W + DI_TW - 1) / DI_TW);
    if (npart != want) {
        l2d_set_error("depth_normalize(tag %d): %d partials, B = %d frames of %d x %d have %lld tiles", op->tag, npart, B, H, W, want);
        return L2D_EINVAL;
    }
    if ((flags & DI_FIXED) && (op->f[0] != op->f[0] || op->f[1] != op->f[1])) {
        l2d_set_error("depth_normalize(tag %d): the fixed range holds a NaN", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const long long total = (long long)B * (HW / 8);
    hipLaunchKernelGGL(depth_normalize_kernel, dim3((unsigned)((total + DI_THREADS - 1) / DI_THREADS)), dim3(DI_THREADS), 0, s,
                       (const float *)op->p[0], (const float *)op->p[1], (h16 *)op->p[2], B, (int)HW, npart, flags, op->f[0], op->f[1]);
    return l2d_check_launch("depth_normalize", op->tag);
}
