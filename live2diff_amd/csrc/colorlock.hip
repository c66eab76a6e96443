// Colour lock: the decoded frame's per-channel mean and standard deviation -- of the BYTES a viewer sees --
// held to a target (the frame's own source, a running average, a reference image) by one gain and one offset per channel, on the
// device, in front of every outlet (L2D_OP_FRAME_EGRESS, L2D_OP_FRAME_MATTE, the JPEG encoder).  The reference has no counterpart.
// Two launches:
//
//   L2D_OP_FRAME_MOMENTS   b = rint(255 clamp(fp16(fp16(x / 2) + 0.5), 0, 1)), the egress op's byte; per channel S1 = sum b and
//                          S2 = sum b^2 over a block's CL_MOM_PIX pixels as u32 (4096 x 255^2 < 2^32), six plain stores per block
//                          into a partials buffer.  Integers: the sums do not depend on the order of anything; nothing is zeroed
//                          between frames and there is no atomic.
//   L2D_OP_COLOR_LOCK      every block adds the partials up in u64 and derives, redundantly, in fp64:
//                            mean = S1 / n, var = (n S2 - S1^2) / n^2       (integers exact in int64 for n <= 2^22)
//                            state' = moments of the second tensor | state | c, or t + beta (c - t)     (source | freeze | ema)
//                            g = sqrt(var_t / var_s) (1 if either is 0), clamped to [1/4, 4]; g = 1 + a (g - 1)
//                            m = mean_s + a (mean_t - mean_s); s32 = float(2 mean_s / 255 - 1), t32 = float(2 m / 255 - 1)
//                          then o = ((float(x) - s32) g32) + t32 in three fp32 operations, out = fp16(clamp(o, -1, 1)).
//                          Block 0 alone writes state' and the coefficient record.
//
// Every step is one operation with one rounding (the file is built with -ffp-contract=off, see the Makefile); fp64 division and
// square root are the correctly rounded IEEE ones, so numpy restates all of it bit for bit (live2diff_amd/color_lock.py).
// Latency-bound launches like the egress op: one trip over the data each, 16-byte loads, no MFMA.
#include <string.h>

#include "frame_px.h"

#define CL_THREADS 256
#define CL_WAVES (CL_THREADS / L2D_WAVE)
#define CL_MOM_PIX L2D_COLOR_LOCK_BLOCK_PIXELS        // pixels per block of the moments kernel: 2 x (256 lanes x 8 pixels)
#define CL_APPLY_PIX (CL_THREADS * 8)                 // pixels per block of the lock kernel: one 8-pixel group per lane and channel
#define CL_MAX_PIX L2D_COLOR_LOCK_MAX_PIXELS

#define CL_INIT L2D_COLOR_LOCK_INIT
#define CL_SOURCE L2D_COLOR_LOCK_SOURCE
#define CL_FREEZE L2D_COLOR_LOCK_FREEZE

static_assert((long long)CL_MOM_PIX * 255 * 255 < (1ll << 32), "a block's sum of squares must fit u32");
static_assert(CL_MOM_PIX % CL_APPLY_PIX == 0, "a moments block is a whole number of 8-pixel lane groups");

// grid (blocks, tensors): block (i, t) sums pixels [i CL_MOM_PIX, (i + 1) CL_MOM_PIX) of the three planes of tensor t and writes
// partials[t][i][0..5] = S1 of channel 0, 1, 2, S2 of channel 0, 1, 2
__global__ __launch_bounds__(CL_THREADS) void frame_moments_kernel(const h16 *__restrict__ a, const h16 *__restrict__ b,
                                                                   unsigned *__restrict__ partials, int HW, int nblk) {
    __shared__ unsigned red[CL_WAVES][6];
    const int tid = threadIdx.x;
    const h16 *src = blockIdx.y ? b : a;
    unsigned s[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int it = 0; it < CL_MOM_PIX / CL_APPLY_PIX; ++it) {
        const int p = blockIdx.x * CL_MOM_PIX + (it * CL_THREADS + tid) * 8;
        if (p < HW) {                                   // (p + 8 <= HW then: H W % 8 == 0)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const h16x8 v = l2d_ld8(src + (long long)ch * HW + p);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const unsigned q = px_byte(v[e]);
                    s[ch] += q;
                    s[3 + ch] += q * q;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += (unsigned)__shfl_xor((int)s[k], o, 64);
    }
    if ((tid & (L2D_WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[tid / L2D_WAVE][k] = s[k];
    }
    __syncthreads();
    if (tid < 6) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < CL_WAVES; ++w) t += red[w][tid];
        partials[((long long)blockIdx.y * nblk + blockIdx.x) * 6 + tid] = t;
    }
}

struct cl_params {
    double beta, a;
    int flags, nblk;
};

// (mean, var) of n pixels from the exact sums
__device__ __forceinline__ void cl_moments(unsigned long long S1, unsigned long long S2, long long n, double &mean, double &var) {
    const long long D = n * (long long)S2 - (long long)S1 * (long long)S1;
    mean = __ddiv_rn((double)(long long)S1, (double)n);
    var = __ddiv_rn((double)D, (double)(n * n));
}

__global__ __launch_bounds__(CL_THREADS) void color_lock_kernel(const h16 *__restrict__ styled, h16 *__restrict__ out,
                                                                const unsigned *__restrict__ partials, const double *__restrict__ state_in,
                                                                double *__restrict__ state_out, float *__restrict__ coef, int HW, cl_params p) {
    __shared__ unsigned long long red[CL_WAVES][12];
    __shared__ float cf[3][3];
    const int tid = threadIdx.x;
    const bool two = (p.flags & CL_SOURCE) != 0;

    // this lane's pixels: the loads are issued first, the reduction runs under them
    const int px = blockIdx.x * CL_APPLY_PIX + tid * 8;
    const bool live = px < HW;
    h16x8 x[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) x[ch] = live ? l2d_ld8(styled + (long long)ch * HW + px) : l2d_zero8();

    unsigned long long acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0ull;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (t == 0 || two) {
            for (int i = tid; i < p.nblk; i += CL_THREADS) {
                const unsigned *q = partials + ((long long)t * p.nblk + i) * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) acc[t * 6 + k] += q[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    if ((tid & (L2D_WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) red[tid / L2D_WAVE][k] = acc[k];
    }
    __syncthreads();
    if (tid < 3) {
        const int c = tid;
        unsigned long long S[4] = {0ull, 0ull, 0ull, 0ull};          // S1, S2 of the styled frame, S1, S2 of the second tensor
#pragma unroll
        for (int w = 0; w < CL_WAVES; ++w) {
            S[0] += red[w][c];
            S[1] += red[w][3 + c];
            S[2] += red[w][6 + c];
            S[3] += red[w][9 + c];
        }
        const long long n = HW;
        double mean_s, var_s, mean_t, var_t;
        cl_moments(S[0], S[1], n, mean_s, var_s);
        if (two) {
            cl_moments(S[2], S[3], n, mean_t, var_t);
        } else {
            mean_t = state_in[c * 2];
            var_t = state_in[c * 2 + 1];
            if (!(p.flags & CL_FREEZE)) {
                if (p.flags & CL_INIT) {
                    mean_t = mean_s;
                    var_t = var_s;
                } else {
                    mean_t = __dadd_rn(mean_t, __dmul_rn(p.beta, __dsub_rn(mean_s, mean_t)));
                    var_t = __dadd_rn(var_t, __dmul_rn(p.beta, __dsub_rn(var_s, var_t)));
                }
            }
        }
        double g = 1.0;
        if (var_s != 0.0 && var_t != 0.0) g = __dsqrt_rn(__ddiv_rn(var_t, var_s));
        g = fmin(fmax(g, 0.25), 4.0);
        g = __dadd_rn(1.0, __dmul_rn(p.a, __dsub_rn(g, 1.0)));
        const double m = __dadd_rn(mean_s, __dmul_rn(p.a, __dsub_rn(mean_t, mean_s)));
        const float g32 = (float)g;
        const float s32 = (float)__dsub_rn(__ddiv_rn(__dmul_rn(2.0, mean_s), 255.0), 1.0);
        const float t32 = (float)__dsub_rn(__ddiv_rn(__dmul_rn(2.0, m), 255.0), 1.0);
        cf[c][0] = g32;
        cf[c][1] = s32;
        cf[c][2] = t32;
        if (blockIdx.x == 0) {
            state_out[c * 2] = mean_t;
            state_out[c * 2 + 1] = var_t;
            coef[c * 3] = g32;
            coef[c * 3 + 1] = s32;
            coef[c * 3 + 2] = t32;
        }
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float g32 = cf[ch][0], s32 = cf[ch][1], t32 = cf[ch][2];
        h16x8 y;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float o = __fadd_rn(__fmul_rn(__fsub_rn((float)x[ch][e], s32), g32), t32);
            y[e] = (h16)fminf(fmaxf(o, -1.0f), 1.0f);
        }
        l2d_st8(out + (long long)ch * HW + px, y);
    }
}

// the checks both ops share; returns H W, or -1 with the error set
static long long cl_check_frame(const char *what, const l2d_op *op) {
    const int H = op->i[0], W = op->i[1];
    if (H <= 0 || W <= 0) {
        l2d_set_error("%s(tag %d): invalid arguments (non-positive size %d x %d)", what, op->tag, H, W);
        return -1;
    }
    const long long HW = (long long)H * W;
    if (W % 8 || HW % 16) {
        l2d_set_error("%s(tag %d): W = %d must be a multiple of 8 and H W = %lld a multiple of 16", what, op->tag, W, HW);
        return -1;
    }
    if (HW > CL_MAX_PIX) {
        l2d_set_error("%s(tag %d): H W = %lld is above %d pixels (n S2 - S1^2 must stay exact in int64)", what, op->tag, HW, CL_MAX_PIX);
        return -1;
    }
    if (op->i[3] != (int)((HW + CL_MOM_PIX - 1) / CL_MOM_PIX)) {
        l2d_set_error("%s(tag %d): %d partial blocks, H W = %lld needs ceil(H W / %d) = %lld", what, op->tag, op->i[3], HW, CL_MOM_PIX,
                      (HW + CL_MOM_PIX - 1) / CL_MOM_PIX);
        return -1;
    }
    return HW;
}

int l2d_launch_frame_moments(const l2d_op *op, hipStream_t s) {
    const long long HW = cl_check_frame("frame_moments", op);
    if (HW < 0) return L2D_EINVAL;
    const int nt = op->i[2], nblk = op->i[3];
    if (nt != 1 && nt != 2) {
        l2d_set_error("frame_moments(tag %d): %d tensors, need 1 or 2", op->tag, nt);
        return L2D_EINVAL;
    }
    if (!op->p[0] || !op->p[2] || (nt == 2) != (op->p[1] != nullptr)) {
        l2d_set_error("frame_moments(tag %d): invalid arguments (null pointer, or a second tensor that does not match i2 = %d)", op->tag, nt);
        return L2D_EINVAL;
    }
    for (int k = 0; k < 3; ++k) {
        if (((uintptr_t)op->p[k]) & 15) {
            l2d_set_error("frame_moments(tag %d): pointer %d is not 16-byte aligned", op->tag, k);
            return L2D_EINVAL;
        }
    }
    L2D_DRY_RETURN();
    hipLaunchKernelGGL(frame_moments_kernel, dim3((unsigned)nblk, (unsigned)nt), dim3(CL_THREADS), 0, s, (const h16 *)op->p[0],
                       (const h16 *)op->p[1], (unsigned *)op->p[2], (int)HW, nblk);
    return l2d_check_launch("frame_moments", op->tag);
}

int l2d_launch_color_lock(const l2d_op *op, hipStream_t s) {
    const long long HW = cl_check_frame("color_lock", op);
    if (HW < 0) return L2D_EINVAL;
    const int flags = op->i[2];
    for (int k = 0; k < 6; ++k) {
        if (!op->p[k]) {
            l2d_set_error("color_lock(tag %d): invalid arguments (pointer %d is null)", op->tag, k);
            return L2D_EINVAL;
        }
        if (((uintptr_t)op->p[k]) & (k < 3 ? 15 : (k < 5 ? 7 : 3))) {
            l2d_set_error("color_lock(tag %d): pointer %d is not aligned (frames and partials 16 bytes, states 8, coefficients 4)", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if (flags & ~(CL_INIT | CL_SOURCE | CL_FREEZE)) {
        l2d_set_error("color_lock(tag %d): unknown flag bits 0x%x (1 init, 2 source, 4 freeze)", op->tag, flags);
        return L2D_EINVAL;
    }
    if ((flags & CL_SOURCE) && (flags & CL_FREEZE)) {
        l2d_set_error("color_lock(tag %d): the source and freeze flags exclude one another", op->tag);
        return L2D_EINVAL;
    }
    if (px_overlap(op->p[3], 48, op->p[4], 48)) {
        l2d_set_error("color_lock(tag %d): state_in and state_out overlap (block 0 writes what the other blocks read)", op->tag);
        return L2D_EINVAL;
    }
    if (px_overlap(op->p[0], HW * 6, op->p[1], HW * 6)) {
        l2d_set_error("color_lock(tag %d): the output frame overlaps the input frame", op->tag);
        return L2D_EINVAL;
    }
    cl_params p;
    static_assert(sizeof(double) == sizeof(op->l[0]), "beta and a travel as the bits of a double");
    memcpy(&p.beta, &op->l[0], sizeof(double));
    memcpy(&p.a, &op->l[1], sizeof(double));
    if (!(p.beta > 0.0 && p.beta <= 1.0) || !(p.a >= 0.0 && p.a <= 1.0)) {
        l2d_set_error("color_lock(tag %d): rate = %g must lie in (0, 1] and strength = %g in [0, 1]", op->tag, p.beta, p.a);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    p.flags = flags;
    p.nblk = op->i[3];
    hipLaunchKernelGGL(color_lock_kernel, dim3((unsigned)((HW + CL_APPLY_PIX - 1) / CL_APPLY_PIX)), dim3(CL_THREADS), 0, s,
                       (const h16 *)op->p[0], (h16 *)op->p[1], (const unsigned *)op->p[2], (const double *)op->p[3], (double *)op->p[4],
                       (float *)op->p[5], (int)HW, p);
    return l2d_check_launch("color_lock", op->tag);
}
