// The frame's way in and out of the device: what the reference's callers do on the host around
// `wrapper(image)` -- `Resize(min(h, w), antialias=True)` + `CenterCrop` + `x / 255` on the way in (test.py:106-112, with
// `2 x - 1` from VaeImageProcessor), `x / 2 + 0.5 -> clamp -> x 255 -> round -> uint8` on the way out
// (image_utils.py:9-37) -- as one launch each on uint8 frames.  Both are launch-bound (6 MB in for 1080p, 0.75 MB out for
// 512 x 512): no LDS, no MFMA, 16-byte stores.
#include "frame_px.h"

#define FIO_MAX_SCALE 8.0f        // 2 * 8 + 1 = 17 taps per axis at most

// torch's antialiased bilinear filter along one axis (aten UpSampleKernel.cpp, _compute_indices_min_size_weights_aa): output index
// i of n_out samples the input with a triangle of half-width max(scale, 1) around scale * (i + 0.5).
struct fio_axis {
    float c, inv, rsum;       // centre, 1 / support, 1 / (sum of the raw weights)
    int lo, n;                // first tap, number of taps (lo >= 0, lo + n <= n_in)
};

__device__ __forceinline__ float fio_w(const fio_axis &a, int j) {
    const float w = 1.0f - fabsf(((float)(j + a.lo) - a.c + 0.5f) * a.inv);
    return w < 0.f ? 0.f : w;
}

__device__ __forceinline__ fio_axis fio_make_axis(int i, float scale, int n_in) {
    fio_axis a;
    const float support = scale > 1.0f ? scale : 1.0f;
    a.inv = 1.0f / support;
    a.c = scale * ((float)i + 0.5f);
    int lo = (int)(a.c - support + 0.5f), hi = (int)(a.c + support + 0.5f);
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_in ? n_in : hi;
    a.lo = lo;
    a.n = hi - lo;
    float s = 0.f;
    for (int j = 0; j < a.n; ++j) s += fio_w(a, j);
    a.rsum = 1.0f / s;
    return a;
}

// uint8 [B][Hs][Ws][3] -> fp16 [B][3][H][W]: the (top, left, H, W) window of the image resized to (nh, nw), mapped to [-1, 1].
// One lane = 8 consecutive x of one channel plane and one row.
__global__ __launch_bounds__(256) void frame_ingest_kernel(const uint8_t *__restrict__ src, h16 *__restrict__ dst, int B, int Hs, int Ws,
                                                           int H, int W, float sy, float sx, int top, int left) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int w8 = W >> 3;
    const long long total = (long long)B * 3 * H * w8;
    if (idx >= total) return;
    const int xg = (int)(idx % w8);
    long long r = idx / w8;
    const int y = (int)(r % H);
    r /= H;
    const int c = (int)(r % 3), b = (int)(r / 3);

    const fio_axis ay = fio_make_axis(y + top, sy, Hs);
    fio_axis ax[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) ax[e] = fio_make_axis(xg * 8 + e + left, sx, Ws);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    const uint8_t *img = src + (long long)b * Hs * Ws * 3 + c;
    for (int k = 0; k < ay.n; ++k) {
        const float wy = fio_w(ay, k) * ay.rsum;
        const uint8_t *row = img + (long long)(ay.lo + k) * Ws * 3;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint8_t *p = row + ax[e].lo * 3;
            float s = 0.f;
            for (int j = 0; j < ax[e].n; ++j) s = fmaf(fio_w(ax[e], j) * ax[e].rsum, (float)p[j * 3], s);
            acc[e] = fmaf(wy, s, acc[e]);
        }
    }
    h16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (h16)(acc[e] * (2.0f / 255.0f) - 1.0f);
    l2d_st8(dst + (((long long)b * 3 + c) * H + y) * W + xg * 8, o);
}

int l2d_launch_frame_ingest(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], Hs = op->i[1], Ws = op->i[2], H = op->i[3], W = op->i[4];
    const int nh = op->i[5], nw = op->i[6], top = op->i[7], left = op->i[8];
    if (!op->p[0] || !op->p[1] || B <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || nh <= 0 || nw <= 0) {
        l2d_set_error("frame_ingest(tag %d): invalid arguments (null pointer or non-positive size)", op->tag);
        return L2D_EINVAL;
    }
    if (W % 8) {
        l2d_set_error("frame_ingest(tag %d): W = %d is not a multiple of 8 (a lane stores 8 pixels)", op->tag, W);
        return L2D_EINVAL;
    }
    if (((uintptr_t)op->p[1]) & 15) {
        l2d_set_error("frame_ingest(tag %d): dst is not 16-byte aligned", op->tag);
        return L2D_EINVAL;
    }
    if ((long long)B * Hs * Ws * 3 >= (1ll << 31)) {
        l2d_set_error("frame_ingest(tag %d): source of %lld bytes is too large (B Hs Ws 3 must stay below 2^31)", op->tag,
                      (long long)B * Hs * Ws * 3);
        return L2D_EINVAL;
    }
    if (top < 0 || left < 0 || (long long)top + H > nh || (long long)left + W > nw) {
        l2d_set_error("frame_ingest(tag %d): crop window (top %d, left %d, %d x %d) lies outside the resized image %d x %d", op->tag, top,
                      left, H, W, nh, nw);
        return L2D_EINVAL;
    }
    const float sy = (float)Hs / (float)nh, sx = (float)Ws / (float)nw;
    if (sy > FIO_MAX_SCALE || sx > FIO_MAX_SCALE) {
        l2d_set_error("frame_ingest(tag %d): scale %.3f x %.3f exceeds 8 (17 taps per axis)", op->tag, sy, sx);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const long long total = (long long)B * 3 * H * (W / 8);
    hipLaunchKernelGGL(frame_ingest_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const uint8_t *)op->p[0],
                       (h16 *)op->p[1], B, Hs, Ws, H, W, sy, sx, top, left);
    return l2d_check_launch("frame_ingest", op->tag);
}

// fp16 [B][3][HW] -> uint8 [B][HW][3]: u = rint(255 clamp(fp16(fp16(x / 2) + 0.5), 0, 1)), the reference's expression on an fp16 tensor
// with its rounding points (frame_px.h px_byte).  One lane = 16 pixels = 48 bytes, three 16-byte stores.
__global__ __launch_bounds__(256) void frame_egress_kernel(const h16 *__restrict__ src, uint8_t *__restrict__ dst, int B, int HW) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int per = HW >> 4;
    if (idx >= (long long)B * per) return;
    const int b = (int)(idx / per);
    const int p0 = (int)(idx % per) * 16;
    const h16 *pl = src + (long long)b * 3 * HW + p0;
    unsigned char q[48];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const h16x8 v0 = l2d_ld8(pl + (long long)c * HW), v1 = l2d_ld8(pl + (long long)c * HW + 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            q[e * 3 + c] = (unsigned char)px_byte(v0[e]);
            q[(e + 8) * 3 + c] = (unsigned char)px_byte(v1[e]);
        }
    }
    uint4 *out = reinterpret_cast<uint4 *>(dst + ((long long)b * HW + p0) * 3);
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        unsigned wd[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int o = v * 16 + u * 4;
            wd[u] = (unsigned)q[o] | ((unsigned)q[o + 1] << 8) | ((unsigned)q[o + 2] << 16) | ((unsigned)q[o + 3] << 24);
        }
        out[v] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
}

int l2d_launch_frame_egress(const l2d_op *op, hipStream_t s) {
    const int B = op->i[0], H = op->i[1], W = op->i[2];
    if (!op->p[0] || !op->p[1] || B <= 0 || H <= 0 || W <= 0) {
        l2d_set_error("frame_egress(tag %d): invalid arguments (null pointer or non-positive size)", op->tag);
        return L2D_EINVAL;
    }
    const long long HW = (long long)H * W;
    if (HW % 16) {
        l2d_set_error("frame_egress(tag %d): H W = %lld is not a multiple of 16 (a lane stores 16 pixels)", op->tag, HW);
        return L2D_EINVAL;
    }
    if ((((uintptr_t)op->p[0]) & 15) || (((uintptr_t)op->p[1]) & 15)) {
        l2d_set_error("frame_egress(tag %d): src / dst is not 16-byte aligned", op->tag);
        return L2D_EINVAL;
    }
    if ((long long)B * HW * 3 >= (1ll << 31)) {
        l2d_set_error("frame_egress(tag %d): B H W 3 must stay below 2^31", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const long long total = (long long)B * (HW / 16);
    hipLaunchKernelGGL(frame_egress_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const h16 *)op->p[0],
                       (uint8_t *)op->p[1], B, (int)HW);
    return l2d_check_launch("frame_egress", op->tag);
}
