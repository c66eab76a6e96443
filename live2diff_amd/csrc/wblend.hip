// Style switch / style blend over a whole packed weight set in ONE launch: dst_t = sum_k a_k src_{k,t} for
// every tensor t of a set of ~700 separate allocations of mixed dtype, a few hundred bytes to 59 MB each.  The reference has no
// counterpart: it changes style by building a new wrapper (wrapper.py:404-470) and a new TensorRT engine.
//
// A pure HBM stream: no LDS, no MFMA.  The host cuts every tensor into tiles of at most L2D_WBLEND_TILE_BYTES and writes one record per
// tile (l2d_wblend_rec, include/l2d.h); a work-group walks records blockIdx.x, blockIdx.x + gridDim.x, ... so the launch count does
// not depend on the number of tensors, and a lane keeps WB_UNROLL x K 16-byte loads in flight.
//
// The arithmetic is fixed so that numpy restates it bit for bit (style_bank.blend_ref): acc = a_0 s_0, then acc = acc + a_k s_k in
// source order, every product and every sum rounded to fp32 on its own, one round-to-nearest-even to the tensor's dtype at the end.
#include <math.h>

#include "common.h"

// (built with -ffp-contract=off, see the Makefile: a fused multiply-add would differ from the numpy restatement)

#define WB_THREADS 256
#define WB_UNROLL 4
#define WB_MAX_BLOCKS 4096

typedef unsigned __attribute__((ext_vector_type(4))) wb_u4;
// the pointers come out of a record in memory: say that they are global, or every access is a flat one
#define WB_GLOBAL __attribute__((address_space(1)))
typedef WB_GLOBAL wb_u4 *wb_gptr;
typedef const WB_GLOBAL wb_u4 *wb_cgptr;

struct wb_weights {
    float a[L2D_WBLEND_MAX_SRC];
};

template <bool NT>
__device__ __forceinline__ wb_u4 wb_ld16(wb_cgptr p) {
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}

template <bool NT>
__device__ __forceinline__ void wb_st16(wb_gptr p, wb_u4 v) {
    if (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

__device__ __forceinline__ float wb_h2f(unsigned short bits) {
    h16 h;
    __builtin_memcpy(&h, &bits, 2);
    return (float)h;
}

__device__ __forceinline__ unsigned short wb_f2h(float x) {
    const h16 h = (h16)x;          // round to nearest even
    unsigned short bits;
    __builtin_memcpy(&bits, &h, 2);
    return bits;
}

template <int K>
__device__ __forceinline__ float wb_mix(const float (&s)[K], const wb_weights &w) {
    float acc = __fmul_rn(w.a[0], s[0]);
#pragma unroll
    for (int k = 1; k < K; ++k) acc = __fadd_rn(acc, __fmul_rn(w.a[k], s[k]));
    return acc;
}

// 16 bytes of every source -> 16 bytes of the destination
template <int K>
__device__ __forceinline__ wb_u4 wb_mix16(const wb_u4 (&v)[K], const wb_weights &w, int dtype) {
    unsigned in[K][4], out[4];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        in[k][0] = v[k].x; in[k][1] = v[k].y; in[k][2] = v[k].z; in[k][3] = v[k].w;
    }
    if (dtype == L2D_WBLEND_F32) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float s[K];
#pragma unroll
            for (int k = 0; k < K; ++k) s[k] = __uint_as_float(in[k][e]);
            out[e] = __float_as_uint(wb_mix<K>(s, w));
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float lo[K], hi[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                lo[k] = wb_h2f((unsigned short)(in[k][e] & 0xffffu));
                hi[k] = wb_h2f((unsigned short)(in[k][e] >> 16));
            }
            out[e] = (unsigned)wb_f2h(wb_mix<K>(lo, w)) | ((unsigned)wb_f2h(wb_mix<K>(hi, w)) << 16);
        }
    }
    wb_u4 o;
    o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
    return o;
}

template <int K, bool NT>
__global__ __launch_bounds__(WB_THREADS) void wblend_kernel(const l2d_wblend_rec *__restrict__ recs, int n_rec, wb_weights w) {
    for (int r = blockIdx.x; r < n_rec; r += gridDim.x) {
        const l2d_wblend_rec rec = recs[r];          // uniform per work-group
        const int dtype = rec.dtype;
        const int n = (int)rec.n;                    // <= L2D_WBLEND_TILE_BYTES / element size (the launcher checks)
        const int sh = dtype == L2D_WBLEND_F32 ? 2 : 3;   // 4 or 8 elements per 16-byte vector
        const int nvec = n >> sh;
        // K = 1 with weight 1 moves the bits as they are: 1 * x would quieten a signalling NaN (packed tensors may carry padding that
        // was never initialised), and a switch is to leave the destination bit-identical to its source
        const bool copy = K == 1 && w.a[0] == 1.0f;
        wb_gptr dst = (wb_gptr)rec.dst;
        wb_cgptr src[K];
#pragma unroll
        for (int k = 0; k < K; ++k) src[k] = (wb_cgptr)rec.src[k];

        for (int base = threadIdx.x; base < nvec; base += WB_THREADS * WB_UNROLL) {
            wb_u4 v[WB_UNROLL][K];
#pragma unroll
            for (int u = 0; u < WB_UNROLL; ++u) {
                const int i = base + u * WB_THREADS;
                if (i < nvec) {
#pragma unroll
                    for (int k = 0; k < K; ++k) v[u][k] = wb_ld16<NT>(src[k] + i);
                }
            }
#pragma unroll
            for (int u = 0; u < WB_UNROLL; ++u) {
                const int i = base + u * WB_THREADS;
                if (i < nvec) wb_st16<NT>(dst + i, copy ? v[u][0] : wb_mix16<K>(v[u], w, dtype));
            }
        }
        // the tail that is no whole 16-byte vector: at most 7 elements, one lane each
        const int done = nvec << sh, tail = n - done;
        if ((int)threadIdx.x < tail) {
            const int e = done + threadIdx.x;
            float s[K];
            if (copy && dtype == L2D_WBLEND_F32) {
                ((WB_GLOBAL unsigned *)rec.dst)[e] = ((const WB_GLOBAL unsigned *)rec.src[0])[e];
            } else if (copy) {
                ((WB_GLOBAL unsigned short *)rec.dst)[e] = ((const WB_GLOBAL unsigned short *)rec.src[0])[e];
            } else if (dtype == L2D_WBLEND_F32) {
#pragma unroll
                for (int k = 0; k < K; ++k) s[k] = ((const WB_GLOBAL float *)rec.src[k])[e];
                ((WB_GLOBAL float *)rec.dst)[e] = wb_mix<K>(s, w);
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k) s[k] = wb_h2f(((const WB_GLOBAL unsigned short *)rec.src[k])[e]);
                ((WB_GLOBAL unsigned short *)rec.dst)[e] = wb_f2h(wb_mix<K>(s, w));
            }
        }
    }
}

template <int K>
static void wb_launch(bool nt, int grid, hipStream_t s, const l2d_wblend_rec *recs, int n_rec, const wb_weights &w) {
    if (nt)
        hipLaunchKernelGGL((wblend_kernel<K, true>), dim3(grid), dim3(WB_THREADS), 0, s, recs, n_rec, w);
    else
        hipLaunchKernelGGL((wblend_kernel<K, false>), dim3(grid), dim3(WB_THREADS), 0, s, recs, n_rec, w);
}

int l2d_launch_weight_blend(const l2d_op *op, hipStream_t s) {
    const l2d_wblend_rec *dev = (const l2d_wblend_rec *)op->p[0], *host = (const l2d_wblend_rec *)op->p[1];
    const int n_rec = op->i[0], K = op->i[1], nt = op->i[2];
    if (!dev || !host || n_rec <= 0) {
        l2d_set_error("weight_blend(tag %d): invalid arguments (null table or no records)", op->tag);
        return L2D_EINVAL;
    }
    if (((uintptr_t)dev) & 15) {
        l2d_set_error("weight_blend(tag %d): the device table is not 16-byte aligned", op->tag);
        return L2D_EINVAL;
    }
    if (K < 1 || K > L2D_WBLEND_MAX_SRC) {
        l2d_set_error("weight_blend(tag %d): K = %d sources, need 1..%d", op->tag, K, L2D_WBLEND_MAX_SRC);
        return L2D_EINVAL;
    }
    if (nt != 0 && nt != 1) {
        l2d_set_error("weight_blend(tag %d): cache policy %d, need 0 (plain) or 1 (non-temporal)", op->tag, nt);
        return L2D_EINVAL;
    }
    wb_weights w;
    for (int k = 0; k < L2D_WBLEND_MAX_SRC; ++k) w.a[k] = k < K ? op->f[k] : 0.f;
    for (int k = 0; k < K; ++k) {
        if (!isfinite(w.a[k])) {
            l2d_set_error("weight_blend(tag %d): weight %d is not finite", op->tag, k);
            return L2D_EINVAL;
        }
    }
    for (int r = 0; r < n_rec; ++r) {
        const l2d_wblend_rec &c = host[r];
        if (c.dtype != L2D_WBLEND_F16 && c.dtype != L2D_WBLEND_F32) {
            l2d_set_error("weight_blend(tag %d): record %d has unknown dtype %d (0 fp16, 1 fp32)", op->tag, r, c.dtype);
            return L2D_EINVAL;
        }
        const long long esize = c.dtype == L2D_WBLEND_F32 ? 4 : 2;
        if (c.n <= 0 || c.n * esize > L2D_WBLEND_TILE_BYTES) {
            l2d_set_error("weight_blend(tag %d): record %d has %lld elements, need 1..%lld (a tile holds at most %d bytes)", op->tag, r,
                          (long long)c.n, (long long)(L2D_WBLEND_TILE_BYTES / esize), L2D_WBLEND_TILE_BYTES);
            return L2D_EINVAL;
        }
        if (!c.dst) {
            l2d_set_error("weight_blend(tag %d): record %d has a null dst", op->tag, r);
            return L2D_EINVAL;
        }
        if (((uintptr_t)c.dst) & 15) {
            l2d_set_error("weight_blend(tag %d): record %d: dst is not 16-byte aligned", op->tag, r);
            return L2D_EINVAL;
        }
        for (int k = 0; k < K; ++k) {
            if (!c.src[k]) {
                l2d_set_error("weight_blend(tag %d): record %d has a null src %d", op->tag, r, k);
                return L2D_EINVAL;
            }
            if (((uintptr_t)c.src[k]) & 15) {
                l2d_set_error("weight_blend(tag %d): record %d: src %d is not 16-byte aligned", op->tag, r, k);
                return L2D_EINVAL;
            }
        }
    }
    L2D_DRY_RETURN();
    const int grid = n_rec < WB_MAX_BLOCKS ? n_rec : WB_MAX_BLOCKS;
    switch (K) {
        case 1: wb_launch<1>(nt != 0, grid, s, dev, n_rec, w); break;
        case 2: wb_launch<2>(nt != 0, grid, s, dev, n_rec, w); break;
        case 3: wb_launch<3>(nt != 0, grid, s, dev, n_rec, w); break;
        default: wb_launch<4>(nt != 0, grid, s, dev, n_rec, w); break;
    }
    return l2d_check_launch("weight_blend", op->tag);
}
