// Mid-block attention of the SD AutoencoderKL (diffusers `Attention` with one head of d = 512, reached from the encoder's and
// the decoder's `UNetMidBlock2D`), and the posterior draw of its encoder (`DiagonalGaussianDistribution.sample`).
//
//   O[q][:] = softmax_k( Q[q].K[k] / sqrt(512) ) . V[k][:]        per sample, keys and queries = the h x w latent pixels
//
// Three launches per op, none of which leaves a T x T tensor in HBM:
//   * kl_attn_pack_kernel: K and V of one 32-key tile -> two 32 KB images in exactly the order the MFMA fragments are read
//     (the "swapped" form of flash_attn_ring.hip: S^T = K.Q^T, O^T += V^T.P^T with v_mfma_f32_16x16x32_f16, so P never
//     leaves registers).  V is transposed on the way (through LDS), keys beyond T are zero.  The key order inside a tile is
//     permuted so that the 8 scores a lane holds after QK^T are the 8 k slots of its PV B operand.  With the images
//     fragment-ordered, a fragment read is one conflict-free ds_read_b128 (consecutive lanes, consecutive 16 bytes) and a
//     tile is copied to LDS by plain lane-linear global_load_lds_dwordx4.
//   * kl_attn_kernel: a block owns 64 query rows (4 waves x 16) of one sample and a contiguous range of key tiles (a split).
//     Q stays in registers (64 VGPRs), O^T (16 x 512 per wave) in 128 fp32 accumulators per lane; the next tile's images are
//     DMA'd into the other half of a 2-stage LDS ring while the current one is consumed.  Scores and softmax statistics are
//     fp32, P is rounded to fp16 for the PV MFMA.  With one split the block writes the normalised output; otherwise it writes
//     its unnormalised O, running max and row sum (fp32) to the workspace.
//   * kl_attn_merge_kernel (splits > 1): out = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s, summed in split-index order:
//     the result does not depend on which block finished first, and every workspace word it reads was written by this op.
// Splits exist because at B = 1, T = 4096 there are only 64 query tiles for 256 CUs.
#include <math.h>

#include "common.h"

#define KA_GPTR(p) ((__attribute__((address_space(1))) const void *)(p))
#define KA_LPTR(p) ((__attribute__((address_space(3))) void *)(p))

namespace {
constexpr int KD = 512;                  // head size
constexpr int KB = 32;                   // keys per tile
constexpr int KQ = 64;                   // query rows per block: 4 waves x 16
constexpr int KIMG = KB * KD;            // halfs in one K (or V) tile image: 32 KB
constexpr int KLDS = 2 * 2 * KIMG * 2;   // bytes of LDS: two stages of (K image | V image)
constexpr int KMAXS = 16;                // most key splits per query tile

struct KAArgs {
    const h16 *qkv;   // [B*T][ld]: q | k | v at columns 0, 512, 1024
    h16 *img;         // [B][nt][K image | V image]
    h16 *out;         // [B*T][ldo]
    float *ws;        // splits > 1: O [S][B][nqt*64][512], then (m, l) [S][B][nqt*64][2]
    int B, T, ld, ldo, nt, nqt, S, tps;
    float c;          // softmax scale * log2(e)
};
}  // namespace

// keys of a tile in the order of a PV k slot: slot 8 g + j holds key 4 g + j (j < 4) or 16 + 4 g + j - 4 (j >= 4) -- the
// S^T accumulator of 16-key subtile ks gives lane group g the keys 16 ks + 4 g + r
__device__ __forceinline__ int ka_slot_key(int g, int j) { return j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4); }

__global__ __launch_bounds__(256) void kl_attn_pack_kernel(KAArgs a) {
    __shared__ __attribute__((aligned(16))) h16 vs[KB * (KD + 8)];      // the V tile [key][channel], rows padded by 16 bytes
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.nt, t = blockIdx.x % a.nt, key0 = t * KB;
    h16 *kimg = a.img + (size_t)blockIdx.x * 2 * KIMG, *vimg = kimg + KIMG;
    const h16 *src = a.qkv + (size_t)b * a.T * a.ld;
    // K image: chunk (ks 16 + kk) 64 + lane = K[key0 + 16 ks + lane % 16][32 kk + 8 (lane / 16) .. + 8]  (A operand of S^T)
#pragma unroll
    for (int i = 0; i < KIMG / 8 / 256; ++i) {
        const int ci = i * 256 + tid, lane = ci & 63, kk = (ci >> 6) & 15, ks = ci >> 10;
        const int key = key0 + 16 * ks + (lane & 15);
        const h16x8 v = key < a.T ? l2d_ld8(src + (size_t)key * a.ld + KD + 32 * kk + 8 * (lane >> 4)) : l2d_zero8();
        l2d_st8(kimg + (size_t)ci * 8, v);
    }
#pragma unroll
    for (int i = 0; i < KIMG / 8 / 256; ++i) {
        const int ci = i * 256 + tid, key = ci >> 6, c8 = ci & 63;
        const h16x8 v = key0 + key < a.T ? l2d_ld8(src + (size_t)(key0 + key) * a.ld + 2 * KD + 8 * c8) : l2d_zero8();
        l2d_st8(vs + key * (KD + 8) + 8 * c8, v);
    }
    __syncthreads();
    // V image: chunk ds 64 + lane, element j = V[key0 + ka_slot_key(lane / 16, j)][16 ds + lane % 16]  (A operand of O^T)
#pragma unroll
    for (int i = 0; i < KIMG / 8 / 256; ++i) {
        const int ci = i * 256 + tid, lane = ci & 63, ds = ci >> 6, g = lane >> 4, ch = 16 * ds + (lane & 15);
        h16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = vs[ka_slot_key(g, j) * (KD + 8) + ch];
        l2d_st8(vimg + (size_t)ci * 8, v);
    }
}

__global__ __launch_bounds__(256, 1) void kl_attn_kernel(KAArgs a) {
    extern __shared__ __attribute__((aligned(16))) h16 ka_smem[];     // the ONLY LDS object: [stage][K image | V image]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4;
    const int qt = blockIdx.x, sp = blockIdx.y, b = blockIdx.z;
    const int qrow = qt * KQ + wave * 16 + (lane & 15);              // this lane's query: a column of S^T and of O^T
    const int t0 = sp * a.tps, t1 = min(a.nt, t0 + a.tps);           // (the host leaves no split empty)
    const h16 *img = a.img + (size_t)b * a.nt * 2 * KIMG;

    // Q^T fragments (B operand of S^T = K Q^T), loaded before any DMA is in flight
    h16x8 qf[16];
    {
        const bool qv = qrow < a.T;
        const h16 *qp = a.qkv + ((size_t)b * a.T + (qv ? qrow : 0)) * a.ld + 8 * g;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) qf[kk] = qv ? l2d_ld8(qp + 32 * kk) : l2d_zero8();
    }
    // one tile = 64 KB = 16 lane-linear pieces of 4 KB; wave w's lanes fill bytes [1 KB w, 1 KB (w + 1)) of each piece
    auto issue = [&](int t, int stage) {
        const h16 *s = img + (size_t)t * 2 * KIMG + tid * 8;
        h16 *d = ka_smem + stage * 2 * KIMG + wave * 512;
#pragma unroll
        for (int i = 0; i < 2 * KIMG / 2048; ++i)
            __builtin_amdgcn_global_load_lds(KA_GPTR(s + i * 2048), KA_LPTR(d + i * 2048), 16, 0, 0);
    };

    f32x4 o[KD / 16];
#pragma unroll
    for (int ds = 0; ds < KD / 16; ++ds) o[ds] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;          // running maximum (log2 units, same in the 4 lanes of a query) and this lane's row-sum share

    issue(t0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const int stage = (t - t0) & 1;
        if (t + 1 < t1) issue(t + 1, stage ^ 1);      // into the stage everyone finished reading before the last barrier
        const h16 *ki = ka_smem + stage * 2 * KIMG, *vi = ki + KIMG;
        // S^T: two 16-key subtiles, two accumulator chains each (even / odd k steps)
        f32x4 s[2][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) s[ks][0] = s[ks][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const h16x8 kf = *reinterpret_cast<const h16x8 *>(ki + ((ks * 16 + kk) * 64 + lane) * 8);
                s[ks][kk & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[kk], s[ks][kk & 1], 0, 0, 0);
            }
        }
        float p[8], mx = -INFINITY;
        const int kbase = t * KB;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (s[ks][0][r] + s[ks][1][r]) * a.c;
                p[4 * ks + r] = kbase + 16 * ks + 4 * g + r < a.T ? v : -INFINITY;
                mx = fmaxf(mx, p[4 * ks + r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        h16x8 pf;
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float e = __builtin_amdgcn_exp2f(p[j] - mn);
            ps += e;
            pf[j] = (h16)e;
        }
        l = l * alpha + ps;
#pragma unroll
        for (int ds = 0; ds < KD / 16; ++ds) o[ds] *= alpha;
        // O^T += V^T P^T
#pragma unroll
        for (int ds = 0; ds < KD / 16; ++ds) {
            const h16x8 vf = *reinterpret_cast<const h16x8 *>(vi + (ds * 64 + lane) * 8);
            o[ds] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[ds], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's share of tile t + 1 landed
        __syncthreads();                                    // ... everyone's, and everyone is done with tile t
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (a.S == 1) {
        if (qrow < a.T) {
            const float inv = 1.0f / l;
            h16 *op = a.out + ((size_t)b * a.T + qrow) * a.ldo + 4 * g;
#pragma unroll
            for (int ds = 0; ds < KD / 16; ++ds) {
                h16x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (h16)(o[ds][r] * inv);
                *reinterpret_cast<h16x4 *>(op + 16 * ds) = v;
            }
        }
        return;
    }
    const size_t rows = (size_t)a.B * a.nqt * KQ, r = (size_t)sp * rows + (size_t)b * a.nqt * KQ + qrow;
    float *wo = a.ws + r * KD + 4 * g;
#pragma unroll
    for (int ds = 0; ds < KD / 16; ++ds) *reinterpret_cast<f32x4 *>(wo + 16 * ds) = o[ds];
    if (g == 0) *reinterpret_cast<f32x2 *>(a.ws + (size_t)a.S * rows * KD + 2 * r) = f32x2{m, l};
}

__global__ __launch_bounds__(256) void kl_attn_merge_kernel(KAArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), c8 = threadIdx.x & 63;
    if (row >= a.B * a.T) return;
    const int b = row / a.T, q = row - b * a.T;
    const size_t rows = (size_t)a.B * a.nqt * KQ, r0 = (size_t)b * a.nqt * KQ + q;
    const float *ml = a.ws + (size_t)a.S * rows * KD;
    float M = -INFINITY;
    for (int s = 0; s < a.S; ++s) M = fmaxf(M, ml[2 * (s * rows + r0)]);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, L = 0.f;
    for (int s = 0; s < a.S; ++s) {                          // split-index order
        const size_t r = s * rows + r0;
        const float w = __builtin_amdgcn_exp2f(ml[2 * r] - M);
        L += w * ml[2 * r + 1];
        const f32x4 *src = reinterpret_cast<const f32x4 *>(a.ws + r * KD + 8 * c8);
        const f32x4 v0 = src[0], v1 = src[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e] += w * v0[e];
            acc[4 + e] += w * v1[e];
        }
    }
    const float inv = 1.0f / L;
    h16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (h16)(acc[e] * inv);
    l2d_st8(a.out + (size_t)row * a.ldo + 8 * c8, v);
}

int l2d_launch_vae_attn(const l2d_op *op, hipStream_t s) {
    KAArgs a;
    a.qkv = (const h16 *)op->p[0];
    a.out = (h16 *)op->p[1];
    a.img = (h16 *)op->p[2];
    a.ws = (float *)op->p[3];
    a.B = op->i[0], a.T = op->i[1], a.ld = op->i[2], a.ldo = op->i[3], a.S = op->i[4];
    a.c = op->f[0] * 1.4426950408889634f;
    a.nt = (a.T + KB - 1) / KB;
    a.nqt = (a.T + KQ - 1) / KQ;
    a.tps = a.S > 0 ? (a.nt + a.S - 1) / a.S : 0;
    // 16-byte rows (ld, ldo % 8), every split non-empty, the workspace present when the splits are merged
    const bool ok = a.qkv && a.out && a.img && a.B >= 1 && a.T >= 1 && a.ld >= 3 * KD && (a.ld % 8) == 0 && a.ldo >= KD &&
                    (a.ldo % 8) == 0 && a.S >= 1 && a.S <= KMAXS && a.S <= a.nt && (a.S - 1) * a.tps < a.nt && (a.S == 1 || a.ws) &&
                    ((uintptr_t)a.qkv % 16) == 0 && ((uintptr_t)a.out % 16) == 0 && ((uintptr_t)a.img % 16) == 0 &&
                    ((uintptr_t)a.ws % 16) == 0 && (long long)a.B * a.T <= 0x7fffffffLL / 4;
    if (!ok) {
        l2d_set_error("vae_attn(tag %d): invalid arguments (B=%d T=%d ld=%d ldo=%d S=%d; d = 512, ld >= 1536 and ldo >= 512 multiples "
                      "of 8, 1 <= S <= min(16, ceil(T / 32)) with no empty split, 16-byte aligned buffers, a workspace when S > 1)",
                      op->tag, a.B, a.T, a.ld, a.ldo, a.S);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    static bool attr_done_dev[L2D_MAX_DEV] = {false};
    bool &attr_done = attr_done_dev[l2d_dev_ordinal()];
    if (!attr_done) {
        if (hipFuncSetAttribute((const void *)kl_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, KLDS) == hipSuccess)
            attr_done = true;
        else
            (void)hipGetLastError();
    }
    hipLaunchKernelGGL(kl_attn_pack_kernel, dim3(a.B * a.nt), dim3(256), 0, s, a);
    hipLaunchKernelGGL(kl_attn_kernel, dim3(a.nqt, a.S, a.B), dim3(256), KLDS, s, a);
    if (a.S > 1) hipLaunchKernelGGL(kl_attn_merge_kernel, dim3((a.B * a.T + 3) / 4), dim3(256), 0, s, a);
    return l2d_check_launch("vae_attn", op->tag);
}

// z = mean + exp(0.5 clamp(logvar, -30, 20)) eps  on the encoder's NCHW moments [B][8][HW] (mean = channels 0-3)
__global__ __launch_bounds__(256) void kl_posterior_kernel(const h16 *mom, const h16 *eps, h16 *out, int B, int HW) {
    const long long n = (long long)B * 4 * HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long bc = i / HW, p = i - bc * HW, b = bc >> 2, c = bc & 3;
        const h16 *mb = mom + (b * 8 + c) * HW + p;
        const float lv = fminf(fmaxf((float)mb[4 * (long long)HW], -30.f), 20.f);
        out[i] = (h16)((float)mb[0] + __builtin_amdgcn_exp2f(0.7213475204444817f * lv) * (float)eps[i]);
    }
}

int l2d_launch_vae_posterior(const l2d_op *op, hipStream_t s) {
    const h16 *mom = (const h16 *)op->p[0], *eps = (const h16 *)op->p[1];
    h16 *out = (h16 *)op->p[2];
    const int B = op->i[0], HW = op->i[1];
    if (!mom || !eps || !out || B < 1 || HW < 1) {
        l2d_set_error("vae_posterior(tag %d): invalid arguments (B=%d HW=%d)", op->tag, B, HW);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const long long n = (long long)B * 4 * HW;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(kl_posterior_kernel, dim3(blocks), dim3(256), 0, s, mom, eps, out, B, HW);
    return l2d_check_launch("vae_posterior", op->tag);
}
