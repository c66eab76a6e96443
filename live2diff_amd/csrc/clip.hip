// CLIP ViT-L/14 text tower on gfx950: the four kernels that turn token ids into the [B, 77, 768]
// embeddings the UNet's cross-attention reads.
//
// Replaces what the reference runs through transformers' CLIPTextModel inside AnimationDepthPipeline._encode_prompt
// (reference live2diff/animatediff/pipeline/pipeline_animatediff_depth.py:149-248): token + position embedding, 12 pre-LN
// blocks (x += out_proj(attn(LN1(x))); x += fc2(quick_gelu(fc1(LN2(x))))) with causal self-attention, final LayerNorm.
//
// The regime is small-M weight streaming: 77 tokens per prompt, B <= 4 prompts, 14 MB of fp16 weights per layer, every launch
// latency-bound.  One layer is five launches:
//   L2D_OP_CLIP_LINEAR  q|k|v   LayerNorm prologue on the fp32 residual stream, fp16 out
//   L2D_OP_CLIP_ATTN            causal attention, one block per (prompt, head), Q / K / V resident in LDS
//   L2D_OP_CLIP_LINEAR  out_proj  bias + residual add into the fp32 residual stream (in place)
//   L2D_OP_CLIP_LINEAR  fc1     LayerNorm prologue, bias + quick-GELU epilogue, fp16 out
//   L2D_OP_CLIP_LINEAR  fc2     K = 3072, bias + residual add (in place)
// plus L2D_OP_CLIP_EMBED in front and L2D_OP_CLIP_LN (final LayerNorm, fp32 in, fp16 out) behind.
//
// The residual stream is kept in fp32 (77 x 768 x 4 bytes per prompt): CLIP's residual carries a few channels two orders of
// magnitude above the rest, and an fp16 stream would round the small channels at every one of the 24 adds.  Everything the
// GEMMs consume is fp16 (normalised activations, attention output, MLP hidden), accumulation is fp32 on the matrix cores.
//
// clip_linear_kernel: out[m][n] = epi( sum_k pro(x)[m][k] W[n][k] + b[n] ) on v_mfma_f32_32x32x16_f16.  A block owns one tile of
// 32 output channels and MT tiles of 32 tokens; its NW waves split K (12 k steps of 16 per pass), each wave streams its share of the
// weight tile straight into registers (MFMA-fragment order, a 1 KB coalesced load per wave per k step: ops.pack_clip_linear), all
// twelve fragments of a pass requested before the first MFMA.  The activation fragment (16 bytes per lane, 32 rows x 32 bytes per
// wave) comes from L2; with the LayerNorm prologue it is read as fp32 and normalised on the way ((x - mean) rstd gamma + beta ->
// fp16), the row statistics having been taken by the block in front of the k loop (16 lanes per row, the row in registers,
// two-pass exact; K <= 1024).  The NW partial
// accumulators are summed through LDS in the fixed wave order 0..NW-1 (bit-repeatable), then the epilogue runs per element.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CLIP_STEPS 12       // k steps of 16 per wave and pass
#define CLIP_MAX_NW 8
#define CLIP_MAX_T 128      // attention: keys per prompt (two per lane)
#define CLIP_D 64           // attention head size

// ------------------------------------------------------------------------------------------------ token + position embedding
__global__ __launch_bounds__(256) void clip_embed_kernel(const long long *__restrict__ ids, const h16 *__restrict__ tok,
                                                         const h16 *__restrict__ pos, float *__restrict__ out, int rows, int T,
                                                         int C, long long V) {
    const int c8 = C >> 3;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)rows * c8) return;
    const int r = (int)(idx / c8), c = (int)(idx - (long long)r * c8) * 8;
    long long id = ids[r];
    if (id < 0 || id >= V) id = 0;           // (the host checks ids; this only keeps a bad id from reading out of bounds)
    const h16x8 a = l2d_ld8(tok + id * C + c), p = l2d_ld8(pos + (long long)(r % T) * C + c);
    f32x4 lo, hi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        lo[e] = (float)a[e] + (float)p[e];
        hi[e] = (float)a[e + 4] + (float)p[e + 4];
    }
    f32x4 *o = reinterpret_cast<f32x4 *>(out + (long long)r * C + c);
    o[0] = lo;
    o[1] = hi;
}

int l2d_launch_clip_embed(const l2d_op *op, hipStream_t s) {
    const long long *ids = (const long long *)op->p[0];
    const h16 *tok = (const h16 *)op->p[1], *pos = (const h16 *)op->p[2];
    float *out = (float *)op->p[3];
    const int rows = op->i[0], T = op->i[1], C = op->i[2], V = op->i[3], P = op->i[4];
    if (!ids || !tok || !pos || !out || rows <= 0 || T <= 0 || T > P || C <= 0 || (C % 8) || V <= 0 || rows % T) {
        l2d_set_error("clip_embed(tag %d): invalid arguments (rows=%d T=%d C=%d V=%d P=%d)", op->tag, rows, T, C, V, P);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const long long n = (long long)rows * (C / 8);
    hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, tok, pos, out, rows, T, C,
                       (long long)V);
    return l2d_check_launch("clip_embed", op->tag);
}

// ------------------------------------------------------------------------------------------------ LayerNorm, fp32 in, fp16 out
// one wave per row, the row held in registers (C <= 64 * 16): mean, then the centred sum of squares (exact two-pass statistics)
__global__ __launch_bounds__(256) void clip_ln_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                      const float *__restrict__ b, h16 *__restrict__ out, int rows, int C, int ldx,
                                                      int ldo, float eps) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float *xr = x + (long long)r * ldx;
    float v[16];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < C ? xr[c] : 0.f;
        s += v[j];
    }
    const float mean = l2d_wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = lane + 64 * j;
        const float d = c < C ? v[j] - mean : 0.f;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(l2d_wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = lane + 64 * j;
        if (c < C) out[(long long)r * ldo + c] = (h16)((v[j] - mean) * rstd * g[c] + b[c]);
    }
}

int l2d_launch_clip_ln(const l2d_op *op, hipStream_t s) {
    const float *x = (const float *)op->p[0], *g = (const float *)op->p[1], *b = (const float *)op->p[2];
    h16 *out = (h16 *)op->p[3];
    const int rows = op->i[0], C = op->i[1], ldx = op->i[2], ldo = op->i[3];
    if (!x || !g || !b || !out || rows <= 0 || C <= 0 || C > 1024 || ldx < C || ldo < C) {
        l2d_set_error("clip_ln(tag %d): invalid arguments (rows=%d C=%d ldx=%d ldo=%d)", op->tag, rows, C, ldx, ldo);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    hipLaunchKernelGGL(clip_ln_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, g, b, out, rows, C, ldx, ldo, op->f[0]);
    return l2d_check_launch("clip_ln", op->tag);
}

// ------------------------------------------------------------------------------------------------ causal attention
// One block (8 waves) per (prompt, head).  Q, K, V of the head ([T][64] each, fp16) are copied into LDS once; K rows are padded
// to 66 halfs so that 64 lanes reading 64 different keys at the same column hit 32 different banks.  Wave w owns the query rows
// w, w + 8, ...: lane j scores keys j and j + 64 (fp32 dot products), the row maximum / sum are wave reductions, the
// probabilities go through a per-wave LDS row, and lane d forms sum_j p_j V[j][d] for its head channel.  Every row is computed,
// the pad positions behind <|endoftext|> included (the UNet reads them).
#define CLIP_KLD 66
__global__ __launch_bounds__(512) void clip_attn_kernel(const h16 *__restrict__ qkv, h16 *__restrict__ out, int T, int H, int ldq,
                                                        int ldo, float scale, int causal) {
    __shared__ h16 qs[CLIP_MAX_T * CLIP_D];
    __shared__ h16 ks[CLIP_MAX_T * CLIP_KLD];
    __shared__ h16 vs[CLIP_MAX_T * CLIP_D];
    __shared__ float ps[8][CLIP_MAX_T];
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int C = H * CLIP_D;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const h16 *base = qkv + (long long)b * T * ldq + h * CLIP_D;
    for (int q = tid; q < T * 8; q += 512) {            // 8 pieces of 16 bytes per row and operand
        const int t = q >> 3, c = (q & 7) * 8;
        const h16 *row = base + (long long)t * ldq + c;
        l2d_st8(qs + t * CLIP_D + c, l2d_ld8(row));
        const h16x8 kv = l2d_ld8(row + C);
#pragma unroll
        for (int e = 0; e < 8; e += 2) *reinterpret_cast<h16x2 *>(ks + t * CLIP_KLD + c + e) = h16x2{kv[e], kv[e + 1]};
        l2d_st8(vs + t * CLIP_D + c, l2d_ld8(row + 2 * C));
    }
    __syncthreads();
    for (int i = wave; i < T; i += 8) {
        const int kmax = causal ? i + 1 : T;           // keys 0..kmax-1
        float sc[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = lane + 64 * u;
            float acc = 0.f;
            if (j < kmax) {
                const h16 *kr = ks + j * CLIP_KLD;
                const h16 *qr = qs + i * CLIP_D;
#pragma unroll 8
                for (int d = 0; d < CLIP_D; d += 2) {
                    const h16x2 kk = *reinterpret_cast<const h16x2 *>(kr + d);
                    const h16x2 qq = *reinterpret_cast<const h16x2 *>(qr + d);
                    acc = fmaf((float)qq[0], (float)kk[0], acc);
                    acc = fmaf((float)qq[1], (float)kk[1], acc);
                }
                sc[u] = acc * scale;
            } else {
                sc[u] = -INFINITY;
            }
        }
        const float mx = l2d_wave_max(fmaxf(sc[0], sc[1]));      // key 0 is always visible: mx is finite
        float p[2], sum = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            p[u] = lane + 64 * u < kmax ? expf(sc[u] - mx) : 0.f;
            sum += p[u];
        }
        sum = l2d_wave_sum(sum);
        ps[wave][lane] = p[0];
        ps[wave][lane + 64] = p[1];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        int j = 0;
        for (; j + 4 <= kmax; j += 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) o[u] = fmaf(ps[wave][j + u], (float)vs[(j + u) * CLIP_D + lane], o[u]);
        for (; j < kmax; ++j) o[0] = fmaf(ps[wave][j], (float)vs[j * CLIP_D + lane], o[0]);
        out[((long long)b * T + i) * ldo + h * CLIP_D + lane] = (h16)(((o[0] + o[1]) + (o[2] + o[3])) / sum);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

int l2d_launch_clip_attn(const l2d_op *op, hipStream_t s) {
    const h16 *qkv = (const h16 *)op->p[0];
    h16 *out = (h16 *)op->p[1];
    const int B = op->i[0], T = op->i[1], H = op->i[2], d = op->i[3], ldq = op->i[4], ldo = op->i[5], causal = op->i[6];
    if (!qkv || !out || B <= 0 || T <= 0 || T > CLIP_MAX_T || H <= 0 || d != CLIP_D || ldq < 3 * H * d || (ldq % 8) ||
        ldo < H * d || (causal != 0 && causal != 1)) {
        l2d_set_error("clip_attn(tag %d): invalid arguments (B=%d T=%d H=%d d=%d ldq=%d ldo=%d)", op->tag, B, T, H, d, ldq, ldo);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    hipLaunchKernelGGL(clip_attn_kernel, dim3(B * H), dim3(512), 0, s, qkv, out, T, H, ldq, ldo, op->f[0], causal);
    return l2d_check_launch("clip_attn", op->tag);
}

// ------------------------------------------------------------------------------------------------ small-M linear layer
struct ClipLinArgs {
    const void *x;
    const h16 *w;
    const float *bias, *gamma, *beta;
    void *out;
    int M, K, Nout, ldx, ldo, epi, npass;
    float eps;
};

// activation fragment of k step s for token row `row` (the lane's half of the 16 k values): 8 fp16 values
template <int PRO>
__device__ __forceinline__ h16x8 clip_xfrag(const ClipLinArgs &a, int row, int k, float mean, float rstd) {
    if constexpr (PRO == 0) {
        return l2d_ld8((const h16 *)a.x + (long long)row * a.ldx + k);
    } else {
        const f32x4 *p = reinterpret_cast<const f32x4 *>((const float *)a.x + (long long)row * a.ldx + k);
        const f32x4 *gp = reinterpret_cast<const f32x4 *>(a.gamma + k);
        const f32x4 *bp = reinterpret_cast<const f32x4 *>(a.beta + k);
        const f32x4 v0 = p[0], v1 = p[1], g0 = gp[0], g1 = gp[1], b0 = bp[0], b1 = bp[1];
        h16x8 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r[e] = (h16)fmaf((v0[e] - mean) * rstd, g0[e], b0[e]);
            r[e + 4] = (h16)fmaf((v1[e] - mean) * rstd, g1[e], b1[e]);
        }
        return r;
    }
}

template <int PRO, int MT>
__global__ __launch_bounds__(512) void clip_linear_kernel(ClipLinArgs a) {
    __shared__ float red[CLIP_MAX_NW][16][65];           // partial accumulators of one token tile, [wave][acc reg][lane]
    __shared__ float stat[32 * MT][2];                   // LayerNorm prologue: mean, rstd per token row of the block
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, NW = blockDim.x >> 6;
    const int l32 = lane & 31, lh = lane >> 5;
    const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32 * MT;
    const int S = a.K >> 4;                              // k steps of the whole row
    const int s_lo = wave * CLIP_STEPS * a.npass;        // this wave's k steps: [s_lo, s_lo + 12 npass)
    const h16 *wp = a.w + ((long long)blockIdx.x * S * 64 + lane) * 8;

    // token row of each tile for this lane (rows past M are clamped: their results are never stored)
    int row[MT];
    bool live[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int r = m0 + 32 * mt + l32;
        row[mt] = r < a.M ? r : a.M - 1;
        live[mt] = m0 + 32 * mt < a.M;
    }

    h16x8 wr[CLIP_STEPS];
    const bool has = s_lo < S;
    if (has) {
#pragma unroll
        for (int u = 0; u < CLIP_STEPS; ++u) wr[u] = l2d_ld8(wp + (long long)(s_lo + u) * 512);
    }

    float mean[MT], rstd[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) mean[mt] = 0.f, rstd[mt] = 1.f;
    if constexpr (PRO == 1) {
        // 16 lanes per row, the whole row (K <= 1024) in registers: one round of independent 16-byte loads per row group, then
        // the mean and the centred sum of squares from the registers (exact two-pass statistics, one L2 round trip)
        const int sub = lane & 15, nrows = blockDim.x >> 4, K4 = a.K >> 2;
        for (int r0 = 0; r0 < 32 * MT; r0 += nrows) {
            const int r = r0 + (tid >> 4);
            const int gr = m0 + r < a.M ? m0 + r : a.M - 1;
            const f32x4 *xr = reinterpret_cast<const f32x4 *>((const float *)a.x + (long long)gr * a.ldx);
            f32x4 v[16];
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = 16 * j + sub;
                v[j] = c < K4 ? xr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
                sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            const float mu = sum / (float)a.K;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (16 * j + sub < K4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = v[j][e] - mu;
                        q += d * d;
                    }
                }
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
            if (sub == 0 && r < 32 * MT) {
                stat[r][0] = mu;
                stat[r][1] = 1.0f / sqrtf(q / (float)a.K + a.eps);
            }
        }
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            mean[mt] = stat[32 * mt + l32][0];
            rstd[mt] = stat[32 * mt + l32][1];
        }
    }

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[mt][e] = 0.f;

    if (has) {
        for (int p = 0; p < a.npass; ++p) {
            const int sb = s_lo + p * CLIP_STEPS;
            if (p > 0) {
#pragma unroll
                for (int u = 0; u < CLIP_STEPS; ++u) wr[u] = l2d_ld8(wp + (long long)(sb + u) * 512);
            }
#pragma unroll
            for (int u = 0; u < CLIP_STEPS; ++u) {
                const int k = 16 * (sb + u) + 8 * lh;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if (live[mt]) {
                        const h16x8 xf = clip_xfrag<PRO>(a, row[mt], k, mean[mt], rstd[mt]);
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[u], xf, acc[mt], 0, 0, 0);
                    }
                }
            }
        }
    }

    // cross-wave sum (fixed order) + epilogue, one token tile at a time.  Accumulator register j of lane l holds output
    // channel n0 + 8 (j / 4) + 4 (l / 32) + j % 4 of token m0 + 32 mt + l % 32.
    const int nthr = blockDim.x;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (!live[mt]) break;                            // (block-uniform)
#pragma unroll
        for (int j = 0; j < 16; ++j) red[wave][j][lane] = acc[mt][j];
        __syncthreads();
        for (int q = tid; q < 1024; q += nthr) {
            const int n = q & 31, t = q >> 5;
            const int m = m0 + 32 * mt + t;
            const int j = (n >> 3) * 4 + (n & 3), ln = t + 32 * ((n >> 2) & 1);
            float v = 0.f;
            for (int w = 0; w < NW; ++w) v += red[w][j][ln];
            if (m < a.M) {
                if (a.bias) v += a.bias[n0 + n];
                const long long o = (long long)m * a.ldo + n0 + n;
                if (a.epi == 2) {
                    float *out = (float *)a.out;
                    out[o] = out[o] + v;
                } else {
                    if (a.epi == 1) v = v / (1.0f + expf(-1.702f * v));      // quick_gelu
                    ((h16 *)a.out)[o] = (h16)v;
                }
            }
        }
        __syncthreads();
    }
}

template <int PRO>
static void clip_linear_launch(int MT, dim3 grid, dim3 block, hipStream_t s, const ClipLinArgs &a) {
    switch (MT) {
        case 1: hipLaunchKernelGGL((clip_linear_kernel<PRO, 1>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((clip_linear_kernel<PRO, 2>), grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL((clip_linear_kernel<PRO, 3>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((clip_linear_kernel<PRO, 4>), grid, block, 0, s, a); break;
    }
}

int l2d_launch_clip_linear(const l2d_op *op, hipStream_t s) {
    ClipLinArgs a;
    a.x = op->p[0];
    a.w = (const h16 *)op->p[1];
    a.bias = (const float *)op->p[2];
    a.out = op->p[3];
    a.gamma = (const float *)op->p[4];
    a.beta = (const float *)op->p[5];
    a.M = op->i[0], a.K = op->i[1], a.Nout = op->i[2], a.ldx = op->i[3], a.ldo = op->i[4];
    const int pro = op->i[5];
    a.epi = op->i[6];
    const int NW = op->i[7], MT = op->i[8];
    a.eps = op->f[0];
    const int S = a.K / 16;
    a.npass = NW > 0 ? S / (NW * CLIP_STEPS) : 0;
    // K is split into NW x npass passes of exactly 12 k steps; the LayerNorm prologue reads fp32 rows (16-byte aligned pieces)
    const bool ok = a.x && a.w && a.out && a.M > 0 && a.K > 0 && (a.K % (16 * CLIP_STEPS)) == 0 && a.Nout > 0 && (a.Nout % 32) == 0 &&
                    a.ldx >= a.K && (a.ldx % 8) == 0 && a.ldo >= a.Nout && (pro == 0 || pro == 1) && a.epi >= 0 && a.epi <= 2 &&
                    NW >= 1 && NW <= CLIP_MAX_NW && a.npass >= 1 && a.npass * NW * CLIP_STEPS == S && MT >= 1 && MT <= 4 &&
                    (pro == 0 || (a.gamma && a.beta && a.K <= 1024));
    if (!ok) {
        l2d_set_error("clip_linear(tag %d): invalid arguments (M=%d K=%d Nout=%d ldx=%d ldo=%d pro=%d epi=%d NW=%d MT=%d)", op->tag,
                      a.M, a.K, a.Nout, a.ldx, a.ldo, pro, a.epi, NW, MT);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const int mtiles = (a.M + 31) / 32;
    dim3 grid(a.Nout / 32, (mtiles + MT - 1) / MT), block(64 * NW);
    if (pro) clip_linear_launch<1>(MT, grid, block, s, a);
    else clip_linear_launch<0>(MT, grid, block, s, a);
    return l2d_check_launch("clip_linear", op->tag);
}
