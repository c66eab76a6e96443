// Cut detection (the arithmetic is live2diff_amd/cut.py's, held to equality): how far is this frame from
// the one before, on the bytes a viewer would see and in exact integers?
//   L2D_OP_FRAME_CUT_SIG: per pixel b = px_byte of the three channels, Y = px_luma(b) in 0..255.  thumb[by][bx] = the sum of Y over
//   the 8 x 8 block (<= 16,320: uint16); partial[tile] = {the 64 counts of Y >> 2 over the tile, the tile's share of Dt = sum |thumb
//   - thumb'|, 0, 0, 0}.  One work-group per 64 x 64 pixels, ragged in whole blocks at the right and the bottom.
//   L2D_OP_FRAME_CUT: hist = the partials' sum, Dt = the shares' sum, Dh = sum |hist - hist'|, then the decision and the record
//   {cut, Dt, Dh, since, n, E_lo, E_hi, flags} of cut.measure_ref.  One work-group.
// Plain stores only, every output entry written on every launch, nothing zeroed beforehand, no atomics on global memory.
#include "frame_px.h"

#define CUT_BLOCK L2D_CUT_BLOCK
#define CUT_BINS L2D_CUT_BINS
#define CUT_TILE L2D_CUT_TILE
#define CUT_PARTIAL L2D_CUT_PARTIAL
#define CUT_INIT L2D_CUT_INIT
#define CUT_NEVER L2D_CUT_NEVER
#define CUT_SIG_THREADS 512                   // one 8-pixel row of a block per lane; a wave is one row of 8 blocks
#define CUT_THREADS 256                       // L2D_OP_FRAME_CUT: four lanes per bin
#define CUT_SIG_LDS_BYTES (CUT_PARTIAL * 4)
#define CUT_LDS_BYTES (4 * CUT_BINS * 4 + 4 * 8)
static_assert(CUT_SIG_LDS_BYTES == 272 && CUT_LDS_BYTES == 1056,
              "DESIGN.md section 8.z21, l2d.h and tests/test_cut_resources.py state these sizes");
static_assert(CUT_TILE == 8 * CUT_BLOCK && CUT_SIG_THREADS == CUT_TILE * (CUT_TILE / 8) && CUT_BINS == L2D_WAVE && CUT_BLOCK == 8,
              "a wave of 64 lanes is 8 rows x 8 blocks, and the histogram one bin per lane");

// grid (ceil(W / 64), ceil(H / 64)), CUT_SIG_THREADS lanes.  Wave w is block row w of the tile; lane l of it holds row l / 8 of block
// l % 8: one 16-byte load per channel.  The block sums are formed across the lanes 8, 16 and 32 apart; lanes 0..7 own a block each.
// `sh` is the tile's partial as it is stored: 64 bins and the share of Dt under LDS adds (integer sums do not depend on order).
template <bool INIT>
__device__ __forceinline__ void cut_sig_body(const h16 *__restrict__ source, const uint16_t *__restrict__ prev, uint16_t *__restrict__ thumb,
                                             unsigned *__restrict__ partials, int H, int W) {
    __shared__ unsigned sh[CUT_PARTIAL];
    static_assert(sizeof(sh) == CUT_SIG_LDS_BYTES, "the LDS size the file states");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < CUT_PARTIAL) sh[tid] = 0u;
    __syncthreads();
    const int bx = blockIdx.x * 8 + (lane & 7), by = blockIdx.y * 8 + wave;       // the lane's block
    const int x = bx * CUT_BLOCK, y = by * CUT_BLOCK + (lane >> 3);
    const bool in = x < W && y < H;               // (H and W are multiples of 8: a block lies inside the frame or outside it)
    unsigned sum = 0u;
    if (in) {
        const long long HW = (long long)H * W, px = (long long)y * W + x;
        const h16x8 r = l2d_ld8(source + px), g = l2d_ld8(source + HW + px), b = l2d_ld8(source + 2 * HW + px);
        unsigned run = CUT_BINS, cnt = 0u;        // (CUT_BINS: no run yet) equal neighbours go in as one LDS add
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned Y = px_luma(px_byte(r[e]), px_byte(g[e]), px_byte(b[e]));
            sum += Y;
            const unsigned k = min(Y >> 2, (unsigned)(CUT_BINS - 1));      // (Y <= 255 on finite input; a NaN's byte is not defined)
            if (k == run) {
                ++cnt;
            } else {
                if (cnt) atomicAdd(&sh[run], cnt);
                run = k;
                cnt = 1u;
            }
        }
        if (cnt) atomicAdd(&sh[run], cnt);
    }
    // (every lane of the wave takes part: lanes outside the frame hold zero)
    sum += (unsigned)__shfl_xor((int)sum, 8, 64);
    sum += (unsigned)__shfl_xor((int)sum, 16, 64);
    sum += (unsigned)__shfl_xor((int)sum, 32, 64);
    if (lane < 8 && in) {
        const long long at = (long long)by * (W / CUT_BLOCK) + bx;
        thumb[at] = (uint16_t)sum;
        if constexpr (!INIT) {
            const int d = (int)sum - (int)prev[at];
            atomicAdd(&sh[CUT_BINS], (unsigned)(d < 0 ? -d : d));
        }
    }
    __syncthreads();
    if (tid < CUT_PARTIAL) partials[(long long)(blockIdx.y * gridDim.x + blockIdx.x) * CUT_PARTIAL + tid] = sh[tid];
}

__global__ __launch_bounds__(CUT_SIG_THREADS) void frame_cut_sig_init_kernel(const h16 *__restrict__ source, uint16_t *__restrict__ thumb,
                                                                             unsigned *__restrict__ partials, int H, int W) {
    cut_sig_body<true>(source, nullptr, thumb, partials, H, W);
}

__global__ __launch_bounds__(CUT_SIG_THREADS) void frame_cut_sig_diff_kernel(const h16 *__restrict__ source, const uint16_t *__restrict__ prev,
                                                                             uint16_t *__restrict__ thumb, unsigned *__restrict__ partials,
                                                                             int H, int W) {
    cut_sig_body<false>(source, prev, thumb, partials, H, W);
}

struct cut_params {
    int Tt, Th, R, gap;
};

// one work-group of CUT_THREADS lanes: wave q sums bin `lane` over the partials q, q + 4, ... and the shares of Dt over the same
// frame (lane t of the group: partials t, t + 256, ...; 64-bit); wave 0 then owns the bins, and its lane 0 the decision
template <bool INIT>
__device__ __forceinline__ void cut_body(const unsigned *__restrict__ partials, const unsigned *__restrict__ prev_hist,
                                         const int *__restrict__ prev_rec, unsigned *__restrict__ hist, int *__restrict__ rec, int nwg,
                                         cut_params p) {
    __shared__ unsigned hs[4][CUT_BINS];
    __shared__ unsigned long long ds[4];
    static_assert(sizeof(hs) + sizeof(ds) == CUT_LDS_BYTES, "the LDS size the file states");
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    unsigned h = 0u;
#pragma unroll 4
    for (int b = q; b < nwg; b += 4) h += partials[(long long)b * CUT_PARTIAL + lane];
    hs[q][lane] = h;
    unsigned long long dt = 0ull;
    if constexpr (!INIT) {
        for (int b = threadIdx.x; b < nwg; b += CUT_THREADS) dt += partials[(long long)b * CUT_PARTIAL + CUT_BINS];
        unsigned lo = (unsigned)dt, hi = (unsigned)(dt >> 32);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = ((unsigned long long)(unsigned)__shfl_xor((int)hi, o, 64) << 32) | (unsigned)__shfl_xor((int)lo, o, 64);
            dt += other;
            lo = (unsigned)dt;
            hi = (unsigned)(dt >> 32);
        }
    }
    if (lane == 0) ds[q] = dt;
    __syncthreads();
    if (q) return;
    h = hs[0][lane] + hs[1][lane] + hs[2][lane] + hs[3][lane];
    hist[lane] = h;
    if constexpr (INIT) {
        if (lane < 8) rec[lane] = lane == 3 ? CUT_NEVER : 0;
    } else {
        const int e = (int)h - (int)prev_hist[lane];
        int dh = e < 0 ? -e : e;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dh += __shfl_xor(dh, o, 64);
        if (lane) return;
        const unsigned long long total = ds[0] + ds[1] + ds[2] + ds[3];
        const long long Dt = total > 0x7fffffffull ? 0x7fffffffll : (long long)total;     // (at most 255 H W < 2^30 on thumbnails)
        const int since0 = prev_rec[3], n0 = prev_rec[4], flags0 = prev_rec[7];
        long long E = (long long)(((unsigned long long)(unsigned)prev_rec[6] << 32) | (unsigned)prev_rec[5]);
        const int s = min(since0, CUT_NEVER - 1) + 1;                       // min(since' + 1, 2^30)
        const bool has = (flags0 & 1) != 0;
        const bool cut = Dt >= p.Tt && dh >= p.Th && s > p.gap && (p.R == 0 || !has || 65536ll * Dt >= (long long)p.R * E);
        int flags = flags0;
        if (!cut) {
            E = has ? E + ((256ll * Dt - E) >> 3) : 256ll * Dt;               // (>> of a negative long long: arithmetic, the floor)
            flags |= 1;
        }
        rec[0] = cut ? 1 : 0;
        rec[1] = (int)Dt;
        rec[2] = dh;
        rec[3] = cut ? 0 : s;
        rec[4] = n0 + 1;
        rec[5] = (int)(unsigned)(unsigned long long)E;
        rec[6] = (int)(E >> 32);
        rec[7] = flags;
    }
}

__global__ __launch_bounds__(CUT_THREADS) void frame_cut_init_kernel(const unsigned *__restrict__ partials, unsigned *__restrict__ hist,
                                                                     int *__restrict__ rec, int nwg) {
    cut_body<true>(partials, nullptr, nullptr, hist, rec, nwg, cut_params{0, 0, 0, 0});
}

__global__ __launch_bounds__(CUT_THREADS) void frame_cut_decide_kernel(const unsigned *__restrict__ partials,
                                                                       const unsigned *__restrict__ prev_hist, const int *__restrict__ prev_rec,
                                                                       unsigned *__restrict__ hist, int *__restrict__ rec, int nwg, cut_params p) {
    cut_body<false>(partials, prev_hist, prev_rec, hist, rec, nwg, p);
}

// ------------------------------------------------------------------------------------------------------------------------------
// the geometry ops 65 and 66 share: H W, or -1 with the error set (`nwg` must be the tiles of H x W)
static long long cut_check_frame(const char *name, const l2d_op *op, int nwg, int flags) {
    const int H = op->i[0], W = op->i[1];
    if (H <= 0 || W <= 0 || H % CUT_BLOCK || W % CUT_BLOCK || (long long)H * W > L2D_CUT_MAX_PIXELS) {
        l2d_set_error("%s(tag %d): %d x %d: H and W must be positive multiples of %d with H W <= %d", name, op->tag, H, W, CUT_BLOCK,
                      L2D_CUT_MAX_PIXELS);
        return -1;
    }
    const int want = ((H + CUT_TILE - 1) / CUT_TILE) * ((W + CUT_TILE - 1) / CUT_TILE);
    if (nwg != want) {
        l2d_set_error("%s(tag %d): nwg = %d, but %d x %d is %d tiles of %d x %d pixels", name, op->tag, nwg, H, W, want, CUT_TILE, CUT_TILE);
        return -1;
    }
    if (flags & ~CUT_INIT) {
        l2d_set_error("%s(tag %d): unknown flag bits 0x%x (1 init)", name, op->tag, flags);
        return -1;
    }
    return (long long)H * W;
}

// pointer k of the op: not null (unless `optional`), 16-byte aligned
static bool cut_check_pointer(const char *name, const l2d_op *op, int k, bool optional) {
    if (!op->p[k] && !optional) {
        l2d_set_error("%s(tag %d): pointer %d is null", name, op->tag, k);
        return false;
    }
    if (((uintptr_t)op->p[k]) & 15) {
        l2d_set_error("%s(tag %d): pointer %d is not 16-byte aligned", name, op->tag, k);
        return false;
    }
    return true;
}

int l2d_launch_frame_cut_sig(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], flags = op->i[2], nwg = op->i[3];
    const long long HW = cut_check_frame("frame_cut_sig", op, nwg, flags);
    if (HW < 0) return L2D_EINVAL;
    const bool init = (flags & CUT_INIT) != 0;
    for (int k = 0; k < 4; ++k)
        if (!cut_check_pointer("frame_cut_sig", op, k, k == 1 && init)) return L2D_EINVAL;
    const long long tbytes = HW / (CUT_BLOCK * CUT_BLOCK) * 2, pbytes = (long long)nwg * CUT_PARTIAL * 4;
    const void *prev = init ? nullptr : op->p[1];
    if (px_overlap(op->p[2], tbytes, op->p[0], 6 * HW) || px_overlap(op->p[2], tbytes, prev, tbytes) || px_overlap(op->p[3], pbytes, op->p[0], 6 * HW)
        || px_overlap(op->p[3], pbytes, prev, tbytes) || px_overlap(op->p[2], tbytes, op->p[3], pbytes)) {
        l2d_set_error("frame_cut_sig(tag %d): the thumbnail written or the partials overlap the source, the thumbnail read or each other",
                      op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const dim3 grid((unsigned)((W + CUT_TILE - 1) / CUT_TILE), (unsigned)((H + CUT_TILE - 1) / CUT_TILE));
    if (init)
        hipLaunchKernelGGL(frame_cut_sig_init_kernel, grid, dim3(CUT_SIG_THREADS), 0, s, (const h16 *)op->p[0], (uint16_t *)op->p[2],
                           (unsigned *)op->p[3], H, W);
    else
        hipLaunchKernelGGL(frame_cut_sig_diff_kernel, grid, dim3(CUT_SIG_THREADS), 0, s, (const h16 *)op->p[0], (const uint16_t *)op->p[1],
                           (uint16_t *)op->p[2], (unsigned *)op->p[3], H, W);
    return l2d_check_launch("frame_cut_sig", op->tag);
}

int l2d_launch_frame_cut(const l2d_op *op, hipStream_t s) {
    const int nwg = op->i[2], flags = op->i[3];
    const cut_params p{op->i[4], op->i[5], op->i[6], op->i[7]};
    const long long HW = cut_check_frame("frame_cut", op, nwg, flags);
    if (HW < 0) return L2D_EINVAL;
    const bool init = (flags & CUT_INIT) != 0;
    for (int k = 0; k < 5; ++k)
        if (!cut_check_pointer("frame_cut", op, k, (k == 1 || k == 2) && init)) return L2D_EINVAL;
    if (p.Tt < 0 || p.Tt > 255 * HW || p.Th < 0 || p.Th > 2 * HW || p.R < 0 || (p.R && p.R < L2D_CUT_MIN_R) || p.R > L2D_CUT_MAX_R || p.gap < 0
        || p.gap > L2D_CUT_MAX_GAP) {
        l2d_set_error("frame_cut(tag %d): Tt = %d (need 0..%lld), Th = %d (0..%lld), R = %d (0, or %d..%d) or gap = %d (0..%d)", op->tag, p.Tt,
                      255 * HW, p.Th, 2 * HW, p.R, L2D_CUT_MIN_R, L2D_CUT_MAX_R, p.gap, L2D_CUT_MAX_GAP);
        return L2D_EINVAL;
    }
    const long long pbytes = (long long)nwg * CUT_PARTIAL * 4, hbytes = CUT_BINS * 4;
    const void *ph = init ? nullptr : op->p[1], *pr = init ? nullptr : op->p[2];
    const void *reads[3] = {op->p[0], ph, pr};
    const long long rbytes[3] = {pbytes, hbytes, 32};
    bool bad = px_overlap(op->p[3], hbytes, op->p[4], 32);
    for (int k = 0; k < 3; ++k) bad = bad || px_overlap(op->p[3], hbytes, reads[k], rbytes[k]) || px_overlap(op->p[4], 32, reads[k], rbytes[k]);
    if (bad) {
        l2d_set_error("frame_cut(tag %d): the histogram or the record written overlaps the partials, the state read or each other", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    if (init)
        hipLaunchKernelGGL(frame_cut_init_kernel, dim3(1), dim3(CUT_THREADS), 0, s, (const unsigned *)op->p[0], (unsigned *)op->p[3],
                           (int *)op->p[4], nwg);
    else
        hipLaunchKernelGGL(frame_cut_decide_kernel, dim3(1), dim3(CUT_THREADS), 0, s, (const unsigned *)op->p[0], (const unsigned *)op->p[1],
                           (const int *)op->p[2], (unsigned *)op->p[3], (int *)op->p[4], nwg, p);
    return l2d_check_launch("frame_cut", op->tag);
}
