// Follow: steady along the source's motion.  Steady (steady.hip) holds the previous output pixel where the
// source bytes at the SAME coordinates did not change; under a hand-held camera or a pan every pixel moves and nothing is held.
// Two launches put the missing "where" in front of the same arithmetic.  The reference has no counterpart.
//
// L2D_OP_FRAME_MOTION: one vector (dy, dx) per 8 x 8 block, by exhaustive block matching on the bytes a viewer would see
//   window of block (i, j): rows 8i-4 .. 8i+11, columns 8j-4 .. 8j+11 (the block and an apron of 4)
//   cost(dy, dx) = sum over the window and the channels of |now[c, cl(y), cl(x)] - prev[c, cl(y+dy), cl(x+dx)]|     cl: clamp
//   key = (cost + bias (|dy| + |dx|)) 512 + rank            rank: the position in the order (|dy| + |dx|, dy, dx); key < 2^27
//   the vector of the smallest key: exact integers and a minimum, so any order of evaluation gives the same field
// L2D_OP_FRAME_STEADY_FOLLOW: L2D_OP_FRAME_STEADY with prev_bytes and prev_out fetched at (cl(y+dy), cl(x+dx)), (dy, dx) the
//   vector of the pixel's own block; the new state is (o, b) as there, so the next frame measures against this frame's own source.
//
// numpy restates both bit for bit (live2diff_amd/steady.py motion_ref, follow_ref); the file is built with -ffp-contract=off.
#include "steady_px.h"

#define MF_R L2D_FOLLOW_MAX_SEARCH
#define MF_BLOCKS 8                                   // blocks per work-group: a strip of one block row
#define MF_THREADS 256
#define MF_LANES (MF_THREADS / MF_BLOCKS)             // 32 lanes share a block: lane l takes items l, l + 32, ... of four candidates each
#define MF_WIN (L2D_FOLLOW_BLOCK + 2 * L2D_FOLLOW_APRON)
#define MF_NOW_Q ((8 * MF_BLOCKS + 2 * L2D_FOLLOW_APRON) / 4)      // 18 dwords: the 72 columns the strip's windows cover
#define MF_PRV_Q (MF_NOW_Q + 2 * MF_R / 4)            // 22 dwords: ... and the search margin on either side
#define MF_PRV_H (MF_WIN + 2 * MF_R)                  // 32 rows
#define MF_CAND ((2 * MF_R + 1) * (2 * MF_R + 1))     // 289
#define MF_TAB ((MF_CAND + 3) & ~3)                   // 292

static_assert(L2D_FOLLOW_BLOCK == 8 && L2D_FOLLOW_APRON == 4 && MF_WIN == 16, "a window row is four dwords");
static_assert(MF_R % 2 == 0 && MF_CAND <= 512, "the rank takes the key's low nine bits");
static_assert((3ll * MF_WIN * MF_WIN * 255 + (long long)L2D_FOLLOW_MAX_BIAS * 2 * MF_R) * 512 + 511 < (1ll << 27), "the key fits 27 bits");

struct mf_lds {
    unsigned now[3][MF_WIN][MF_NOW_Q];                // this frame's bytes of the strip's windows, clamped while staged
    unsigned prv[3 * MF_PRV_H * MF_PRV_Q + 2];        // the previous bytes with the margin (+ 2: a fifth dword read and shifted out)
    unsigned keys[MF_THREADS];
    unsigned short rank[MF_TAB];                      // candidate (raster index) -> rank
    unsigned short cand[MF_TAB];                      // rank -> candidate
};
#define MF_LDS_BYTES 14104
static_assert(sizeof(mf_lds) == MF_LDS_BYTES, "DESIGN.md section 8.z14 and tests/test_follow_resources.py state this size");

// the rank of (dy, dx): the number of candidates of [-R, R]^2 in front of it in the order (|dy| + |dx|, dy, dx), counted row by row
__device__ __forceinline__ int mf_rank(int dy, int dx, int R) {
    const int s = (dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx);
    int rank = 0;
    for (int oy = -R; oy <= R; ++oy) {
        const int e = s - (oy < 0 ? -oy : oy);                   // |dx'| of this row's candidates at the same distance
        if (e > 0) rank += e - 1 >= R ? 2 * R + 1 : 2 * e - 1;   // the shorter ones: |dx'| <= e - 1
        if (e >= 0 && e <= R) {
            if (oy < dy) rank += e == 0 ? 1 : 2;
            else if (oy == dy && dx > 0) rank += 1;              // (-e, then e = dx)
        }
    }
    return rank;
}

__global__ __launch_bounds__(MF_THREADS) void frame_motion_kernel(const h16 *__restrict__ source, const uint8_t *__restrict__ prev_bytes,
                                                                  signed char *__restrict__ field, int H, int W, int Wb, int R, int bias) {
    __shared__ __attribute__((aligned(16))) mf_lds L;
    const int tid = threadIdx.x;
    const int bi = blockIdx.y, j0 = blockIdx.x * MF_BLOCKS;
    const int n = 2 * R + 1, ncand = n * n;
    const long long HW = (long long)H * W;

    for (int c = tid; c < ncand; c += MF_THREADS) {
        const int rank = mf_rank(c / n - R, c % n - R, R);
        L.rank[c] = (unsigned short)rank;
        L.cand[rank] = (unsigned short)c;
    }
    const int wy0 = 8 * bi - L2D_FOLLOW_APRON, wx0 = 8 * j0 - L2D_FOLLOW_APRON;
    for (int g = tid; g < 3 * MF_WIN * MF_NOW_Q; g += MF_THREADS) {
        const int ch = g / (MF_WIN * MF_NOW_Q), yy = g % (MF_WIN * MF_NOW_Q) / MF_NOW_Q, xq = g % MF_NOW_Q;
        const h16 *row = source + ch * HW + (long long)px_clampi(wy0 + yy, 0, H - 1) * W;
        unsigned v = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) v |= px_byte(row[px_clampi(wx0 + 4 * xq + e, 0, W - 1)]) << (8 * e);
        L.now[ch][yy][xq] = v;
    }
    const int ph = MF_WIN + 2 * R, pq = MF_NOW_Q + (2 * R + 3) / 4;           // rows and dwords per row that the search reaches
    const int xq = tid % 32;                                                   // (32 lanes a row, pq <= 22 of them busy: no division)
    if (xq < pq) {
        for (int ch = 0; ch < 3; ++ch) {
            for (int yy = tid / 32; yy < ph; yy += MF_THREADS / 32) {
                const uint8_t *row = prev_bytes + ch * HW + (long long)px_clampi(wy0 - R + yy, 0, H - 1) * W;
                unsigned v = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) v |= (unsigned)row[px_clampi(wx0 - R + 4 * xq + e, 0, W - 1)] << (8 * e);
                L.prv[(ch * MF_PRV_H + yy) * MF_PRV_Q + xq] = v;
            }
        }
    }
    __syncthreads();

    // One item = one dy and four neighbouring dx whose windows start in the same staged dword: the five aligned dwords of a
    // previous row serve all four (v_alignbyte_b32 by 0..3 bytes), the four dwords of the now row are a broadcast.
    const int b = tid / MF_LANES, l = tid % MF_LANES;
    const int ng = (2 * R) / 4 + 1, items = n * ng;
    unsigned best = 0xffffffffu;
    if (j0 + b < Wb) {
        for (int t = l; t < items; t += MF_LANES) {
            const int dy = t / ng - R, gq = t % ng;
            const int q0 = 2 * b + gq;                                         // the staged dword of column 8 b + 4 gq: dx = 4 gq + s - R
            unsigned cost[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
#pragma unroll 4
                for (int row = 0; row < MF_WIN; ++row) {
                    const unsigned *a = &L.now[ch][row][2 * b];
                    const unsigned *p = &L.prv[(ch * MF_PRV_H + row + R + dy) * MF_PRV_Q + q0];
                    const unsigned pv[5] = {p[0], p[1], p[2], p[3], p[4]};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const unsigned an = a[k];
                        cost[0] = __builtin_amdgcn_sad_u8(an, pv[k], cost[0]);
                        cost[1] = __builtin_amdgcn_sad_u8(an, __builtin_amdgcn_alignbyte(pv[k + 1], pv[k], 1u), cost[1]);
                        cost[2] = __builtin_amdgcn_sad_u8(an, __builtin_amdgcn_alignbyte(pv[k + 1], pv[k], 2u), cost[2]);
                        cost[3] = __builtin_amdgcn_sad_u8(an, __builtin_amdgcn_alignbyte(pv[k + 1], pv[k], 3u), cost[3]);
                    }
                }
            }
#pragma unroll
            for (int sft = 0; sft < 4; ++sft) {
                const int u = 4 * gq + sft;                                    // dx + R
                if (u <= 2 * R) {
                    const int dx = u - R;
                    const unsigned l1 = (unsigned)((dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx));
                    const unsigned key = (cost[sft] + (unsigned)bias * l1) * 512u + L.rank[(dy + R) * n + u];
                    best = key < best ? key : best;
                }
            }
        }
    }
    L.keys[tid] = best;
    __syncthreads();
    if (tid < MF_BLOCKS && j0 + tid < Wb) {
        unsigned m = 0xffffffffu;
        for (int k = 0; k < MF_LANES; ++k) {
            const unsigned v = L.keys[tid * MF_LANES + k];
            m = v < m ? v : m;
        }
        const int c = L.cand[m & 511u];
        signed char *v = field + 2 * ((long long)bi * Wb + j0 + tid);
        v[0] = (signed char)(c / n - R);
        v[1] = (signed char)(c % n - R);
    }
}

// the box kernel of steady.hip with displaced fetches of the previous record: an 8-aligned pixel group lies inside one block of
// the field, so it has one vector; its previous samples are 8 consecutive pixels of row cl(y + dy) from column x + dx on.  A
// vector is used only through clamped coordinates: whatever a field holds, nothing outside the previous record is read.
__global__ __launch_bounds__(SD_THREADS) void frame_steady_follow_kernel(const h16 *__restrict__ styled, const h16 *__restrict__ source,
                                                                         const h16 *__restrict__ prev_out,
                                                                         const uint8_t *__restrict__ prev_bytes, h16 *__restrict__ out,
                                                                         uint8_t *__restrict__ next_bytes, h16 *__restrict__ picture,
                                                                         const signed char *__restrict__ field, int H, int W, sd_params p) {
    __shared__ __attribute__((aligned(16))) unsigned char dd[SD_DH][SD_DW];       // d of the tile and its halo
    __shared__ __attribute__((aligned(16))) unsigned short hh[SD_DH][SD_TW];      // the horizontal sums
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SD_TW, y0 = blockIdx.y * SD_TH;
    const int r = p.r, taps = 2 * r + 1, rows = SD_TH + 2 * r;
    const bool show = (p.flags & SD_SHOW) != 0;
    const long long HW = (long long)H * W;
    const int Wb = W >> 3;

    const int by = tid >> 3, bx = (tid & 7) * 8;
    const int y = y0 + by, x = x0 + bx;
    const bool live = y < H && x < W;           // (x + 8 <= W then: W % 8 == 0)
    const long long px = (long long)y * W + x;
    h16x8 S[3], P[3];
    if (live) {
        const signed char *v = field + 2 * ((long long)(y >> 3) * Wb + (x >> 3));
        const int dy = v[0], dx = v[1];
        const long long prow = (long long)px_clampi(y + dy, 0, H - 1) * W;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            S[ch] = l2d_ld8(styled + ch * HW + px);
#pragma unroll
            for (int e = 0; e < 8; ++e) P[ch][e] = prev_out[ch * HW + prow + px_clampi(x + dx + e, 0, W - 1)];
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) S[ch] = P[ch] = l2d_zero8();
    }

    for (int g = tid; g < rows * (SD_DW / 8); g += SD_THREADS) {
        const int j = g / (SD_DW / 8), cg = g % (SD_DW / 8);
        const int yu = y0 - r + j;
        const int yy = yu < 0 ? 0 : (yu > H - 1 ? H - 1 : yu);
        const int gx = x0 - 8 + cg * 8;
        unsigned d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (gx < 0 || gx >= W) {
            const int ex = gx < 0 ? 0 : W - 1;                                  // the edge pixel, with its own block's vector
            const signed char *v = field + 2 * ((long long)(yy >> 3) * Wb + (ex >> 3));
            const long long e0 = (long long)yy * W + ex;
            const long long q0 = (long long)px_clampi(yy + v[0], 0, H - 1) * W + px_clampi(ex + v[1], 0, W - 1);
            unsigned m = 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const unsigned a = sd_absdiff(px_byte(source[ch * HW + e0]), (unsigned)prev_bytes[ch * HW + q0]);
                m = a > m ? a : m;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = m;
        } else {
            const signed char *v = field + 2 * ((long long)(yy >> 3) * Wb + (gx >> 3));
            const int dx = v[1];
            const long long g0 = (long long)yy * W + gx;
            const long long prow = (long long)px_clampi(yy + v[0], 0, H - 1) * W;
            const bool own = yu == yy && j >= r && j < r + SD_TH && cg >= 1 && cg <= SD_TW / 8;     // a group of the tile itself
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const uint2 now = sd_bytes8(l2d_ld8(source + ch * HW + g0));
                sd_motion8(now, fl_bytes8(prev_bytes + ch * HW + prow, gx + dx, W), d);
                if (own) *reinterpret_cast<uint2 *>(next_bytes + ch * HW + g0) = now;
            }
        }
        *reinterpret_cast<uint2 *>(&dd[j][cg * 8]) = px_pack8(d);
    }
    __syncthreads();

    // horizontal: hh[j][c] = dd[j][8 + c - r] + ... + dd[j][8 + c + r]
    for (int i = tid; i < rows * SD_TW; i += SD_THREADS) {
        const int j = i / SD_TW, cc = i % SD_TW;
        const unsigned char *src = &dd[j][8 + cc - r];
        unsigned acc = 0u;
        for (int k = 0; k < taps; ++k) acc += src[k];
        hh[j][cc] = (unsigned short)acc;
    }
    __syncthreads();
    if (!live) return;

    // vertical: D[e] = hh[by][bx + e] + ... + hh[by + 2 r][bx + e]
    unsigned D[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (int k = 0; k < taps; ++k) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&hh[by + k][bx]);
        D[0] += v.x & 65535u; D[1] += v.x >> 16;
        D[2] += v.y & 65535u; D[3] += v.y >> 16;
        D[4] += v.z & 65535u; D[5] += v.z >> 16;
        D[6] += v.w & 65535u; D[7] += v.w >> 16;
    }
    const float n = (float)(taps * taps);
    float w[8], a[8];
    h16x8 pic;
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = sd_weight(__fdiv_rn((float)D[e], n), p);
    sd_alpha8(w, p.s, a, pic);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        l2d_st8(out + ch * HW + px, sd_blend8(S[ch], P[ch], a));
        if (show) l2d_st8(picture + ch * HW + px, pic);
    }
}
#define FL_LDS_BYTES (SD_DH * SD_DW + 2 * SD_DH * SD_TW)
static_assert(FL_LDS_BYTES == 6656, "DESIGN.md section 8.z14 and tests/test_follow_resources.py state this size");

static long long fl_field_bytes(int H, int W) { return 2ll * ((H + 7) / 8) * (W / 8); }

int l2d_launch_frame_motion(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], R = op->i[2], bias = op->i[3];
    for (int k = 0; k < 3; ++k) {
        if (!op->p[k]) {
            l2d_set_error("frame_motion(tag %d): pointer %d is null", op->tag, k);
            return L2D_EINVAL;
        }
    }
    if ((((uintptr_t)op->p[0]) & 15) || (((uintptr_t)op->p[1]) & 7)) {
        l2d_set_error("frame_motion(tag %d): a pointer is not aligned (the source frame 16 bytes, the byte planes 8)", op->tag);
        return L2D_EINVAL;
    }
    const long long HW = px_check_frame("frame_motion", op->tag, H, W);
    if (HW < 0) return L2D_EINVAL;
    if (R < 1 || R > MF_R) {
        l2d_set_error("frame_motion(tag %d): search %d, need 1..%d", op->tag, R, MF_R);
        return L2D_EINVAL;
    }
    if (bias < 0 || bias > L2D_FOLLOW_MAX_BIAS) {
        l2d_set_error("frame_motion(tag %d): bias %d, need 0..%d", op->tag, bias, L2D_FOLLOW_MAX_BIAS);
        return L2D_EINVAL;
    }
    if (px_overlap(op->p[2], fl_field_bytes(H, W), op->p[0], HW * 6) || px_overlap(op->p[2], fl_field_bytes(H, W), op->p[1], HW * 3)) {
        l2d_set_error("frame_motion(tag %d): the field overlaps an input (the source frame or prev_bytes)", op->tag);
        return L2D_EINVAL;
    }
    L2D_DRY_RETURN();
    const int Hb = (H + 7) / 8, Wb = W / 8;
    hipLaunchKernelGGL(frame_motion_kernel, dim3((Wb + MF_BLOCKS - 1) / MF_BLOCKS, Hb), dim3(MF_THREADS), 0, s, (const h16 *)op->p[0],
                       (const uint8_t *)op->p[1], (signed char *)op->p[2], H, W, Wb, R, bias);
    return l2d_check_launch("frame_motion", op->tag);
}

int l2d_launch_frame_steady_follow(const l2d_op *op, hipStream_t s) {
    const int H = op->i[0], W = op->i[1], r = op->i[2], flags = op->i[3];
    if (flags & ~(SD_HARD | SD_SHOW)) {
        l2d_set_error("frame_steady_follow(tag %d): unknown flag bits 0x%x (1 hard, 2 show; an init frame is L2D_OP_FRAME_STEADY's)", op->tag,
                      flags);
        return L2D_EINVAL;
    }
    const bool show = (flags & SD_SHOW) != 0;
    for (int k = 0; k < 8; ++k) {
        if (!op->p[k] && !(!show && k == 6)) {
            l2d_set_error("frame_steady_follow(tag %d): pointer %d is null (6 may be without the show flag)", op->tag, k);
            return L2D_EINVAL;
        }
        if (k < 7 && (((uintptr_t)op->p[k]) & ((k == 3 || k == 5) ? 7 : 15))) {
            l2d_set_error("frame_steady_follow(tag %d): pointer %d is not aligned (fp16 frames 16 bytes, byte planes 8)", op->tag, k);
            return L2D_EINVAL;
        }
    }
    const long long HW = px_check_frame("frame_steady_follow", op->tag, H, W);
    if (HW < 0) return L2D_EINVAL;
    if (r < 0 || r > SD_MAX_R) {
        l2d_set_error("frame_steady_follow(tag %d): radius %d, need 0..%d", op->tag, r, SD_MAX_R);
        return L2D_EINVAL;
    }
    // as L2D_OP_FRAME_STEADY: the new state never lies where this launch reads.  Displaced reads still touch only the previous
    // record (every coordinate is clamped to the image), so the same tests hold
    const void *const hread[3] = {op->p[0], op->p[1], op->p[2]};
    const void *const hwrite[2] = {op->p[4], show ? op->p[6] : nullptr};
    for (int a = 0; a < 2; ++a) {
        for (int b = 0; b < 3; ++b) {
            if (px_overlap(hwrite[a], HW * 6, hread[b], HW * 6)) {
                l2d_set_error("frame_steady_follow(tag %d): output frame %d overlaps input frame %d (out / the picture against styled, "
                              "source, prev_out)", op->tag, a ? 6 : 4, b);
                return L2D_EINVAL;
            }
        }
        if (px_overlap(hwrite[a], HW * 6, op->p[3], HW * 3)) {
            l2d_set_error("frame_steady_follow(tag %d): output frame %d overlaps prev_bytes", op->tag, a ? 6 : 4);
            return L2D_EINVAL;
        }
    }
    if (show && px_overlap(op->p[4], HW * 6, op->p[6], HW * 6)) {
        l2d_set_error("frame_steady_follow(tag %d): the picture overlaps the output frame", op->tag);
        return L2D_EINVAL;
    }
    if (px_overlap(op->p[5], HW * 3, op->p[3], HW * 3)) {
        l2d_set_error("frame_steady_follow(tag %d): next_bytes overlaps prev_bytes (displaced fetches and a tile's halo read what its "
                      "neighbour would write)", op->tag);
        return L2D_EINVAL;
    }
    for (int b = 0; b < 3; ++b) {
        if (px_overlap(op->p[5], HW * 3, hread[b], HW * 6)) {
            l2d_set_error("frame_steady_follow(tag %d): next_bytes overlaps input frame %d", op->tag, b);
            return L2D_EINVAL;
        }
    }
    const long long fb = fl_field_bytes(H, W);
    if (px_overlap(op->p[7], fb, op->p[4], HW * 6) || px_overlap(op->p[7], fb, op->p[5], HW * 3) ||
        (show && px_overlap(op->p[7], fb, op->p[6], HW * 6))) {
        l2d_set_error("frame_steady_follow(tag %d): the field overlaps an output (out, next_bytes or the picture)", op->tag);
        return L2D_EINVAL;
    }
    const float lo = op->f[0], inv = op->f[1], st = op->f[2];
    if (!sd_check_floats("frame_steady_follow", op->tag, lo, inv, st)) return L2D_EINVAL;
    L2D_DRY_RETURN();
    sd_params p;
    p.lo = lo; p.inv = inv; p.s = st; p.flags = flags; p.r = r;
    hipLaunchKernelGGL(frame_steady_follow_kernel, dim3((W + SD_TW - 1) / SD_TW, (H + SD_TH - 1) / SD_TH), dim3(SD_THREADS), 0, s,
                       (const h16 *)op->p[0], (const h16 *)op->p[1], (const h16 *)op->p[2], (const uint8_t *)op->p[3], (h16 *)op->p[4],
                       (uint8_t *)op->p[5], (h16 *)op->p[6], (const signed char *)op->p[7], H, W, p);
    return l2d_check_launch("frame_steady_follow", op->tag);
}
