// Re-warm commit: the sink slots 0..F-1 of every (row, k|v, token) line of every layer's KV cache, copied
// from a shadow cache list into the live one in ONE launch.  The reference has no counterpart: its sinks are rewritten only by
// running `prepare` again.
//
// A strided copy and nothing else: no LDS, no arithmetic, no atomics.  The host writes one record per layer (l2d_sink_rec,
// include/l2d.h); every work-group walks all records (there are a few tens) and takes its share of the 16-byte vectors of each, a
// lane keeping SC_UNROLL loads in flight.  A line's sink part is contiguous (F * C * 2 bytes, 5 KB at C = 320), so consecutive lanes
// read and write consecutive vectors; what lies behind it in a destination line -- the window slots F..L-1 -- is never addressed.
// Whole rounds of SC_UNROLL vectors per lane run without a guard between the loads -- with one, the compiler waits for all four
// loads before the first store, 0.62 against 0.55 ms on the cfg-2 caches --; the ragged end goes vector by vector.  Plain loads and
// stores: non-temporal ones measured the same.
#include "common.h"

#define SC_THREADS 256
#define SC_UNROLL 4
#define SC_MAX_BLOCKS 2048

typedef unsigned __attribute__((ext_vector_type(4))) sc_u4;
// the pointers come out of a record in memory: say that they are global, or every access is a flat one
#define SC_GLOBAL __attribute__((address_space(1)))
typedef SC_GLOBAL sc_u4 *sc_gptr;
typedef const SC_GLOBAL sc_u4 *sc_cgptr;

__global__ __launch_bounds__(SC_THREADS) void sink_commit_kernel(const l2d_sink_rec *__restrict__ recs, int n_rec) {
    const unsigned first = blockIdx.x * SC_THREADS + threadIdx.x, step = gridDim.x * SC_THREADS;
    for (int r = 0; r < n_rec; ++r) {
        const l2d_sink_rec rec = recs[r];          // uniform
        // all in units of 16-byte vectors; the launcher checked that lines * pitch (and with it lines * vpl) stays below 2^31
        const unsigned vpl = (unsigned)(rec.line_bytes >> 4), dpv = (unsigned)(rec.dst_pitch >> 4), spv = (unsigned)(rec.src_pitch >> 4);
        const unsigned nvec = (unsigned)rec.lines * vpl;
        sc_gptr dst = (sc_gptr)rec.dst;
        sc_cgptr src = (sc_cgptr)rec.src;
        unsigned base = first;
        // whole rounds: SC_UNROLL loads with nothing between them, then the stores
        for (; base + (SC_UNROLL - 1) * step < nvec; base += step * SC_UNROLL) {
            sc_u4 v[SC_UNROLL];
            unsigned at[SC_UNROLL];
#pragma unroll
            for (int u = 0; u < SC_UNROLL; ++u) {
                const unsigned i = base + u * step, line = i / vpl, w = i - line * vpl;
                at[u] = line * dpv + w;
                v[u] = src[line * spv + w];
            }
#pragma unroll
            for (int u = 0; u < SC_UNROLL; ++u) dst[at[u]] = v[u];
        }
        // the ragged end: fewer than SC_UNROLL vectors of this lane are left
        for (; base < nvec; base += step) {
            const unsigned line = base / vpl, w = base - line * vpl;
            dst[line * dpv + w] = src[line * spv + w];
        }
    }
}

int l2d_launch_sink_commit(const l2d_op *op, hipStream_t s) {
    const l2d_sink_rec *dev = (const l2d_sink_rec *)op->p[0], *host = (const l2d_sink_rec *)op->p[1];
    const int n_rec = op->i[0];
    if (!dev || !host || n_rec <= 0) {
        l2d_set_error("sink_commit(tag %d): invalid arguments (null table or no records)", op->tag);
        return L2D_EINVAL;
    }
    if (((uintptr_t)dev) & 15) {
        l2d_set_error("sink_commit(tag %d): the device table is not 16-byte aligned", op->tag);
        return L2D_EINVAL;
    }
    long long total = 0;
    for (int r = 0; r < n_rec; ++r) {
        const l2d_sink_rec &c = host[r];
        if (!c.dst || !c.src) {
            l2d_set_error("sink_commit(tag %d): record %d has a null %s", op->tag, r, c.dst ? "src" : "dst");
            return L2D_EINVAL;
        }
        if ((((uintptr_t)c.dst) | ((uintptr_t)c.src)) & 15) {
            l2d_set_error("sink_commit(tag %d): record %d: dst or src is not 16-byte aligned", op->tag, r);
            return L2D_EINVAL;
        }
        if (c.lines <= 0) {
            l2d_set_error("sink_commit(tag %d): record %d has %lld lines, need at least one", op->tag, r, (long long)c.lines);
            return L2D_EINVAL;
        }
        if (c.line_bytes <= 0 || c.dst_pitch <= 0 || c.src_pitch <= 0 || ((c.line_bytes | c.dst_pitch | c.src_pitch) & 15)) {
            l2d_set_error("sink_commit(tag %d): record %d: bytes per line %lld, pitches %lld / %lld: need positive multiples of 16", op->tag,
                          r, (long long)c.line_bytes, (long long)c.dst_pitch, (long long)c.src_pitch);
            return L2D_EINVAL;
        }
        if (c.line_bytes > c.dst_pitch || c.line_bytes > c.src_pitch) {
            l2d_set_error("sink_commit(tag %d): record %d: %lld bytes per line do not fit the pitches %lld / %lld", op->tag, r,
                          (long long)c.line_bytes, (long long)c.dst_pitch, (long long)c.src_pitch);
            return L2D_EINVAL;
        }
        // the kernel's offsets are int32 counts of 16-byte vectors (the first comparison keeps the products inside int64)
        const long long pitch = c.dst_pitch > c.src_pitch ? c.dst_pitch : c.src_pitch;
        if (c.lines >= (1ll << 31) || pitch >= (1ll << 35) || c.lines * (pitch >> 4) >= (1ll << 31)) {
            l2d_set_error("sink_commit(tag %d): record %d: %lld lines of pitch %lld do not fit 2^31 16-byte vectors", op->tag, r,
                          (long long)c.lines, pitch);
            return L2D_EINVAL;
        }
        const uintptr_t d0 = (uintptr_t)c.dst, d1 = d0 + (uintptr_t)((c.lines - 1) * c.dst_pitch + c.line_bytes);
        const uintptr_t s0 = (uintptr_t)c.src, s1 = s0 + (uintptr_t)((c.lines - 1) * c.src_pitch + c.line_bytes);
        if (d0 < s1 && s0 < d1) {
            l2d_set_error("sink_commit(tag %d): record %d: the destination range overlaps the source range", op->tag, r);
            return L2D_EINVAL;
        }
        total += c.lines * (c.line_bytes >> 4);
    }
    L2D_DRY_RETURN();
    const long long per_block = (long long)SC_THREADS * SC_UNROLL;
    long long grid = (total + per_block - 1) / per_block;
    if (grid > SC_MAX_BLOCKS) grid = SC_MAX_BLOCKS;
    hipLaunchKernelGGL(sink_commit_kernel, dim3((unsigned)grid), dim3(SC_THREADS), 0, s, dev, n_rec);
    return l2d_check_launch("sink_commit", op->tag);
}
