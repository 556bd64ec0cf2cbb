/*
 * sre_hip_lines_context.hip — the context pass of the line filter (sregex_hip.h sre_hip_filter_lines_context, DESIGN.md
 * §4.11.5): grep -A / -B / -C as a dilation of the filter's per-line values, between the last batch's select pass and
 * the scan to the offset table.  Line i is matched when val[i] > 0; the pass gives every line within `after` lines
 * behind a matched line or `before` lines in front of one its value len + 1 too, so that the filter's scan, gather and
 * cut see it as selected.
 *
 *   marks      per workgroup of 1024 lines: the block words, its last and its first matched line;
 *   carry      one workgroup: a forward maximum scan of the last lines and a backward minimum scan of the first ones
 *              turn the block words into p_in / q_in, the nearest matched line in front of / behind each block;
 *   apply      per workgroup: the same two scans over its 1024 lines (shuffles inside a wave, one exchange through
 *              LDS between its four waves), seeded with p_in / q_in; the selection rule of sre_lines_context.h; the
 *              values of the context-only lines, the context bitmap, the block's counts of matched lines and groups;
 *   totals     one workgroup: the sums of the counts, into the words the host reads with the filter's four;
 *   index      the filter's rows with a fifth word: context-only (from the bitmap) and first line of a group.
 *
 * The cost per line does not depend on before and after: nothing here looks at a line's neighbours one by one.
 *
 * IN PLACE AND RACE-FREE.  apply reads val only inside its own workgroup's 1024 lines, every lane its own four words
 * before it writes any of them, and writes only there.  What it needs from the other workgroups are the block words,
 * which marks took from the ORIGINAL values and carry finished before apply starts: separate launches on one stream.
 * No kernel reads a val that another workgroup of the same launch writes.
 *
 * Without context (before == after == 0) none of the three kernels runs; the groups are then counted from the offset
 * table (runs), which says the same: every selected line is matched.
 *
 * No workgroup waits for another.  Plain C++ and vector memory operations only.
 */
#include "sre_hip_lines.h"
#include "sre_lines_context.h"
#include "sre_hip_lines_block.h"

static_assert(SRE_LC_ITEMS == SRE_LINES_ITEMS && SRE_LC_THREADS * SRE_LC_PER_LANE == SRE_LC_ITEMS, "one geometry");

namespace {

/* lane x of workgroup b: lines b * 1024 + 4x .. + 3 (0 beyond n) */
__device__ inline void
load_values(const uint64_t *__restrict__ val, uint64_t n, uint64_t q0, uint64_t v[SRE_LC_PER_LANE])
{
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) v[k] = q0 + k < n ? val[q0 + k] : 0;
}

/* ---- marks ---- */

/* last[b] = the P word of workgroup b's last matched line, first[b] = the Q word of its first one */
__global__ __launch_bounds__(SRE_LC_THREADS) void
sre_k_context_marks(const uint64_t *__restrict__ val, uint64_t n, uint64_t *__restrict__ last, uint64_t *__restrict__ first)
{
    __shared__ uint32_t wp[SRE_LC_WAVES], wq[SRE_LC_WAVES];
    const uint64_t      base = (uint64_t) blockIdx.x * SRE_LC_ITEMS;
    uint64_t            v[SRE_LC_PER_LANE];
    load_values(val, n, base + SRE_LC_PER_LANE * threadIdx.x, v);
    uint32_t p, q, ptot, qtot;
    sre_lc_lane_marks(v, threadIdx.x, &p, &q);
    block_excl_marks<uint32_t, SRE_LC_WAVES>(p, q, wp, wq, ptot, qtot);
    if (threadIdx.x == 0) {
        last[blockIdx.x] = sre_lc_p_global(base, ptot, 0);
        first[blockIdx.x] = sre_lc_q_global(base, qtot, SRE_LC_NONE);
    }
}

/* ---- carry ---- */

/* one workgroup over the nblk block words, a contiguous run per lane (as sre_k_filter_scan): last[b] becomes p_in of
 * workgroup b, first[b] its q_in */
__global__ __launch_bounds__(SRE_LC_CARRY_LANES) void
sre_k_context_carry(uint64_t *__restrict__ last, uint64_t *__restrict__ first, uint64_t nblk)
{
    __shared__ uint64_t wp[SRE_LC_CARRY_LANES / 64], wq[SRE_LC_CARRY_LANES / 64];
    const uint64_t      per = (nblk + SRE_LC_CARRY_LANES - 1) / SRE_LC_CARRY_LANES;
    const uint64_t      lo = min(nblk, (uint64_t) threadIdx.x * per), hi = min(nblk, lo + per);
    uint64_t            p, q, ptot, qtot;
    sre_lc_run_marks(last, first, lo, hi, &p, &q);
    block_excl_marks<uint64_t, SRE_LC_CARRY_LANES / 64>(p, q, wp, wq, ptot, qtot);
    sre_lc_run_carry(last, first, lo, hi, p, q);
}

/* ---- apply ---- */

/* workgroup b: its 1024 values in place, its 16 words of the bitmap (nwords = ceil(n / 64) in all), its counts */
__global__ __launch_bounds__(SRE_LC_THREADS) void
sre_k_context_apply(uint64_t *__restrict__ val, const uint64_t *__restrict__ ends, uint64_t n, uint64_t before, uint64_t after,
                    const uint64_t *__restrict__ pin, const uint64_t *__restrict__ qin, uint64_t *__restrict__ bits,
                    uint64_t *__restrict__ blkm, uint64_t *__restrict__ blkg)
{
    __shared__ uint32_t wp[SRE_LC_WAVES], wq[SRE_LC_WAVES], cm[SRE_LC_WAVES], cg[SRE_LC_WAVES];
    const uint32_t      lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t      base = (uint64_t) blockIdx.x * SRE_LC_ITEMS, q0 = base + SRE_LC_PER_LANE * threadIdx.x;
    uint64_t            v[SRE_LC_PER_LANE];
    load_values(val, n, q0, v);
    uint32_t p, q, ptot, qtot;
    sre_lc_lane_marks(v, threadIdx.x, &p, &q);
    block_excl_marks<uint32_t, SRE_LC_WAVES>(p, q, wp, wq, ptot, qtot);
    uint32_t fl[SRE_LC_PER_LANE];
    sre_lc_lane_lines(q0, n, v, sre_lc_p_global(base, p, pin[blockIdx.x]), sre_lc_q_global(base, q, qin[blockIdx.x]), before,
                      after, fl);
    uint64_t bm[SRE_LC_PER_LANE], bc[SRE_LC_PER_LANE], bg[SRE_LC_PER_LANE];
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
        /* (a context-only line is a line of the buffer: sre_lc_line gives no bit beyond n) */
        if (fl[k] & SRE_LC_CONTEXT) val[q0 + k] = ends[q0 + k] - line_start(ends, q0 + k) + 1;
        bm[k] = __ballot(v[k] != 0);
        bc[k] = __ballot((fl[k] & SRE_LC_CONTEXT) != 0);
        bg[k] = __ballot((fl[k] & SRE_LC_GROUP) != 0);
    }
    /* the wave's 256 lines are four whole words of the bitmap: lanes 0 .. 3 store one each */
    const uint64_t word = base / 64 + (SRE_LC_WAVE * SRE_LC_PER_LANE / 64) * w + lane;
    if (lane < SRE_LC_WAVE * SRE_LC_PER_LANE / 64 && word < (n + 63) / 64) bits[word] = sre_lc_bitmap_word(bc, lane);
    if (lane == 0) {
        cm[w] = sre_lc_count(bm);
        cg[w] = sre_lc_count(bg);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t m = 0, g = 0;
        for (uint32_t i = 0; i < SRE_LC_WAVES; i++) {
            m += cm[i];
            g += cg[i];
        }
        blkm[blockIdx.x] = m;
        blkg[blockIdx.x] = g;
    }
}

/* ---- runs, totals ---- */

/* without context: the groups of workgroup b's lines from the offset table (line i is selected iff off[i + 1] > off[i]) */
__global__ __launch_bounds__(SRE_LC_THREADS) void
sre_k_context_runs(const uint64_t *__restrict__ off, uint64_t n, uint64_t *__restrict__ blkg)
{
    __shared__ uint64_t wsum[SRE_LC_WAVES];
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LC_ITEMS + SRE_LC_PER_LANE * threadIdx.x;
    uint64_t            s = 0;
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
        const uint64_t i = q0 + k;
        if (i < n && off[i + 1] > off[i] && (i == 0 || off[i] == off[i - 1])) s++;
    }
    uint64_t total;
    (void) block_excl_scan<SRE_LC_THREADS>(s, wsum, total);
    if (threadIdx.x == 0) blkg[blockIdx.x] = total;
}

/* one workgroup: info->cgroups = the sum of blkg, info->cmatched = the sum of blkm (no blkm: the call has no context) */
__global__ __launch_bounds__(1024) void
sre_k_context_totals(const uint64_t *__restrict__ blkm, const uint64_t *__restrict__ blkg, uint64_t nblk,
                     sre_lines_info_t *__restrict__ info)
{
    __shared__ uint64_t wsum[16];
    uint64_t            m = 0, g = 0;
    for (uint64_t i = threadIdx.x; i < nblk; i += 1024) {
        m += blkm ? blkm[i] : 0;
        g += blkg[i];
    }
    uint64_t tm, tg;
    (void) block_excl_scan<1024>(m, wsum, tm);
    (void) block_excl_scan<1024>(g, wsum, tg);
    if (threadIdx.x == 0) {
        info->cmatched = tm;
        info->cgroups = tg;
    }
}

/* ---- index ---- */

/* sre_k_filter_index with rows of five words: [4] bit 0 from the context bitmap (no bitmap: the call has no context),
 * bit 1 for line 0 or a line whose predecessor is not selected, off[i] == off[i - 1] */
__global__ __launch_bounds__(256) void
sre_k_context_index(const uint64_t *__restrict__ off, const uint64_t *__restrict__ ends, uint64_t n,
                    const uint64_t *__restrict__ blkc, const uint64_t *__restrict__ bits, const sre_lines_info_t *__restrict__ info,
                    uint64_t index_cap, int64_t *__restrict__ rows)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      limit = index_cap < info->fwritten ? index_cap : info->fwritten;
    if (blkc[blockIdx.x] >= limit) return;      /* (the whole workgroup) */
    const uint64_t q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint32_t       f[4];
    uint64_t       s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        f[q] = q0 + q < n && off[q0 + q + 1] > off[q0 + q];
        s += f[q];
    }
    uint64_t total;
    uint64_t r = blkc[blockIdx.x] + block_excl_scan<256>(s, wsum, total);
    for (uint32_t q = 0; q < 4; q++) {
        if (!f[q]) continue;
        if (r < limit) {
            const uint64_t i = q0 + q, st = line_start(ends, i);
            const bool     ctx = bits != nullptr && ((bits[i / 64] >> (i % 64)) & 1u) != 0;
            const bool     group = i == 0 || off[i] == off[i - 1];
            int64_t       *row = rows + r * 5;
            row[0] = (int64_t) i;
            row[1] = (int64_t) st;
            row[2] = (int64_t) (ends[i] - st);
            row[3] = (int64_t) off[i];
            row[4] = (int64_t) ((ctx ? SRE_LC_CONTEXT : 0u) | (group ? SRE_LC_GROUP : 0u));
        }
        r++;
    }
}

}  // namespace

extern "C" hipError_t
sre_launch_context_select(uint64_t *d_val, const uint64_t *d_ends, uint64_t n, uint64_t before, uint64_t after, uint64_t *d_bits,
                          uint64_t *d_blk, sre_lines_info_t *d_info, hipStream_t stream)
{
    if (n == 0) return hipErrorInvalidValue;
    const uint64_t nblk = (n + SRE_LC_ITEMS - 1) / SRE_LC_ITEMS;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    uint64_t *pin = d_blk, *qin = d_blk + nblk, *blkm = d_blk + 2 * nblk, *blkg = d_blk + 3 * nblk;
    hipLaunchKernelGGL(sre_k_context_marks, dim3((uint32_t) nblk), dim3(SRE_LC_THREADS), 0, stream, d_val, n, pin, qin);
    hipLaunchKernelGGL(sre_k_context_carry, dim3(1), dim3(SRE_LC_CARRY_LANES), 0, stream, pin, qin, nblk);
    hipLaunchKernelGGL(sre_k_context_apply, dim3((uint32_t) nblk), dim3(SRE_LC_THREADS), 0, stream, d_val, d_ends, n, before, after,
                       pin, qin, d_bits, blkm, blkg);
    hipLaunchKernelGGL(sre_k_context_totals, dim3(1), dim3(1024), 0, stream, blkm, blkg, nblk, d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_context_runs(const uint64_t *d_off, uint64_t n, uint64_t *d_blk, sre_lines_info_t *d_info, hipStream_t stream)
{
    if (n == 0) return hipErrorInvalidValue;
    const uint64_t nblk = (n + SRE_LC_ITEMS - 1) / SRE_LC_ITEMS;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_context_runs, dim3((uint32_t) nblk), dim3(SRE_LC_THREADS), 0, stream, d_off, n, d_blk);
    hipLaunchKernelGGL(sre_k_context_totals, dim3(1), dim3(1024), 0, stream, static_cast<const uint64_t *>(nullptr), d_blk, nblk,
                       d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_context_index(const uint64_t *d_off, const uint64_t *d_ends, uint64_t n, const uint64_t *d_blk, const uint64_t *d_bits,
                         const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index, hipStream_t stream)
{
    if (n == 0 || index_cap == 0) return hipSuccess;
    const uint64_t nblk = (n + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    hipLaunchKernelGGL(sre_k_context_index, dim3((uint32_t) nblk), dim3(256), 0, stream, d_off, d_ends, n, d_blk + nblk, d_bits,
                       d_info, index_cap, d_index);
    return hipGetLastError();
}
