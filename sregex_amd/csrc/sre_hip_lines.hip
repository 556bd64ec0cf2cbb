/*
 * sre_hip_lines.hip — line mode on the device (sregex_hip.h sre_hip_scan_lines).
 *
 *   split      count the line ends of every 64 KiB tile, exclusive-scan the tile counts in a
 *              launch of its own, then write the line ends in order (wave prefix + LDS);
 *   geometry   per batch: how many lines fit, the segment size, and the stream arrays
 *              (ptrs / lens / seg_first) the scan kernels read;
 *   settle     two counters over the batch's status words instead of the words themselves;
 *   compact    count / scan / scatter of the reported lines' rows behind a running count.
 *
 * A "line end" is the offset of a delimiter, or len for a final line without one: a line's
 * first byte is one past the end in front of it.  No workgroup waits for another; the scans
 * between the passes are single-workgroup launches.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"

namespace {

/* bit j (0..3): byte j of w equals the delimiter (pat = delim x 0x01010101).  Exact: the high
 * bit of every byte of t is set iff that byte of w ^ pat is zero. */
__device__ inline uint32_t
eq_bits4(uint32_t w, uint32_t pat)
{
    const uint32_t y = w ^ pat;
    const uint32_t t = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

/* line ends in aligned chunk c (bit j: byte 16c + j - head), masked to the buffer; the last byte
 * of the buffer ends the final line when it is no delimiter (its end is then len, not its offset) */
__device__ inline uint32_t
chunk_ends(const uint4 v, uint64_t c, uint64_t head, uint64_t len, uint32_t pat)
{
    uint32_t       m = eq_bits4(v.x, pat) | (eq_bits4(v.y, pat) << 4) | (eq_bits4(v.z, pat) << 8) | (eq_bits4(v.w, pat) << 12);
    const uint64_t lo = c * 16, end = head + len;
    if (lo < head || lo + 16 > end) {
        uint32_t valid = 0xFFFFu;
        if (lo < head) valid &= 0xFFFFu << (uint32_t) (head - lo);
        if (lo + 16 > end) valid &= end > lo ? 0xFFFFu >> (uint32_t) (16 - (end - lo)) : 0u;
        m &= valid;
    }
    if (end > lo && end <= lo + 16) m |= 1u << (uint32_t) (end - 1 - lo);
    return m & 0xFFFFu;
}

/* exclusive prefix of v over the workgroup (NT lanes, a multiple of 64), and the total */
template <uint32_t NT>
__device__ inline uint64_t
block_excl_scan(uint64_t v, uint64_t *wsum, uint64_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t       x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < NT / 64; i++) {
        const uint64_t s = wsum[i];
        before += i < w ? s : 0;
        all += s;
    }
    __syncthreads();
    total = all;
    return before + x - v;
}

__device__ inline uint64_t
line_start(const uint64_t *ends, uint64_t i)
{
    return i == 0 ? 0 : ends[i - 1] + 1;
}

/* ---- split ---- */

__global__ __launch_bounds__(SRE_LINES_THREADS) void
sre_k_lines_count(const uint4 *__restrict__ src, uint64_t head, uint64_t len, uint32_t pat, uint64_t *__restrict__ tiles)
{
    __shared__ uint64_t wsum[SRE_LINES_THREADS / 64];
    const uint64_t nchunks = (head + len + 15) / 16;
    const uint64_t c0 = (uint64_t) blockIdx.x * (SRE_LINES_THREADS * SRE_LINES_CHUNKS) + threadIdx.x;
    uint4          v[SRE_LINES_CHUNKS];
#pragma unroll
    for (uint32_t k = 0; k < SRE_LINES_CHUNKS; k++) {
        const uint64_t c = c0 + (uint64_t) k * SRE_LINES_THREADS;
        v[k] = c < nchunks ? src[c] : make_uint4(0, 0, 0, 0);
    }
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < SRE_LINES_CHUNKS; k++) {
        const uint64_t c = c0 + (uint64_t) k * SRE_LINES_THREADS;
        if (c < nchunks) cnt += __popc(chunk_ends(v[k], c, head, len, pat));
    }
    uint64_t total;
    (void) block_excl_scan<SRE_LINES_THREADS>(cnt, wsum, total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

/* in-place exclusive scan of n words by one workgroup (a contiguous run per lane); *total =
 * (accumulate ? *total : 0) + their sum, and the prefixes start there */
__global__ __launch_bounds__(1024) void
sre_k_lines_scan(uint64_t *__restrict__ vals, uint64_t n, uint64_t *__restrict__ total, int accumulate)
{
    __shared__ uint64_t wsum[16];
    const uint64_t      base = accumulate ? *total : 0;
    const uint64_t      per = (n + 1023) / 1024;
    const uint64_t      lo = min(n, (uint64_t) threadIdx.x * per), hi = min(n, lo + per);
    uint64_t            s = 0;
    for (uint64_t i = lo; i < hi; i++) s += vals[i];
    uint64_t all;
    uint64_t run = base + block_excl_scan<1024>(s, wsum, all);
    for (uint64_t i = lo; i < hi; i++) {
        const uint64_t x = vals[i];
        vals[i] = run;
        run += x;
    }
    if (threadIdx.x == 0) *total = base + all;
}

/* the tile's line ends in order: per lane 16 chunk masks, their popcounts packed two to a word
 * (a field sums to at most 256 x 16), one wave-level inclusive scan of the 8 words, the waves'
 * totals through LDS; then chunk k of lane x writes at tile + sum(step totals < k) + prefix */
__global__ __launch_bounds__(SRE_LINES_THREADS) void
sre_k_lines_write(const uint4 *__restrict__ src, uint64_t head, uint64_t len, uint32_t pat, const uint64_t *__restrict__ tiles,
                  uint64_t *__restrict__ ends)
{
    constexpr uint32_t NW = SRE_LINES_THREADS / 64, NP = SRE_LINES_CHUNKS / 2;
    __shared__ uint32_t wsum[NW][NP];
    const uint64_t      nchunks = (head + len + 15) / 16;
    const uint64_t      c0 = (uint64_t) blockIdx.x * (SRE_LINES_THREADS * SRE_LINES_CHUNKS) + threadIdx.x;
    const uint32_t      lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint4               v[SRE_LINES_CHUNKS];
#pragma unroll
    for (uint32_t k = 0; k < SRE_LINES_CHUNKS; k++) {
        const uint64_t c = c0 + (uint64_t) k * SRE_LINES_THREADS;
        v[k] = c < nchunks ? src[c] : make_uint4(0, 0, 0, 0);
    }
    uint32_t m[SRE_LINES_CHUNKS], P[NP], X[NP];
#pragma unroll
    for (uint32_t k = 0; k < SRE_LINES_CHUNKS; k++) {
        const uint64_t c = c0 + (uint64_t) k * SRE_LINES_THREADS;
        m[k] = c < nchunks ? chunk_ends(v[k], c, head, len, pat) : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < NP; i++) X[i] = P[i] = (uint32_t) __popc(m[2 * i]) | ((uint32_t) __popc(m[2 * i + 1]) << 16);
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (uint32_t i = 0; i < NP; i++) {
            const uint32_t y = __shfl_up(X[i], d, 64);
            if (lane >= d) X[i] += y;
        }
    }
    if (lane == 63) {
#pragma unroll
        for (uint32_t i = 0; i < NP; i++) wsum[w][i] = X[i];
    }
    __syncthreads();
    uint64_t off = tiles[blockIdx.x];
#pragma unroll
    for (uint32_t i = 0; i < NP; i++) {
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t q = 0; q < NW; q++) {
            const uint32_t s = wsum[q][i];
            before += q < w ? s : 0u;
            all += s;
        }
        const uint32_t ex = X[i] - P[i] + before;      /* fields never borrow: X >= P field by field */
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t k = 2 * i + h;
            uint64_t       o = off + ((ex >> (16 * h)) & 0xFFFFu);
            uint32_t       bits = m[k];
            const uint64_t lo = (c0 + (uint64_t) k * SRE_LINES_THREADS) * 16;
            while (bits) {
                const uint32_t j = (uint32_t) __ffs(bits) - 1;
                bits &= bits - 1;
                uint64_t pos = lo + j - head;
                if (pos == len - 1 && reinterpret_cast<const uint8_t *>(src)[head + pos] != (uint8_t) pat) pos = len;
                ends[o++] = pos;
            }
            off += (all >> (16 * h)) & 0xFFFFu;
        }
    }
}

/* ---- geometry of one batch ---- */

/* one lane: the longest batch from i0 of at most nmax lines whose capture scratch fits (a single
 * line always does); the rule of the segment size is not monotone in the byte total across a
 * change of the number of rounds, so the search keeps the last size that fitted */
__global__ void
sre_k_lines_plan(const uint64_t *__restrict__ ends, uint64_t i0, uint64_t nmax, uint64_t scratch_max, uint64_t seg_fixed,
                 uint64_t resident, uint64_t seg_cap, sre_lines_info_t *__restrict__ info)
{
    if (threadIdx.x != 0) return;
    const uint64_t s0 = line_start(ends, i0);
    auto bytes = [&](uint64_t i1) { return ends[i1 - 1] - s0 - (i1 - 1 - i0); };
    auto seg_of = [&](uint64_t total) { return seg_fixed ? seg_fixed : sre_scan_auto_segment(total, resident, seg_cap); };
    auto fits = [&](uint64_t i1) { return (i1 - i0) * (seg_of(bytes(i1)) + 16) * 2 <= scratch_max; };
    uint64_t lo = i0 + 1, hi = i0 + nmax;
    if (fits(hi)) {
        lo = hi;
    } else {
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (fits(mid)) lo = mid;
            else hi = mid - 1;
        }
    }
    info->i1 = lo;
    info->bytes = bytes(lo);
    info->seg = seg_of(info->bytes);
}

/* segments of line i (an empty line still takes its EOF step) */
__device__ inline uint64_t
line_segs(const uint64_t *ends, uint64_t i, uint64_t seg)
{
    const uint64_t n = ends[i] - line_start(ends, i);
    return n ? (n + seg - 1) / seg : 1;
}

/* lane x of workgroup b: lines i0 + b * 1024 + 4x .. + 3 */
__global__ __launch_bounds__(256) void
sre_k_lines_geom_count(const uint64_t *__restrict__ ends, uint64_t i0, const sre_lines_info_t *__restrict__ info,
                       uint64_t *__restrict__ blk)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      nb = info->i1 - i0, seg = info->seg;
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint64_t            s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        if (q0 + q < nb) s += line_segs(ends, i0 + q0 + q, seg);
    }
    uint64_t total;
    (void) block_excl_scan<256>(s, wsum, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void
sre_k_lines_geom_write(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ ends, uint64_t i0,
                       const sre_lines_info_t *__restrict__ info, const uint64_t *__restrict__ blk,
                       const uint8_t **__restrict__ ptrs, uint64_t *__restrict__ lens, uint64_t *__restrict__ seg_first)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      nb = info->i1 - i0, seg = info->seg;
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint64_t            k[4], s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        k[q] = q0 + q < nb ? line_segs(ends, i0 + q0 + q, seg) : 0;
        s += k[q];
    }
    uint64_t total;
    uint64_t run = blk[blockIdx.x] + block_excl_scan<256>(s, wsum, total);
    for (uint32_t q = 0; q < 4; q++) {
        const uint64_t j = q0 + q;
        if (j >= nb) break;
        const uint64_t st = line_start(ends, i0 + j);
        ptrs[j] = buf + st;
        lens[j] = ends[i0 + j] - st;
        seg_first[j] = run;
        run += k[q];
        if (j == nb - 1) seg_first[nb] = run;
    }
}

/* ---- geometry of one batch on the NFA tier ---- */

/* one lane: the longest batch from i0 of at most nmax lines whose per-segment working set fits.  The segments
 * of a batch are at most bytes / seg + lines whatever the short-line limit takes away */
__global__ void
sre_k_lines_plan_nfa(const uint64_t *__restrict__ ends, uint64_t i0, uint64_t nmax, uint64_t work_max, uint64_t seg_cost,
                     uint64_t seg_fixed, uint64_t resident, uint64_t seg_cap, sre_lines_info_t *__restrict__ info)
{
    if (threadIdx.x != 0) return;
    const uint64_t s0 = line_start(ends, i0);
    auto bytes = [&](uint64_t i1) { return ends[i1 - 1] - s0 - (i1 - 1 - i0); };
    auto seg_of = [&](uint64_t total) { return seg_fixed ? seg_fixed : sre_scan_auto_segment(total, resident, seg_cap); };
    auto fits = [&](uint64_t i1) { return (bytes(i1) / seg_of(bytes(i1)) + (i1 - i0)) * seg_cost <= work_max; };
    uint64_t lo = i0 + 1, hi = i0 + nmax;
    if (fits(hi)) {
        lo = hi;
    } else {
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (fits(mid)) lo = mid;
            else hi = mid - 1;
        }
    }
    info->i1 = lo;
    info->bytes = bytes(lo);
    info->seg = seg_of(info->bytes);
    info->nshort = 0;
}

/* segments of line i: none for a line the short-line kernel takes */
__device__ inline uint64_t
line_segs_nfa(const uint64_t *ends, uint64_t i, uint64_t seg, uint64_t short_lim)
{
    const uint64_t n = ends[i] - line_start(ends, i);
    if (n < short_lim) return 0;
    return n ? (n + seg - 1) / seg : 1;
}

__global__ __launch_bounds__(256) void
sre_k_lines_geom_count_nfa(const uint64_t *__restrict__ ends, uint64_t i0, uint64_t short_lim,
                           sre_lines_info_t *__restrict__ info, uint64_t *__restrict__ blk)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      nb = info->i1 - i0, seg = info->seg;
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint64_t            s = 0, sh = 0;
    for (uint32_t q = 0; q < 4; q++) {
        if (q0 + q < nb) {
            s += line_segs_nfa(ends, i0 + q0 + q, seg, short_lim);
            sh += ends[i0 + q0 + q] - line_start(ends, i0 + q0 + q) < short_lim ? 1 : 0;
        }
    }
    uint64_t total, nshort;
    (void) block_excl_scan<256>(s, wsum, total);
    (void) block_excl_scan<256>(sh, wsum, nshort);
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = total;
        if (nshort) atomicAdd(reinterpret_cast<unsigned long long *>(&info->nshort), (unsigned long long) nshort);
    }
}

__global__ __launch_bounds__(256) void
sre_k_lines_geom_write_nfa(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ ends, uint64_t i0, uint64_t short_lim,
                           const sre_lines_info_t *__restrict__ info, const uint64_t *__restrict__ blk,
                           const uint8_t **__restrict__ ptrs, uint64_t *__restrict__ lens, uint64_t *__restrict__ seg_first)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      nb = info->i1 - i0, seg = info->seg;
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint64_t            k[4], s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        k[q] = q0 + q < nb ? line_segs_nfa(ends, i0 + q0 + q, seg, short_lim) : 0;
        s += k[q];
    }
    uint64_t total;
    uint64_t run = blk[blockIdx.x] + block_excl_scan<256>(s, wsum, total);
    for (uint32_t q = 0; q < 4; q++) {
        const uint64_t j = q0 + q;
        if (j >= nb) break;
        const uint64_t st = line_start(ends, i0 + j);
        ptrs[j] = buf + st;
        lens[j] = ends[i0 + j] - st;
        seg_first[j] = run;
        run += k[q];
        if (j == nb - 1) seg_first[nb] = run;
    }
}

/* ---- settle counters ---- */

__global__ __launch_bounds__(256) void
sre_k_lines_settle(const sre_stream_status_t *__restrict__ status, uint32_t n, sre_lines_info_t *__restrict__ info)
{
    __shared__ uint64_t wsum[4];
    uint64_t            pending = 0, maps = 0;
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < n; s += gridDim.x * 256u) {
        pending += status[s].done ? 0 : 1;
        maps += status[s].need_maps ? 1 : 0;
    }
    uint64_t tp, tm;
    (void) block_excl_scan<256>(pending, wsum, tp);
    (void) block_excl_scan<256>(maps, wsum, tm);
    if (threadIdx.x == 0) {
        if (tp) atomicAdd(reinterpret_cast<unsigned long long *>(&info->pending), (unsigned long long) tp);
        if (tm) atomicAdd(reinterpret_cast<unsigned long long *>(&info->maps), (unsigned long long) tm);
    }
}

/* ---- compaction ---- */

/* the row rule of line mode (sre_lines_select.h): the hits, or every line with `all` */
__device__ inline uint32_t
reported(const int64_t *records, uint32_t slots, uint64_t j, int all)
{
    return sre_sel_row(records + j * slots, SRE_DECLINED, all ? 2 : 0);
}

__global__ __launch_bounds__(256) void
sre_k_lines_flag_count(const int64_t *__restrict__ records, uint32_t slots, uint64_t i0, int all,
                       const sre_lines_info_t *__restrict__ info, uint64_t *__restrict__ blk)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      nb = info->i1 - i0;
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint64_t            s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        if (q0 + q < nb) s += reported(records, slots, q0 + q, all);
    }
    uint64_t total;
    (void) block_excl_scan<256>(s, wsum, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void
sre_k_lines_scatter(const int64_t *__restrict__ records, uint32_t slots, uint64_t i0, int all,
                    const uint64_t *__restrict__ ends, const sre_lines_info_t *__restrict__ info,
                    const uint64_t *__restrict__ blk, int64_t *__restrict__ rows, uint64_t cap)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      nb = info->i1 - i0;
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint32_t            f[4], s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        f[q] = q0 + q < nb ? reported(records, slots, q0 + q, all) : 0u;
        s += f[q];
    }
    uint64_t total;
    uint64_t r = blk[blockIdx.x] + block_excl_scan<256>(s, wsum, total);
    for (uint32_t q = 0; q < 4; q++) {
        if (!f[q]) continue;
        if (r < cap) {
            const uint64_t j = q0 + q, st = line_start(ends, i0 + j);
            int64_t       *row = rows + r * (3 + (uint64_t) slots);
            const int64_t *rec = records + j * slots;
            row[0] = (int64_t) (i0 + j);
            row[1] = (int64_t) st;
            row[2] = (int64_t) (ends[i0 + j] - st);
            for (uint32_t x = 0; x < slots; x++) row[3 + x] = rec[x];
        }
        r++;
    }
}

}  // namespace

extern "C" hipError_t
sre_launch_lines_count(const void *d_buf, uint64_t len, uint32_t delim, uint64_t *d_tiles, sre_lines_info_t *d_info,
                       hipStream_t stream)
{
    const uint64_t head = reinterpret_cast<uintptr_t>(d_buf) & 15u;
    const uint4   *src = reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(d_buf) - head);
    const uint64_t ntiles = (head + len + SRE_LINES_TILE_BYTES - 1) / SRE_LINES_TILE_BYTES;
    if (ntiles == 0) return hipSuccess;
    hipLaunchKernelGGL(sre_k_lines_count, dim3((uint32_t) ntiles), dim3(SRE_LINES_THREADS), 0, stream, src, head, len,
                       delim * 0x01010101u, d_tiles);
    hipLaunchKernelGGL(sre_k_lines_scan, dim3(1), dim3(1024), 0, stream, d_tiles, ntiles, &d_info->nlines, 0);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_lines_write(const void *d_buf, uint64_t len, uint32_t delim, const uint64_t *d_tiles, uint64_t *d_ends,
                       hipStream_t stream)
{
    const uint64_t head = reinterpret_cast<uintptr_t>(d_buf) & 15u;
    const uint4   *src = reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(d_buf) - head);
    const uint64_t ntiles = (head + len + SRE_LINES_TILE_BYTES - 1) / SRE_LINES_TILE_BYTES;
    if (ntiles == 0) return hipSuccess;
    hipLaunchKernelGGL(sre_k_lines_write, dim3((uint32_t) ntiles), dim3(SRE_LINES_THREADS), 0, stream, src, head, len,
                       delim * 0x01010101u, d_tiles, d_ends);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_lines_geometry(const void *d_buf, const uint64_t *d_ends, uint64_t nlines, uint64_t i0, uint64_t nmax,
                          uint64_t scratch_max, uint64_t seg_fixed, uint64_t resident, uint64_t seg_cap,
                          const uint8_t **d_ptrs, uint64_t *d_lens, uint64_t *d_seg_first, uint64_t *d_blk,
                          sre_lines_info_t *d_info, hipStream_t stream)
{
    if (nmax == 0 || i0 + nmax > nlines) return hipErrorInvalidValue;
    const uint32_t nblk = (uint32_t) ((nmax + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS);
    hipLaunchKernelGGL(sre_k_lines_plan, dim3(1), dim3(64), 0, stream, d_ends, i0, nmax, scratch_max, seg_fixed, resident,
                       seg_cap, d_info);
    hipLaunchKernelGGL(sre_k_lines_geom_count, dim3(nblk), dim3(256), 0, stream, d_ends, i0, d_info, d_blk);
    hipLaunchKernelGGL(sre_k_lines_scan, dim3(1), dim3(1024), 0, stream, d_blk, (uint64_t) nblk, &d_info->nsegs, 0);
    hipLaunchKernelGGL(sre_k_lines_geom_write, dim3(nblk), dim3(256), 0, stream, static_cast<const uint8_t *>(d_buf), d_ends,
                       i0, d_info, d_blk, d_ptrs, d_lens, d_seg_first);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_lines_geometry_nfa(const void *d_buf, const uint64_t *d_ends, uint64_t nlines, uint64_t i0, uint64_t nmax,
                              uint64_t short_lim, uint64_t work_max, uint64_t seg_cost, uint64_t seg_fixed, uint64_t resident,
                              uint64_t seg_cap, const uint8_t **d_ptrs, uint64_t *d_lens, uint64_t *d_seg_first,
                              uint64_t *d_blk, sre_lines_info_t *d_info, hipStream_t stream)
{
    if (nmax == 0 || i0 + nmax > nlines || seg_cost == 0) return hipErrorInvalidValue;
    const uint32_t nblk = (uint32_t) ((nmax + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS);
    hipLaunchKernelGGL(sre_k_lines_plan_nfa, dim3(1), dim3(64), 0, stream, d_ends, i0, nmax, work_max, seg_cost, seg_fixed,
                       resident, seg_cap, d_info);
    hipLaunchKernelGGL(sre_k_lines_geom_count_nfa, dim3(nblk), dim3(256), 0, stream, d_ends, i0, short_lim, d_info, d_blk);
    hipLaunchKernelGGL(sre_k_lines_scan, dim3(1), dim3(1024), 0, stream, d_blk, (uint64_t) nblk, &d_info->nsegs, 0);
    hipLaunchKernelGGL(sre_k_lines_geom_write_nfa, dim3(nblk), dim3(256), 0, stream, static_cast<const uint8_t *>(d_buf),
                       d_ends, i0, short_lim, d_info, d_blk, d_ptrs, d_lens, d_seg_first);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_lines_settle(const sre_stream_status_t *d_status, uint32_t n, sre_lines_info_t *d_info, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(&d_info->pending, 0, 2 * sizeof(uint64_t), stream);
    if (e != hipSuccess || n == 0) return e;
    const uint32_t want = (n + 255u) / 256u, grid = want < 2048u ? want : 2048u;
    hipLaunchKernelGGL(sre_k_lines_settle, dim3(grid), dim3(256), 0, stream, d_status, n, d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_lines_compact(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0, int all,
                         const uint64_t *d_ends, uint64_t *d_blk, sre_lines_info_t *d_info, int64_t *d_rows, uint64_t cap,
                         hipStream_t stream)
{
    if (nmax == 0) return hipSuccess;
    const uint32_t nblk = (uint32_t) ((nmax + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS);
    hipLaunchKernelGGL(sre_k_lines_flag_count, dim3(nblk), dim3(256), 0, stream, d_records, slots, i0, all, d_info, d_blk);
    hipLaunchKernelGGL(sre_k_lines_scan, dim3(1), dim3(1024), 0, stream, d_blk, (uint64_t) nblk, &d_info->reported, 1);
    hipLaunchKernelGGL(sre_k_lines_scatter, dim3(nblk), dim3(256), 0, stream, d_records, slots, i0, all, d_ends, d_info,
                       d_blk, d_rows, cap);
    return hipGetLastError();
}
