/*
 * sre_hip_lines_gather.hip — the line filter on the device (sregex_hip.h sre_hip_filter_lines).
 *
 *   select     per batch: val[i] = len + 1 of a selected line, 0 of the others, from the batch's records.  The kernels
 *              only index: the rules are sre_lines_select.h's, which the host route and the CPU models compile too;
 *   scan       after the last batch: val becomes the offset table off[0 .. n] in place (per-workgroup sums, a
 *              single-workgroup scan of the sums, then the prefixes), the sums of the selected lines stay in
 *              blk for the index; `finish` cuts the output at whole lines that fit out_cap;
 *   gather     output-driven: a workgroup owns 16 KiB of the output, a lane builds 16-byte chunks of it at a
 *              stride of the workgroup with the chunk logic of sre_lines_gather.h;
 *   index      the rows [line, start, len, output offset] of the first written lines.
 *
 * The line extract (sre_hip_extract_lines) runs the same passes over a table of entries
 * e = line * K + f, one per chosen capture group of a line: its own select (field length + 1 and the field's
 * source offset, from the batch's records), the same scan kernels over n * K entries with the cut made at a line
 * boundary, the gather over the entry table (sre_lg_tab_fields) and index rows of 4 + 2 K words.
 *
 * The line substitute (sre_hip_substitute_lines) runs them over a table of pieces e = line * P + f:
 * the text in front of the first match, the template's pieces, the text behind the match and the delimiter.  Entries of
 * a selected line may be empty there, so its sums, finish and index count LINES by their last entries, which always
 * take a byte; the gather is the same chunk walk over sre_lg_tab_pieces with the literal block as a second source.
 *
 * The line join (sre_hip_join_lines) fills its table of entries e = line * P + f, the line and P - 1
 * values of its dictionary row, in a pass of its own (sre_hip_lines_keyset.hip); every entry of a selected line takes a
 * byte, so the extract's scan and finish run over it as they are, the gather is the same chunk walk over sre_lg_tab_join
 * with the key map's copy of the dictionary as the second source, and the index rows have 5 + 2 (P - 1) words.
 *
 * No workgroup waits for another.  Plain C++ and vector memory operations only.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"
#include "sre_lines_gather.h"
#include "sre_hip_tile.h"
#include "sre_hip_lines_block.h"

namespace {

/* ---- select ---- */

/* lane per line of the batch (lines i0 .. info->i1): the rows of sre_sel_row under mode 0 / 1 / 2 */
__global__ __launch_bounds__(256) void
sre_k_filter_select(const int64_t *__restrict__ records, uint32_t slots, uint64_t i0, int mode,
                    const uint64_t *__restrict__ ends, const sre_lines_info_t *__restrict__ info, uint64_t *__restrict__ val)
{
    const uint64_t nb = info->i1 - i0;
    const uint64_t j = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (j >= nb) return;
    const uint64_t i = i0 + j;
    val[i] = sre_sel_row(records + j * slots, SRE_DECLINED, mode) ? ends[i] - line_start(ends, i) + 1 : 0;
}

/* the line extract's: LANE PER ENTRY of the batch, entry x = j * K + f of line i0 + j.  The stores of val and start
 * are then consecutive words of consecutive lanes; the K lanes of a line read the same record, whose two ovector
 * words lie in the cache lines the neighbouring lanes read too (a lane per line would read the same records and
 * scatter 2 K stores at a stride of K words).  The two words are sre_sel_extract_entry's */
__global__ __launch_bounds__(256) void
sre_k_extract_select(const int64_t *__restrict__ records, uint32_t slots, uint64_t i0, int all, sre_extract_groups_t gr,
                     const uint64_t *__restrict__ ends, const sre_lines_info_t *__restrict__ info, uint64_t *__restrict__ val,
                     uint64_t *__restrict__ start)
{
    const uint64_t nb = info->i1 - i0;
    const uint64_t x = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (x >= nb * gr.k) return;
    const uint32_t j = (uint32_t) x / gr.k, f = (uint32_t) x - j * gr.k;       /* (a batch has fewer than 2^32 entries) */
    const uint64_t i = i0 + j, st = line_start(ends, i), len = ends[i] - st;
    const uint64_t e = (i0 * gr.k) + x;
    sre_sel_extract_entry(records + (uint64_t) j * slots, SRE_DECLINED, all, st, len, f, gr.k, gr.g[f], val + e, start + e);
}

/* the line substitute's: LANE PER ENTRY of the batch, entry x = j * P + f of line i0 + j, P = pieces + 2; the two words
 * are sre_sel_subst_entry's */
__global__ __launch_bounds__(256) void
sre_k_subst_select(const int64_t *__restrict__ records, uint32_t slots, uint64_t i0, int all, sre_subst_pieces_t pc,
                   const uint64_t *__restrict__ ends, const sre_lines_info_t *__restrict__ info, uint64_t *__restrict__ val,
                   uint64_t *__restrict__ start)
{
    const uint64_t nb = info->i1 - i0;
    const uint32_t P = pc.np + 2;
    const uint64_t x = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (x >= nb * P) return;
    const uint32_t j = (uint32_t) x / P, f = (uint32_t) x - j * P;             /* (a batch has fewer than 2^32 entries) */
    const uint64_t i = i0 + j, st = line_start(ends, i), len = ends[i] - st;
    const uint64_t e = (i0 * P) + x;
    sre_sel_subst_entry(records + (uint64_t) j * slots, SRE_DECLINED, all, st, len, f, &pc, val + e, start + e);
}

/* ---- scan ---- */

/* lane x of workgroup b: lines b * 1024 + 4x .. + 3; the workgroup's bytes and selected lines */
__global__ __launch_bounds__(256) void
sre_k_filter_sums(const uint64_t *__restrict__ val, uint64_t n, uint64_t *__restrict__ blkv, uint64_t *__restrict__ blkc)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint64_t            s = 0, k = 0;
    for (uint32_t q = 0; q < 4; q++) {
        if (q0 + q < n) {
            const uint64_t v = val[q0 + q];
            s += v;
            k += v ? 1 : 0;
        }
    }
    uint64_t ts, tk;
    (void) block_excl_scan<256>(s, wsum, ts);
    (void) block_excl_scan<256>(k, wsum, tk);
    if (threadIdx.x == 0) {
        blkv[blockIdx.x] = ts;
        blkc[blockIdx.x] = tk;
    }
}

/* in-place exclusive scan of the two arrays of n sums by one workgroup (a contiguous run per lane);
 * info->fneed / fsel = their totals */
__global__ __launch_bounds__(1024) void
sre_k_filter_scan(uint64_t *__restrict__ blkv, uint64_t *__restrict__ blkc, uint64_t n, sre_lines_info_t *__restrict__ info)
{
    __shared__ uint64_t wsum[16];
    const uint64_t      per = (n + 1023) / 1024;
    const uint64_t      lo = min(n, (uint64_t) threadIdx.x * per), hi = min(n, lo + per);
    uint64_t            s = 0, k = 0;
    for (uint64_t i = lo; i < hi; i++) {
        s += blkv[i];
        k += blkc[i];
    }
    uint64_t ts, tk;
    uint64_t rs = block_excl_scan<1024>(s, wsum, ts);
    uint64_t rk = block_excl_scan<1024>(k, wsum, tk);
    for (uint64_t i = lo; i < hi; i++) {
        const uint64_t x = blkv[i], y = blkc[i];
        blkv[i] = rs;
        blkc[i] = rk;
        rs += x;
        rk += y;
    }
    if (threadIdx.x == 0) {
        info->fneed = ts;
        info->fsel = tk;
    }
}

/* val[0 .. n) becomes off[0 .. n] in place: a lane reads its own four values before it writes them */
__global__ __launch_bounds__(256) void
sre_k_filter_offsets(uint64_t *__restrict__ val, uint64_t n, const uint64_t *__restrict__ blkv)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint64_t            v[4], s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        v[q] = q0 + q < n ? val[q0 + q] : 0;
        s += v[q];
    }
    uint64_t total;
    uint64_t run = blkv[blockIdx.x] + block_excl_scan<256>(s, wsum, total);
    for (uint32_t q = 0; q < 4; q++) {
        if (q0 + q >= n) break;
        val[q0 + q] = run;
        run += v[q];
        if (q0 + q == n - 1) val[n] = run;
    }
}

/* one workgroup: the first line i whose end lies beyond out_cap (n when all fit) cuts the output:
 * info->fbytes = off[i], info->fwritten = selected lines in front of i */
__global__ __launch_bounds__(1024) void
sre_k_filter_finish(const uint64_t *__restrict__ off, uint64_t n, const uint64_t *__restrict__ blkc, uint64_t out_cap,
                    sre_lines_info_t *__restrict__ info)
{
    __shared__ uint64_t cut;
    if (threadIdx.x == 0) {
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (off[mid + 1] > out_cap) hi = mid;
            else lo = mid + 1;
        }
        cut = lo;
    }
    __syncthreads();
    const uint64_t i = cut, b = i / SRE_LINES_ITEMS, j = b * SRE_LINES_ITEMS + threadIdx.x;
    const int      before = __syncthreads_count(j < i && off[j + 1] > off[j]);
    if (threadIdx.x == 0) {
        info->fbytes = off[i];
        info->fwritten = i == n ? info->fsel : blkc[b] + (uint64_t) before;
    }
}

/* the same over the entry table of n lines x k fields: the cut is the first LINE i with off[(i + 1) k] > out_cap,
 * so a row is written whole or not at all.  The sums counted selected entries; all k entries of a selected line
 * are selected, so the entries in front of a line boundary divide by k exactly: info->fsel and info->fwritten
 * become counts of lines.  (k need not divide the entries of a workgroup: the boundary entry i k lies anywhere in
 * its workgroup, and the count in front of it is taken there.) */
__global__ __launch_bounds__(1024) void
sre_k_extract_finish(const uint64_t *__restrict__ off, uint64_t n, uint64_t k, const uint64_t *__restrict__ blkc,
                     uint64_t out_cap, sre_lines_info_t *__restrict__ info)
{
    __shared__ uint64_t cut;
    if (threadIdx.x == 0) cut = sre_lg_row_cut(off, n, k, out_cap);
    __syncthreads();
    const uint64_t i = cut, e = i * k, b = e / SRE_LINES_ITEMS, j = b * SRE_LINES_ITEMS + threadIdx.x;
    const int      before = __syncthreads_count(j < e && off[j + 1] > off[j]);
    if (threadIdx.x == 0) {
        const uint64_t sel = info->fsel / k;
        info->fsel = sel;
        info->fbytes = off[e];
        info->fwritten = i == n ? sel : (blkc[b] + (uint64_t) before) / k;
    }
}

/* the line substitute's sums over n entries of lines of p pieces: the workgroup's bytes as sre_k_filter_sums has them,
 * and its selected LINES.  Entries of a selected line may be empty here, but its last one (e % p == p - 1) always
 * takes the delimiter: the lines are the last entries with a value */
__global__ __launch_bounds__(256) void
sre_k_subst_sums(const uint64_t *__restrict__ val, uint64_t n, uint64_t p, uint64_t *__restrict__ blkv, uint64_t *__restrict__ blkc)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint64_t            s = 0, k = 0, r = q0 % p;
    for (uint32_t q = 0; q < 4; q++) {
        if (q0 + q < n) {
            const uint64_t v = val[q0 + q];
            s += v;
            k += (v && r == p - 1) ? 1 : 0;
        }
        r = r + 1 == p ? 0 : r + 1;
    }
    uint64_t ts, tk;
    (void) block_excl_scan<256>(s, wsum, ts);
    (void) block_excl_scan<256>(k, wsum, tk);
    if (threadIdx.x == 0) {
        blkv[blockIdx.x] = ts;
        blkc[blockIdx.x] = tk;
    }
}

/* the cut at a line boundary as sre_k_extract_finish makes it; info->fsel counts lines already, and the written lines
 * in front of the boundary entry i p are the selected last entries in front of it */
__global__ __launch_bounds__(1024) void
sre_k_subst_finish(const uint64_t *__restrict__ off, uint64_t n, uint64_t p, const uint64_t *__restrict__ blkc,
                   uint64_t out_cap, sre_lines_info_t *__restrict__ info)
{
    __shared__ uint64_t cut;
    if (threadIdx.x == 0) cut = sre_lg_row_cut(off, n, p, out_cap);
    __syncthreads();
    const uint64_t i = cut, e = i * p, b = e / SRE_LINES_ITEMS, j = b * SRE_LINES_ITEMS + threadIdx.x;
    const int      before = __syncthreads_count(j < e && j % p == p - 1 && off[j + 1] > off[j]);
    if (threadIdx.x == 0) {
        info->fbytes = off[e];
        info->fwritten = i == n ? info->fsel : blkc[b] + (uint64_t) before;
    }
}

/* ---- gather ---- */

typedef const __attribute__((address_space(1))) sre_u32x4_unaligned *lg_unaligned_ptr;

/* 16-byte loads and stores of the two aligned extents (sre_lines_gather.h) */
struct GatherMem {
    const uint8_t *src;         /* the 16-byte aligned address at or below d_buf */
    uint8_t       *dst;         /* ... at or below d_out */

    __device__ inline sre_lg_u128 load(uint64_t q) const
    {
        const uint4 v = reinterpret_cast<const uint4 *>(src)[q];
        sre_lg_u128 r;
        r.lo = ((uint64_t) v.y << 32) | v.x;
        r.hi = ((uint64_t) v.w << 32) | v.z;
        return r;
    }
    __device__ inline sre_lg_u128 loadu(uint64_t s) const
    {
        /* any alignment, which the hardware handles (as sre_hip_tile.h loads its rows) */
        const sre_u32x4 v = *reinterpret_cast<lg_unaligned_ptr>(reinterpret_cast<uintptr_t>(src) + s);
        sre_lg_u128     r;
        r.lo = ((uint64_t) v.y << 32) | v.x;
        r.hi = ((uint64_t) v.w << 32) | v.z;
        return r;
    }
    __device__ inline void store(uint64_t c, sre_lg_u128 v) const
    {
        reinterpret_cast<uint4 *>(dst)[c] = make_uint4((uint32_t) v.lo, (uint32_t) (v.lo >> 32), (uint32_t) v.hi, (uint32_t) (v.hi >> 32));
    }
    __device__ inline void store_bytes(uint64_t c, sre_lg_u128 v, uint32_t first, uint32_t count) const
    {
        for (uint32_t k = first; k < first + count; k++) {
            dst[c * 16 + k] = (uint8_t) ((k < 8 ? v.lo >> (8 * k) : v.hi >> (8 * (k - 8))) & 0xFFu);
        }
    }
};

/* ... and of the literal block of the line substitute: a 16-byte aligned address, a multiple of 16 bytes */
struct SubstMem : GatherMem {
    const uint8_t *lit;

    __device__ inline sre_lg_u128 lit_load(uint64_t q) const
    {
        const uint4 v = reinterpret_cast<const uint4 *>(lit)[q];
        sre_lg_u128 r;
        r.lo = ((uint64_t) v.y << 32) | v.x;
        r.hi = ((uint64_t) v.w << 32) | v.z;
        return r;
    }
    __device__ inline sre_lg_u128 lit_loadu(uint64_t s) const
    {
        const sre_u32x4 v = *reinterpret_cast<lg_unaligned_ptr>(reinterpret_cast<uintptr_t>(lit) + s);
        sre_lg_u128     r;
        r.lo = ((uint64_t) v.y << 32) | v.x;
        r.hi = ((uint64_t) v.w << 32) | v.z;
        return r;
    }
};

/* sre_lg_find over the global table by a whole wave: 64 probes a step, so a table of a million lines takes four
 * dependent loads instead of twenty.  Every lane of the wave calls it and gets the same answer */
__device__ inline uint64_t
wave_find(const uint64_t *__restrict__ off, uint64_t o, uint64_t lo, uint64_t hi)
{
    const uint32_t lane = threadIdx.x & 63u;
    while (hi - lo >= 64) {
        /* probes lo + step, lo + 2 step, ..: the last one is at or beyond hi and clamped to it */
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t p = min(lo + step * (lane + 1), hi);
        const uint32_t k = (uint32_t) __popcll(__ballot(off[p] <= o));     /* monotone: the first k probes hold */
        if (k == 64) return hi;
        const uint64_t nlo = k ? lo + step * k : lo;
        hi = min(lo + step * (k + 1), hi + 1) - 1;
        lo = nlo;
    }
    const uint64_t p = lo + 1 + lane;
    return lo + (uint32_t) __popcll(__ballot(p <= hi && off[p] <= o));
}

template <class Tab, class Mem>
__device__ inline void
gather_tile(const Tab &tab, const sre_lg_geom_t &g, uint64_t la, uint64_t lb, const Mem &mem)
{
    const uint64_t nchunks = sre_lg_nchunks(g);
    const uint64_t c0 = (uint64_t) blockIdx.x * SRE_LG_TILE_CHUNKS + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < SRE_LG_CHUNKS; k++) {
        const uint64_t c = c0 + (uint64_t) k * SRE_LG_THREADS;
        if (c < nchunks) sre_lg_chunk(tab, g, c, la, lb, mem);
    }
}

/* what a window keeps of entry i of the table: the line's start, resp. the entry's start word with its flags */
__device__ inline uint64_t
window_start(const sre_lg_tab_global &tab, uint64_t i)
{
    return tab.start(i);
}

__device__ inline uint64_t
window_start(const sre_lg_tab_fields &tab, uint64_t i)
{
    return tab.raw(i);
}

__device__ inline uint64_t
window_start(const sre_lg_tab_pieces &tab, uint64_t i)
{
    return tab.raw(i);
}

__device__ inline uint64_t
window_start(const sre_lg_tab_join &tab, uint64_t i)
{
    return tab.raw(i);
}

/* one tile of the output over the table `tab` (global memory), WTab its window type */
template <class GTab, class WTab, class Mem>
__device__ inline void
gather_body(const GTab &tab, const uint64_t *__restrict__ off, const sre_lg_geom_t &g, const Mem &mem, uint64_t *w_off,
            uint64_t *w_start, uint64_t *slice)
{
    /* the tile's slice of the table, found once: wave 0 searches the line of the tile's first byte, wave 1 that
     * of its last byte */
    if (threadIdx.x < 128) {
        uint64_t o_lo = 0, o_hi = 1;
        (void) sre_lg_span(g, (uint64_t) blockIdx.x * SRE_LG_TILE_CHUNKS, ((uint64_t) blockIdx.x + 1) * SRE_LG_TILE_CHUNKS, &o_lo,
                           &o_hi);
        const uint64_t i = wave_find(off, threadIdx.x < 64 ? o_lo : o_hi - 1, 0, g.nlines - 1);
        if ((threadIdx.x & 63u) == 0) slice[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    const uint64_t la = slice[0], lb = slice[1], cnt = lb - la + 1;
    if (cnt <= SRE_LG_WINDOW) {
        for (uint64_t x = threadIdx.x; x <= cnt; x += SRE_LG_THREADS) {
            w_off[x] = off[la + x];
            if (x < cnt) w_start[x] = window_start(tab, la + x);
        }
        __syncthreads();
        const WTab win = {w_off, w_start, la};
        gather_tile(win, g, la, lb, mem);
    } else {
        /* more lines than the window holds (up to one line per output byte when every selected line is
         * empty, and any number of unselected ones): the lanes search the slice in the global table */
        gather_tile(tab, g, la, lb, mem);
    }
}

__global__ __launch_bounds__(SRE_LG_THREADS) void
sre_k_lines_gather(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const uint64_t *__restrict__ off,
                   const uint64_t *__restrict__ ends, sre_lg_geom_t g)
{
    __shared__ uint64_t w_off[SRE_LG_WINDOW + 1], w_start[SRE_LG_WINDOW], slice[2];
    const sre_lg_tab_global tab = {off, ends};
    const GatherMem         mem = {src, dst};
    gather_body<sre_lg_tab_global, sre_lg_tab_window>(tab, off, g, mem, w_off, w_start, slice);
}

/* the line extract's: g.nlines counts entries, the window holds at most SRE_LG_WINDOW of them */
__global__ __launch_bounds__(SRE_LG_THREADS) void
sre_k_extract_gather(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const uint64_t *__restrict__ off,
                     const uint64_t *__restrict__ starts, sre_lg_geom_t g)
{
    __shared__ uint64_t w_off[SRE_LG_WINDOW + 1], w_start[SRE_LG_WINDOW], slice[2];
    const sre_lg_tab_fields tab = {off, starts, 0};
    const GatherMem         mem = {src, dst};
    gather_body<sre_lg_tab_fields, sre_lg_tab_fields>(tab, off, g, mem, w_off, w_start, slice);
}

/* the line substitute's: g.nlines counts the entries of the piece table, lit is the literal block */
__global__ __launch_bounds__(SRE_LG_THREADS) void
sre_k_subst_gather(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const uint64_t *__restrict__ off,
                   const uint64_t *__restrict__ starts, const uint8_t *__restrict__ lit, sre_lg_geom_t g)
{
    __shared__ uint64_t w_off[SRE_LG_WINDOW + 1], w_start[SRE_LG_WINDOW], slice[2];
    const sre_lg_tab_pieces tab = {off, starts, 0};
    SubstMem                mem;
    mem.src = src;
    mem.dst = dst;
    mem.lit = lit;
    gather_body<sre_lg_tab_pieces, sre_lg_tab_pieces>(tab, off, g, mem, w_off, w_start, slice);
}

/* the line join's (sre_hip_join_lines): g.nlines counts the entries of the join table, g.fsep is the
 * join separator, lit is the key map's copy of the dictionary: hipMalloc aligns it, and it is allocated 16 bytes beyond its
 * text.  An unaligned 16-byte load of it holds 16 bytes of one value; an aligned block holds at least one byte of a value,
 * so it starts below the text's end and ends inside those 16 bytes */
__global__ __launch_bounds__(SRE_LG_THREADS) void
sre_k_join_gather(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const uint64_t *__restrict__ off,
                  const uint64_t *__restrict__ starts, const uint8_t *__restrict__ lit, sre_lg_geom_t g)
{
    __shared__ uint64_t w_off[SRE_LG_WINDOW + 1], w_start[SRE_LG_WINDOW], slice[2];
    const sre_lg_tab_join tab = {off, starts, 0};
    SubstMem              mem;
    mem.src = src;
    mem.dst = dst;
    mem.lit = lit;
    gather_body<sre_lg_tab_join, sre_lg_tab_join>(tab, off, g, mem, w_off, w_start, slice);
}

/* ---- index ---- */

/* rows of the first `limit` written lines, limit = min(index_cap, info->fwritten); workgroups as in the scan */
__global__ __launch_bounds__(256) void
sre_k_filter_index(const uint64_t *__restrict__ off, const uint64_t *__restrict__ ends, uint64_t n,
                   const uint64_t *__restrict__ blkc, const sre_lines_info_t *__restrict__ info, uint64_t index_cap,
                   int64_t *__restrict__ rows)
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
            int64_t       *row = rows + r * 4;
            row[0] = (int64_t) i;
            row[1] = (int64_t) st;
            row[2] = (int64_t) (ends[i] - st);
            row[3] = (int64_t) off[i];
        }
        r++;
    }
}

/* the line extract's rows, 4 + 2 k words: workgroups over the ENTRIES as in the scan; the lane that holds the first
 * entry of a selected line writes the line's row.  Its rank is the selected entries in front of it over k */
__global__ __launch_bounds__(256) void
sre_k_extract_index(const uint64_t *__restrict__ off, const uint64_t *__restrict__ starts, const uint64_t *__restrict__ ends,
                    uint64_t nent, uint64_t k, const uint64_t *__restrict__ blkc, const sre_lines_info_t *__restrict__ info,
                    uint64_t index_cap, int64_t *__restrict__ rows)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      limit = index_cap < info->fwritten ? index_cap : info->fwritten;
    if (blkc[blockIdx.x] >= limit * k) return;      /* (the whole workgroup) */
    const uint64_t q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint32_t       f[4];
    uint64_t       s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        f[q] = q0 + q < nent && off[q0 + q + 1] > off[q0 + q];
        s += f[q];
    }
    uint64_t total;
    uint64_t r = blkc[blockIdx.x] + block_excl_scan<256>(s, wsum, total);
    for (uint32_t q = 0; q < 4; q++) {
        if (!f[q]) continue;
        const uint64_t e = q0 + q;
        if ((starts[e] & SRE_LG_ENTRY_FIRST) && r / k < limit) {
            const uint64_t i = e / k, st = line_start(ends, i);
            int64_t       *row = rows + (r / k) * (4 + 2 * k);
            row[0] = (int64_t) i;
            row[1] = (int64_t) st;
            row[2] = (int64_t) (ends[i] - st);
            row[3] = (int64_t) off[e];
            for (uint64_t x = 0; x < k; x++) {
                const uint64_t w = starts[e + x];
                const bool     unset = (w & SRE_LG_ENTRY_UNSET) != 0;
                row[4 + 2 * x] = unset ? -1 : (int64_t) (w & SRE_LG_ENTRY_START);
                row[5 + 2 * x] = unset ? -1 : (int64_t) (off[e + x + 1] - off[e + x] - 1);
            }
        }
        r++;
    }
}

/* the line join's rows, 5 + 2 (p - 1) words, as sre_k_extract_index finds and ranks them over the p entries of a line:
 * [4] is the line's key id (a dictionary row, -1, -2), then per value column its offset in the OUTPUT and its length, or
 * (-1, -1) for a line without a dictionary row */
__global__ __launch_bounds__(256) void
sre_k_join_index(const uint64_t *__restrict__ off, const uint64_t *__restrict__ starts, const uint64_t *__restrict__ ends,
                 const int64_t *__restrict__ keyid, uint64_t nent, uint64_t p, const uint64_t *__restrict__ blkc,
                 const sre_lines_info_t *__restrict__ info, uint64_t index_cap, int64_t *__restrict__ rows)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      limit = index_cap < info->fwritten ? index_cap : info->fwritten;
    if (blkc[blockIdx.x] >= limit * p) return;      /* (the whole workgroup) */
    const uint64_t q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint32_t       f[4];
    uint64_t       s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        f[q] = q0 + q < nent && off[q0 + q + 1] > off[q0 + q];
        s += f[q];
    }
    uint64_t total;
    uint64_t r = blkc[blockIdx.x] + block_excl_scan<256>(s, wsum, total);
    for (uint32_t q = 0; q < 4; q++) {
        if (!f[q]) continue;
        const uint64_t e = q0 + q;
        if ((starts[e] & SRE_LG_ENTRY_FIRST) && r / p < limit) {
            const uint64_t i = e / p, st = line_start(ends, i);
            int64_t       *row = rows + (r / p) * (3 + 2 * p);
            row[0] = (int64_t) i;
            row[1] = (int64_t) st;
            row[2] = (int64_t) (ends[i] - st);
            row[3] = (int64_t) off[e];
            row[4] = keyid[i];
            for (uint64_t x = 1; x < p; x++) {
                const bool unset = (starts[e + x] & SRE_LG_ENTRY_UNSET) != 0;
                row[3 + 2 * x] = unset ? -1 : (int64_t) off[e + x];
                row[4 + 2 * x] = unset ? -1 : (int64_t) (off[e + x + 1] - off[e + x] - 1);
            }
        }
        r++;
    }
}

/* the line substitute's rows of 8 words: workgroups over the ENTRIES as in the scan; the lane that holds the LAST entry
 * of a selected line writes the line's row, its rank the selected last entries in front of it (what the sums counted).
 * Everything in the row comes from the table: the match starts where the first entry's text ends and ends where the
 * last entry's text starts, the replacement is the output between them */
__global__ __launch_bounds__(256) void
sre_k_subst_index(const uint64_t *__restrict__ off, const uint64_t *__restrict__ starts, const uint64_t *__restrict__ ends,
                  uint64_t nent, uint64_t p, const uint64_t *__restrict__ blkc, const sre_lines_info_t *__restrict__ info,
                  uint64_t index_cap, int64_t *__restrict__ rows)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      limit = index_cap < info->fwritten ? index_cap : info->fwritten;
    if (blkc[blockIdx.x] >= limit) return;      /* (the whole workgroup) */
    const uint64_t q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint32_t       f[4];
    uint64_t       s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        f[q] = q0 + q < nent && (starts[q0 + q] & SRE_LG_ENTRY_LAST) && off[q0 + q + 1] > off[q0 + q];
        s += f[q];
    }
    uint64_t total;
    uint64_t r = blkc[blockIdx.x] + block_excl_scan<256>(s, wsum, total);
    for (uint32_t q = 0; q < 4; q++) {
        if (!f[q]) continue;
        if (r < limit) {
            const uint64_t z = q0 + q, e = z - (p - 1), i = e / p, st = line_start(ends, i);
            const bool     matched = (starts[e] & SRE_LG_ENTRY_UNSET) == 0;
            const uint64_t m0 = st + (off[e + 1] - off[e]), m1 = starts[z] & SRE_LG_PIECE_START;
            int64_t       *row = rows + r * 8;
            row[0] = (int64_t) i;
            row[1] = (int64_t) st;
            row[2] = (int64_t) (ends[i] - st);
            row[3] = (int64_t) off[e];
            row[4] = matched ? (int64_t) m0 : -1;
            row[5] = matched ? (int64_t) (m1 - m0) : -1;
            row[6] = matched ? (int64_t) off[e + 1] : -1;
            row[7] = matched ? (int64_t) (off[z] - off[e + 1]) : -1;
        }
        r++;
    }
}

}  // namespace

extern "C" hipError_t
sre_launch_filter_select(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0, int mode,
                         const uint64_t *d_ends, const sre_lines_info_t *d_info, uint64_t *d_val, hipStream_t stream)
{
    if (nmax == 0) return hipSuccess;
    hipLaunchKernelGGL(sre_k_filter_select, dim3((uint32_t) ((nmax + 255) / 256)), dim3(256), 0, stream, d_records, slots, i0,
                       mode, d_ends, d_info, d_val);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_filter_offsets(uint64_t *d_val, uint64_t n, uint64_t *d_blk, uint64_t out_cap, sre_lines_info_t *d_info,
                          hipStream_t stream)
{
    if (n == 0) return hipErrorInvalidValue;
    const uint64_t nblk = (n + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    uint64_t      *blkv = d_blk, *blkc = d_blk + nblk;
    hipLaunchKernelGGL(sre_k_filter_sums, dim3((uint32_t) nblk), dim3(256), 0, stream, d_val, n, blkv, blkc);
    hipLaunchKernelGGL(sre_k_filter_scan, dim3(1), dim3(1024), 0, stream, blkv, blkc, nblk, d_info);
    hipLaunchKernelGGL(sre_k_filter_offsets, dim3((uint32_t) nblk), dim3(256), 0, stream, d_val, n, blkv);
    hipLaunchKernelGGL(sre_k_filter_finish, dim3(1), dim3(1024), 0, stream, d_val, n, blkc, out_cap, d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_lines_gather(const void *d_buf, void *d_out, const uint64_t *d_off, const uint64_t *d_ends, uint64_t nlines,
                        uint64_t out_bytes, uint32_t delim, hipStream_t stream)
{
    if (out_bytes == 0) return hipSuccess;
    sre_lg_geom_t g;
    g.nlines = nlines;
    g.out_bytes = out_bytes;
    g.src_head = (uint32_t) (reinterpret_cast<uintptr_t>(d_buf) & 15u);
    g.dst_head = (uint32_t) (reinterpret_cast<uintptr_t>(d_out) & 15u);
    g.delim = delim;
    g.fsep = delim;
    const uint64_t ntiles = (sre_lg_nchunks(g) + SRE_LG_TILE_CHUNKS - 1) / SRE_LG_TILE_CHUNKS;
    if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_lines_gather, dim3((uint32_t) ntiles), dim3(SRE_LG_THREADS), 0, stream,
                       static_cast<const uint8_t *>(d_buf) - g.src_head, static_cast<uint8_t *>(d_out) - g.dst_head, d_off, d_ends,
                       g);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_filter_index(const uint64_t *d_off, const uint64_t *d_ends, uint64_t n, const uint64_t *d_blk,
                        const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index, hipStream_t stream)
{
    if (n == 0 || index_cap == 0) return hipSuccess;
    const uint64_t nblk = (n + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    hipLaunchKernelGGL(sre_k_filter_index, dim3((uint32_t) nblk), dim3(256), 0, stream, d_off, d_ends, n, d_blk + nblk, d_info,
                       index_cap, d_index);
    return hipGetLastError();
}

/* ---- the line extract ---- */

extern "C" hipError_t
sre_launch_extract_select(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0, int all,
                          const sre_extract_groups_t *groups, const uint64_t *d_ends, const sre_lines_info_t *d_info,
                          uint64_t *d_val, uint64_t *d_start, hipStream_t stream)
{
    if (nmax == 0) return hipSuccess;
    const uint64_t nent = nmax * groups->k;
    if (groups->k == 0 || groups->k > SRE_EXTRACT_MAX_FIELDS || nent > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_extract_select, dim3((uint32_t) ((nent + 255) / 256)), dim3(256), 0, stream, d_records, slots, i0, all,
                       *groups, d_ends, d_info, d_val, d_start);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_extract_offsets(uint64_t *d_val, uint64_t n, uint32_t k, uint64_t *d_blk, uint64_t out_cap,
                           sre_lines_info_t *d_info, hipStream_t stream)
{
    if (n == 0 || k == 0) return hipErrorInvalidValue;
    const uint64_t nent = n * k, nblk = (nent + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    uint64_t      *blkv = d_blk, *blkc = d_blk + nblk;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_filter_sums, dim3((uint32_t) nblk), dim3(256), 0, stream, d_val, nent, blkv, blkc);
    hipLaunchKernelGGL(sre_k_filter_scan, dim3(1), dim3(1024), 0, stream, blkv, blkc, nblk, d_info);
    hipLaunchKernelGGL(sre_k_filter_offsets, dim3((uint32_t) nblk), dim3(256), 0, stream, d_val, nent, blkv);
    hipLaunchKernelGGL(sre_k_extract_finish, dim3(1), dim3(1024), 0, stream, d_val, n, (uint64_t) k, blkc, out_cap, d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_extract_gather(const void *d_buf, void *d_out, const uint64_t *d_off, const uint64_t *d_start, uint64_t nentries,
                          uint64_t out_bytes, uint32_t delim, uint32_t fsep, hipStream_t stream)
{
    if (out_bytes == 0) return hipSuccess;
    sre_lg_geom_t g;
    g.nlines = nentries;
    g.out_bytes = out_bytes;
    g.src_head = (uint32_t) (reinterpret_cast<uintptr_t>(d_buf) & 15u);
    g.dst_head = (uint32_t) (reinterpret_cast<uintptr_t>(d_out) & 15u);
    g.delim = delim;
    g.fsep = fsep;
    const uint64_t ntiles = (sre_lg_nchunks(g) + SRE_LG_TILE_CHUNKS - 1) / SRE_LG_TILE_CHUNKS;
    if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_extract_gather, dim3((uint32_t) ntiles), dim3(SRE_LG_THREADS), 0, stream,
                       static_cast<const uint8_t *>(d_buf) - g.src_head, static_cast<uint8_t *>(d_out) - g.dst_head, d_off,
                       d_start, g);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_extract_index(const uint64_t *d_off, const uint64_t *d_start, const uint64_t *d_ends, uint64_t n, uint32_t k,
                         const uint64_t *d_blk, const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index,
                         hipStream_t stream)
{
    if (n == 0 || index_cap == 0) return hipSuccess;
    const uint64_t nent = n * k, nblk = (nent + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    hipLaunchKernelGGL(sre_k_extract_index, dim3((uint32_t) nblk), dim3(256), 0, stream, d_off, d_start, d_ends, nent,
                       (uint64_t) k, d_blk + nblk, d_info, index_cap, d_index);
    return hipGetLastError();
}

/* ---- the line substitute ---- */

extern "C" hipError_t
sre_launch_subst_select(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0, int all,
                        const sre_subst_pieces_t *pieces, const uint64_t *d_ends, const sre_lines_info_t *d_info, uint64_t *d_val,
                        uint64_t *d_start, hipStream_t stream)
{
    if (nmax == 0) return hipSuccess;
    const uint64_t nent = nmax * (pieces->np + 2);
    if (pieces->np > SRE_SUBST_MAX_PIECES || nent > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_subst_select, dim3((uint32_t) ((nent + 255) / 256)), dim3(256), 0, stream, d_records, slots, i0, all,
                       *pieces, d_ends, d_info, d_val, d_start);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_subst_offsets(uint64_t *d_val, uint64_t n, uint32_t p, uint64_t *d_blk, uint64_t out_cap, sre_lines_info_t *d_info,
                         hipStream_t stream)
{
    if (n == 0 || p < 2) return hipErrorInvalidValue;
    const uint64_t nent = n * p, nblk = (nent + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    uint64_t      *blkv = d_blk, *blkc = d_blk + nblk;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_subst_sums, dim3((uint32_t) nblk), dim3(256), 0, stream, d_val, nent, (uint64_t) p, blkv, blkc);
    hipLaunchKernelGGL(sre_k_filter_scan, dim3(1), dim3(1024), 0, stream, blkv, blkc, nblk, d_info);
    hipLaunchKernelGGL(sre_k_filter_offsets, dim3((uint32_t) nblk), dim3(256), 0, stream, d_val, nent, blkv);
    hipLaunchKernelGGL(sre_k_subst_finish, dim3(1), dim3(1024), 0, stream, d_val, n, (uint64_t) p, blkc, out_cap, d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_subst_gather(const void *d_buf, void *d_out, const uint64_t *d_off, const uint64_t *d_start, const void *d_lit,
                        uint64_t nentries, uint64_t out_bytes, uint32_t delim, hipStream_t stream)
{
    if (out_bytes == 0) return hipSuccess;
    if (d_lit == NULL || (reinterpret_cast<uintptr_t>(d_lit) & 15u) != 0) return hipErrorInvalidValue;
    sre_lg_geom_t g;
    g.nlines = nentries;
    g.out_bytes = out_bytes;
    g.src_head = (uint32_t) (reinterpret_cast<uintptr_t>(d_buf) & 15u);
    g.dst_head = (uint32_t) (reinterpret_cast<uintptr_t>(d_out) & 15u);
    g.delim = delim;
    g.fsep = delim;
    const uint64_t ntiles = (sre_lg_nchunks(g) + SRE_LG_TILE_CHUNKS - 1) / SRE_LG_TILE_CHUNKS;
    if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_subst_gather, dim3((uint32_t) ntiles), dim3(SRE_LG_THREADS), 0, stream,
                       static_cast<const uint8_t *>(d_buf) - g.src_head, static_cast<uint8_t *>(d_out) - g.dst_head, d_off,
                       d_start, static_cast<const uint8_t *>(d_lit), g);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_subst_index(const uint64_t *d_off, const uint64_t *d_start, const uint64_t *d_ends, uint64_t n, uint32_t p,
                       const uint64_t *d_blk, const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index,
                       hipStream_t stream)
{
    if (n == 0 || index_cap == 0) return hipSuccess;
    const uint64_t nent = n * p, nblk = (nent + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    hipLaunchKernelGGL(sre_k_subst_index, dim3((uint32_t) nblk), dim3(256), 0, stream, d_off, d_start, d_ends, nent,
                       (uint64_t) p, d_blk + nblk, d_info, index_cap, d_index);
    return hipGetLastError();
}

/* ---- the line join ---- */

extern "C" hipError_t
sre_launch_join_gather(const void *d_buf, void *d_out, const uint64_t *d_off, const uint64_t *d_start, const void *d_dict,
                       uint64_t nentries, uint64_t out_bytes, uint32_t delim, uint32_t jsep, hipStream_t stream)
{
    if (out_bytes == 0) return hipSuccess;
    /* (d_dict == NULL: the empty map, no entry of the table is a value) */
    if ((reinterpret_cast<uintptr_t>(d_dict) & 15u) != 0) return hipErrorInvalidValue;
    sre_lg_geom_t g;
    g.nlines = nentries;
    g.out_bytes = out_bytes;
    g.src_head = (uint32_t) (reinterpret_cast<uintptr_t>(d_buf) & 15u);
    g.dst_head = (uint32_t) (reinterpret_cast<uintptr_t>(d_out) & 15u);
    g.delim = delim;
    g.fsep = jsep;
    const uint64_t ntiles = (sre_lg_nchunks(g) + SRE_LG_TILE_CHUNKS - 1) / SRE_LG_TILE_CHUNKS;
    if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_join_gather, dim3((uint32_t) ntiles), dim3(SRE_LG_THREADS), 0, stream,
                       static_cast<const uint8_t *>(d_buf) - g.src_head, static_cast<uint8_t *>(d_out) - g.dst_head, d_off,
                       d_start, static_cast<const uint8_t *>(d_dict), g);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_join_index(const uint64_t *d_off, const uint64_t *d_start, const uint64_t *d_ends, const int64_t *d_keyid, uint64_t n,
                      uint32_t p, const uint64_t *d_blk, const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index,
                      hipStream_t stream)
{
    if (n == 0 || index_cap == 0) return hipSuccess;
    if (p < 2) return hipErrorInvalidValue;
    const uint64_t nent = n * p, nblk = (nent + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    hipLaunchKernelGGL(sre_k_join_index, dim3((uint32_t) nblk), dim3(256), 0, stream, d_off, d_start, d_ends, d_keyid, nent,
                       (uint64_t) p, d_blk + nblk, d_info, index_cap, d_index);
    return hipGetLastError();
}
