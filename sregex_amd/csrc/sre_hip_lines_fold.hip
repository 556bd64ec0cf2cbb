/*
 * sre_hip_lines_fold.hip — the fold pass of the line fold (sregex_hip.h sre_hip_fold_lines): the lines of
 * a buffer joined into multi-line records, between the last batch's select pass and the scan to the offset table.  Line i is
 * MARKED when val[i] > 0; a marked line belongs to the record of the line in front of it, or (SRE_LF_NEXT) continues into
 * the line behind it.  The rules are sre_lines_fold.h's, the geometry and the scans those of the context pass
 * (sre_hip_lines_context.hip): a workgroup of 256 lanes owns 1024 lines, a lane four consecutive ones.
 *
 *   marks      per workgroup: the bitmap of its marked lines, and its block words: the last and the first natural head its
 *              lines generate;
 *   carry      one workgroup: a forward maximum scan of the last heads and a backward minimum scan of the first ones turn
 *              the block words into h_in / q_in, the nearest natural head in front of / behind each block's own;
 *   apply      per workgroup, from the BITMAP: the same two scans over its 1024 lines seeded with h_in / q_in; head(i) and
 *              head(i + 1) of every line; the extract's entry table with one entry a line (val[i] = len + 1, start[i] the
 *              line's start with SRE_LG_ENTRY_LAST where the delimiter follows); aux[i]; the head bitmap; the block's
 *              counts of heads and marked lines and its longest record;
 *   totals     one workgroup: the counts of heads become the heads in front of each block; info->gnrec, gmarked, glongest;
 *   finish     behind the extract's scan over the entry table: the cut at out_cap moved back to the first line of its
 *              record; info->fwritten counts RECORDS;
 *   recid      the record number of every line of the first recid_cap;
 *   records    a row for each of the first records_cap written records.
 *
 * IN PLACE AND RACE-FREE.  marks reads val and writes only its own words of the bitmap and its two block words.  apply
 * does not read val at all: the marked bits come from the bitmap, the one bit it needs of the next workgroup's first line
 * too, and marks finished before apply starts: separate launches on one stream.  apply writes val, start and aux only at
 * its own 1024 lines.  No kernel reads a word that another workgroup of the same launch writes.
 *
 * No workgroup waits for another.  Plain C++ and vector memory operations only.
 */
#include "sre_hip_lines.h"
#include "sre_lines_fold.h"
#include "sre_hip_lines_block.h"

static_assert(SRE_LC_ITEMS == SRE_LINES_ITEMS && SRE_LC_THREADS * SRE_LC_PER_LANE == SRE_LC_ITEMS, "one geometry");
static_assert(SRE_LC_WAVE * SRE_LC_PER_LANE / 64 == 4, "a wave owns four words of a bitmap");

namespace {

/* the wave's 256 lines are four whole words of a bitmap: lanes 0 .. 3 store one each (b: the ballots of the lanes' four
 * lines; nothing beyond the ceil(n / 64) words) */
__device__ inline void
store_bitmap(uint64_t *__restrict__ bits, const uint64_t b[SRE_LC_PER_LANE], uint64_t base, uint64_t n)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t word = base / 64 + (SRE_LC_WAVE * SRE_LC_PER_LANE / 64) * w + lane;
    if (lane < SRE_LC_WAVE * SRE_LC_PER_LANE / 64 && word < (n + 63) / 64) bits[word] = sre_lc_bitmap_word(b, lane);
}

/* the maximum of v over the workgroup (NT lanes); wmax holds NT / 64 words */
template <uint32_t NT>
__device__ inline uint64_t
block_max(uint64_t v, uint64_t *wmax)
{
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        const uint64_t y = __shfl_xor(v, d, 64);
        v = y > v ? y : v;
    }
    if ((threadIdx.x & 63u) == 0) wmax[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t r = 0;
#pragma unroll
    for (uint32_t i = 0; i < NT / 64; i++) r = wmax[i] > r ? wmax[i] : r;
    __syncthreads();
    return r;
}

/* ---- marks ---- */

__global__ __launch_bounds__(SRE_LC_THREADS) void
sre_k_fold_marks(const uint64_t *__restrict__ val, uint64_t n, uint32_t s, uint64_t *__restrict__ mbits, uint64_t *__restrict__ last,
                 uint64_t *__restrict__ first)
{
    __shared__ uint32_t wp[SRE_LC_WAVES], wq[SRE_LC_WAVES];
    const uint64_t      base = (uint64_t) blockIdx.x * SRE_LC_ITEMS, q0 = base + SRE_LC_PER_LANE * threadIdx.x;
    uint64_t            v[SRE_LC_PER_LANE], b[SRE_LC_PER_LANE];
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) v[k] = q0 + k < n ? val[q0 + k] : 0;
    const uint32_t m = sre_lf_lane_bits(v, q0, n);
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) b[k] = __ballot((m >> k) & 1u);
    store_bitmap(mbits, b, base, n);
    uint32_t p, q, ptot, qtot;
    sre_lf_lane_marks(m, sre_lf_lane_valid(q0, n), threadIdx.x, s, &p, &q);
    block_excl_marks<uint32_t, SRE_LC_WAVES>(p, q, wp, wq, ptot, qtot);
    if (threadIdx.x == 0) {
        last[blockIdx.x] = sre_lc_p_global(base, ptot, 0);
        first[blockIdx.x] = sre_lc_q_global(base, qtot, SRE_LC_NONE);
    }
}

/* ---- carry ---- */

/* one workgroup over the nblk block words, a contiguous run per lane: last[b] becomes h_in of workgroup b, first[b] its q_in */
__global__ __launch_bounds__(SRE_LC_CARRY_LANES) void
sre_k_fold_carry(uint64_t *__restrict__ last, uint64_t *__restrict__ first, uint64_t nblk)
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

__global__ __launch_bounds__(SRE_LC_THREADS) void
sre_k_fold_apply(uint64_t *__restrict__ val, uint64_t *__restrict__ start, const uint64_t *__restrict__ ends, uint64_t n, uint32_t s,
                 uint64_t max_lines, const uint64_t *__restrict__ mbits, const uint64_t *__restrict__ hin,
                 const uint64_t *__restrict__ qin, uint64_t *__restrict__ aux, uint64_t *__restrict__ hbits, uint64_t *__restrict__ blkh,
                 uint64_t *__restrict__ blkm, uint64_t *__restrict__ blkl)
{
    __shared__ uint32_t wp[SRE_LC_WAVES], wq[SRE_LC_WAVES], ch[SRE_LC_WAVES], cm[SRE_LC_WAVES];
    __shared__ uint64_t wmax[SRE_LC_WAVES];
    const uint32_t      lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t      base = (uint64_t) blockIdx.x * SRE_LC_ITEMS, q0 = base + SRE_LC_PER_LANE * threadIdx.x;
    const uint32_t      nv = sre_lf_lane_valid(q0, n);
    /* (words of the bitmap at or beyond ceil(n / 64) do not exist: no line of theirs is in the buffer) */
    const uint32_t m = nv ? sre_lf_word_bits(mbits[q0 / 64], q0) : 0;
    const uint32_t mnext = q0 + SRE_LC_PER_LANE < n ? (uint32_t) (mbits[(q0 + SRE_LC_PER_LANE) / 64] >> ((q0 + SRE_LC_PER_LANE) % 64)) & 1u : 0;
    uint32_t       p, q, ptot, qtot;
    sre_lf_lane_marks(m, nv, threadIdx.x, s, &p, &q);
    block_excl_marks<uint32_t, SRE_LC_WAVES>(p, q, wp, wq, ptot, qtot);
    uint32_t fl[SRE_LC_PER_LANE];
    uint64_t ax[SRE_LC_PER_LANE], bh[SRE_LC_PER_LANE], bm[SRE_LC_PER_LANE], longest = 0;
    sre_lf_lane_lines(q0, n, nv, m, mnext, s, max_lines, sre_lc_p_global(base, p, hin[blockIdx.x]),
                      sre_lc_q_global(base, q, qin[blockIdx.x]), fl, ax);
    /* (the lane's four line ends and the one in front of them) */
    uint64_t st = nv ? line_start(ends, q0) : 0;
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
        if (k < nv) {
            const uint64_t i = q0 + k, e = ends[i];
            val[i] = e - st + 1;
            start[i] = sre_lf_entry_start(st, fl[k]);
            aux[i] = ax[k];
            if ((fl[k] & SRE_LF_HEAD) && ax[k] - i > longest) longest = ax[k] - i;
            st = e + 1;
        }
        bh[k] = __ballot((fl[k] & SRE_LF_HEAD) != 0);
        bm[k] = __ballot((m >> k) & 1u);
    }
    store_bitmap(hbits, bh, base, n);
    if (lane == 0) {
        ch[w] = sre_lc_count(bh);
        cm[w] = sre_lc_count(bm);
    }
    longest = block_max<SRE_LC_THREADS>(longest, wmax);      /* (its barrier publishes ch and cm too) */
    if (threadIdx.x == 0) {
        uint64_t h = 0, c = 0;
        for (uint32_t i = 0; i < SRE_LC_WAVES; i++) {
            h += ch[i];
            c += cm[i];
        }
        blkh[blockIdx.x] = h;
        blkm[blockIdx.x] = c;
        blkl[blockIdx.x] = longest;
    }
}

/* ---- totals ---- */

/* one workgroup (a contiguous run of the block words per lane, as sre_k_filter_scan): blkh becomes its exclusive sums in
 * place; info->gnrec = the heads, gmarked = the marked lines, glongest = the lines of the longest record */
__global__ __launch_bounds__(1024) void
sre_k_fold_totals(uint64_t *__restrict__ blkh, const uint64_t *__restrict__ blkm, const uint64_t *__restrict__ blkl, uint64_t nblk,
                  sre_lines_info_t *__restrict__ info)
{
    __shared__ uint64_t wsum[16];
    const uint64_t      per = (nblk + 1023) / 1024;
    const uint64_t      lo = min(nblk, (uint64_t) threadIdx.x * per), hi = min(nblk, lo + per);
    uint64_t            h = 0, m = 0, l = 0;
    for (uint64_t i = lo; i < hi; i++) {
        h += blkh[i];
        m += blkm[i];
        l = blkl[i] > l ? blkl[i] : l;
    }
    uint64_t th, tm;
    uint64_t rh = block_excl_scan<1024>(h, wsum, th);
    (void) block_excl_scan<1024>(m, wsum, tm);
    l = block_max<1024>(l, wsum);
    for (uint64_t i = lo; i < hi; i++) {
        const uint64_t x = blkh[i];
        blkh[i] = rh;
        rh += x;
    }
    if (threadIdx.x == 0) {
        info->gnrec = th;
        info->gmarked = tm;
        info->glongest = l;
    }
}

/* ---- finish ---- */

/* one workgroup, behind the scan of the entry table to off[0 .. n]: the first line c whose end lies beyond out_cap, the cut
 * at the first line of c's record; info->fbytes = off[cut], info->fwritten = heads in front of the cut */
__global__ __launch_bounds__(1024) void
sre_k_fold_finish(const uint64_t *__restrict__ off, uint64_t n, const uint64_t *__restrict__ hbits, const uint64_t *__restrict__ aux,
                  const uint64_t *__restrict__ blkh, uint64_t out_cap, sre_lines_info_t *__restrict__ info)
{
    __shared__ uint64_t cut;
    if (threadIdx.x == 0) cut = sre_lf_cut(sre_lf_first_beyond(off, n, out_cap), n, hbits, aux);
    __syncthreads();
    const uint64_t i = cut, b = i / SRE_LINES_ITEMS, j = b * SRE_LINES_ITEMS + threadIdx.x;
    const int      before = __syncthreads_count(j < i && ((hbits[j / 64] >> (j % 64)) & 1u) != 0);
    if (threadIdx.x == 0) {
        info->fbytes = off[i];
        info->fwritten = i == n ? info->gnrec : blkh[b] + (uint64_t) before;
    }
}

/* ---- record ids, records ---- */

/* lane x of workgroup b: the heads among lines b * 1024 + 4x .. + 3 from the head bitmap, and the number of the record of
 * the lane's first line LESS the lane's own first head bit: line q0 + k lies in record r + (heads among its first k + 1) - 1 */
__device__ inline uint64_t
lane_records(const uint64_t *__restrict__ hbits, const uint64_t *__restrict__ blkh, uint64_t n, uint64_t q0, uint64_t *wsum, uint32_t *hb)
{
    const uint32_t h = sre_lf_lane_valid(q0, n) ? sre_lf_word_bits(hbits[q0 / 64], q0) : 0;
    uint64_t       total;
    *hb = h;
    return blkh[blockIdx.x] + block_excl_scan<SRE_LC_THREADS>((uint64_t) __builtin_popcount(h), wsum, total);
}

__global__ __launch_bounds__(SRE_LC_THREADS) void
sre_k_fold_recid(const uint64_t *__restrict__ hbits, const uint64_t *__restrict__ blkh, uint64_t n, uint64_t limit,
                 int64_t *__restrict__ recid)
{
    __shared__ uint64_t wsum[SRE_LC_WAVES];
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LC_ITEMS + SRE_LC_PER_LANE * threadIdx.x;
    uint32_t            h;
    uint64_t            r = lane_records(hbits, blkh, n, q0, wsum, &h);
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
        r += (h >> k) & 1u;
        if (q0 + k < limit) recid[q0 + k] = (int64_t) r - 1;
    }
}

/* the rows of the first `limit` written records, limit = min(records_cap, info->fwritten): the head of record r writes row r */
__global__ __launch_bounds__(SRE_LC_THREADS) void
sre_k_fold_records(const uint64_t *__restrict__ off, const uint64_t *__restrict__ ends, const uint64_t *__restrict__ hbits,
                   const uint64_t *__restrict__ aux, const uint64_t *__restrict__ blkh, uint64_t n,
                   const sre_lines_info_t *__restrict__ info, uint64_t records_cap, int64_t *__restrict__ rows)
{
    __shared__ uint64_t wsum[SRE_LC_WAVES];
    const uint64_t      limit = records_cap < info->fwritten ? records_cap : info->fwritten;
    if (blkh[blockIdx.x] >= limit) return;      /* (the whole workgroup) */
    const uint64_t q0 = (uint64_t) blockIdx.x * SRE_LC_ITEMS + SRE_LC_PER_LANE * threadIdx.x;
    uint32_t       h;
    uint64_t       r = lane_records(hbits, blkh, n, q0, wsum, &h);
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
        if (((h >> k) & 1u) == 0) continue;
        if (r < limit) sre_lf_record_row(rows + r * SRE_LF_ROW, q0 + k, aux[q0 + k], line_start(ends, q0 + k), off);
        r++;
    }
}

}  // namespace

extern "C" hipError_t
sre_launch_fold_select(uint64_t *d_val, uint64_t *d_start, const uint64_t *d_ends, uint64_t n, int next, uint64_t max_lines,
                       uint64_t *d_bits, uint64_t *d_aux, uint64_t *d_blk, sre_lines_info_t *d_info, hipStream_t stream)
{
    if (n == 0) return hipErrorInvalidValue;
    const uint64_t nblk = (n + SRE_LC_ITEMS - 1) / SRE_LC_ITEMS, nwords = (n + 63) / 64;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint32_t s = next ? 1u : 0u;
    uint64_t      *hin = d_blk, *qin = d_blk + nblk, *blkh = d_blk + 2 * nblk, *blkm = d_blk + 3 * nblk, *blkl = d_blk + 4 * nblk;
    uint64_t      *mbits = d_bits, *hbits = d_bits + nwords;
    hipLaunchKernelGGL(sre_k_fold_marks, dim3((uint32_t) nblk), dim3(SRE_LC_THREADS), 0, stream, d_val, n, s, mbits, hin, qin);
    hipLaunchKernelGGL(sre_k_fold_carry, dim3(1), dim3(SRE_LC_CARRY_LANES), 0, stream, hin, qin, nblk);
    hipLaunchKernelGGL(sre_k_fold_apply, dim3((uint32_t) nblk), dim3(SRE_LC_THREADS), 0, stream, d_val, d_start, d_ends, n, s, max_lines,
                       mbits, hin, qin, d_aux, hbits, blkh, blkm, blkl);
    hipLaunchKernelGGL(sre_k_fold_totals, dim3(1), dim3(1024), 0, stream, blkh, blkm, blkl, nblk, d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_fold_finish(const uint64_t *d_off, uint64_t n, const uint64_t *d_bits, const uint64_t *d_aux, const uint64_t *d_blk,
                       uint64_t out_cap, sre_lines_info_t *d_info, hipStream_t stream)
{
    if (n == 0) return hipErrorInvalidValue;
    const uint64_t nblk = (n + SRE_LC_ITEMS - 1) / SRE_LC_ITEMS, nwords = (n + 63) / 64;
    hipLaunchKernelGGL(sre_k_fold_finish, dim3(1), dim3(1024), 0, stream, d_off, n, d_bits + nwords, d_aux, d_blk + 2 * nblk, out_cap,
                       d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_fold_tables(const uint64_t *d_off, const uint64_t *d_ends, uint64_t n, const uint64_t *d_bits, const uint64_t *d_aux,
                       const uint64_t *d_blk, const sre_lines_info_t *d_info, int64_t *d_recid, uint64_t recid_cap, int64_t *d_records,
                       uint64_t records_cap, uint64_t nwritten, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t  nblk = (n + SRE_LC_ITEMS - 1) / SRE_LC_ITEMS, nwords = (n + 63) / 64;
    const uint64_t *hbits = d_bits + nwords, *blkh = d_blk + 2 * nblk;
    if (recid_cap != 0) {
        const uint64_t limit = recid_cap < n ? recid_cap : n;
        hipLaunchKernelGGL(sre_k_fold_recid, dim3((uint32_t) ((limit + SRE_LC_ITEMS - 1) / SRE_LC_ITEMS)), dim3(SRE_LC_THREADS), 0, stream,
                           hbits, blkh, n, limit, d_recid);
    }
    if (records_cap != 0 && nwritten != 0) {
        hipLaunchKernelGGL(sre_k_fold_records, dim3((uint32_t) nblk), dim3(SRE_LC_THREADS), 0, stream, d_off, d_ends, hbits, d_aux, blkh,
                           n, d_info, records_cap, d_records);
    }
    return hipGetLastError();
}
