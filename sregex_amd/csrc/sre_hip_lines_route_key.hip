/*
 * sre_hip_lines_route_key.hip — the line route by key on the device (sregex_hip.h sre_hip_route_lines_by_key, DESIGN.md
 * §4.11.11): a stable partition of the lines by the dictionary row of their key, an LSD radix sort of (sort key, line)
 * items, into a compact table the extract's gather writes out.  The rules are those of sre_lines_route_key.h and
 * sre_lines_route.h, which the CPU model compiles too.
 *
 *   count      per pass: a workgroup takes 1024 items in order and writes how many have each digit to cnt[d * nwg + w];
 *              the filter's scan (sre_launch_filter_offsets) over those words gives every (digit, workgroup) its first rank;
 *   scatter    the same workgroups recompute the rank of every item and store it at that rank of the other array.  Pass 0
 *              makes the items from the key ids in line order and drops the unselected;
 *   table      a lane per rank of the sorted items: the entry of the compact table and the head flag;
 *   heads      behind the scan of the head flags: a lane per rank, a head leaves its rank at its bucket number;
 *   buckets    a lane per bucket: its row;
 *   finish     one lane: the cut at out_cap and the words the host reads;
 *   gather     sre_launch_extract_gather over the compact table, unchanged (sre_hip_lines_gather.hip);
 *   index      a lane per written rank.
 *
 * No workgroup waits for another and no rank comes from an atomic.  Plain C++ and vector memory operations only.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"
#include "sre_lines_route_key.h"
#include "sre_hip_lines_block.h"
#include "sre_hip_lines_rank.h"

namespace {

/* item i of a pass: pass 0 (FIRST) makes it from the key id of line i, a later pass reads it */
template <bool FIRST>
__device__ inline uint64_t
load_item(const int64_t *__restrict__ keyid, const uint64_t *__restrict__ src, uint64_t i, uint64_t n, uint64_t rows, int all)
{
    if (i >= n) return SRE_LRK_DROPPED;
    return FIRST ? sre_lrk_first_item(keyid[i], i, rows, all) : src[i];
}

/* workgroup w: cnt[d * nwg + w] = its items of digit d */
template <bool FIRST, int RULE>
__global__ __launch_bounds__(SRE_LR_THREADS) void
sre_k_route_key_count(const int64_t *__restrict__ keyid, const uint64_t *__restrict__ src, uint64_t n, uint64_t rows, int all,
                      uint32_t pass, uint32_t bits, uint64_t nwg, uint64_t *__restrict__ cnt)
{
    __shared__ uint32_t c[SRE_LR_SLOTS << SRE_LRK_MAX_BITS];
    const uint32_t      lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nd = 1u << bits;
    for (uint32_t x = threadIdx.x; x < SRE_LR_SLOTS * nd; x += SRE_LR_THREADS) c[x] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
        const uint32_t slot = sre_lr_slot(wave, q);
        const uint64_t it = load_item<FIRST>(keyid, src, sre_lr_line(blockIdx.x, slot, lane), n, rows, all);
        (void) slot_rank<RULE>(it != SRE_LRK_DROPPED, sre_lrk_digit(it, pass, bits), bits, lane, c + slot * nd);
    }
    __syncthreads();
    if (threadIdx.x < nd) cnt[sre_lr_cnt_index(threadIdx.x, nwg, blockIdx.x)] = sre_lr_slot_prefix(c + threadIdx.x, nd);
}

/* the same workgroups over the scanned counts `first`: every item goes to its rank of dst (total items) */
template <bool FIRST, int RULE>
__global__ __launch_bounds__(SRE_LR_THREADS) void
sre_k_route_key_scatter(const int64_t *__restrict__ keyid, const uint64_t *__restrict__ src, uint64_t n, uint64_t rows, int all,
                        uint32_t pass, uint32_t bits, uint64_t nwg, const uint64_t *__restrict__ first, uint64_t total,
                        uint64_t *__restrict__ dst)
{
    __shared__ uint32_t c[SRE_LR_SLOTS << SRE_LRK_MAX_BITS];
    __shared__ uint64_t gbase[1u << SRE_LRK_MAX_BITS];
    const uint32_t      lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nd = 1u << bits;
    uint64_t            it[SRE_LR_ROUNDS];
    uint32_t            rk[SRE_LR_ROUNDS];
    for (uint32_t x = threadIdx.x; x < SRE_LR_SLOTS * nd; x += SRE_LR_THREADS) c[x] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
        const uint32_t slot = sre_lr_slot(wave, q);
        it[q] = load_item<FIRST>(keyid, src, sre_lr_line(blockIdx.x, slot, lane), n, rows, all);
        rk[q] = slot_rank<RULE>(it[q] != SRE_LRK_DROPPED, sre_lrk_digit(it[q], pass, bits), bits, lane, c + slot * nd);
    }
    __syncthreads();
    if (threadIdx.x < nd) {
        (void) sre_lr_slot_prefix(c + threadIdx.x, nd);
        gbase[threadIdx.x] = first[sre_lr_cnt_index(threadIdx.x, nwg, blockIdx.x)];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
        if (it[q] == SRE_LRK_DROPPED) continue;
        const uint32_t d = sre_lrk_digit(it[q], pass, bits);
        const uint64_t r = gbase[d] + c[sre_lr_slot(wave, q) * nd + d] + rk[q];
        if (r >= total) continue;       /* (cannot happen: the ranks are a permutation of 0 .. total - 1) */
        dst[r] = it[q];
    }
}

/* a lane per rank of the sorted items: its entry of the compact table, and head[r] = 1 for the first rank of a bucket */
__global__ __launch_bounds__(256) void
sre_k_route_key_table(const uint64_t *__restrict__ items, const uint64_t *__restrict__ ends, uint64_t nsel, uint64_t nlines,
                      uint64_t *__restrict__ cstart, uint64_t *__restrict__ cval, uint64_t *__restrict__ head)
{
    const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (r >= nsel) return;
    const uint64_t i = sre_lrk_item_line(items[r]);
    head[r] = sre_lrk_is_head(items, r) ? 1 : 0;
    if (i >= nlines) {                  /* (cannot happen: an item carries the number of its line) */
        cstart[r] = sre_lr_entry_start(0);
        cval[r] = 1;
        return;
    }
    const uint64_t st = line_start(ends, i);
    sre_lrk_entry(st, ends[i] - st, cstart + r, cval + r);
}

/* behind the scan of head[] to hoff[0 .. nsel]: hrank[b] = the rank of bucket b's head, hrank[nbuckets] = nsel */
__global__ __launch_bounds__(256) void
sre_k_route_key_heads(const uint64_t *__restrict__ items, const uint64_t *__restrict__ hoff, uint64_t nsel,
                      uint64_t *__restrict__ hrank)
{
    const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (r >= nsel) return;
    const uint64_t b = hoff[r];
    if (b > r) return;                  /* (cannot happen: at most r heads in front of rank r) */
    if (sre_lrk_is_head(items, r)) hrank[b] = r;
    if (r == nsel - 1) hrank[hoff[nsel] <= nsel ? hoff[nsel] : nsel] = nsel;
}

/* a lane per bucket in front of min(buckets_cap, nbuckets): its row of five words */
__global__ __launch_bounds__(256) void
sre_k_route_key_buckets(const uint64_t *__restrict__ items, const uint64_t *__restrict__ hoff, const uint64_t *__restrict__ hrank,
                        const uint64_t *__restrict__ coff, uint64_t nsel, uint64_t rows, uint64_t buckets_cap,
                        int64_t *__restrict__ out)
{
    const uint64_t nb = hoff[nsel];
    const uint64_t limit = buckets_cap < nb ? buckets_cap : nb;
    const uint64_t b = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (b >= limit || b >= nsel) return;
    if (hrank[b] >= nsel || hrank[b + 1] > nsel) return;        /* (cannot happen) */
    sre_lrk_bucket_row(items, hrank, b, coff, rows, out + b * 5);
}

/* one lane: the cut and the words the host reads.  coff and hoff are not read when nsel == 0 */
__global__ __launch_bounds__(64) void
sre_k_route_key_finish(const uint64_t *__restrict__ coff, const uint64_t *__restrict__ hoff, uint64_t nsel, uint64_t out_cap,
                       const sre_lines_info_t *__restrict__ info, uint64_t *__restrict__ res)
{
    if (threadIdx.x != 0) return;
    const uint64_t cut = nsel ? sre_lr_cut(coff, nsel, out_cap) : 0;
    res[SRE_LRK_RES_NSEL] = nsel;
    res[SRE_LRK_RES_NEED] = nsel ? coff[nsel] : 0;
    res[SRE_LRK_RES_WRITTEN] = cut;
    res[SRE_LRK_RES_BYTES] = nsel ? coff[cut] : 0;
    res[SRE_LRK_RES_NBUCKETS] = nsel ? hoff[nsel] : 0;
    res[SRE_LRK_RES_NKEYED] = info->knkeyed;
    res[SRE_LRK_RES_NMEMBERS] = info->knmembers;
}

/* rows [line, start, len, output offset, id] of the first min(index_cap, written) ranks */
__global__ __launch_bounds__(256) void
sre_k_route_key_index(const uint64_t *__restrict__ items, const uint64_t *__restrict__ cstart, const uint64_t *__restrict__ coff,
                      const uint64_t *__restrict__ res, uint64_t rows, uint64_t index_cap, int64_t *__restrict__ out)
{
    const uint64_t written = res[SRE_LRK_RES_WRITTEN];
    const uint64_t limit = index_cap < written ? index_cap : written;
    const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (r >= limit) return;
    sre_lrk_index_row(items, cstart, coff, r, rows, out + r * 5);
}

template <bool FIRST>
hipError_t
launch_pass(bool scatter, int rule, const int64_t *d_keyid, const uint64_t *d_src, uint64_t n, uint64_t rows, int all, uint32_t pass,
            uint32_t bits, uint64_t *d_cnt, const uint64_t *d_first, uint64_t total, uint64_t *d_dst, hipStream_t stream)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || bits < 1 || bits > SRE_LRK_MAX_BITS || pass * bits >= SRE_LRK_LINE_BITS || nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t) nwg), block(SRE_LR_THREADS);
    if (!scatter) {
        if (rule == SRE_LRK_RANK_TURNS) {
            hipLaunchKernelGGL((sre_k_route_key_count<FIRST, SRE_LRK_RANK_TURNS>), grid, block, 0, stream, d_keyid, d_src, n, rows, all,
                               pass, bits, nwg, d_cnt);
        } else {
            hipLaunchKernelGGL((sre_k_route_key_count<FIRST, SRE_LRK_RANK_BITS>), grid, block, 0, stream, d_keyid, d_src, n, rows, all,
                               pass, bits, nwg, d_cnt);
        }
    } else {
        if (total == 0) return hipSuccess;
        if (rule == SRE_LRK_RANK_TURNS) {
            hipLaunchKernelGGL((sre_k_route_key_scatter<FIRST, SRE_LRK_RANK_TURNS>), grid, block, 0, stream, d_keyid, d_src, n, rows, all,
                               pass, bits, nwg, d_first, total, d_dst);
        } else {
            hipLaunchKernelGGL((sre_k_route_key_scatter<FIRST, SRE_LRK_RANK_BITS>), grid, block, 0, stream, d_keyid, d_src, n, rows, all,
                               pass, bits, nwg, d_first, total, d_dst);
        }
    }
    return hipGetLastError();
}

}  // namespace

extern "C" hipError_t
sre_launch_route_key_count(const int64_t *d_keyid, const uint64_t *d_src, uint64_t n, uint64_t rows, int all, uint32_t pass,
                           uint32_t bits, int rule, uint64_t *d_cnt, hipStream_t stream)
{
    return d_keyid ? launch_pass<true>(false, rule, d_keyid, NULL, n, rows, all, 0, bits, d_cnt, NULL, 0, NULL, stream)
                   : launch_pass<false>(false, rule, NULL, d_src, n, rows, all, pass, bits, d_cnt, NULL, 0, NULL, stream);
}

extern "C" hipError_t
sre_launch_route_key_scatter(const int64_t *d_keyid, const uint64_t *d_src, uint64_t n, uint64_t rows, int all, uint32_t pass,
                             uint32_t bits, int rule, const uint64_t *d_first, uint64_t total, uint64_t *d_dst, hipStream_t stream)
{
    return d_keyid ? launch_pass<true>(true, rule, d_keyid, NULL, n, rows, all, 0, bits, NULL, d_first, total, d_dst, stream)
                   : launch_pass<false>(true, rule, NULL, d_src, n, rows, all, pass, bits, NULL, d_first, total, d_dst, stream);
}

extern "C" hipError_t
sre_launch_route_key_table(const uint64_t *d_items, const uint64_t *d_ends, uint64_t nsel, uint64_t nlines, uint64_t *d_cstart,
                           uint64_t *d_cval, uint64_t *d_head, hipStream_t stream)
{
    if (nsel == 0) return hipSuccess;
    const uint64_t nblk = (nsel + 255) / 256;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_route_key_table, dim3((uint32_t) nblk), dim3(256), 0, stream, d_items, d_ends, nsel, nlines, d_cstart,
                       d_cval, d_head);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_route_key_buckets(const uint64_t *d_items, const uint64_t *d_hoff, uint64_t *d_hrank, const uint64_t *d_coff, uint64_t nsel,
                             uint64_t rows, uint64_t buckets_cap, int64_t *d_buckets, hipStream_t stream)
{
    if (nsel == 0 || buckets_cap == 0) return hipSuccess;
    const uint64_t nblk = (nsel + 255) / 256, most = buckets_cap < nsel ? buckets_cap : nsel;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_route_key_heads, dim3((uint32_t) nblk), dim3(256), 0, stream, d_items, d_hoff, nsel, d_hrank);
    hipLaunchKernelGGL(sre_k_route_key_buckets, dim3((uint32_t) ((most + 255) / 256)), dim3(256), 0, stream, d_items, d_hoff, d_hrank,
                       d_coff, nsel, rows, buckets_cap, d_buckets);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_route_key_finish(const uint64_t *d_coff, const uint64_t *d_hoff, uint64_t nsel, uint64_t out_cap,
                            const sre_lines_info_t *d_info, uint64_t *d_res, hipStream_t stream)
{
    hipLaunchKernelGGL(sre_k_route_key_finish, dim3(1), dim3(64), 0, stream, d_coff, d_hoff, nsel, out_cap, d_info, d_res);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_route_key_index(const uint64_t *d_items, const uint64_t *d_cstart, const uint64_t *d_coff, const uint64_t *d_res,
                           uint64_t rows, uint64_t nrows, uint64_t index_cap, int64_t *d_index, hipStream_t stream)
{
    if (nrows == 0 || index_cap == 0) return hipSuccess;
    const uint64_t nblk = (nrows + 255) / 256;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_route_key_index, dim3((uint32_t) nblk), dim3(256), 0, stream, d_items, d_cstart, d_coff, d_res, rows,
                       index_cap, d_index);
    return hipGetLastError();
}
