/*
 * sre_hip_lines_partition.h — the stable partition pass of the line route (sre_hip_lines_route.hip), of every digit pass of
 * the line route by key (sre_hip_lines_route_key.hip) and of the line sort (sre_hip_lines_sort.hip), DESIGN.md §4.11.6.  The
 * geometry and the rules are those of sre_lines_route.h, the rank inside a slot is slot_rank of sre_hip_lines_rank.h.
 * Device code only.
 *
 *   count      a workgroup takes SRE_LR_ITEMS items in order and writes how many have each digit to cnt[d * nwg + w]; the
 *              filter's scan (sre_launch_filter_offsets) over those words gives every (digit, workgroup) its first rank;
 *   scatter    the same workgroups recompute the rank of every item and store it at that rank.
 *
 * What an item is belongs to the caller: a PASS type P, handed to the kernels by value, with
 *   P::MAX_DIGITS      the most digits a pass has (the size of the LDS arrays), P::RULE the rank rule of a slot;
 *   nd(), bits()       the digits of this pass and the width of a digit;
 *   load(i)            item i (one word), whatever i is: an i beyond the items gives an item that is not taken;
 *   taken(item)        the item takes part: it is counted and stored;
 *   digit(item)        its digit, below nd() when it is taken;
 *   store(r, item, i)  scatter only: item i goes to rank r.
 *
 * No workgroup waits for another and no rank comes from an atomic.  Plain C++ and vector memory operations only.
 */
#ifndef SRE_HIP_LINES_PARTITION_H
#define SRE_HIP_LINES_PARTITION_H

#include "sre_hip_lines_block.h"
#include "sre_hip_lines_rank.h"

namespace {

/* workgroup w: cnt[d * nwg + w] = its items of digit d */
template <class P>
__global__ __launch_bounds__(SRE_LR_THREADS) void
sre_k_partition_count(const P p, uint64_t nwg, uint64_t *__restrict__ cnt)
{
    __shared__ uint32_t c[SRE_LR_SLOTS * P::MAX_DIGITS];
    const uint32_t      lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nd = p.nd();
    for (uint32_t x = threadIdx.x; x < SRE_LR_SLOTS * nd; x += SRE_LR_THREADS) c[x] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
        const uint32_t slot = sre_lr_slot(wave, q);
        const uint64_t it = p.load(sre_lr_line(blockIdx.x, slot, lane));
        (void) slot_rank<P::RULE>(p.taken(it), p.digit(it), p.bits(), lane, c + slot * nd);
    }
    __syncthreads();
    if (threadIdx.x < nd) cnt[sre_lr_cnt_index(threadIdx.x, nwg, blockIdx.x)] = sre_lr_slot_prefix(c + threadIdx.x, nd);
}

/* the same workgroups over the scanned counts `first`: every taken item is stored at its rank (total items) */
template <class P>
__global__ __launch_bounds__(SRE_LR_THREADS) void
sre_k_partition_scatter(const P p, uint64_t nwg, const uint64_t *__restrict__ first, uint64_t total)
{
    __shared__ uint32_t c[SRE_LR_SLOTS * P::MAX_DIGITS];
    __shared__ uint64_t gbase[P::MAX_DIGITS];
    const uint32_t      lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nd = p.nd();
    uint64_t            it[SRE_LR_ROUNDS];
    uint32_t            rk[SRE_LR_ROUNDS];
    for (uint32_t x = threadIdx.x; x < SRE_LR_SLOTS * nd; x += SRE_LR_THREADS) c[x] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
        const uint32_t slot = sre_lr_slot(wave, q);
        it[q] = p.load(sre_lr_line(blockIdx.x, slot, lane));
        rk[q] = slot_rank<P::RULE>(p.taken(it[q]), p.digit(it[q]), p.bits(), lane, c + slot * nd);
    }
    __syncthreads();
    if (threadIdx.x < nd) {
        (void) sre_lr_slot_prefix(c + threadIdx.x, nd);
        gbase[threadIdx.x] = first[sre_lr_cnt_index(threadIdx.x, nwg, blockIdx.x)];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
        if (!p.taken(it[q])) continue;
        const uint32_t slot = sre_lr_slot(wave, q);
        const uint32_t d = p.digit(it[q]);
        const uint64_t r = gbase[d] + c[slot * nd + d] + rk[q];
        if (r >= total) continue;       /* (cannot happen: the ranks are a permutation of 0 .. total - 1) */
        p.store(r, it[q], sre_lr_line(blockIdx.x, slot, lane));
    }
}

/* behind the last pass of a sort: the compact-table entry of line i at rank r */
__device__ inline void
compact_entry(const uint64_t *__restrict__ ends, uint64_t i, uint64_t nlines, uint64_t r, uint64_t *__restrict__ cstart,
              uint64_t *__restrict__ cval)
{
    if (i >= nlines) {                  /* (cannot happen: an item carries the number of its line) */
        cstart[r] = sre_lr_entry_start(0);
        cval[r] = 1;
        return;
    }
    const uint64_t st = line_start(ends, i);
    sre_lrk_entry(st, ends[i] - st, cstart + r, cval + r);
}

}  // namespace

#endif
