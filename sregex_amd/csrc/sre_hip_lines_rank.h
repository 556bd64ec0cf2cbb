/*
 * sre_hip_lines_rank.h — the rank of an item inside its 64-lane slot, for the partition pass (sre_hip_lines_partition.h) of
 * the line route, the line route by key and the line sort; the rules are those of sre_lines_route_key.h.  Device code only.
 */
#ifndef SRE_HIP_LINES_RANK_H
#define SRE_HIP_LINES_RANK_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sre_lines_route_key.h"

namespace {

/* the rank of the lane among the lanes of its slot with its digit; the lowest lane of every digit present leaves the
 * slot's count of it in c[digit].  Every lane of the wave calls it.  RULE: SRE_LRK_RANK_BITS or SRE_LRK_RANK_TURNS */
template <int RULE>
__device__ inline uint32_t
slot_rank(bool sel, uint32_t digit, uint32_t bits, uint32_t lane, uint32_t *c)
{
    if (RULE == SRE_LRK_RANK_TURNS) {
        uint32_t rank = 0;
        uint64_t rem = __ballot(sel);
        while (rem) {
            const uint32_t lead = sre_lr_leader(rem);
            const uint32_t kd = (uint32_t) __shfl((int) digit, (int) lead, 64);
            const uint64_t m = __ballot(sel && digit == kd);
            if (sel && digit == kd) rank = sre_lr_rank_in(m, lane);
            if (lane == lead) c[kd] = sre_lr_popc(m);
            rem &= ~m;
        }
        return rank;
    }
    uint64_t m = __ballot(sel);
    for (uint32_t bit = 0; bit < bits; bit++) m = sre_lrk_agree(m, __ballot(sel && ((digit >> bit) & 1u)), digit, bit);
    const uint32_t rank = sre_lr_rank_in(m, lane);
    if (sel && rank == 0) c[digit] = sre_lr_popc(m);
    return sel ? rank : 0;
}

}  // namespace

#endif
