/*
 * sre_hip_lines_distinct.hip — the line distinct on the device (sregex_hip.h sre_hip_distinct_lines):
 * behind the tally's insert over the key table (sre_hip_lines_tally.hip), which leaves every line's slot, every slot's
 * first line and count, the selection of lines by first, last or count of their key.  The rules are those of
 * sre_lines_distinct.h, which the CPU model compiles too.
 *
 *   last       (SRE_HIP_DISTINCT_LAST only) a lane per line: the wave groups its lanes by slot, and the highest lane of
 *              every group sends its line to an atomic maximum of the slot's word of the third run: one atomic per
 *              distinct slot of a wave;
 *   pick       a lane per line: the slot's first line, count and last line with plain loads, behind the kernel boundary;
 *              the filter's per-line value stays for a selected line and becomes 0 for every other; per workgroup one
 *              add of the qualifying keys, each counted at its first line;
 *   (the filter's scan, cut, gather and index run over the values unchanged: sre_hip_lines_gather.hip)
 *   perline    a lane per line: the count and the first line of the line's key to the caller's arrays.
 *
 * The maximum of `last` and the add of `pick` are atomics at agent scope: the L2s of the eight XCDs do not see one
 * another's plain stores within a kernel.  Everything else is plain loads and stores.  No workgroup waits for another,
 * no kernel loops more than 64 times.  Plain C++ and vector memory operations only.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"
#include "sre_lines_distinct.h"

namespace {

#define LD_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

/* the finished runs of the table as pick and perline read them */
struct DistinctTab {
    const uint64_t *tab, *cnt, *lastrun;
    __device__ inline uint64_t first(uint32_t slot) const { return tab[slot]; }
    __device__ inline uint64_t count(uint32_t slot) const { return cnt[slot]; }
    __device__ inline uint64_t last(uint32_t slot) const { return lastrun[slot]; }
};

/* lane per line */
__global__ __launch_bounds__(SRE_LD_THREADS) void
sre_k_distinct_last(const uint32_t *__restrict__ lslot, uint64_t n, uint64_t *lastrun)
{
    const uint64_t i = (uint64_t) blockIdx.x * SRE_LD_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = i < n ? lslot[i] : SRE_LT_NONE;
    /* the wave's groups: a turn per distinct slot of its 64 lines */
    uint64_t rem = __ballot(slot != SRE_LT_NONE);
    while (rem) {
        const uint32_t lead = sre_lr_leader(rem);
        const uint32_t ls = (uint32_t) __shfl((int) slot, (int) lead, 64);
        const bool     mine = ((rem >> lane) & 1u) != 0 && slot == ls;
        const uint64_t m = __ballot(mine);
        if (mine && lane == sre_ld_sender(m)) (void) __hip_atomic_fetch_max(&lastrun[slot], i, LD_RELAXED_AGENT);
        rem &= ~m;
    }
}

/* lane per line; the counts of the workgroup's waves meet in LDS, and one lane adds them to the call's word */
__global__ __launch_bounds__(SRE_LD_THREADS) void
sre_k_distinct_pick(const uint32_t *__restrict__ lslot, uint64_t n, const uint64_t *__restrict__ tab,
                    const uint64_t *__restrict__ cnt, const uint64_t *__restrict__ lastrun, int which, uint64_t min_count,
                    uint64_t max_count, int invert, uint64_t *__restrict__ fval, sre_lines_info_t *info)
{
    __shared__ uint32_t wkept[SRE_LD_THREADS / 64u];
    const uint64_t      i = (uint64_t) blockIdx.x * SRE_LD_THREADS + threadIdx.x;
    const uint32_t      lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const DistinctTab   t = {tab, cnt, lastrun};
    bool                counts = false;
    if (i < n) {
        const uint64_t v = fval[i];
        const uint64_t keep = sre_ld_value(t, which, min_count, max_count, invert != 0, i, lslot[i], v, &counts);
        if (keep != v) fval[i] = keep;
    }
    const uint32_t kept = sre_lr_popc(__ballot(counts));
    if (lane == 0) wkept[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0;
        for (uint32_t w = 0; w < SRE_LD_THREADS / 64u; w++) a += wkept[w];
        if (a) (void) __hip_atomic_fetch_add(&info->dkept, a, LD_RELAXED_AGENT);
    }
}

/* lane per line */
__global__ __launch_bounds__(SRE_LD_THREADS) void
sre_k_distinct_perline(const uint32_t *__restrict__ lslot, const uint64_t *__restrict__ tab, const uint64_t *__restrict__ cnt,
                       uint64_t *__restrict__ keycount, uint64_t keycount_n, int64_t *__restrict__ keyline, uint64_t keyline_n)
{
    const uint64_t i = (uint64_t) blockIdx.x * SRE_LD_THREADS + threadIdx.x;
    if (i >= keycount_n && i >= keyline_n) return;
    const DistinctTab t = {tab, cnt, nullptr};
    const uint32_t    slot = lslot[i];
    if (i < keycount_n) keycount[i] = sre_ld_keycount(t, slot);
    if (i < keyline_n) keyline[i] = sre_ld_keyline(t, slot);
}

bool
geometry_ok(uint64_t n, uint64_t nslots)
{
    /* (the slots of d_lslot are below nslots: sre_launch_tally_insert took the same table) */
    return n != 0 && (n + SRE_LD_THREADS - 1) / SRE_LD_THREADS <= 0x7FFFFFFFull && nslots >= SRE_LT_MIN_SLOTS
           && (nslots & (nslots - 1)) == 0 && nslots <= ((uint64_t) 1 << 31);
}

}  // namespace

extern "C" hipError_t
sre_launch_distinct_last(const uint32_t *d_lslot, uint64_t n, uint64_t nslots, uint64_t *d_last, hipStream_t stream)
{
    if (!geometry_ok(n, nslots) || d_last == NULL) return hipErrorInvalidValue;
    const uint64_t nwg = (n + SRE_LD_THREADS - 1) / SRE_LD_THREADS;
    hipLaunchKernelGGL(sre_k_distinct_last, dim3((uint32_t) nwg), dim3(SRE_LD_THREADS), 0, stream, d_lslot, n, d_last);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_distinct_pick(const uint32_t *d_lslot, uint64_t n, uint64_t nslots, const uint64_t *d_tab, const uint64_t *d_cnt,
                         const uint64_t *d_last, int which, uint64_t min_count, uint64_t max_count, int invert, uint64_t *d_fval,
                         sre_lines_info_t *d_info, hipStream_t stream)
{
    if (!geometry_ok(n, nslots) || which < SRE_LD_FIRST || which > SRE_LD_EVERY || !sre_ld_range_ok(min_count, max_count)
        || (which == SRE_LD_LAST && d_last == NULL))
    {
        return hipErrorInvalidValue;
    }
    const uint64_t nwg = (n + SRE_LD_THREADS - 1) / SRE_LD_THREADS;
    hipLaunchKernelGGL(sre_k_distinct_pick, dim3((uint32_t) nwg), dim3(SRE_LD_THREADS), 0, stream, d_lslot, n, d_tab, d_cnt, d_last,
                       which, min_count, max_count, invert, d_fval, d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_distinct_perline(const uint32_t *d_lslot, uint64_t n, uint64_t nslots, const uint64_t *d_tab, const uint64_t *d_cnt,
                            uint64_t *d_keycount, uint64_t keycount_cap, int64_t *d_keyline, uint64_t keyline_cap,
                            hipStream_t stream)
{
    if (!geometry_ok(n, nslots)) return hipErrorInvalidValue;
    const uint64_t kc = keycount_cap < n ? keycount_cap : n, kl = keyline_cap < n ? keyline_cap : n, m = kc > kl ? kc : kl;
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(sre_k_distinct_perline, dim3((uint32_t) ((m + SRE_LD_THREADS - 1) / SRE_LD_THREADS)), dim3(SRE_LD_THREADS), 0,
                       stream, d_lslot, d_tab, d_cnt, d_keycount, kc, d_keyline, kl);
    return hipGetLastError();
}
