/*
 * sre_hip_lines_tally.hip — the line tally on the device (sregex_hip.h sre_hip_tally_lines): the
 * distinct keys of the extract's entry table (the tuple of a line's field texts) and how many lines carry each, through
 * a hash table of line numbers.  The rules are those of sre_lines_tally.h, which the CPU model compiles too.
 *
 *   insert     after the extract's last select pass, a lane per line: hash the fields, group the wave's lines by key;
 *              the lowest lane of a group probes linearly, claims an empty word with a compare-and-swap or joins the
 *              word of an equal key with a minimum; per wave one add of the selected lines, one of the claims, and one
 *              add to the counts per distinct key of the wave;
 *   keep       a lane per entry: the entries of every line that is not the final word of its slot become 0, so the
 *              entry table selects exactly the first line of every key;
 *   (the extract's scan, finish, gather and index run over that table unchanged: sre_hip_lines_gather.hip)
 *   ranks      workgroups over the entries as the extract's index has them: the rank of a kept line among the kept
 *              lines is the number of its key; the line delivers its slot's count there and leaves the number in the
 *              count's place;
 *   keyid      a lane per line: the number found through the line's slot.
 *
 * The tally with sums (sre_hip_tally_sums_lines, DESIGN.md §4.11.8, rules in sre_lines_sums.h) adds behind the ranks
 *   sums       a lane per line: the key number through the slot, the line's numbers through the value table; the wave
 *              groups its lanes by key number, merges the members' numbers across the lanes and sends one add, minimum,
 *              maximum and add per key and column of the wave, to the wave's COPY of the rows (a hot row would otherwise
 *              take the atomics of every wave on one cache line).  Every access to the aggregates is an atomic at agent
 *              scope; the copies were set to the identity by a kernel in front, and a kernel behind merges them into the
 *              caller's rows.
 *
 * Inside the insert every access to the table, the counts and the three info words is an atomic at agent scope: the
 * L2s of the eight XCDs do not see one another's plain stores within a kernel.  The later kernels read all of it with
 * plain loads, behind the kernel boundary.  No workgroup waits for another.  Plain C++ and vector memory operations only.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"
#include "sre_lines_tally.h"
#include "sre_lines_sums.h"
#include "sre_hip_lines_block.h"

namespace {

#define LT_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

/* the entry table as the insert reads it (written by earlier kernels or copies: plain loads) */
struct TallyKeys {
    const uint8_t  *buf;
    const uint64_t *val, *start;
    uint32_t        k;
    __device__ inline bool     selected(uint64_t line) const { return val[line * k] != 0; }
    __device__ inline uint64_t len(uint64_t line, uint32_t f) const { return val[line * k + f] - 1; }
    __device__ inline uint8_t  byte(uint64_t line, uint32_t f, uint64_t j) const
    {
        return buf[(start[line * k + f] & SRE_LG_ENTRY_START) + j];
    }
};

struct TallyMem {
    uint64_t         *tab;
    sre_lines_info_t *info;
    __device__ inline uint64_t cas(uint64_t idx, uint64_t expect, uint64_t v)
    {
        (void) __hip_atomic_compare_exchange_strong(&tab[idx], &expect, v, __ATOMIC_RELAXED, LT_RELAXED_AGENT);
        return expect;
    }
    __device__ inline void min(uint64_t idx, uint64_t v) { (void) __hip_atomic_fetch_min(&tab[idx], v, LT_RELAXED_AGENT); }
    __device__ inline bool raised() { return __hip_atomic_load(&info->tover, LT_RELAXED_AGENT) != 0; }
};

__global__ __launch_bounds__(SRE_LT_THREADS) void
sre_k_tally_insert(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ val, const uint64_t *__restrict__ start,
                   uint64_t n, uint32_t k, sre_lt_params_t p, uint64_t *tab, uint64_t *cnt, uint32_t *__restrict__ lslot,
                   sre_lines_info_t *info)
{
    const uint64_t  i = (uint64_t) blockIdx.x * SRE_LT_THREADS + threadIdx.x;
    const uint32_t  lane = threadIdx.x & 63u;
    const TallyKeys keys = {buf, val, start, k};
    TallyMem        mem = {tab, info};
    const bool      sel = i < n && keys.selected(i);
    const uint64_t  h = sel ? sre_lt_hash(keys, i) : 0;
    /* the wave's groups: a turn per distinct key of its 64 lines */
    uint64_t rem = __ballot(sel);
    uint32_t lead_of = lane, group = 0;
    while (rem) {
        const uint32_t lead = sre_lr_leader(rem);
        const uint64_t lh = (uint64_t) __shfl((unsigned long long) h, (int) lead, 64);
        const bool     mine = ((rem >> lane) & 1u) != 0 && sre_lt_same_key(keys, h, i, lh, i - lane + lead);
        const uint64_t m = __ballot(mine);
        if (mine) lead_of = lead;
        if (lane == lead) group = sre_lr_popc(m);
        rem &= ~m;
    }
    const bool    leads = sel && lead_of == lane;
    sre_lt_lane_t L;
    sre_lt_begin(L, i, leads, h, p);
    while (!sre_lt_done(L)) sre_lt_step(L, keys, mem, p);
    /* the wave settles: its selected lines, its claims, then every leader's group to the count of its slot */
    const uint64_t msel = __ballot(sel), mclaim = __ballot(L.claimed), mwrap = __ballot(L.wrapped);
    if (lane == 0) {
        bool over = mwrap != 0;
        if (msel) (void) __hip_atomic_fetch_add(&info->tsel, (uint64_t) sre_lr_popc(msel), LT_RELAXED_AGENT);
        if (mclaim) {
            const uint32_t mine = sre_lr_popc(mclaim);
            const uint64_t base = __hip_atomic_fetch_add(&info->tclaims, (uint64_t) mine, LT_RELAXED_AGENT);
            over = over || sre_lt_claims_overflow(base, mine, p);
        }
        if (over) __hip_atomic_store(&info->tover, (uint64_t) 1, LT_RELAXED_AGENT);
    }
    if (leads && L.slot != SRE_LT_NONE) (void) __hip_atomic_fetch_add(&cnt[L.slot], (uint64_t) group, LT_RELAXED_AGENT);
    const uint32_t slot = (uint32_t) __shfl((int) L.slot, (int) lead_of, 64);
    if (i < n) lslot[i] = sel ? slot : SRE_LT_NONE;
}

/* lane per entry */
__global__ __launch_bounds__(256) void
sre_k_tally_keep(uint64_t *__restrict__ val, uint64_t nent, uint32_t k, const uint64_t *__restrict__ tab,
                 const uint32_t *__restrict__ lslot)
{
    const uint64_t e = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (e >= nent) return;
    const uint64_t line = e / k;
    if (!sre_lt_keeps(lslot[line], line, tab)) val[e] = 0;
}

/* workgroups over the ENTRIES as in the extract's scan and index: the lane that holds the first entry of a kept line
 * has the line's rank among the kept lines, the selected entries in front of it over k */
__global__ __launch_bounds__(256) void
sre_k_tally_ranks(const uint64_t *__restrict__ off, const uint64_t *__restrict__ starts, uint64_t nent, uint64_t k,
                  const uint64_t *__restrict__ blkc, const uint32_t *__restrict__ lslot, uint64_t *__restrict__ cnt,
                  uint64_t *__restrict__ counts, uint64_t counts_cap)
{
    __shared__ uint64_t wsum[4];
    const uint64_t      q0 = (uint64_t) blockIdx.x * SRE_LINES_ITEMS + 4u * threadIdx.x;
    uint32_t            f[4];
    uint64_t            s = 0;
    for (uint32_t q = 0; q < 4; q++) {
        f[q] = q0 + q < nent && off[q0 + q + 1] > off[q0 + q];
        s += f[q];
    }
    uint64_t total;
    uint64_t r = blkc[blockIdx.x] + block_excl_scan<256>(s, wsum, total);
    for (uint32_t q = 0; q < 4; q++) {
        if (!f[q]) continue;
        const uint64_t e = q0 + q;
        if (starts[e] & SRE_LG_ENTRY_FIRST) {
            const uint64_t rank = r / k;
            const uint32_t slot = lslot[e / k];         /* (a kept line has one) */
            if (slot != SRE_LT_NONE) {
                if (rank < counts_cap) counts[rank] = cnt[slot];
                cnt[slot] = rank;
            }
        }
        r++;
    }
}

/* lane per line */
__global__ __launch_bounds__(256) void
sre_k_tally_keyid(const uint32_t *__restrict__ lslot, const uint64_t *__restrict__ cnt, uint64_t n, int64_t *__restrict__ keyid)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = lslot[i];
    keyid[i] = slot == SRE_LT_NONE ? -1 : (int64_t) cnt[slot];
}

/* ---- the sums (sre_lines_sums.h) ---- */

/* the value table as the sums kernel reads it (written by earlier kernels or copies: plain loads) */
struct SumVals {
    const uint8_t  *buf;
    const uint64_t *vval, *vstart;
    uint32_t        v;
    __device__ inline uint64_t val(uint64_t line, uint32_t c) const { return vval[line * v + c]; }
    __device__ inline uint64_t raw(uint64_t line, uint32_t c) const { return vstart[line * v + c]; }
    __device__ inline uint8_t  byte(uint64_t at) const { return buf[at]; }
};

struct SumMem {
    sre_ls_agg_t *sums;
    __device__ inline void add_sum(uint64_t idx, int64_t v)
    {
        (void) __hip_atomic_fetch_add(reinterpret_cast<uint64_t *>(&sums[idx].sum), (uint64_t) v, LT_RELAXED_AGENT);
    }
    __device__ inline void min(uint64_t idx, int64_t v) { (void) __hip_atomic_fetch_min(&sums[idx].min, v, LT_RELAXED_AGENT); }
    __device__ inline void max(uint64_t idx, int64_t v) { (void) __hip_atomic_fetch_max(&sums[idx].max, v, LT_RELAXED_AGENT); }
    __device__ inline void add_n(uint64_t idx, uint64_t v) { (void) __hip_atomic_fetch_add(&sums[idx].n, v, LT_RELAXED_AGENT); }
};

__device__ inline uint64_t
wave_get(uint64_t v, uint32_t lane)
{
    return (uint64_t) __shfl((unsigned long long) v, (int) lane, 64);
}

/* every lane gets the merge of all 64 lanes' aggregates */
__device__ inline sre_ls_agg_t
wave_merge(sre_ls_agg_t g)
{
    for (int d = 1; d < 64; d <<= 1) {
        sre_ls_agg_t o;
        o.sum = (int64_t) __shfl_xor((long long) g.sum, d, 64);
        o.min = (int64_t) __shfl_xor((long long) g.min, d, 64);
        o.max = (int64_t) __shfl_xor((long long) g.max, d, 64);
        o.n = (uint64_t) __shfl_xor((unsigned long long) g.n, d, 64);
        g = sre_ls_merge(g, o);
    }
    return g;
}

/* lane per aggregate */
__global__ __launch_bounds__(256) void
sre_k_tally_sums_init(sre_ls_agg_t *__restrict__ sums, uint64_t count)
{
    const uint64_t x = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (x < count) sums[x] = sre_ls_identity();
}

/* lane per aggregate, behind the sums: the caller's aggregate is the merge of its copies (plain loads and a plain store,
 * behind the kernel boundary) */
__global__ __launch_bounds__(256) void
sre_k_tally_sums_merge(const sre_ls_agg_t *__restrict__ copy, uint32_t copies, uint64_t count, sre_ls_agg_t *__restrict__ sums)
{
    const uint64_t x = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (x >= count) return;
    sre_ls_agg_t a = sre_ls_identity();
    for (uint32_t c = 0; c < copies; c++) a = sre_ls_merge(a, copy[(uint64_t) c * count + x]);
    sums[x] = a;
}

/* lane per line, behind the ranks: cnt[slot] is the key number.  tests/lines_sums_sim.cpp re-types this kernel's grouping
 * loop, its alone / shared split and its merge lane by lane; only sre_lines_sums.h is common text, so a change here has to
 * be made there too, or the model's atomic counts no longer speak for the kernel */
__global__ __launch_bounds__(SRE_LS_THREADS) void
sre_k_tally_sums(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ vval, const uint64_t *__restrict__ vstart,
                 uint64_t n, uint32_t v, const uint32_t *__restrict__ lslot, const uint64_t *__restrict__ cnt, uint64_t rows,
                 uint32_t copies, sre_ls_agg_t *sums)
{
    const uint64_t i = (uint64_t) blockIdx.x * SRE_LS_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const SumVals  vals = {buf, vval, vstart, v};
    /* the wave's copy of the rows */
    SumMem         mem = {sums + (uint64_t) sre_ls_copy_of(i / 64u, copies) * rows * v};
    const uint32_t slot = i < n ? lslot[i] : SRE_LT_NONE;
    const uint64_t key = slot != SRE_LT_NONE ? cnt[slot] : 0;
    const bool     part = sre_ls_takes_part(slot, key, rows);
    /* the wave's groups: a turn per distinct key number of its lanes; every member keeps the group's ballot */
    uint64_t rem = __ballot(part), members = 0;
    while (rem) {
        const uint32_t lead = sre_lr_leader(rem);
        const uint64_t lk = wave_get(key, lead);
        const bool     mine = ((rem >> lane) & 1u) != 0 && key == lk;
        const uint64_t m = __ballot(mine);
        if (mine) members = m;
        rem &= ~m;
    }
    const bool     alone = part && sre_lr_popc(members) == 1;
    /* the leaders of the groups of more than one lane */
    const uint64_t shared = __ballot(part && !alone && sre_lr_leader(members) == lane);
    for (uint32_t c = 0; c < v; c++) {
        const sre_ls_agg_t a = part ? sre_ls_line(vals, i, c) : sre_ls_identity();
        const uint64_t     idx = sre_ls_index(key, v, c);
        if (alone) sre_ls_flush(mem, idx, a);
        for (uint64_t todo = shared; todo; todo &= todo - 1) {
            const uint32_t lead = sre_lr_leader(todo);
            const bool     in = ((wave_get(members, lead) >> lane) & 1u) != 0;
            if (__ballot(in && a.n != 0) == 0) continue;            /* no number in the group: nothing is sent */
            const sre_ls_agg_t g = wave_merge(in ? a : sre_ls_identity());
            if (lane == lead) sre_ls_flush(mem, idx, g);
        }
    }
}

}  // namespace

extern "C" hipError_t
sre_launch_tally_insert(const void *d_buf, uint64_t *d_val, const uint64_t *d_start, uint64_t n, uint32_t k, uint64_t nslots,
                        uint64_t max_keys, uint64_t hash_mask, uint64_t *d_tab, uint64_t *d_cnt, uint32_t *d_lslot,
                        sre_lines_info_t *d_info, hipStream_t stream)
{
    if (n == 0 || k == 0 || k > SRE_EXTRACT_MAX_FIELDS) return hipErrorInvalidValue;
    /* (a slot number fits the 32-bit word of a line, SRE_LT_NONE apart) */
    if (nslots < SRE_LT_MIN_SLOTS || (nslots & (nslots - 1)) != 0 || nslots > ((uint64_t) 1 << 31) || max_keys == 0
        || 2 * max_keys > nslots)
    {
        return hipErrorInvalidValue;
    }
    const uint64_t nent = n * k, nwg = (n + SRE_LT_THREADS - 1) / SRE_LT_THREADS, nwe = (nent + 255) / 256;
    if (nwg > 0x7FFFFFFFull || nwe > 0x7FFFFFFFull) return hipErrorInvalidValue;
    sre_lt_params_t p;
    p.nslots = nslots;
    p.max_keys = max_keys;
    p.hash_mask = hash_mask;
    hipLaunchKernelGGL(sre_k_tally_insert, dim3((uint32_t) nwg), dim3(SRE_LT_THREADS), 0, stream,
                       static_cast<const uint8_t *>(d_buf), d_val, d_start, n, k, p, d_tab, d_cnt, d_lslot, d_info);
    hipLaunchKernelGGL(sre_k_tally_keep, dim3((uint32_t) nwe), dim3(256), 0, stream, d_val, nent, k, d_tab, d_lslot);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_tally_ranks(const uint64_t *d_off, const uint64_t *d_start, uint64_t n, uint32_t k, const uint64_t *d_blk,
                       const uint32_t *d_lslot, uint64_t *d_cnt, uint64_t *d_counts, uint64_t counts_cap, int64_t *d_keyid,
                       uint64_t keyid_cap, hipStream_t stream)
{
    if (n == 0 || k == 0) return hipErrorInvalidValue;
    if (counts_cap == 0 && keyid_cap == 0) return hipSuccess;
    const uint64_t nent = n * k, nblk = (nent + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_tally_ranks, dim3((uint32_t) nblk), dim3(256), 0, stream, d_off, d_start, nent, (uint64_t) k,
                       d_blk + nblk, d_lslot, d_cnt, d_counts, counts_cap);
    if (keyid_cap != 0) {
        const uint64_t m = keyid_cap < n ? keyid_cap : n;
        hipLaunchKernelGGL(sre_k_tally_keyid, dim3((uint32_t) ((m + 255) / 256)), dim3(256), 0, stream, d_lslot, d_cnt, m, d_keyid);
    }
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_tally_numbers(const uint64_t *d_off, const uint64_t *d_start, uint64_t n, uint32_t k, const uint64_t *d_blk,
                         const uint32_t *d_lslot, uint64_t *d_cnt, hipStream_t stream)
{
    if (n == 0 || k == 0) return hipErrorInvalidValue;
    const uint64_t nent = n * k, nblk = (nent + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_tally_ranks, dim3((uint32_t) nblk), dim3(256), 0, stream, d_off, d_start, nent, (uint64_t) k,
                       d_blk + nblk, d_lslot, d_cnt, static_cast<uint64_t *>(nullptr), (uint64_t) 0);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_tally_sums(const void *d_buf, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n, uint32_t v,
                      const uint32_t *d_lslot, const uint64_t *d_cnt, uint64_t rows, void *d_sums, void *d_copies, uint32_t copies,
                      hipStream_t stream)
{
    if (n == 0 || v == 0 || v > SRE_LS_MAX_VALUES || rows > SRE_LT_MAX_KEYS || copies == 0 || copies > SRE_LS_MAX_COPIES
        || (copies > 1 && d_copies == NULL))
    {
        return hipErrorInvalidValue;
    }
    if (rows == 0) return hipSuccess;
    const uint64_t nwg = (n + SRE_LS_THREADS - 1) / SRE_LS_THREADS, count = rows * v, all = count * copies;
    if (nwg > 0x7FFFFFFFull || (all + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    sre_ls_agg_t *sums = static_cast<sre_ls_agg_t *>(d_sums);
    sre_ls_agg_t *to = copies > 1 ? static_cast<sre_ls_agg_t *>(d_copies) : sums;
    hipLaunchKernelGGL(sre_k_tally_sums_init, dim3((uint32_t) ((all + 255) / 256)), dim3(256), 0, stream, to, all);
    hipLaunchKernelGGL(sre_k_tally_sums, dim3((uint32_t) nwg), dim3(SRE_LS_THREADS), 0, stream, static_cast<const uint8_t *>(d_buf),
                       d_vval, d_vstart, n, v, d_lslot, d_cnt, rows, copies, to);
    if (copies > 1) {
        hipLaunchKernelGGL(sre_k_tally_sums_merge, dim3((uint32_t) ((count + 255) / 256)), dim3(256), 0, stream, to, copies, count,
                           sums);
    }
    return hipGetLastError();
}
