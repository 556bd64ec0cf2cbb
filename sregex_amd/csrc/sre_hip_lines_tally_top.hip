/*
 * sre_hip_lines_tally_top.hip — the ordered tally on the device (sregex_hip.h sre_hip_tally_top_lines):
 * the tally's keys ordered by their count or by an aggregate, the line sort's radix sort over (order value, key number)
 * items, and the rows, counts, aggregates, index rows and ranks in that order.  The rules are those of
 * sre_lines_tally_top.h, which the CPU model compiles too.
 *
 *   first      behind the tally's ranks, a lane per line: the line the keep pass left selected for a key is the key's
 *              first line, first[key number] = line;
 *   values     the values pass of sre_hip_lines_values.h, a lane per key: the order value and the class of the key, and the
 *              four totals of the call;
 *   (the sort's digit passes run over the keys unchanged: sre_hip_lines_sort.hip, all = 1, the "line" of an item is the
 *   key's number)
 *   table      a lane per entry of the rows in front of the limit: the entries of the key's first line, copied from the
 *              extract's scanned entry table to the ordered table;
 *   (the extract's scan, finish and gather run over the ordered table unchanged: sre_hip_lines_gather.hip)
 *   permute    a lane per rank: the inverse permutation, and the count, the aggregates and the index row of the rank's key;
 *   ranks      a lane per line: the rank of the line's key through its slot and the inverse permutation.
 *
 * Every kernel reads what earlier kernels wrote with plain loads, behind the kernel boundary; only the four totals take
 * atomics, at agent scope.  No workgroup waits for another.  Plain C++ and vector memory operations only.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"
#include "sre_lines_tally_top.h"
#include "sre_hip_lines_block.h"
#include "sre_hip_lines_values.h"

namespace {

/* lane per line */
__global__ __launch_bounds__(256) void
sre_k_tally_top_first(const uint64_t *__restrict__ tab, const uint32_t *__restrict__ lslot, const uint64_t *__restrict__ cnt,
                      uint64_t n, uint64_t nkeys, uint64_t *__restrict__ first)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = lslot[i];
    if (!sre_lt_keeps(slot, i, tab)) return;
    const uint64_t key = cnt[slot];
    if (key < nkeys) first[key] = i;        /* (always: the ranks numbered the kept lines 0 .. nkeys - 1) */
}

/* the counts and the aggregates of the keys: the source of the values pass (sre_hip_lines_values.h), item i is key i */
struct TopVals {
    const uint64_t *__restrict__ counts;
    const sre_ls_agg_t *__restrict__ sums;
    uint64_t n;
    uint32_t v, by_col;
    int      by;
    __device__ inline int32_t classify(uint64_t k, int64_t *x) const
    {
        sre_ls_agg_t a = sre_ls_identity();
        if (by != SRE_LTT_COUNT) a = sums[k * v + by_col];
        return sre_ltt_order(by, counts[k], &a, x);
    }
};

/* lane per entry x = r * k + f of the ordered table */
__global__ __launch_bounds__(256) void
sre_k_tally_top_table(const uint32_t *__restrict__ keys, const uint64_t *__restrict__ first, const uint64_t *__restrict__ off,
                      const uint64_t *__restrict__ start, uint64_t nent, uint64_t nkeys, uint64_t n, uint32_t k,
                      uint64_t *__restrict__ cstart, uint64_t *__restrict__ cval)
{
    const uint64_t x = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (x >= nent) return;
    const uint64_t r = x / k, f = x - r * k;
    const uint64_t key = keys[r];
    const uint64_t line = key < nkeys ? first[key] : n;
    if (line >= n) {                    /* (cannot happen: an item carries the number of a key, a key has a first line) */
        cstart[x] = SRE_LG_ENTRY_UNSET | (f == 0 ? SRE_LG_ENTRY_FIRST : 0) | (f == k - 1 ? SRE_LG_ENTRY_LAST : 0);
        cval[x] = 1;
        return;
    }
    sre_ltt_entry(off, start, line * k + f, cstart + x, cval + x);
}

/* lane per rank */
__global__ __launch_bounds__(256) void
sre_k_tally_top_permute(const uint32_t *__restrict__ keys, uint64_t nkeys, const uint64_t *__restrict__ counts,
                        const sre_ls_agg_t *__restrict__ sums, uint32_t v, const uint64_t *__restrict__ first,
                        const uint64_t *__restrict__ ends, uint64_t n, const uint64_t *__restrict__ cstart,
                        const uint64_t *__restrict__ coff, uint32_t k, const int64_t *__restrict__ value,
                        const int8_t *__restrict__ cls, uint64_t *__restrict__ ocounts, uint64_t counts_rows,
                        sre_ls_agg_t *__restrict__ osums, uint64_t sums_rows, int64_t *__restrict__ index, uint64_t index_rows,
                        uint32_t *__restrict__ inv)
{
    const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (r >= nkeys) return;
    const uint64_t key = keys[r];
    if (key >= nkeys) return;           /* (cannot happen) */
    inv[key] = (uint32_t) r;
    if (r < counts_rows) ocounts[r] = counts[key];
    if (r < sums_rows) {
        for (uint32_t c = 0; c < v; c++) osums[r * v + c] = sums[key * v + c];
    }
    if (r < index_rows) {
        const uint64_t line = first[key];
        if (line >= n) return;          /* (cannot happen) */
        const uint64_t st = line_start(ends, line);
        sre_ltt_index_row(line, st, ends[line] - st, cstart, coff, r, k, key, cls[key] == SRE_LSO_NUMBER ? value[key] : 0,
                          index + r * sre_ltt_index_words(k));
    }
}

/* lane per line */
__global__ __launch_bounds__(256) void
sre_k_tally_top_ranks(const uint32_t *__restrict__ lslot, const uint64_t *__restrict__ cnt, const uint32_t *__restrict__ inv,
                      uint64_t m, uint64_t nkeys, int64_t *__restrict__ rank)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint32_t slot = lslot[i];
    int64_t        r = -1;
    if (slot != SRE_LT_NONE) {
        const uint64_t key = cnt[slot];
        if (key < nkeys) r = (int64_t) inv[key];
    }
    rank[i] = r;
}

bool
grid_of(uint64_t items, uint64_t per, uint32_t *grid)
{
    const uint64_t nblk = (items + per - 1) / per;
    if (nblk == 0 || nblk > 0x7FFFFFFFull) return false;
    *grid = (uint32_t) nblk;
    return true;
}

}  // namespace

extern "C" hipError_t
sre_launch_tally_top_first(const uint64_t *d_tab, const uint32_t *d_lslot, const uint64_t *d_cnt, uint64_t n, uint64_t nkeys,
                           uint64_t *d_first, hipStream_t stream)
{
    uint32_t grid;
    if (nkeys == 0) return hipSuccess;
    if (!grid_of(n, 256, &grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_tally_top_first, dim3(grid), dim3(256), 0, stream, d_tab, d_lslot, d_cnt, n, nkeys, d_first);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_tally_top_values(const uint64_t *d_counts, const void *d_sums, uint64_t nkeys, uint32_t v, int by, uint32_t by_col,
                            int64_t *d_value, int8_t *d_class, uint64_t *d_totals, hipStream_t stream)
{
    if (!sre_ltt_by_ok(by, by_col, v) || (by != SRE_LTT_COUNT && d_sums == NULL)) return hipErrorInvalidValue;
    const TopVals src = {d_counts, static_cast<const sre_ls_agg_t *>(d_sums), nkeys, v, by_col, by};
    return values_launch(src, d_value, d_class, d_totals, stream);
}

extern "C" hipError_t
sre_launch_tally_top_table(const uint32_t *d_keys, const uint64_t *d_first, const uint64_t *d_off, const uint64_t *d_start,
                           uint64_t nrows, uint64_t nkeys, uint64_t n, uint32_t k, uint64_t *d_cstart, uint64_t *d_cval,
                           hipStream_t stream)
{
    uint32_t grid;
    if (nrows == 0) return hipSuccess;
    if (k == 0 || k > SRE_EXTRACT_MAX_FIELDS || nrows > nkeys || !grid_of(nrows * k, 256, &grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_tally_top_table, dim3(grid), dim3(256), 0, stream, d_keys, d_first, d_off, d_start, nrows * k, nkeys, n, k,
                       d_cstart, d_cval);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_tally_top_permute(const uint32_t *d_keys, uint64_t nkeys, uint64_t nrows, const uint64_t *d_counts, const void *d_sums,
                             uint32_t v, const uint64_t *d_first, const uint64_t *d_ends, uint64_t n, const uint64_t *d_cstart,
                             const uint64_t *d_coff, uint32_t k, const int64_t *d_value, const int8_t *d_class, uint64_t *d_ocounts,
                             uint64_t counts_rows, void *d_osums, uint64_t sums_rows, int64_t *d_index, uint64_t index_rows,
                             uint32_t *d_inv, hipStream_t stream)
{
    uint32_t grid;
    if (nkeys == 0) return hipSuccess;
    if (counts_rows > nrows || sums_rows > nrows || index_rows > nrows || nrows > nkeys || (sums_rows != 0 && (v == 0 || d_sums == NULL))
        || !grid_of(nkeys, 256, &grid))
    {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(sre_k_tally_top_permute, dim3(grid), dim3(256), 0, stream, d_keys, nkeys, d_counts,
                       static_cast<const sre_ls_agg_t *>(d_sums), v, d_first, d_ends, n, d_cstart, d_coff, k, d_value, d_class,
                       d_ocounts, counts_rows, static_cast<sre_ls_agg_t *>(d_osums), sums_rows, d_index, index_rows, d_inv);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_tally_top_ranks(const uint32_t *d_lslot, const uint64_t *d_cnt, const uint32_t *d_inv, uint64_t m, uint64_t nkeys,
                           int64_t *d_rank, hipStream_t stream)
{
    uint32_t grid;
    if (m == 0) return hipSuccess;
    if (!grid_of(m, 256, &grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_tally_top_ranks, dim3(grid), dim3(256), 0, stream, d_lslot, d_cnt, d_inv, m, nkeys, d_rank);
    return hipGetLastError();
}
