/*
 * sre_hip_lines_sort.hip — the line sort on the device (sregex_hip.h sre_hip_sort_lines): the lines of a
 * buffer ordered by the number in a capture group, an LSD radix sort of (key, line) items into a compact table the
 * extract's gather writes out.  The rules are those of sre_lines_sort.h, sre_lines_route_key.h and sre_lines_route.h, which
 * the CPU model compiles too.
 *
 *   values     the values pass of sre_hip_lines_values.h, a lane per line: the class and the value of the line from its entry
 *              of the value table, and the four totals of the call;
 *   partition  per digit: the count and the scatter of sre_hip_lines_partition.h, the filter's scan between them; key and line
 *              of an item go to the same rank of the other pair of arrays.  Pass 0 makes the items from the values in line
 *              order and drops the unselected;
 *   table      a lane per rank in front of the limit: the entry of the compact table;
 *   finish     one lane: the cut at out_cap and the words the host reads;
 *   gather     sre_launch_extract_gather over the compact table, unchanged (sre_hip_lines_gather.hip);
 *   index      a lane per written rank.
 *
 * No workgroup waits for another and no rank comes from an atomic.  Plain C++ and vector memory operations only.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"
#include "sre_lines_sort.h"
#include "sre_hip_lines_partition.h"
#include "sre_hip_lines_values.h"

namespace {

/* the value table of the one sort group as the values pass reads it (written by earlier kernels or copies: plain loads): the
 * source of the values pass (sre_hip_lines_values.h), item i is line i */
struct SortVals {
    const uint8_t *__restrict__ buf;
    const uint64_t *__restrict__ vval, *__restrict__ vstart;
    uint64_t n;
    __device__ inline uint64_t val(uint64_t line, uint32_t) const { return vval[line]; }
    __device__ inline uint64_t raw(uint64_t line, uint32_t) const { return vstart[line]; }
    __device__ inline uint8_t  byte(uint64_t at) const { return buf[at]; }
    __device__ inline int32_t  classify(uint64_t i, int64_t *v) const { return sre_lso_line(*this, i, v); }
};

/* what every digit pass knows of the call */
struct SortKeys {
    int64_t  vmin, vmax;
    uint64_t range;
    int      desc, all;
};

/* a digit pass (sre_hip_lines_partition.h) over the keys, 8-bit digits and the ballots per digit bit: pass 0 (FIRST) makes key i
 * from the value and the class of line i, a later pass reads it; key and line of every item go to its rank of dkey / dline.
 * Pass 0: the line of item i is i; a later pass reads it from sline */
template <bool FIRST>
struct SortPass {
    static constexpr uint32_t MAX_DIGITS = 1u << SRE_LSO_DIGIT_BITS;
    static constexpr int      RULE = SRE_LRK_RANK_BITS;
    const int64_t *__restrict__ value;
    const int8_t *__restrict__ cls;
    const uint64_t *__restrict__ src;
    const uint32_t *__restrict__ sline;
    uint64_t n;
    SortKeys k;
    uint32_t pass;
    uint64_t *__restrict__ dkey;
    uint32_t *__restrict__ dline;
    __device__ uint32_t nd() const { return MAX_DIGITS; }
    __device__ uint32_t bits() const { return SRE_LSO_DIGIT_BITS; }
    __device__ uint64_t load(uint64_t i) const
    {
        if (i >= n) return SRE_LSO_DROPPED;
        return FIRST ? sre_lso_key(cls[i], value[i], k.vmin, k.vmax, k.range, k.desc, k.all) : src[i];
    }
    __device__ bool     taken(uint64_t key) const { return key != SRE_LSO_DROPPED; }
    __device__ uint32_t digit(uint64_t key) const { return sre_lso_digit(key, pass); }
    __device__ void     store(uint64_t r, uint64_t key, uint64_t i) const
    {
        dkey[r] = key;
        dline[r] = FIRST ? (uint32_t) i : sline[i];
    }
};

/* a lane per rank in front of nout: its entry of the compact table */
__global__ __launch_bounds__(256) void
sre_k_sort_table(const uint32_t *__restrict__ lines, const uint64_t *__restrict__ ends, uint64_t nout, uint64_t nlines,
                 uint64_t *__restrict__ cstart, uint64_t *__restrict__ cval)
{
    const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (r >= nout) return;
    compact_entry(ends, lines[r], nlines, r, cstart, cval);
}

/* one lane: the cut and the words the host reads.  coff is not read when nout == 0 */
__global__ __launch_bounds__(64) void
sre_k_sort_finish(const uint64_t *__restrict__ coff, uint64_t nout, uint64_t out_cap, uint64_t *__restrict__ res)
{
    if (threadIdx.x != 0) return;
    sre_lr_result(coff, nout, out_cap, res);
}

/* rows [line, start, len, output offset, value, class] of the first min(index_cap, written) ranks */
__global__ __launch_bounds__(256) void
sre_k_sort_index(const uint32_t *__restrict__ lines, const uint64_t *__restrict__ cstart, const uint64_t *__restrict__ coff,
                 const uint64_t *__restrict__ res, const int64_t *__restrict__ value, const int8_t *__restrict__ cls, uint64_t nlines,
                 uint64_t index_cap, int64_t *__restrict__ out)
{
    const uint64_t written = res[SRE_LSO_RES_WRITTEN];
    const uint64_t limit = index_cap < written ? index_cap : written;
    const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (r >= limit) return;
    const uint64_t i = lines[r];
    if (i >= nlines) return;            /* (cannot happen) */
    sre_lso_index_row(i, cstart, coff, r, value[i], cls[i], out + r * SRE_LSO_INDEX_WORDS);
}

SortKeys
sort_keys(int64_t vmin, int64_t vmax, uint64_t nnumbered, int desc, int all)
{
    SortKeys k;
    k.vmin = vmin;
    k.vmax = vmax;
    k.range = sre_lso_range(nnumbered, vmin, vmax);
    k.desc = desc;
    k.all = all;
    return k;
}

}  // namespace

extern "C" hipError_t
sre_launch_sort_values(const void *d_buf, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n, int64_t *d_value,
                       int8_t *d_class, uint64_t *d_totals, hipStream_t stream)
{
    if (n == 0) return hipErrorInvalidValue;
    const SortVals src = {static_cast<const uint8_t *>(d_buf), d_vval, d_vstart, n};
    return values_launch(src, d_value, d_class, d_totals, stream);
}

extern "C" hipError_t
sre_launch_sort_count(const int64_t *d_value, const int8_t *d_class, const uint64_t *d_src, uint64_t n, int64_t vmin, int64_t vmax,
                      uint64_t nnumbered, int desc, int all, uint32_t pass, uint64_t *d_cnt, hipStream_t stream)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || pass >= SRE_LSO_MAX_PASSES || nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const SortKeys k = sort_keys(vmin, vmax, nnumbered, desc, all);
    const dim3     grid((uint32_t) nwg), block(SRE_LR_THREADS);
    if (d_value) {
        if (pass != 0 || d_class == NULL) return hipErrorInvalidValue;
        const SortPass<true> p = {d_value, d_class, NULL, NULL, n, k, 0u, NULL, NULL};
        hipLaunchKernelGGL(sre_k_partition_count<SortPass<true>>, grid, block, 0, stream, p, nwg, d_cnt);
    } else {
        const SortPass<false> p = {NULL, NULL, d_src, NULL, n, k, pass, NULL, NULL};
        hipLaunchKernelGGL(sre_k_partition_count<SortPass<false>>, grid, block, 0, stream, p, nwg, d_cnt);
    }
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_sort_scatter(const int64_t *d_value, const int8_t *d_class, const uint64_t *d_src, const uint32_t *d_sline, uint64_t n,
                        int64_t vmin, int64_t vmax, uint64_t nnumbered, int desc, int all, uint32_t pass, const uint64_t *d_first,
                        uint64_t total, uint64_t *d_dkey, uint32_t *d_dline, hipStream_t stream)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || n > SRE_LRK_MAX_LINES || pass >= SRE_LSO_MAX_PASSES || nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (total == 0) return hipSuccess;
    const SortKeys k = sort_keys(vmin, vmax, nnumbered, desc, all);
    const dim3     grid((uint32_t) nwg), block(SRE_LR_THREADS);
    if (d_value) {
        if (pass != 0 || d_class == NULL) return hipErrorInvalidValue;
        const SortPass<true> p = {d_value, d_class, NULL, NULL, n, k, 0u, d_dkey, d_dline};
        hipLaunchKernelGGL(sre_k_partition_scatter<SortPass<true>>, grid, block, 0, stream, p, nwg, d_first, total);
    } else {
        if (total != n) return hipErrorInvalidValue;       /* (a later pass moves every item) */
        const SortPass<false> p = {NULL, NULL, d_src, d_sline, n, k, pass, d_dkey, d_dline};
        hipLaunchKernelGGL(sre_k_partition_scatter<SortPass<false>>, grid, block, 0, stream, p, nwg, d_first, total);
    }
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_sort_table(const uint32_t *d_lines, const uint64_t *d_ends, uint64_t nout, uint64_t nlines, uint64_t *d_cstart,
                      uint64_t *d_cval, hipStream_t stream)
{
    if (nout == 0) return hipSuccess;
    const uint64_t nblk = (nout + 255) / 256;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_sort_table, dim3((uint32_t) nblk), dim3(256), 0, stream, d_lines, d_ends, nout, nlines, d_cstart, d_cval);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_sort_finish(const uint64_t *d_coff, uint64_t nout, uint64_t out_cap, uint64_t *d_res, hipStream_t stream)
{
    hipLaunchKernelGGL(sre_k_sort_finish, dim3(1), dim3(64), 0, stream, d_coff, nout, out_cap, d_res);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_sort_index(const uint32_t *d_lines, const uint64_t *d_cstart, const uint64_t *d_coff, const uint64_t *d_res,
                      const int64_t *d_value, const int8_t *d_class, uint64_t nlines, uint64_t nrows, uint64_t index_cap,
                      int64_t *d_index, hipStream_t stream)
{
    if (nrows == 0 || index_cap == 0) return hipSuccess;
    const uint64_t nblk = (nrows + 255) / 256;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_sort_index, dim3((uint32_t) nblk), dim3(256), 0, stream, d_lines, d_cstart, d_coff, d_res, d_value, d_class,
                       nlines, index_cap, d_index);
    return hipGetLastError();
}
