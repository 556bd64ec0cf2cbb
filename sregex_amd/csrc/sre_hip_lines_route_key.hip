/*
 * sre_hip_lines_route_key.hip — the line route by key on the device (sregex_hip.h sre_hip_route_lines_by_key, DESIGN.md
 * §4.11.11): a stable partition of the lines by the dictionary row of their key, an LSD radix sort of (sort key, line)
 * items, into a compact table the extract's gather writes out.  The rules are those of sre_lines_route_key.h and
 * sre_lines_route.h, which the CPU model compiles too.
 *
 *   partition  per digit: the count and the scatter of sre_hip_lines_partition.h over one-word items, the filter's scan between
 *              them.  Pass 0 makes the items from the key ids in line order and drops the unselected;
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
#include "sre_hip_lines_partition.h"

namespace {

/* a digit pass (sre_hip_lines_partition.h): pass 0 (FIRST) makes item i from the key id of line i, a later pass reads it;
 * every item goes to its rank of dst */
template <bool FIRST, int RANK_RULE>
struct KeyPass {
    static constexpr uint32_t MAX_DIGITS = 1u << SRE_LRK_MAX_BITS;
    static constexpr int      RULE = RANK_RULE;
    const int64_t *__restrict__ keyid;
    const uint64_t *__restrict__ src;
    uint64_t n, rows;
    int      all;
    uint32_t pass, width;
    uint64_t *__restrict__ dst;
    __device__ uint32_t nd() const { return 1u << width; }
    __device__ uint32_t bits() const { return width; }
    __device__ uint64_t load(uint64_t i) const
    {
        if (i >= n) return SRE_LRK_DROPPED;
        return FIRST ? sre_lrk_first_item(keyid[i], i, rows, all) : src[i];
    }
    __device__ bool     taken(uint64_t it) const { return it != SRE_LRK_DROPPED; }
    __device__ uint32_t digit(uint64_t it) const { return sre_lrk_digit(it, pass, width); }
    __device__ void     store(uint64_t r, uint64_t it, uint64_t) const { dst[r] = it; }
};

/* a lane per rank of the sorted items: its entry of the compact table, and head[r] = 1 for the first rank of a bucket */
__global__ __launch_bounds__(256) void
sre_k_route_key_table(const uint64_t *__restrict__ items, const uint64_t *__restrict__ ends, uint64_t nsel, uint64_t nlines,
                      uint64_t *__restrict__ cstart, uint64_t *__restrict__ cval, uint64_t *__restrict__ head)
{
    const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (r >= nsel) return;
    const uint64_t i = sre_lrk_item_line(items[r]);
    head[r] = sre_lrk_is_head(items, r) ? 1 : 0;
    compact_entry(ends, i, nlines, r, cstart, cval);
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
    sre_lr_result(coff, nsel, out_cap, res);
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

/* the count or the scatter of one pass */
template <bool FIRST, int RULE>
hipError_t
launch_pass(bool scatter, const int64_t *d_keyid, const uint64_t *d_src, uint64_t n, uint64_t rows, int all, uint32_t pass, uint32_t bits,
            uint64_t *d_cnt, const uint64_t *d_first, uint64_t total, uint64_t *d_dst, hipStream_t stream)
{
    typedef KeyPass<FIRST, RULE> Pass;
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || bits < 1 || bits > SRE_LRK_MAX_BITS || pass * bits >= SRE_LRK_LINE_BITS || nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t) nwg), block(SRE_LR_THREADS);
    const Pass p = {d_keyid, d_src, n, rows, all, pass, bits, d_dst};
    if (!scatter) {
        hipLaunchKernelGGL(sre_k_partition_count<Pass>, grid, block, 0, stream, p, nwg, d_cnt);
    } else {
        if (total == 0) return hipSuccess;
        hipLaunchKernelGGL(sre_k_partition_scatter<Pass>, grid, block, 0, stream, p, nwg, d_first, total);
    }
    return hipGetLastError();
}

/* ... with the pass type the arguments name: pass 0 over the key ids when d_keyid != NULL, and the rank rule */
hipError_t
launch_pass(bool scatter, int rule, const int64_t *d_keyid, const uint64_t *d_src, uint64_t n, uint64_t rows, int all, uint32_t pass,
            uint32_t bits, uint64_t *d_cnt, const uint64_t *d_first, uint64_t total, uint64_t *d_dst, hipStream_t stream)
{
    const bool turns = rule == SRE_LRK_RANK_TURNS;
    if (d_keyid) {
        return (turns ? launch_pass<true, SRE_LRK_RANK_TURNS> : launch_pass<true, SRE_LRK_RANK_BITS>)(
            scatter, d_keyid, NULL, n, rows, all, 0, bits, d_cnt, d_first, total, d_dst, stream);
    }
    return (turns ? launch_pass<false, SRE_LRK_RANK_TURNS> : launch_pass<false, SRE_LRK_RANK_BITS>)(
        scatter, NULL, d_src, n, rows, all, pass, bits, d_cnt, d_first, total, d_dst, stream);
}

}  // namespace

extern "C" hipError_t
sre_launch_route_key_count(const int64_t *d_keyid, const uint64_t *d_src, uint64_t n, uint64_t rows, int all, uint32_t pass,
                           uint32_t bits, int rule, uint64_t *d_cnt, hipStream_t stream)
{
    return launch_pass(false, rule, d_keyid, d_src, n, rows, all, pass, bits, d_cnt, NULL, 0, NULL, stream);
}

extern "C" hipError_t
sre_launch_route_key_scatter(const int64_t *d_keyid, const uint64_t *d_src, uint64_t n, uint64_t rows, int all, uint32_t pass,
                             uint32_t bits, int rule, const uint64_t *d_first, uint64_t total, uint64_t *d_dst, hipStream_t stream)
{
    return launch_pass(true, rule, d_keyid, d_src, n, rows, all, pass, bits, NULL, d_first, total, d_dst, stream);
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
