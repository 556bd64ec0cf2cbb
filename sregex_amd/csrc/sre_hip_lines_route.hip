/*
 * sre_hip_lines_route.hip — the line route on the device (sregex_hip.h sre_hip_route_lines): a stable
 * multi-way partition of the lines by the bucket of the regex that matched, into a compact table the extract's gather
 * writes out.  The rules are those of sre_lines_route.h, which the CPU model compiles too.
 *
 *   select     per batch: key[i] = bucket << 56 | (len + 1) of a routed line, 0 of a dropped one, from the
 *              batch's records and the call's map;
 *   partition  after the last batch: the count and the scatter of sre_hip_lines_partition.h with the bucket as the digit and
 *              the wave rule; a line's entry of the compact table goes to its global rank;
 *   offsets    the filter's scan, over the counts and then over cval[0 .. nsel);
 *   finish     one workgroup: the cut at out_cap, the per-bucket totals, the words the host reads;
 *   gather     sre_launch_extract_gather over the compact table, unchanged (sre_hip_lines_gather.hip);
 *   index      a lane per written rank.
 *
 * No workgroup waits for another.  Plain C++ and vector memory operations only.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"
#include "sre_lines_route.h"
#include "sre_hip_lines_block.h"
#include "sre_hip_lines_partition.h"

namespace {

/* lane per line of the batch (lines i0 .. info->i1) */
__global__ __launch_bounds__(256) void
sre_k_route_select(const int64_t *__restrict__ records, uint32_t slots, uint64_t i0, uint32_t nreg,
                   const int32_t *__restrict__ map, const uint64_t *__restrict__ ends, const sre_lines_info_t *__restrict__ info,
                   uint64_t *__restrict__ key)
{
    const uint64_t nb = info->i1 - i0;
    const uint64_t j = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (j >= nb) return;
    const int32_t  b = sre_lr_bucket(records[j * slots], SRE_DECLINED, nreg, map);
    const uint64_t i = i0 + j;
    key[i] = sre_lr_key(b, ends[i] - line_start(ends, i));
}

/* the route's partition pass (sre_hip_lines_partition.h): an item is the key of a line, its digit the bucket, taken only with
 * a bucket the call has (the select pass writes no other); the wave rule ranks it, one ballot per distinct bucket of a slot */
struct RoutePass {
    static constexpr uint32_t MAX_DIGITS = SRE_LR_MAX_BUCKETS;
    static constexpr int      RULE = SRE_LRK_RANK_TURNS;
    const uint64_t *__restrict__ key;
    const uint64_t *__restrict__ ends;
    uint64_t n;
    uint32_t nb;
    uint64_t *__restrict__ cstart;
    uint64_t *__restrict__ cval;
    uint64_t *__restrict__ cmeta;
    __device__ uint32_t nd() const { return nb; }
    __device__ uint32_t bits() const { return 0; }      /* (the wave rule does not look at it) */
    __device__ uint64_t load(uint64_t i) const { return i < n ? key[i] : 0; }
    __device__ bool     taken(uint64_t k) const { return sre_lr_key_selected(k) && sre_lr_key_bucket(k) < nb; }
    __device__ uint32_t digit(uint64_t k) const { return sre_lr_key_bucket(k); }
    /* the line's entry of the compact table */
    __device__ void store(uint64_t r, uint64_t k, uint64_t i) const
    {
        const uint64_t v = sre_lr_key_val(k);
        cstart[r] = sre_lr_entry_start(ends[i] - (v - 1));
        cval[r] = v;
        cmeta[r] = sre_lr_entry_meta(sre_lr_key_bucket(k), i);
    }
};

/* one workgroup: res[0 .. 4) = selected lines, bytes they take, rows that fit out_cap whole, bytes of those; then
 * per bucket [lines, bytes].  coff is not read when nsel == 0 */
__global__ __launch_bounds__(SRE_LR_MAX_BUCKETS) void
sre_k_route_finish(const uint64_t *__restrict__ first, uint64_t nwg, uint32_t nb, const uint64_t *__restrict__ coff, uint64_t nsel,
                   uint64_t out_cap, uint64_t *__restrict__ res)
{
    if (threadIdx.x == 0) sre_lr_result(coff, nsel, out_cap, res);
    if (threadIdx.x < nb) {
        uint64_t lines = 0, bytes = 0;
        if (nsel) sre_lr_bucket_totals(first, nwg, threadIdx.x, coff, &lines, &bytes);
        res[SRE_LR_RES_WORDS + 2 * threadIdx.x] = lines;
        res[SRE_LR_RES_WORDS + 2 * threadIdx.x + 1] = bytes;
    }
}

/* rows [line, start, len, output offset, bucket] of the first min(index_cap, written) ranks */
__global__ __launch_bounds__(256) void
sre_k_route_index(const uint64_t *__restrict__ coff, const uint64_t *__restrict__ cstart, const uint64_t *__restrict__ cmeta,
                  const uint64_t *__restrict__ res, uint64_t index_cap, int64_t *__restrict__ rows)
{
    const uint64_t written = res[SRE_LR_RES_WRITTEN];
    const uint64_t limit = index_cap < written ? index_cap : written;
    const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (r >= limit) return;
    const uint64_t m = cmeta[r], o = coff[r];
    int64_t       *row = rows + r * 5;
    row[0] = (int64_t) sre_lr_meta_line(m);
    row[1] = (int64_t) (cstart[r] & SRE_LG_ENTRY_START);
    row[2] = (int64_t) (coff[r + 1] - o - 1);
    row[3] = (int64_t) o;
    row[4] = (int64_t) sre_lr_meta_bucket(m);
}

}  // namespace

extern "C" hipError_t
sre_launch_route_select(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0, uint32_t nreg, const int32_t *d_map,
                        const uint64_t *d_ends, const sre_lines_info_t *d_info, uint64_t *d_key, hipStream_t stream)
{
    if (nmax == 0) return hipSuccess;
    hipLaunchKernelGGL(sre_k_route_select, dim3((uint32_t) ((nmax + 255) / 256)), dim3(256), 0, stream, d_records, slots, i0, nreg,
                       d_map, d_ends, d_info, d_key);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_route_count(const uint64_t *d_key, uint64_t n, uint32_t nbuckets, uint64_t *d_cnt, hipStream_t stream)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || nbuckets == 0 || nbuckets > SRE_LR_MAX_BUCKETS || nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const RoutePass p = {d_key, NULL, n, nbuckets, NULL, NULL, NULL};
    hipLaunchKernelGGL(sre_k_partition_count<RoutePass>, dim3((uint32_t) nwg), dim3(SRE_LR_THREADS), 0, stream, p, nwg, d_cnt);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_route_scatter(const uint64_t *d_key, const uint64_t *d_ends, uint64_t n, uint32_t nbuckets, const uint64_t *d_first,
                         uint64_t nsel, uint64_t *d_cstart, uint64_t *d_cval, uint64_t *d_cmeta, hipStream_t stream)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || nbuckets == 0 || nbuckets > SRE_LR_MAX_BUCKETS || nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (nsel == 0) return hipSuccess;
    const RoutePass p = {d_key, d_ends, n, nbuckets, d_cstart, d_cval, d_cmeta};
    hipLaunchKernelGGL(sre_k_partition_scatter<RoutePass>, dim3((uint32_t) nwg), dim3(SRE_LR_THREADS), 0, stream, p, nwg, d_first,
                       nsel);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_route_finish(const uint64_t *d_first, uint64_t n, uint32_t nbuckets, const uint64_t *d_coff, uint64_t nsel,
                        uint64_t out_cap, uint64_t *d_res, hipStream_t stream)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || nbuckets == 0 || nbuckets > SRE_LR_MAX_BUCKETS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_route_finish, dim3(1), dim3(SRE_LR_MAX_BUCKETS), 0, stream, d_first, nwg, nbuckets, d_coff, nsel,
                       out_cap, d_res);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_route_index(const uint64_t *d_coff, const uint64_t *d_cstart, const uint64_t *d_cmeta, const uint64_t *d_res,
                       uint64_t nrows, uint64_t index_cap, int64_t *d_index, hipStream_t stream)
{
    if (nrows == 0 || index_cap == 0) return hipSuccess;
    const uint64_t nblk = (nrows + 255) / 256;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_route_index, dim3((uint32_t) nblk), dim3(256), 0, stream, d_coff, d_cstart, d_cmeta, d_res, index_cap,
                       d_index);
    return hipGetLastError();
}
