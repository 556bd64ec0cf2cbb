/*
 * sre_hip_lines_route.hip — the line route on the device (sregex_hip.h sre_hip_route_lines): a stable
 * multi-way partition of the lines by the bucket of the regex that matched, into a compact table the extract's gather
 * writes out.  The rules are those of sre_lines_route.h, which the CPU model compiles too.
 *
 *   select     per batch: key[i] = bucket << 56 | (len + 1) of a routed line, 0 of a dropped one, from the
 *              batch's records and the call's map;
 *   count      after the last batch: a workgroup takes 1024 lines and writes how many fall in each bucket to
 *              cnt[b * nwg + w]; the filter's scan (sre_launch_filter_offsets) over those words gives every (bucket,
 *              workgroup) the rank of its first line;
 *   scatter    the same workgroups recompute the rank of every line among the lines of its bucket (the wave rule:
 *              one ballot per distinct bucket present in a wave) and write the line's entry of the compact table
 *              at its global rank;
 *   offsets    the filter's scan again, over cval[0 .. nsel);
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

/* the wave rule over one slot: the lane's rank among the lanes of the slot with its bucket; the lowest lane of every
 * bucket present leaves the slot's count of it in c[bucket].  Every lane of the wave calls it */
__device__ inline uint32_t
wave_rank(bool sel, uint32_t bucket, uint32_t lane, uint32_t *c)
{
    uint32_t rank = 0;
    uint64_t rem = __ballot(sel);
    while (rem) {
        const uint32_t lead = sre_lr_leader(rem);
        const uint32_t kb = (uint32_t) __shfl((int) bucket, (int) lead, 64);
        const uint64_t m = __ballot(sel && bucket == kb);
        if (sel && bucket == kb) rank = sre_lr_rank_in(m, lane);
        if (lane == lead) c[kb] = sre_lr_popc(m);
        rem &= ~m;
    }
    return rank;
}

/* a line's key as the passes take it: selected only with a bucket the call has (the select pass writes no other) */
__device__ inline bool
key_take(uint64_t k, uint32_t nb, uint32_t *bucket)
{
    *bucket = sre_lr_key_bucket(k);
    return sre_lr_key_selected(k) && *bucket < nb;
}

/* workgroup w: cnt[b * nwg + w] = its lines of bucket b */
__global__ __launch_bounds__(SRE_LR_THREADS) void
sre_k_route_count(const uint64_t *__restrict__ key, uint64_t n, uint32_t nb, uint64_t nwg, uint64_t *__restrict__ cnt)
{
    __shared__ uint32_t c[SRE_LR_SLOTS * SRE_LR_MAX_BUCKETS];
    const uint32_t      lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t x = threadIdx.x; x < SRE_LR_SLOTS * nb; x += SRE_LR_THREADS) c[x] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
        const uint32_t slot = sre_lr_slot(wave, q);
        const uint64_t i = sre_lr_line(blockIdx.x, slot, lane);
        const uint64_t k = i < n ? key[i] : 0;
        uint32_t       b;
        const bool     sel = key_take(k, nb, &b);
        (void) wave_rank(sel, b, lane, c + slot * nb);
    }
    __syncthreads();
    if (threadIdx.x < nb) cnt[sre_lr_cnt_index(threadIdx.x, nwg, blockIdx.x)] = sre_lr_slot_prefix(c + threadIdx.x, nb);
}

/* the same workgroups over the scanned counts `first`: every selected line writes its entry at its global rank */
__global__ __launch_bounds__(SRE_LR_THREADS) void
sre_k_route_scatter(const uint64_t *__restrict__ key, const uint64_t *__restrict__ ends, uint64_t n, uint32_t nb, uint64_t nwg,
                    const uint64_t *__restrict__ first, uint64_t nsel, uint64_t *__restrict__ cstart, uint64_t *__restrict__ cval,
                    uint64_t *__restrict__ cmeta)
{
    __shared__ uint32_t c[SRE_LR_SLOTS * SRE_LR_MAX_BUCKETS];
    __shared__ uint64_t gbase[SRE_LR_MAX_BUCKETS];
    const uint32_t      lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t            k[SRE_LR_ROUNDS];
    uint32_t            rk[SRE_LR_ROUNDS];
    for (uint32_t x = threadIdx.x; x < SRE_LR_SLOTS * nb; x += SRE_LR_THREADS) c[x] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
        const uint32_t slot = sre_lr_slot(wave, q);
        const uint64_t i = sre_lr_line(blockIdx.x, slot, lane);
        k[q] = i < n ? key[i] : 0;
        uint32_t   b;
        const bool sel = key_take(k[q], nb, &b);
        rk[q] = wave_rank(sel, b, lane, c + slot * nb);
    }
    __syncthreads();
    if (threadIdx.x < nb) {
        (void) sre_lr_slot_prefix(c + threadIdx.x, nb);
        gbase[threadIdx.x] = first[sre_lr_cnt_index(threadIdx.x, nwg, blockIdx.x)];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
        uint32_t b;
        if (!key_take(k[q], nb, &b)) continue;
        const uint32_t slot = sre_lr_slot(wave, q);
        const uint64_t i = sre_lr_line(blockIdx.x, slot, lane);
        const uint64_t r = gbase[b] + c[slot * nb + b] + rk[q];
        if (r >= nsel) continue;        /* (cannot happen: the ranks are a permutation of 0 .. nsel - 1) */
        const uint64_t v = sre_lr_key_val(k[q]);
        cstart[r] = sre_lr_entry_start(ends[i] - (v - 1));
        cval[r] = v;
        cmeta[r] = sre_lr_entry_meta(b, i);
    }
}

/* one workgroup: res[0 .. 4) = selected lines, bytes they take, rows that fit out_cap whole, bytes of those; then
 * per bucket [lines, bytes].  coff is not read when nsel == 0 */
__global__ __launch_bounds__(SRE_LR_MAX_BUCKETS) void
sre_k_route_finish(const uint64_t *__restrict__ first, uint64_t nwg, uint32_t nb, const uint64_t *__restrict__ coff, uint64_t nsel,
                   uint64_t out_cap, uint64_t *__restrict__ res)
{
    if (threadIdx.x == 0) {
        const uint64_t cut = nsel ? sre_lr_cut(coff, nsel, out_cap) : 0;
        res[SRE_LR_RES_NSEL] = nsel;
        res[SRE_LR_RES_NEED] = nsel ? coff[nsel] : 0;
        res[SRE_LR_RES_WRITTEN] = cut;
        res[SRE_LR_RES_BYTES] = nsel ? coff[cut] : 0;
    }
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
    hipLaunchKernelGGL(sre_k_route_count, dim3((uint32_t) nwg), dim3(SRE_LR_THREADS), 0, stream, d_key, n, nbuckets, nwg, d_cnt);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_route_scatter(const uint64_t *d_key, const uint64_t *d_ends, uint64_t n, uint32_t nbuckets, const uint64_t *d_first,
                         uint64_t nsel, uint64_t *d_cstart, uint64_t *d_cval, uint64_t *d_cmeta, hipStream_t stream)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || nbuckets == 0 || nbuckets > SRE_LR_MAX_BUCKETS || nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (nsel == 0) return hipSuccess;
    hipLaunchKernelGGL(sre_k_route_scatter, dim3((uint32_t) nwg), dim3(SRE_LR_THREADS), 0, stream, d_key, d_ends, n, nbuckets, nwg,
                       d_first, nsel, d_cstart, d_cval, d_cmeta);
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
