/*
 * sre_hip_streams.hip — stream sets (sre_hip_streams_*): the kernels around the
 * scan of one call that feeds a chunk to each of many device-resident streams.
 *
 *   sre_k_streams_reset      fresh contexts for the listed rows
 *   sre_k_streams_prologue   which streams take part (fed and not closed), the segment geometry
 *                            the scan kernels read, and the state each stream is entered with
 * The tail (sre_k_streams_tail) is in sre_hip_scan.hip: it shares the single-stream tail's device
 * function, the lineage walker and the staged tables.
 */
#include <hip/hip_runtime.h>
#include "sre_hip_streams.h"

namespace {

__global__ __launch_bounds__(256) void
sre_k_streams_reset(int64_t *__restrict__ rows, uint32_t row_words, const uint64_t *__restrict__ idx, uint64_t n)
{
    const uint64_t total = n * row_words;
    for (uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x; t < total; t += (uint64_t) gridDim.x * 256u) {
        const uint64_t r = t / row_words, w = t % row_words;
        rows[(idx != nullptr ? idx[r] : r) * row_words + w] = 0;
    }
}

#define SRE_STREAMS_PRO_THREADS 1024u

/* sum of v over the workgroup, in every thread (sh: SRE_STREAMS_PRO_THREADS words) */
__device__ inline uint64_t
block_sum(uint64_t v, uint64_t *sh)
{
    const uint32_t tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (uint32_t d = SRE_STREAMS_PRO_THREADS / 2; d >= 1; d >>= 1) {
        if (tid < d) sh[tid] += sh[tid + d];
        __syncthreads();
    }
    return sh[0];
}

/* One workgroup; thread t owns the streams [t * per, (t + 1) * per): the prefix of the segment
 * counts is a scan over the threads' sums, and nothing here grows a launch with the set. */
__global__ __launch_bounds__(SRE_STREAMS_PRO_THREADS) void
sre_k_streams_prologue(const sre_streams_feed_t *__restrict__ feed, uint32_t n, const int64_t *__restrict__ rows,
                       sre_streams_layout_t L, const uint8_t *__restrict__ rekind, uint32_t init0, uint64_t seg_fixed,
                       uint64_t resident, uint64_t seg_cap, const uint8_t **__restrict__ ptrs, uint64_t *__restrict__ lens,
                       uint64_t *__restrict__ seg_first, uint32_t *__restrict__ sentry, int64_t *__restrict__ recs,
                       sre_streams_info_t *__restrict__ info)
{
    __shared__ uint64_t sh[SRE_STREAMS_PRO_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + SRE_STREAMS_PRO_THREADS - 1) / SRE_STREAMS_PRO_THREADS;
    const uint32_t i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    auto active = [&](uint32_t i) {
        return (feed[i].flags & SRE_SFEED_FED) != 0
               && ((uint64_t) rows[(size_t) i * L.row_words + SRE_SROW_FLAGS] & SRE_SFL_CLOSED) == 0;
    };
    uint64_t bytes = 0, nact = 0;
    for (uint32_t i = i0; i < i1; i++) {
        if (active(i)) {
            bytes += feed[i].len;
            nact++;
        }
    }
    bytes = block_sum(bytes, sh);
    nact = block_sum(nact, sh);
    const uint64_t seg = seg_fixed ? seg_fixed : sre_scan_auto_segment(bytes, resident, seg_cap);
    uint64_t       mine = 0;
    for (uint32_t i = i0; i < i1; i++) {
        if (active(i)) {
            const uint64_t k = (feed[i].len + seg - 1) / seg;
            mine += k ? k : 1;                  /* an empty chunk is still a call */
        }
    }
    /* exclusive prefix of the threads' counts */
    __syncthreads();
    sh[tid] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < SRE_STREAMS_PRO_THREADS; d <<= 1) {
        const uint64_t v = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    uint64_t       run = sh[tid] - mine;
    const uint64_t nsegs = sh[SRE_STREAMS_PRO_THREADS - 1];
    for (uint32_t i = i0; i < i1; i++) {
        const sre_streams_feed_t f = feed[i];
        const int64_t           *row = rows + (size_t) i * L.row_words;
        const uint64_t           fl = (uint64_t) row[SRE_SROW_FLAGS];
        const bool               fed = (f.flags & SRE_SFEED_FED) != 0, closed = (fl & SRE_SFL_CLOSED) != 0;
        const bool               act = fed && !closed;
        uint32_t                 e = 0;
        seg_first[i] = run;
        ptrs[i] = reinterpret_cast<const uint8_t *>(f.ptr);
        lens[i] = act ? f.len : 0;
        if (act) {
            const uint64_t k = (f.len + seg - 1) / seg;
            run += k ? k : 1;
            if (fl & SRE_SFL_STARTED) {
                /* the carried state as the chunk boundary leaves it: a look-ahead thread at the
                 * chunk's first byte goes by the context's flags (sre_dfa.h `rekind`) */
                const uint32_t st = (uint32_t) ((uint64_t) row[SRE_SROW_STATE] & 0xffffffffu);
                const uint32_t kind = (fl & SRE_SFL_NEWLINE) ? 1u : (fl & SRE_SFL_WORD) ? 2u : 0u;
                e = (rekind != nullptr ? (uint32_t) rekind[4 * (size_t) st + kind] : st) | SRE_SENTRY_CONTINUES;
            } else {
                e = init0;
            }
            if (!(f.flags & SRE_SFEED_EOF)) e |= SRE_SENTRY_NO_EOF;
        }
        sentry[i] = e;
        recs[(size_t) i * L.rec_slots + 1] = !fed ? SRE_SSTATE_NOT_FED : closed ? SRE_SSTATE_WAS_CLOSED : SRE_SSTATE_OPEN;
    }
    if (tid == 0) {
        seg_first[n] = nsegs;
        info->seg = seg;
        info->nsegs = nsegs;
        info->nactive = nact;
        info->bytes = bytes;
        info->unsettled = 0;
    }
}

}  // namespace

extern "C" hipError_t
sre_launch_streams_reset(int64_t *d_rows, uint32_t row_words, const uint64_t *d_idx, uint64_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t total = n * row_words;
    const uint32_t grid = (uint32_t) ((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(sre_k_streams_reset, dim3(grid), dim3(256), 0, stream, d_rows, row_words, d_idx, n);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_streams_prologue(const sre_streams_feed_t *d_feed, uint32_t n, const int64_t *d_rows,
                            sre_streams_layout_t layout, const uint8_t *d_rekind, uint32_t init0, uint64_t seg_fixed,
                            uint64_t resident, uint64_t seg_cap, const uint8_t **d_ptrs, uint64_t *d_lens,
                            uint64_t *d_seg_first, uint32_t *d_sentry, int64_t *d_recs, sre_streams_info_t *d_info,
                            hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sre_k_streams_prologue, dim3(1), dim3(SRE_STREAMS_PRO_THREADS), 0, stream, d_feed, n, d_rows, layout,
                       d_rekind, init0, seg_fixed, resident, seg_cap, d_ptrs, d_lens, d_seg_first, d_sentry, d_recs, d_info);
    return hipGetLastError();
}
