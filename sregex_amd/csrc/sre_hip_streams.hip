/*
 * sre_hip_streams.hip — stream sets (sre_hip_streams_*): the kernels around the
 * scan of one call that feeds a chunk to each of many device-resident streams.
 *
 *   sre_k_streams_reset      fresh contexts for the listed rows
 *   sre_k_streams_prologue   which streams take part (fed and not closed), the segment geometry
 *                            the scan kernels read, and the state each stream is entered with
 *   sre_k_streams_nfa_*      the same around the set kernels of the bit-parallel NFA tier: prologue
 *                            (entry SETS), the chain check's status words as a fix-up round's
 *                            work list, and the tail (sre_streams_nfa.h: the rule of one call)
 * The tail (sre_k_streams_tail) is in sre_hip_scan.hip: it shares the single-stream tail's device
 * function, the lineage walker and the staged tables.
 */
#include <hip/hip_runtime.h>
#include "sre_hip_streams.h"
#include "sre_streams_nfa.h"

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

/* ===================================================================== the NFA tier */

/* the whole record of a stream: [rc, state, 0, -1, -1, ovector all -1] (Thompson) */
__device__ inline void
snfa_record(int64_t *rec, uint32_t rec_slots, int64_t rc, int32_t state)
{
    rec[0] = rc;
    rec[1] = state;
    rec[2] = 0;
    for (uint32_t q = 3; q < rec_slots; q++) rec[q] = -1;
}

/* As sre_k_streams_prologue, for rows of 1 + W words (sre_streams_nfa.h).  A stream whose call is
 * decided without a byte — not fed, closed, MATCH pending — gets no segments and its record (and
 * row) here; the others enter with their row's set, a fresh row with init0. */
__global__ __launch_bounds__(SRE_STREAMS_PRO_THREADS) void
sre_k_streams_nfa_prologue(const sre_streams_feed_t *__restrict__ feed, uint32_t n, int64_t *__restrict__ rows, uint32_t W,
                           sre_streams_nfa_init_t init0, uint32_t rec_slots, uint64_t seg_fixed, uint64_t resident,
                           uint64_t seg_cap, const uint8_t **__restrict__ ptrs, uint64_t *__restrict__ lens,
                           uint64_t *__restrict__ seg_first, uint8_t *__restrict__ sflags, uint64_t *__restrict__ eset,
                           int64_t *__restrict__ recs, sre_streams_info_t *__restrict__ info)
{
    __shared__ uint64_t sh[SRE_STREAMS_PRO_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + SRE_STREAMS_PRO_THREADS - 1) / SRE_STREAMS_PRO_THREADS;
    const uint32_t i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    const uint32_t row_words = 1 + W;
    auto scans = [&](uint32_t i) {
        return sre_streams_nfa_scans((uint64_t) rows[(size_t) i * row_words], (feed[i].flags & SRE_SFEED_FED) != 0) != 0;
    };
    uint64_t bytes = 0, nact = 0;
    for (uint32_t i = i0; i < i1; i++) {
        if (scans(i)) {
            bytes += feed[i].len;
            nact++;
        }
    }
    bytes = block_sum(bytes, sh);
    nact = block_sum(nact, sh);
    const uint64_t seg = seg_fixed ? seg_fixed : sre_scan_auto_segment(bytes, resident, seg_cap);
    uint64_t       mine = 0;
    for (uint32_t i = i0; i < i1; i++) {
        if (scans(i)) {
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
        int64_t                 *row = rows + (size_t) i * row_words;
        const uint64_t           fl = (uint64_t) row[0];
        const bool               fed = (f.flags & SRE_SFEED_FED) != 0, eof = (f.flags & SRE_SFEED_EOF) != 0;
        const bool               act = sre_streams_nfa_scans(fl, fed) != 0;
        seg_first[i] = run;
        ptrs[i] = reinterpret_cast<const uint8_t *>(f.ptr);
        lens[i] = act ? f.len : 0;
        sflags[i] = eof ? 0u : (uint8_t) SRE_SFLAG_NO_EOF;
        for (uint32_t w = 0; w < W; w++) eset[(size_t) i * W + w] = (fl & SRE_SNFA_STARTED) ? (uint64_t) row[1 + w] : init0.w[w];
        int64_t *rec = recs + (size_t) i * rec_slots;
        if (act) {
            const uint64_t k = (f.len + seg - 1) / seg;
            run += k ? k : 1;
            rec[1] = SRE_SSTATE_OPEN;           /* the tail writes the record */
        } else {
            const sre_snfa_step_t r = sre_streams_nfa_rule(fl, fed, f.len, eof, -1, 0);
            if (r.state == SRE_SNFA_NOT_FED) {
                rec[1] = SRE_SSTATE_NOT_FED;
            } else {
                snfa_record(rec, rec_slots, r.rc, r.state);
                row[0] = (int64_t) r.flags;
            }
        }
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

/* the work list of a fix-up round from the chain check's status words: lo[s] = the first segment of
 * stream s whose entry set was wrong, -1 for a stream that is verified; *pending += how many are not */
__global__ __launch_bounds__(256) void
sre_k_streams_nfa_lo(const sre_nfa_status_t *__restrict__ status, uint32_t n, int64_t *__restrict__ lo,
                     unsigned long long *__restrict__ pending)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    bool           open = false;
    if (i < n) {
        const sre_nfa_status_t st = status[i];
        open = !st.done;
        lo[i] = open ? st.first_bad : -1;
    }
    const uint64_t m = __builtin_amdgcn_ballot_w64(open);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(pending, (unsigned long long) __builtin_popcountll(m));
}

#define SRE_SNFA_UNSETTLED (-1)     /* state slot of a record between the first tail and the one behind the fix-up rounds */

/* One lane per stream: the rule of sre_streams_nfa.h on the chain check's verdict and the exit set of
 * the stream's last segment (sum[].s_out, or W words of the wide kernel's sets); writes the row and
 * the record.  A stream whose pass is not verified waits for the fix-up rounds (only_unsettled: the
 * second tail takes those alone) and is counted in info->unsettled. */
__global__ __launch_bounds__(256) void
sre_k_streams_nfa_tail(const sre_streams_feed_t *__restrict__ feed, uint32_t n, int64_t *__restrict__ rows, uint32_t W,
                       const uint64_t *__restrict__ seg_first, const sre_nfa_status_t *__restrict__ status,
                       const sre_nfa_summary_t *__restrict__ sum, const uint64_t *__restrict__ wsets, uint32_t rec_slots,
                       int64_t *__restrict__ recs, sre_streams_info_t *__restrict__ info, int only_unsettled)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const sre_streams_feed_t f = feed[i];
    int64_t                 *row = rows + (size_t) i * (1 + W);
    int64_t                 *rec = recs + (size_t) i * rec_slots;
    const uint64_t           fl = (uint64_t) row[0];
    /* (a row the prologue or the first tail advanced no longer scans, or its record says so) */
    if (only_unsettled ? rec[1] != SRE_SNFA_UNSETTLED : rec[1] != SRE_SSTATE_OPEN) return;
    if (!sre_streams_nfa_scans(fl, (f.flags & SRE_SFEED_FED) != 0) || seg_first[i + 1] == seg_first[i]) return;
    const sre_nfa_status_t st = status[i];
    if (!st.done) {
        rec[1] = SRE_SNFA_UNSETTLED;
        atomicAdd(reinterpret_cast<unsigned long long *>(&info->unsettled), 1ull);
        return;
    }
    const uint64_t g = seg_first[i + 1] - 1;
    uint64_t       out[4] = {0, 0, 0, 0}, any = 0;
    if (st.ev_pos < 0) {
        for (uint32_t w = 0; w < W; w++) {
            out[w] = wsets != nullptr ? wsets[(g * 2 + 1) * W + w] : sum[g].s_out;
            any |= out[w];
        }
    }
    const sre_snfa_step_t r = sre_streams_nfa_rule(fl, 1, f.len, (f.flags & SRE_SFEED_EOF) != 0, st.ev_pos, any == 0);
    if (!r.keep_set) {
        for (uint32_t w = 0; w < W; w++) row[1 + w] = (int64_t) out[w];
    }
    row[0] = (int64_t) r.flags;
    snfa_record(rec, rec_slots, r.rc, r.state);
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

extern "C" hipError_t
sre_launch_streams_nfa_prologue(const sre_streams_feed_t *d_feed, uint32_t n, int64_t *d_rows, uint32_t W,
                                sre_streams_nfa_init_t init0, uint32_t rec_slots, uint64_t seg_fixed, uint64_t resident,
                                uint64_t seg_cap, const uint8_t **d_ptrs, uint64_t *d_lens, uint64_t *d_seg_first,
                                uint8_t *d_sflags, uint64_t *d_eset, int64_t *d_recs, sre_streams_info_t *d_info,
                                hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (W < 1 || W > 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_streams_nfa_prologue, dim3(1), dim3(SRE_STREAMS_PRO_THREADS), 0, stream, d_feed, n, d_rows, W, init0,
                       rec_slots, seg_fixed, resident, seg_cap, d_ptrs, d_lens, d_seg_first, d_sflags, d_eset, d_recs, d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_streams_nfa_lo(const sre_nfa_status_t *d_status, uint32_t n, int64_t *d_lo, uint64_t *d_pending, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_pending, 0, sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sre_k_streams_nfa_lo, dim3((n + 255) / 256), dim3(256), 0, stream, d_status, n, d_lo,
                       reinterpret_cast<unsigned long long *>(d_pending));
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_streams_nfa_tail(const sre_streams_feed_t *d_feed, uint32_t n, int64_t *d_rows, uint32_t W,
                            const uint64_t *d_seg_first, const sre_nfa_status_t *d_status, const sre_nfa_summary_t *d_sum,
                            const uint64_t *d_wsets, uint32_t rec_slots, int64_t *d_recs, sre_streams_info_t *d_info,
                            int only_unsettled, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (W < 1 || W > 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_streams_nfa_tail, dim3((n + 255) / 256), dim3(256), 0, stream, d_feed, n, d_rows, W, d_seg_first,
                       d_status, d_sum, d_wsets, rec_slots, d_recs, d_info, only_unsettled);
    return hipGetLastError();
}
