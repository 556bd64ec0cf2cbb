/*
 * sre_hip_lines_values.h — the values pass of the line sort (sre_hip_lines_sort.hip) and of the ordered tally
 * (sre_hip_lines_tally_top.hip), DESIGN.md §4.11.12: the value and the class of every item and the four totals of the call.
 * The geometry, the totals, their merge and their flush are those of sre_lines_sort.h.  Device code only.
 *
 *   init       one lane: the identities of the four words;
 *   values     a workgroup takes SRE_LSO_LINES items, a lane SRE_LSO_PER_LANE of them: value[i] and cls[i] of each, the totals
 *              merged over the lane, the wave and the workgroup, and at most one add per count, one minimum and one maximum
 *              to the four words.
 *
 * What an item is belongs to the caller: a source type Src, handed to the kernel by value, with
 *   n                  the items of the call;
 *   classify(i, &v)    the class of item i < n, v its value.
 *
 * Only the four totals take atomics, at agent scope.  No workgroup waits for another.  Plain C++ and vector memory
 * operations only.
 */
#ifndef SRE_HIP_LINES_VALUES_H
#define SRE_HIP_LINES_VALUES_H

#include "sre_lines_sort.h"

#define LSO_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

namespace {

/* the four words of the call: skeyed, snumbered, svmin, svmax of sre_lines_info_t, in that order */
struct ValuesMem {
    uint64_t *w;
    __device__ inline void add_keyed(uint64_t v) { (void) __hip_atomic_fetch_add(w + 0, v, LSO_RELAXED_AGENT); }
    __device__ inline void add_numbered(uint64_t v) { (void) __hip_atomic_fetch_add(w + 1, v, LSO_RELAXED_AGENT); }
    __device__ inline void min(int64_t v) { (void) __hip_atomic_fetch_min(reinterpret_cast<int64_t *>(w + 2), v, LSO_RELAXED_AGENT); }
    __device__ inline void max(int64_t v) { (void) __hip_atomic_fetch_max(reinterpret_cast<int64_t *>(w + 3), v, LSO_RELAXED_AGENT); }
};

/* every lane gets the merge of all 64 lanes' totals */
__device__ inline sre_lso_totals_t
wave_merge(sre_lso_totals_t t)
{
    for (int d = 1; d < 64; d <<= 1) {
        sre_lso_totals_t o;
        o.nkeyed = (uint64_t) __shfl_xor((unsigned long long) t.nkeyed, d, 64);
        o.nnumbered = (uint64_t) __shfl_xor((unsigned long long) t.nnumbered, d, 64);
        o.vmin = (int64_t) __shfl_xor((long long) t.vmin, d, 64);
        o.vmax = (int64_t) __shfl_xor((long long) t.vmax, d, 64);
        t = sre_lso_merge(t, o);
    }
    return t;
}

/* one lane, in front of the values pass: the identities of the four words */
__global__ __launch_bounds__(64) void
sre_k_values_init(uint64_t *__restrict__ w)
{
    if (threadIdx.x != 0) return;
    const sre_lso_totals_t t = sre_lso_identity();
    w[0] = t.nkeyed;
    w[1] = t.nnumbered;
    w[2] = (uint64_t) t.vmin;
    w[3] = (uint64_t) t.vmax;
}

/* workgroup w: the items w * SRE_LSO_LINES + j * SRE_LSO_THREADS + lane, j = 0 .. SRE_LSO_PER_LANE - 1 */
template <class Src>
__global__ __launch_bounds__(SRE_LSO_THREADS) void
sre_k_values(const Src src, int64_t *__restrict__ value, int8_t *__restrict__ cls, uint64_t *totals)
{
    __shared__ sre_lso_totals_t part[SRE_LSO_THREADS / 64u];
    sre_lso_totals_t            t = sre_lso_identity();
#pragma unroll
    for (uint32_t j = 0; j < SRE_LSO_PER_LANE; j++) {
        const uint64_t i = (uint64_t) blockIdx.x * SRE_LSO_LINES + j * SRE_LSO_THREADS + threadIdx.x;
        if (i >= src.n) continue;
        int64_t       v;
        const int32_t c = src.classify(i, &v);
        value[i] = v;
        cls[i] = (int8_t) c;
        t = sre_lso_merge(t, sre_lso_single(c, v));
    }
    t = wave_merge(t);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (uint32_t w = 1; w < SRE_LSO_THREADS / 64u; w++) t = sre_lso_merge(t, part[w]);
    ValuesMem mem = {totals};
    sre_lso_flush(mem, t);
}

/* the init and, over src.n items (none: the identities stand), the values pass, queued */
template <class Src>
hipError_t
values_launch(const Src &src, int64_t *d_value, int8_t *d_class, uint64_t *d_totals, hipStream_t stream)
{
    const uint64_t nwg = (src.n + SRE_LSO_LINES - 1) / SRE_LSO_LINES;
    if (nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sre_k_values_init, dim3(1), dim3(64), 0, stream, d_totals);
    if (nwg == 0) return hipGetLastError();
    hipLaunchKernelGGL(sre_k_values<Src>, dim3((uint32_t) nwg), dim3(SRE_LSO_THREADS), 0, stream, src, d_value, d_class, d_totals);
    return hipGetLastError();
}

}  // namespace

#endif
