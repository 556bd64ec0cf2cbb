/*
 * sre_hip_lines_block.h — what the kernels of the line sinks share (sre_hip_lines_gather.hip, sre_hip_lines_context.hip,
 * sre_hip_lines_fold.hip): the workgroup's exclusive prefix sum, where a line starts, and the workgroup's two scans of
 * "nearest marked line" words (sre_lines_context.h).  Device code only.
 */
#ifndef SRE_HIP_LINES_BLOCK_H
#define SRE_HIP_LINES_BLOCK_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sre_lines_context.h"

namespace {

/* exclusive prefix of v over the workgroup (NT lanes, a multiple of 64), and the total */
template <uint32_t NT>
__device__ inline uint64_t
block_excl_scan(uint64_t v, uint64_t *wsum, uint64_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t       x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < NT / 64; i++) {
        const uint64_t s = wsum[i];
        before += i < w ? s : 0;
        all += s;
    }
    __syncthreads();
    total = all;
    return before + x - v;
}

__device__ inline uint64_t
line_start(const uint64_t *ends, uint64_t i)
{
    return i == 0 ? 0 : ends[i - 1] + 1;
}

/* a wave's exclusive scans (sre_lc_wave_scan_fwd / _bwd run the same steps over an array): the lane's word over the
 * lanes in front of it, resp. behind it, and in `total` of lane 63, resp. lane 0, the wave's */
template <class T>
__device__ inline T
wave_excl_fwd(T v, uint32_t lane, T &total)
{
    T x = __shfl_up(v, 1, 64);
    if (lane == 0) x = 0;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) x = sre_lc_fwd(x, (T) __shfl_up(x, d, 64), lane, d);
    total = x > v ? x : v;
    return x;
}

template <class T>
__device__ inline T
wave_excl_bwd(T v, uint32_t lane, T &total)
{
    T x = __shfl_down(v, 1, 64);
    if (lane == 63) x = (T) ~(T) 0;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) x = sre_lc_bwd(x, (T) __shfl_down(x, d, 64), lane, d);
    total = x < v ? x : v;
    return x;
}

/* ... and the workgroup's (NW waves; sre_lc_block_scan): p and q become exclusive over the workgroup, ptot / qtot its
 * totals; wp and wq hold NW words each */
template <class T, uint32_t NW>
__device__ inline void
block_excl_marks(T &p, T &q, T *wp, T *wq, T &ptot, T &qtot)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    T              tp, tq;
    p = wave_excl_fwd(p, lane, tp);
    q = wave_excl_bwd(q, lane, tq);
    if (lane == 63) wp[w] = tp;
    if (lane == 0) wq[w] = tq;
    __syncthreads();
    const T pin = sre_lc_waves_fwd(wp, NW, w), qin = sre_lc_waves_bwd(wq, NW, w);
    p = pin > p ? pin : p;
    q = qin < q ? qin : q;
    ptot = sre_lc_waves_fwd(wp, NW, NW);
    T qt = wq[0];
#pragma unroll
    for (uint32_t i = 1; i < NW; i++) qt = wq[i] < qt ? wq[i] : qt;
    qtot = qt;
    __syncthreads();
}

}  // namespace

#endif
