/*
 * sre_hip_lines_block.h — what the kernels of the line sinks share (sre_hip_lines_gather.hip, sre_hip_lines_context.hip):
 * the workgroup's exclusive prefix sum and where a line starts.  Device code only.
 */
#ifndef SRE_HIP_LINES_BLOCK_H
#define SRE_HIP_LINES_BLOCK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace

#endif
