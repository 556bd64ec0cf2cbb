/*
 * sre_hip_lines_sort_text.hip — the line sort by text on the device (sregex_hip.h sre_hip_sort_lines_text):
 * the lines of a buffer ordered by the bytes of a capture group, an LSD radix sort over chunks of 7 bytes, every chunk through
 * the digit passes of the numeric sort (sre_hip_lines_sort.hip).  The rules are those of sre_lines_sort_text.h, which the CPU
 * model compiles too.
 *
 *   values     the values pass of sre_hip_lines_values.h, a lane per line: a line with a match is keyed and its value is its
 *              compared length, so the four totals are (keyed, keyed, minlen, maxlen);
 *   keys       a lane per item: the key of one chunk, from the item's line through the value table's start and length to
 *              at most 7 bytes of the source buffer.  For the first chunk a call processes the items are the lines in line
 *              order, the key of an unselected line is "dropped";
 *   first      the one digit pass that makes the items: count and scatter of sre_hip_lines_partition.h over the keys of the
 *              lines, key and line number of every selected line to its rank.  Every later pass is the numeric sort's;
 *   index      a lane per written rank.
 *
 * Table, scan and cut, finish and gather are the numeric sort's, unchanged.  No workgroup waits for another and no rank comes
 * from an atomic.  Plain C++ and vector memory operations only; the source buffer is read a byte at a time and never at or
 * past `len`.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"
#include "sre_lines_sort_text.h"
#include "sre_hip_lines_partition.h"
#include "sre_hip_lines_values.h"

namespace {

/* the value table of the one sort group (written by earlier kernels or copies: plain loads) and the source buffer: the source
 * of the values pass (item i is line i) and the text of the keys */
struct TextVals {
    const uint8_t *__restrict__ buf;
    uint64_t len;
    const uint64_t *__restrict__ vval, *__restrict__ vstart;
    uint64_t n, max_bytes;
    __device__ inline uint64_t val(uint64_t line, uint32_t) const { return vval[line]; }
    __device__ inline uint64_t raw(uint64_t line, uint32_t) const { return vstart[line]; }
    __device__ inline uint8_t  byte(uint64_t at) const { return at < len ? buf[at] : (uint8_t) 0; }
    __device__ inline int32_t  classify(uint64_t i, int64_t *v) const { return sre_lst_line(*this, i, max_bytes, v); }
};

/* a lane per item: the key of chunk `chunk`.  lines == NULL: item i is line i of the n lines, unselected ones included (their
 * key is "dropped"); otherwise item i is line lines[i], selected */
__global__ __launch_bounds__(256) void
sre_k_sort_text_keys(const TextVals vals, const uint32_t *__restrict__ lines, uint64_t nitems, uint64_t chunk, int desc, int all,
                     uint64_t *__restrict__ keys)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= nitems) return;
    const uint64_t line = lines ? lines[i] : i;
    /* (a line number beyond the table cannot happen: an item carries the number of its line) */
    keys[i] = line < vals.n ? sre_lst_line_key(vals, line, chunk, vals.max_bytes, desc, all) : sre_lst_rest_key(chunk, desc);
}

/* the digit pass that makes the items (sre_hip_lines_partition.h): key i is that of line i, "dropped" for an unselected line;
 * key and line number of every other go to the same rank of dkey / dline */
struct TextFirstPass {
    static constexpr uint32_t MAX_DIGITS = 1u << SRE_LSO_DIGIT_BITS;
    static constexpr int      RULE = SRE_LRK_RANK_BITS;
    const uint64_t *__restrict__ src;
    uint64_t n;
    uint32_t pass;
    uint64_t *__restrict__ dkey;
    uint32_t *__restrict__ dline;
    __device__ uint32_t nd() const { return MAX_DIGITS; }
    __device__ uint32_t bits() const { return SRE_LSO_DIGIT_BITS; }
    __device__ uint64_t load(uint64_t i) const { return i < n ? src[i] : SRE_LSO_DROPPED; }
    __device__ bool     taken(uint64_t key) const { return key != SRE_LSO_DROPPED; }
    __device__ uint32_t digit(uint64_t key) const { return sre_lso_digit(key, pass); }
    __device__ void     store(uint64_t r, uint64_t key, uint64_t i) const
    {
        dkey[r] = key;
        dline[r] = (uint32_t) i;
    }
};

/* rows [line, start, len, output offset, field start, field length] of the first min(index_cap, written) ranks */
__global__ __launch_bounds__(256) void
sre_k_sort_text_index(const TextVals vals, const uint32_t *__restrict__ lines, const uint64_t *__restrict__ cstart,
                      const uint64_t *__restrict__ coff, const uint64_t *__restrict__ res, uint64_t index_cap, int64_t *__restrict__ out)
{
    const uint64_t written = res[SRE_LSO_RES_WRITTEN];
    const uint64_t limit = index_cap < written ? index_cap : written;
    const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (r >= limit) return;
    const uint64_t i = lines[r];
    if (i >= vals.n) return;            /* (cannot happen) */
    sre_lst_index_row(vals, i, cstart, coff, r, out + r * SRE_LST_INDEX_WORDS);
}

}  // namespace

extern "C" hipError_t
sre_launch_sort_text_values(const void *d_buf, uint64_t len, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n,
                            uint64_t max_bytes, int64_t *d_value, int8_t *d_class, uint64_t *d_totals, hipStream_t stream)
{
    if (n == 0) return hipErrorInvalidValue;
    const TextVals src = {static_cast<const uint8_t *>(d_buf), len, d_vval, d_vstart, n, max_bytes};
    return values_launch(src, d_value, d_class, d_totals, stream);
}

extern "C" hipError_t
sre_launch_sort_text_keys(const void *d_buf, uint64_t len, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n,
                          uint64_t max_bytes, const uint32_t *d_lines, uint64_t nitems, uint64_t chunk, int desc, int all,
                          uint64_t *d_keys, hipStream_t stream)
{
    if (nitems == 0) return hipSuccess;
    const uint64_t nblk = (nitems + 255) / 256;
    if (n == 0 || (d_lines == NULL && nitems != n) || nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const TextVals vals = {static_cast<const uint8_t *>(d_buf), len, d_vval, d_vstart, n, max_bytes};
    hipLaunchKernelGGL(sre_k_sort_text_keys, dim3((uint32_t) nblk), dim3(256), 0, stream, vals, d_lines, nitems, chunk, desc, all,
                       d_keys);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_sort_text_count(const uint64_t *d_lkeys, uint64_t n, uint32_t pass, uint64_t *d_cnt, hipStream_t stream)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || pass >= SRE_LSO_MAX_PASSES || nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const TextFirstPass p = {d_lkeys, n, pass, NULL, NULL};
    hipLaunchKernelGGL(sre_k_partition_count<TextFirstPass>, dim3((uint32_t) nwg), dim3(SRE_LR_THREADS), 0, stream, p, nwg, d_cnt);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_sort_text_scatter(const uint64_t *d_lkeys, uint64_t n, uint32_t pass, const uint64_t *d_first, uint64_t total,
                             uint64_t *d_dkey, uint32_t *d_dline, hipStream_t stream)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    if (n == 0 || n > SRE_LRK_MAX_LINES || pass >= SRE_LSO_MAX_PASSES || nwg > 0x7FFFFFFFull || total > n) return hipErrorInvalidValue;
    if (total == 0) return hipSuccess;
    const TextFirstPass p = {d_lkeys, n, pass, d_dkey, d_dline};
    hipLaunchKernelGGL(sre_k_partition_scatter<TextFirstPass>, dim3((uint32_t) nwg), dim3(SRE_LR_THREADS), 0, stream, p, nwg, d_first,
                       total);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_sort_text_index(const void *d_buf, uint64_t len, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n,
                           const uint32_t *d_lines, const uint64_t *d_cstart, const uint64_t *d_coff, const uint64_t *d_res,
                           uint64_t nrows, uint64_t index_cap, int64_t *d_index, hipStream_t stream)
{
    if (nrows == 0 || index_cap == 0) return hipSuccess;
    const uint64_t nblk = (nrows + 255) / 256;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const TextVals vals = {static_cast<const uint8_t *>(d_buf), len, d_vval, d_vstart, n, 0};
    hipLaunchKernelGGL(sre_k_sort_text_index, dim3((uint32_t) nblk), dim3(256), 0, stream, vals, d_lines, d_cstart, d_coff, d_res,
                       index_cap, d_index);
    return hipGetLastError();
}
