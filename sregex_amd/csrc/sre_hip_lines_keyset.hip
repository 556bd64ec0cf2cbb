/*
 * sre_hip_lines_keyset.hip — the key set and the line lookup on the device (sregex_hip.h sre_hip_keyset_create and
 * sre_hip_lookup_lines).  The rules are those of sre_lines_keyset.h and sre_lines_tally.h, which the
 * CPU model compiles too.
 *
 *   fields     behind the split of the dictionary (the kernels of line mode), a lane per row: the row's K fields by the
 *              field rule; a row that breaks it sends its number to a minimum, so the lowest such row is reported;
 *   insert     a lane per row: hash the fields and run the tally's insert (sre_lt_step) over the dictionary's keys: a
 *              compare-and-swap claims an empty word, a minimum lowers the word of an equal key.  No counts, no
 *              max_keys; per workgroup one add of its claims, the distinct keys;
 *   probe      in sre_hip_lookup_lines, behind the last select pass and in front of the filter's scan, a lane per line
 *              (SRE_LK_ITEMS lines one after the other): hash the line's fields from the source buffer, walk the set's
 *              table from the home slot, compare every occupied word's row field by field; write the line's key id, keep
 *              or clear its filter value; per WORKGROUP one add of its keyed lines and one of its members (the two words
 *              share a cache line, which takes about 90 atomics a microsecond: an add per wave and word, 32 768 in a
 *              million lines, took longer than everything else in the kernel).
 *
 * The key map and the line join (sre_hip_keyset_create_map, sre_hip_join_lines, DESIGN.md §4.11.10, rules in
 * sre_lines_join.h) add two kernels:
 *   map fields the fields pass of a set whose rows carry value columns behind the key: one split of the row, the key fields
 *              to the arrays the insert and the probe read, the value columns to two arrays of their own;
 *   join       in sre_hip_join_lines, in the probe's place: the probe's walk, key id and counts, and in place of the filter
 *              value the line's 1 + columns entries of the join table (the extract's entry table), which the extract's
 *              scan and the join's gather (sre_hip_lines_gather.hip) take from there.
 *
 * Inside the insert every access to the table and the two counters is an atomic at agent scope: the L2s of the eight
 * XCDs do not see one another's plain stores within a kernel.  The probe runs behind the kernel boundary (usually calls
 * later) over a table nobody writes any more: plain loads, no atomics, no store to anything of the set.  The adds to the
 * call's two info words are atomics at agent scope.  No workgroup waits for another.  Plain C++ and vector memory
 * operations only.
 */
#include <sregex/sregex.h>
#include "sre_hip_lines.h"
#include "sre_lines_keyset.h"
#include "sre_lines_join.h"

namespace {

#define LK_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct DictBytes {
    const uint8_t *buf;
    __device__ inline uint8_t byte(uint64_t at) const { return buf[at]; }
};

/* lane per row */
__global__ __launch_bounds__(SRE_LK_THREADS) void
sre_k_keyset_fields(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ ends, uint64_t rows, uint32_t k, uint32_t fsep,
                    uint64_t *__restrict__ fstart, uint64_t *__restrict__ flen, uint64_t *bad)
{
    const uint64_t r = (uint64_t) blockIdx.x * SRE_LK_THREADS + threadIdx.x;
    if (r >= rows) return;
    const DictBytes b = {buf};
    uint64_t        st, end;
    sre_lk_row_span(ends, r, &st, &end);
    if (!sre_lk_row_fields(b, st, end, k, fsep, fstart + r * k, flen + r * k)) {
        (void) __hip_atomic_fetch_min(bad, r, LK_RELAXED_AGENT);
    }
}

/* a key map's (sre_lines_join.h): the row is split once over all its nf fields, the first k entries are its key fields, the
 * others its value columns.  A kernel of its own, so that a plain set's rows go through the kernel above as before */
__global__ __launch_bounds__(SRE_LK_THREADS) void
sre_k_keymap_fields(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ ends, uint64_t rows, uint32_t nf, uint32_t k,
                    uint32_t fsep, uint64_t *__restrict__ fstart, uint64_t *__restrict__ flen, uint64_t *__restrict__ vstart,
                    uint64_t *__restrict__ vlen, uint64_t *bad)
{
    const uint64_t r = (uint64_t) blockIdx.x * SRE_LK_THREADS + threadIdx.x;
    if (r >= rows) return;
    const DictBytes b = {buf};
    uint64_t        st, end, s[SRE_EXTRACT_MAX_FIELDS], l[SRE_EXTRACT_MAX_FIELDS];
    sre_lk_row_span(ends, r, &st, &end);
    if (!sre_lk_row_fields(b, st, end, nf, fsep, s, l)) {
        (void) __hip_atomic_fetch_min(bad, r, LK_RELAXED_AGENT);
        return;
    }
    sre_lj_part(s, l, nf, k, fstart + r * k, flen + r * k, vstart + r * (nf - k), vlen + r * (nf - k));
}

struct KeysetMem {
    uint64_t *tab;
    __device__ inline uint64_t cas(uint64_t idx, uint64_t expect, uint64_t v)
    {
        (void) __hip_atomic_compare_exchange_strong(&tab[idx], &expect, v, __ATOMIC_RELAXED, LK_RELAXED_AGENT);
        return expect;
    }
    __device__ inline void min(uint64_t idx, uint64_t v) { (void) __hip_atomic_fetch_min(&tab[idx], v, LK_RELAXED_AGENT); }
    __device__ inline bool raised() { return false; }       /* (no max_keys: nothing overflows at load <= 1/2) */
};

/* lane per row; every row leads its own search */
__global__ __launch_bounds__(SRE_LK_THREADS) void
sre_k_keyset_insert(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ fstart, const uint64_t *__restrict__ flen,
                    uint64_t rows, uint32_t k, sre_lt_params_t p, uint64_t *tab, uint64_t *distinct)
{
    __shared__ uint32_t    wclaim[SRE_LK_THREADS / 64u];
    const uint64_t         r = (uint64_t) blockIdx.x * SRE_LK_THREADS + threadIdx.x;
    const uint32_t         lane = threadIdx.x & 63u;
    const sre_lk_dict_keys keys = {buf, fstart, flen, k};
    KeysetMem              mem = {tab};
    const bool             in = r < rows;
    sre_lt_lane_t          L;
    sre_lt_begin(L, r, in, in ? sre_lt_hash(keys, r) : 0, p);
    while (!sre_lt_done(L)) sre_lt_step(L, keys, mem, p);
    /* the claims of the workgroup's waves meet in LDS: one add per workgroup */
    const uint64_t mclaim = __ballot(L.claimed);
    if (lane == 0) wclaim[threadIdx.x >> 6] = sre_lr_popc(mclaim);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0;
        for (uint32_t w = 0; w < SRE_LK_THREADS / 64u; w++) a += wclaim[w];
        if (a) (void) __hip_atomic_fetch_add(distinct, a, LK_RELAXED_AGENT);
    }
}

/* the finished table as the probe reads it */
struct ProbeMem {
    const uint64_t *tab;
    __device__ inline uint64_t load(uint64_t idx) const { return tab[idx]; }
};

/* a workgroup takes SRE_LK_ITEMS x SRE_LK_THREADS consecutive lines, lane x the lines x, x + SRE_LK_THREADS, ..; the
 * counts of its waves meet in LDS, and one lane adds them to the call's words */
__global__ __launch_bounds__(SRE_LK_THREADS) void
sre_k_keyset_probe(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ vval, const uint64_t *__restrict__ vstart,
                   uint64_t n, uint32_t k, const uint8_t *__restrict__ dict, const uint64_t *__restrict__ fstart,
                   const uint64_t *__restrict__ flen, const uint64_t *__restrict__ tab, sre_lt_params_t p, int invert,
                   uint64_t *__restrict__ fval, int64_t *__restrict__ keyid, uint64_t keyid_n, sre_lines_info_t *info)
{
    __shared__ uint32_t    wkeyed[SRE_LK_THREADS / 64u], wmember[SRE_LK_THREADS / 64u];
    const uint32_t         lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const sre_lk_line_keys lines = {buf, vval, vstart, k};
    const sre_lk_dict_keys rows = {dict, fstart, flen, k};
    const ProbeMem         mem = {tab};
    uint32_t               nkeyed = 0, nmember = 0;         /* of the wave */
    for (uint32_t q = 0; q < SRE_LK_ITEMS; q++) {
        const uint64_t i = ((uint64_t) blockIdx.x * SRE_LK_ITEMS + q) * SRE_LK_THREADS + threadIdx.x;
        const bool     keyed = i < n && lines.selected(i);
        sre_lk_probe_t P;
        P.id = SRE_LK_NOT_MEMBER;
        if (keyed) {
            sre_lk_probe_begin(P, sre_lt_hash(lines, i), p);
            while (!P.done) sre_lk_probe_step(P, i, lines, rows, mem, p);
        }
        if (i < keyid_n) keyid[i] = sre_lk_keyid(keyed, P.id);
        if (i < n) fval[i] = sre_lk_value(keyed, P.id, invert != 0, fval[i]);
        nkeyed += sre_lr_popc(__ballot(keyed));
        nmember += sre_lr_popc(__ballot(keyed && P.id >= 0));
    }
    if (lane == 0) {
        wkeyed[wave] = nkeyed;
        wmember[wave] = nmember;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, b = 0;
        for (uint32_t w = 0; w < SRE_LK_THREADS / 64u; w++) {
            a += wkeyed[w];
            b += wmember[w];
        }
        if (a) (void) __hip_atomic_fetch_add(&info->knkeyed, a, LK_RELAXED_AGENT);
        if (b) (void) __hip_atomic_fetch_add(&info->knmembers, b, LK_RELAXED_AGENT);
    }
}

/* the join pass (sre_hip_join_lines, sre_lines_join.h): the probe's walk and its two counts, lane for lane; in place of the
 * filter value every line gets its P = 1 + c.n entries of the join table, P consecutive words of val and of start per
 * lane (the stride the extract's table has; a lane per entry would walk the table P times).  own: the scanner's copy of
 * the key ids, all n of them, for the index; keyid: the caller's first keyid_n.  Nothing of the set is written */
__global__ __launch_bounds__(SRE_LK_THREADS) void
sre_k_keyset_join(const uint8_t *__restrict__ buf, const uint64_t *__restrict__ vval, const uint64_t *__restrict__ vstart,
                  const uint64_t *__restrict__ ends, uint64_t n, uint32_t k, const uint8_t *__restrict__ dict,
                  const uint64_t *__restrict__ fstart, const uint64_t *__restrict__ flen, const uint64_t *__restrict__ mstart,
                  const uint64_t *__restrict__ mlen, uint32_t nvalues, const uint64_t *__restrict__ tab, sre_lt_params_t p,
                  sre_lj_cols_t c, int all, uint64_t *__restrict__ val, uint64_t *__restrict__ start, int64_t *__restrict__ own,
                  int64_t *__restrict__ keyid, uint64_t keyid_n, sre_lines_info_t *info)
{
    __shared__ uint32_t    wkeyed[SRE_LK_THREADS / 64u], wmember[SRE_LK_THREADS / 64u];
    const uint32_t         lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, P = 1 + c.n;
    const sre_lk_line_keys lines = {buf, vval, vstart, k};
    const sre_lk_dict_keys rows = {dict, fstart, flen, k};
    const ProbeMem         mem = {tab};
    uint32_t               nkeyed = 0, nmember = 0;         /* of the wave */
    for (uint32_t q = 0; q < SRE_LK_ITEMS; q++) {
        const uint64_t i = ((uint64_t) blockIdx.x * SRE_LK_ITEMS + q) * SRE_LK_THREADS + threadIdx.x;
        const bool     keyed = i < n && lines.selected(i);
        sre_lk_probe_t R;
        R.id = SRE_LK_NOT_MEMBER;
        if (keyed) {
            sre_lk_probe_begin(R, sre_lt_hash(lines, i), p);
            while (!R.done) sre_lk_probe_step(R, i, lines, rows, mem, p);
        }
        if (i < n) {
            const int64_t  id = sre_lk_keyid(keyed, R.id);
            const uint64_t st = i ? ends[i - 1] + 1 : 0;
            own[i] = id;
            if (i < keyid_n) keyid[i] = id;
            sre_lj_entries(keyed, R.id, all != 0, st, ends[i] - st, mstart, mlen, nvalues, c, val + i * P, start + i * P);
        }
        nkeyed += sre_lr_popc(__ballot(keyed));
        nmember += sre_lr_popc(__ballot(keyed && R.id >= 0));
    }
    if (lane == 0) {
        wkeyed[wave] = nkeyed;
        wmember[wave] = nmember;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, b = 0;
        for (uint32_t w = 0; w < SRE_LK_THREADS / 64u; w++) {
            a += wkeyed[w];
            b += wmember[w];
        }
        if (a) (void) __hip_atomic_fetch_add(&info->knkeyed, a, LK_RELAXED_AGENT);
        if (b) (void) __hip_atomic_fetch_add(&info->knmembers, b, LK_RELAXED_AGENT);
    }
}

bool
table_ok(uint64_t nslots)
{
    /* (a slot number fits the 32-bit word of sre_lt_lane_t) */
    return nslots >= SRE_LT_MIN_SLOTS && (nslots & (nslots - 1)) == 0 && nslots <= ((uint64_t) 1 << 31);
}

}  // namespace

extern "C" hipError_t
sre_launch_keyset_fields(const void *d_rows, const uint64_t *d_ends, uint64_t rows, uint32_t k, uint32_t fsep, uint64_t *d_fstart,
                         uint64_t *d_flen, uint64_t *d_bad, hipStream_t stream)
{
    if (rows == 0 || rows > SRE_LK_MAX_ROWS || k == 0 || k > SRE_EXTRACT_MAX_FIELDS) return hipErrorInvalidValue;
    const uint64_t nwg = (rows + SRE_LK_THREADS - 1) / SRE_LK_THREADS;
    hipLaunchKernelGGL(sre_k_keyset_fields, dim3((uint32_t) nwg), dim3(SRE_LK_THREADS), 0, stream, static_cast<const uint8_t *>(d_rows),
                       d_ends, rows, k, fsep, d_fstart, d_flen, d_bad);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_keyset_insert(const void *d_rows, const uint64_t *d_fstart, const uint64_t *d_flen, uint64_t rows, uint32_t k,
                         uint64_t nslots, uint64_t hash_mask, uint64_t *d_tab, uint64_t *d_distinct, hipStream_t stream)
{
    if (rows == 0 || rows > SRE_LK_MAX_ROWS || k == 0 || k > SRE_EXTRACT_MAX_FIELDS || !table_ok(nslots) || 2 * rows > nslots) {
        return hipErrorInvalidValue;
    }
    sre_lt_params_t p;
    p.nslots = nslots;
    p.max_keys = rows;
    p.hash_mask = hash_mask;
    const uint64_t nwg = (rows + SRE_LK_THREADS - 1) / SRE_LK_THREADS;
    hipLaunchKernelGGL(sre_k_keyset_insert, dim3((uint32_t) nwg), dim3(SRE_LK_THREADS), 0, stream, static_cast<const uint8_t *>(d_rows),
                       d_fstart, d_flen, rows, k, p, d_tab, d_distinct);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_keyset_probe(const void *d_buf, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n, uint32_t k,
                        const void *d_rows, const uint64_t *d_fstart, const uint64_t *d_flen, const uint64_t *d_tab, uint64_t nslots,
                        uint64_t hash_mask, int invert, uint64_t *d_fval, int64_t *d_keyid, uint64_t keyid_cap,
                        sre_lines_info_t *d_info, hipStream_t stream)
{
    if (n == 0 || k == 0 || k > SRE_EXTRACT_MAX_FIELDS || !table_ok(nslots)) return hipErrorInvalidValue;
    const uint64_t per = (uint64_t) SRE_LK_THREADS * SRE_LK_ITEMS, nwg = (n + per - 1) / per;
    if (nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    sre_lt_params_t p;
    p.nslots = nslots;
    p.max_keys = nslots / 2;
    p.hash_mask = hash_mask;
    hipLaunchKernelGGL(sre_k_keyset_probe, dim3((uint32_t) nwg), dim3(SRE_LK_THREADS), 0, stream, static_cast<const uint8_t *>(d_buf),
                       d_vval, d_vstart, n, k, static_cast<const uint8_t *>(d_rows), d_fstart, d_flen, d_tab, p, invert, d_fval, d_keyid,
                       keyid_cap < n ? keyid_cap : n, d_info);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_keymap_fields(const void *d_rows, const uint64_t *d_ends, uint64_t rows, uint32_t nfields, uint32_t k, uint32_t fsep,
                         uint64_t *d_fstart, uint64_t *d_flen, uint64_t *d_vstart, uint64_t *d_vlen, uint64_t *d_bad,
                         hipStream_t stream)
{
    if (rows == 0 || rows > SRE_LK_MAX_ROWS || k == 0 || k >= nfields || nfields > SRE_EXTRACT_MAX_FIELDS) return hipErrorInvalidValue;
    const uint64_t nwg = (rows + SRE_LK_THREADS - 1) / SRE_LK_THREADS;
    hipLaunchKernelGGL(sre_k_keymap_fields, dim3((uint32_t) nwg), dim3(SRE_LK_THREADS), 0, stream, static_cast<const uint8_t *>(d_rows),
                       d_ends, rows, nfields, k, fsep, d_fstart, d_flen, d_vstart, d_vlen, d_bad);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_keyset_join(const void *d_buf, const uint64_t *d_vval, const uint64_t *d_vstart, const uint64_t *d_ends, uint64_t n,
                       uint32_t k, const void *d_rows, const uint64_t *d_fstart, const uint64_t *d_flen, const uint64_t *d_mstart,
                       const uint64_t *d_mlen, uint32_t nvalues, const uint64_t *d_tab, uint64_t nslots, uint64_t hash_mask,
                       const sre_lj_cols_t *cols, int all, uint64_t *d_val, uint64_t *d_start, int64_t *d_own, int64_t *d_keyid,
                       uint64_t keyid_cap, sre_lines_info_t *d_info, hipStream_t stream)
{
    if (n == 0 || k == 0 || k > SRE_EXTRACT_MAX_FIELDS || !table_ok(nslots) || cols->n < 1 || cols->n > SRE_LJ_MAX_VALUES) {
        return hipErrorInvalidValue;
    }
    for (uint32_t x = 0; x < cols->n; x++) {
        if (cols->col[x] >= nvalues) return hipErrorInvalidValue;       /* (a column of every row: entry row * nvalues + col) */
    }
    const uint64_t per = (uint64_t) SRE_LK_THREADS * SRE_LK_ITEMS, nwg = (n + per - 1) / per;
    if (nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    sre_lt_params_t p;
    p.nslots = nslots;
    p.max_keys = nslots / 2;
    p.hash_mask = hash_mask;
    hipLaunchKernelGGL(sre_k_keyset_join, dim3((uint32_t) nwg), dim3(SRE_LK_THREADS), 0, stream, static_cast<const uint8_t *>(d_buf),
                       d_vval, d_vstart, d_ends, n, k, static_cast<const uint8_t *>(d_rows), d_fstart, d_flen, d_mstart, d_mlen, nvalues,
                       d_tab, p, *cols, all, d_val, d_start, d_own, d_keyid, keyid_cap < n ? keyid_cap : n, d_info);
    return hipGetLastError();
}
