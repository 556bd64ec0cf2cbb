/*
 * sre_lines_route.h — the rules of the line route (sre_hip_route_lines): the per-line key, which
 * lines a workgroup and a wave of the count and scatter passes own, the stable rank of a line among the lines of its
 * bucket, and the per-bucket totals.  The kernels (sre_hip_lines_route.hip), the host route of the batched API and the
 * CPU model (tests/lines_route_sim.cpp) compile this text; nothing here touches memory except through its arguments.
 *
 * The KEY of line i, one word: 0 for a dropped line, else bucket << 56 | (len + 1).  bucket < 256 takes the top byte
 * whole (bucket + 1 would not fit it with 256 buckets); len + 1 is never 0, so no routed line has the word 0, and a
 * line is shorter than 2^56 - 1 bytes.
 *
 * The partition.  A workgroup w of SRE_LR_THREADS lanes owns the SRE_LR_ITEMS lines from w * SRE_LR_ITEMS, as SRE_LR_SLOTS
 * SLOTS of 64 consecutive lines: wave v takes the slots v * SRE_LR_ROUNDS + q, q = 0 .. SRE_LR_ROUNDS - 1, one after the
 * other, lane x of it the line w * SRE_LR_ITEMS + slot * 64 + x.  Line order is therefore (workgroup, slot, lane) order.
 *   count    cnt[b * nwg + w] = lines of bucket b in workgroup w (bucket-major); the exclusive scan of that array
 *            gives first[b * nwg + w], the rank of the first such line among ALL selected lines in output order
 *            (bucket-major, line order inside a bucket), and first[nbuckets * nwg] = nsel;
 *   scatter  the rank of a line = first[b * nwg + w] + lines of bucket b in the slots in front of its slot
 *            + lines of bucket b in its slot at lower lanes.
 * The last term is the wave rule: for every distinct bucket present in the slot, in the order of the lowest lane
 * that holds it, the ballot m of the lanes with that bucket; a lane's rank is the set bits of m below it, the
 * slot's count of the bucket all bits of m.  The loop runs once per DISTINCT bucket of the slot, whatever nbuckets is.
 *
 * The compact table has one entry per selected line at its rank r: cstart[r] = the line's source offset with
 * SRE_LG_ENTRY_LAST | SRE_LG_ENTRY_FIRST (an entry table of sre_lines_gather.h with one entry a line), cval[r] = len + 1
 * (scanned to coff[0 .. nsel] like any table of the sinks), cmeta[r] = bucket << 56 | line for the index.
 */
#ifndef SRE_LINES_ROUTE_H
#define SRE_LINES_ROUTE_H

#include <stdint.h>
#include "sre_lines_gather.h"

#define SRE_LR_THREADS      256u
#define SRE_LR_ROUNDS       4u
#define SRE_LR_WAVES        (SRE_LR_THREADS / 64u)
#define SRE_LR_SLOTS        (SRE_LR_WAVES * SRE_LR_ROUNDS)          /* 16 */
#define SRE_LR_ITEMS        (SRE_LR_SLOTS * 64u)                    /* 1024 = SRE_LINES_ITEMS */
#define SRE_LR_MAX_BUCKETS  256u

#define SRE_LR_KEY_SHIFT    56u
#define SRE_LR_KEY_LEN      ((1ull << SRE_LR_KEY_SHIFT) - 1)

/* words the finish pass leaves for the host (sre_lr_result) in front of the 2 * nbuckets per-bucket words [nlines, bytes] */
#define SRE_LR_RES_NSEL     0u
#define SRE_LR_RES_NEED     1u
#define SRE_LR_RES_WRITTEN  2u
#define SRE_LR_RES_BYTES    3u
#define SRE_LR_RES_WORDS    4u

/* the bucket of a line from its record's rc and the call's map of nreg + 1 entries (entry nreg: no match); -1 drops
 * the line.  An rc that is neither a regex id nor `declined` (an error) drops it too */
SRE_LG_FN int32_t
sre_lr_bucket(int64_t rc, int64_t declined, uint32_t nreg, const int32_t *map)
{
    if (rc >= 0 && rc < (int64_t) nreg) return map[rc];
    return rc == declined ? map[nreg] : -1;
}

SRE_LG_FN uint64_t
sre_lr_key(int32_t bucket, uint64_t len)
{
    return bucket < 0 ? 0 : ((uint64_t) bucket << SRE_LR_KEY_SHIFT) | (len + 1);
}

SRE_LG_FN bool     sre_lr_key_selected(uint64_t key) { return key != 0; }
SRE_LG_FN uint32_t sre_lr_key_bucket(uint64_t key) { return (uint32_t) (key >> SRE_LR_KEY_SHIFT); }
SRE_LG_FN uint64_t sre_lr_key_val(uint64_t key) { return key & SRE_LR_KEY_LEN; }      /* len + 1 */

/* the line of (workgroup, slot, lane) */
SRE_LG_FN uint64_t
sre_lr_line(uint64_t wg, uint32_t slot, uint32_t lane)
{
    return wg * SRE_LR_ITEMS + (uint64_t) slot * 64u + lane;
}

SRE_LG_FN uint32_t sre_lr_slot(uint32_t wave, uint32_t round) { return wave * SRE_LR_ROUNDS + round; }

/* the wave rule on ballots: the lane whose bucket the next turn of the loop takes, a lane's rank in the ballot of its
 * bucket, and the slot's count of it */
SRE_LG_FN uint32_t
sre_lr_leader(uint64_t remaining)
{
    return (uint32_t) __builtin_ctzll(remaining);       /* (remaining != 0) */
}

SRE_LG_FN uint32_t
sre_lr_popc(uint64_t m)
{
    return (uint32_t) __builtin_popcountll(m);
}

SRE_LG_FN uint32_t sre_lr_rank_in(uint64_t m, uint32_t lane) { return sre_lr_popc(m & (((uint64_t) 1 << lane) - 1)); }

/* the word array of the counts: nbuckets * nwg words and the total behind them */
SRE_LG_FN uint64_t sre_lr_cnt_index(uint32_t bucket, uint64_t nwg, uint64_t wg) { return (uint64_t) bucket * nwg + wg; }

/* slot counts c[slot][bucket] of one bucket become the lines of the bucket in front of each slot; returns the total */
SRE_LG_FN uint32_t
sre_lr_slot_prefix(uint32_t *c, uint32_t stride)
{
    uint32_t run = 0;
    for (uint32_t s = 0; s < SRE_LR_SLOTS; s++) {
        const uint32_t v = c[s * stride];
        c[s * stride] = run;
        run += v;
    }
    return run;
}

/* the entry of the compact table a selected line writes */
SRE_LG_FN uint64_t sre_lr_entry_start(uint64_t start) { return start | SRE_LG_ENTRY_LAST | SRE_LG_ENTRY_FIRST; }
SRE_LG_FN uint64_t sre_lr_entry_meta(uint32_t bucket, uint64_t line) { return ((uint64_t) bucket << SRE_LR_KEY_SHIFT) | line; }
SRE_LG_FN uint32_t sre_lr_meta_bucket(uint64_t meta) { return (uint32_t) (meta >> SRE_LR_KEY_SHIFT); }
SRE_LG_FN uint64_t sre_lr_meta_line(uint64_t meta) { return meta & SRE_LR_KEY_LEN; }

/* finish: the totals of bucket b from the scanned counts first[0 .. nbuckets * nwg] and the scanned table coff[0 .. nsel] */
SRE_LG_FN void
sre_lr_bucket_totals(const uint64_t *first, uint64_t nwg, uint32_t b, const uint64_t *coff, uint64_t *nlines, uint64_t *bytes)
{
    const uint64_t r0 = first[sre_lr_cnt_index(b, nwg, 0)], r1 = first[sre_lr_cnt_index(b + 1, nwg, 0)];
    *nlines = r1 - r0;
    *bytes = coff[r1] - coff[r0];
}

/* ... and the cut at out_cap: every entry is a whole row, so rows in front of the cut = sre_lg_row_cut with k = 1 */
SRE_LG_FN uint64_t
sre_lr_cut(const uint64_t *coff, uint64_t nsel, uint64_t out_cap)
{
    return sre_lg_row_cut(coff, nsel, 1, out_cap);
}

/* the first SRE_LR_RES_WORDS result words of every call with a compact table (the route, the route by key, the sort), from
 * the scanned table coff[0 .. nrows] (not read when nrows == 0): the rows, their bytes, the rows that fit out_cap whole and
 * the bytes of those */
SRE_LG_FN void
sre_lr_result(const uint64_t *coff, uint64_t nrows, uint64_t out_cap, uint64_t *res)
{
    const uint64_t cut = nrows ? sre_lr_cut(coff, nrows, out_cap) : 0;
    res[SRE_LR_RES_NSEL] = nrows;
    res[SRE_LR_RES_NEED] = nrows ? coff[nrows] : 0;
    res[SRE_LR_RES_WRITTEN] = cut;
    res[SRE_LR_RES_BYTES] = nrows ? coff[cut] : 0;
}

#endif
