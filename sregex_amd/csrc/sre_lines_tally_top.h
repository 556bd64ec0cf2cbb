/*
 * sre_lines_tally_top.h — the rules of the ordered tally (sre_hip_tally_top_lines): the order value and
 * the class of a key from its count and its aggregates, what a workgroup of the order-values pass sends to the four words of
 * the call, the range a call may have, the rows in front of the limit, the entries of the ordered table and the index row.
 * The kernels (sre_hip_lines_tally_top.hip), the host code of the batched API and the CPU model
 * (tests/lines_tally_top_sim.cpp) compile this text; nothing here touches memory except through its arguments.  The tally
 * and its aggregates are sre_lines_tally.h's and sre_lines_sums.h's; the totals, their flush, the sort key, the digit, the
 * pass count and the limit are the line sort's (sre_lines_sort.h), over KEYS in the place of lines.
 *
 * An ITEM of the sort is a key of the tally: its "line" is the key's number in first-appearance order (below 2^30), its
 * VALUE the order value, its CLASS SRE_LSO_NUMBER when the key is ORDERED and SRE_LSO_TEXT when it is not.  The passes run
 * with all = 1, so a key that is not ordered has the sort key RANGE + 1 and comes behind every ordered key in both
 * directions, in first-appearance order, as the sort's rule for unnumbered lines has it.
 *
 * The ORDER VALUE of key k under `by`, from count[k] and the aggregate a = agg[k * v + by_col]:
 *   SRE_LTT_COUNT   count[k]     always ordered
 *   SRE_LTT_N       a.n          always ordered
 *   SRE_LTT_SUM     a.sum        ordered when a.n != 0 (the sum as the tally stores it, after wrapping)
 *   SRE_LTT_MIN     a.min        ordered when a.n != 0
 *   SRE_LTT_MAX     a.max        ordered when a.n != 0
 * A key that is not ordered has the value 0.
 *
 * The TOTALS are the sort's four words (sre_lso_totals_t): nkeyed counts the keys, nnumbered the ordered ones, vmin / vmax
 * the extremes of their values.  A workgroup of the order-values pass owns SRE_LTT_KEYS keys and sends what sre_lso_flush
 * sends: at most one add per count, one minimum and one maximum.
 *
 * The RANGE.  The sort reserves the all-ones key (SRE_LSO_DROPPED) and gives the keys that are not ordered RANGE + 1, so a
 * call may have RANGE = vmax - vmin up to 2^64 - 3 (SRE_LTT_MAX_RANGE).  Counts, n, minima and maxima stay far below; only
 * sums that wrapped reach it.
 */
#ifndef SRE_LINES_TALLY_TOP_H
#define SRE_LINES_TALLY_TOP_H

#include <stdint.h>
#include "sre_lines_tally.h"
#include "sre_lines_sort.h"

/* the values of `by`: SRE_HIP_TOP_* of sregex_hip.h */
#define SRE_LTT_COUNT       0
#define SRE_LTT_SUM         1
#define SRE_LTT_MIN         2
#define SRE_LTT_MAX         3
#define SRE_LTT_N           4

/* a workgroup of the order-values pass is a workgroup of the sort's values pass: 256 lanes x 4 keys */
#define SRE_LTT_THREADS     SRE_LSO_THREADS
#define SRE_LTT_PER_LANE    SRE_LSO_PER_LANE
#define SRE_LTT_KEYS        SRE_LSO_LINES

#define SRE_LTT_MAX_RANGE   (~(uint64_t) 0 - 2)                         /* 2^64 - 3 */

/* words of an index row for k key fields: the extract's 4 + 2 k, the key's number and its order value */
SRE_LG_FN uint32_t sre_ltt_index_words(uint32_t k) { return 4u + 2u * k + 2u; }

/* `by` names an order, and by_col a column the call has (v value columns) */
SRE_LG_FN bool
sre_ltt_by_ok(int by, uint64_t by_col, uint64_t v)
{
    if (by == SRE_LTT_COUNT) return by_col == 0;
    if (by != SRE_LTT_SUM && by != SRE_LTT_MIN && by != SRE_LTT_MAX && by != SRE_LTT_N) return false;
    return by_col < v;
}

/* the class of a key and its order value; a: the aggregate of column by_col (not read for SRE_LTT_COUNT) */
SRE_LG_FN int32_t
sre_ltt_order(int by, uint64_t count, const sre_ls_agg_t *a, int64_t *value)
{
    *value = 0;
    if (by == SRE_LTT_COUNT) {
        *value = (int64_t) count;
        return SRE_LSO_NUMBER;
    }
    if (by == SRE_LTT_N) {
        *value = (int64_t) a->n;
        return SRE_LSO_NUMBER;
    }
    if (a->n == 0) return SRE_LSO_TEXT;
    *value = by == SRE_LTT_SUM ? a->sum : by == SRE_LTT_MIN ? a->min : a->max;
    return SRE_LSO_NUMBER;
}

/* the range of the ordered keys fits the sort's keys */
SRE_LG_FN bool
sre_ltt_range_ok(uint64_t nordered, int64_t vmin, int64_t vmax)
{
    return sre_lso_range(nordered, vmin, vmax) <= SRE_LTT_MAX_RANGE;
}

/* the rows of the limited output */
SRE_LG_FN uint64_t sre_ltt_rows(uint64_t nkeys, uint64_t limit) { return sre_lso_limited(nkeys, limit); }

/* the digit passes of a call over nkeys keys, nordered of them ordered */
SRE_LG_FN uint32_t
sre_ltt_passes(uint64_t nkeys, uint64_t nordered, int64_t vmin, int64_t vmax)
{
    return sre_lso_passes(nkeys, nordered, sre_lso_range(nordered, vmin, vmax), 1);
}

/* entry f of the k entries of rank r in the ordered table, from entry e = line * k + f of the scanned entry table
 * (off[0 .. ], start[]) of the key's first line: the start word with its flags, and the value len + 1 */
SRE_LG_FN void
sre_ltt_entry(const uint64_t *off, const uint64_t *start, uint64_t e, uint64_t *cstart, uint64_t *cval)
{
    *cstart = start[e];
    *cval = off[e + 1] - off[e];
}

/* the index row of rank r: the extract's row of the key's first line `line` = [lstart, lstart + llen) with [3] the row's
 * offset in THIS output, then the key's number and its order value.  cstart / coff: the ordered table, scanned */
SRE_LG_FN void
sre_ltt_index_row(uint64_t line, uint64_t lstart, uint64_t llen, const uint64_t *cstart, const uint64_t *coff, uint64_t r,
                  uint32_t k, uint64_t key, int64_t value, int64_t *row)
{
    const uint64_t e = r * k;
    row[0] = (int64_t) line;
    row[1] = (int64_t) lstart;
    row[2] = (int64_t) llen;
    row[3] = (int64_t) coff[e];
    for (uint32_t x = 0; x < k; x++) {
        const uint64_t w = cstart[e + x];
        const bool     unset = (w & SRE_LG_ENTRY_UNSET) != 0;
        row[4 + 2 * x] = unset ? -1 : (int64_t) (w & SRE_LG_ENTRY_START);
        row[5 + 2 * x] = unset ? -1 : (int64_t) (coff[e + x + 1] - coff[e + x] - 1);
    }
    row[4 + 2 * k] = (int64_t) key;
    row[5 + 2 * k] = value;
}

#endif
