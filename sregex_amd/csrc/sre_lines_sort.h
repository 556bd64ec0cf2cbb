/*
 * sre_lines_sort.h — the rules of the line sort (sre_hip_sort_lines): the value and the class of a line
 * from its entry of the value table, what a workgroup of the values pass sends to the four words of the call, the sort key
 * of a line from its value, the largest key and the number of passes, the digit a pass looks at and the index row.  The kernels (sre_hip_lines_sort.hip), the host code of the batched API and the
 * CPU model (tests/lines_sort_sim.cpp) compile this text; nothing here touches memory except through its arguments.  The
 * number rule is the tally's (sre_ls_number, sre_lines_sums.h); the slot geometry, the slot prefix, the count index, the
 * cut and the result words are the route's (sre_lines_route.h); the pass formula, the rank rule of a slot and the entry of the compact table are
 * the route by key's (sre_lines_route_key.h).
 *
 * The CLASS of a line, from entry `line` of the value table of the ONE sort group (sre_lines_sums.h, V = 1):
 *   SRE_LSO_NUMBER    1   the line has a match and the group's text is a number; its VALUE is that number;
 *   SRE_LSO_TEXT     -1   the line has a match, the group is unset, empty or no number; value 0;
 *   SRE_LSO_NOMATCH  -2   the line has no match (val == 0 under the filter's row rule); value 0.
 *
 * The TOTALS of the call, four words: the keyed lines (classes 1 and -1), the numbered lines, the minimum and the maximum
 * of the values (int64 in uint64 words, INT64_MAX / INT64_MIN before).  A workgroup of the values pass owns SRE_LSO_LINES
 * lines, reduces the four over its lanes and sends at most ONE add per count, one minimum and one maximum; a workgroup
 * without a keyed line sends nothing, one without a numbered line only the keyed count.  Add, minimum and maximum are
 * commutative and associative, so the words do not depend on the order of the workgroups.
 *
 * The SORT KEY of a line, an unsigned 64-bit word, from the totals (vmin, vmax) the host read: a numbered line has
 * v - vmin ascending, vmax - v descending, computed in uint64_t; RANGE = vmax - vmin (0 without a numbered line).  18
 * digits keep |v| below 10^18 and RANGE below 2^61.  Under ALL every other line has RANGE + 1, which therefore fits;
 * without ALL it is dropped (SRE_LSO_DROPPED, all ones: no key).  The largest key that occurs is RANGE, or RANGE + 1 under
 * ALL when a line is not numbered; the passes are sre_lrk_passes of it with 8-bit digits: 1 to 8.
 *
 * An ITEM is two words that move together: the key (64 bits) and the line (32 bits; at most SRE_LRK_MAX_LINES lines).  The
 * sort is the route by key's LSD radix sort, one 8-bit digit of the KEY per pass, the digit shift pass * 8 up to 56: count
 * over the keys, the filter's scan, scatter of key and line to the same rank of the other pair of arrays.  Pass 0 makes the
 * items from the per-line values and classes in line order and drops the unselected.  Every pass is stable, so after the
 * last the items are sorted by (key, line): value order, equal values in line order, in both directions, the lines that
 * are not numbered behind all numbered ones in line order.
 *
 * Behind the sort the first nout = min(limit, nsel) ranks (limit == 0: all) make the compact table (sre_lrk_entry), the
 * filter's scan cuts it at out_cap, the finish leaves SRE_LSO_RES_WORDS words, the extract's gather writes the rows.
 */
#ifndef SRE_LINES_SORT_H
#define SRE_LINES_SORT_H

#include <stdint.h>
#include "sre_lines_sums.h"
#include "sre_lines_route_key.h"

#define SRE_LSO_NUMBER      1
#define SRE_LSO_TEXT        (-1)
#define SRE_LSO_NOMATCH     (-2)

#define SRE_LSO_THREADS     256u
#define SRE_LSO_PER_LANE    4u
#define SRE_LSO_LINES       (SRE_LSO_THREADS * SRE_LSO_PER_LANE)       /* 1024 lines a workgroup of the values pass */

#define SRE_LSO_DIGIT_BITS  8u
#define SRE_LSO_MAX_PASSES  8u
#define SRE_LSO_DROPPED     (~(uint64_t) 0)         /* the key of a line that is not selected (a key stays below 2^62) */

#define SRE_LSO_INDEX_WORDS 6u

/* the words the finish pass leaves for the host: the route's four (sre_lr_result) */
#define SRE_LSO_RES_NSEL     SRE_LR_RES_NSEL
#define SRE_LSO_RES_NEED     SRE_LR_RES_NEED
#define SRE_LSO_RES_WRITTEN  SRE_LR_RES_WRITTEN
#define SRE_LSO_RES_BYTES    SRE_LR_RES_BYTES
#define SRE_LSO_RES_WORDS    SRE_LR_RES_WORDS

/* the four totals of a call, or of a part of it */
typedef struct {
    uint64_t nkeyed;
    uint64_t nnumbered;
    int64_t  vmin;
    int64_t  vmax;
} sre_lso_totals_t;

SRE_LG_FN sre_lso_totals_t
sre_lso_identity(void)
{
    sre_lso_totals_t t;
    t.nkeyed = 0;
    t.nnumbered = 0;
    t.vmin = INT64_MAX;
    t.vmax = INT64_MIN;
    return t;
}

/* the class and the value of line `line`; vals: the value table (sre_lines_sums.h) with one column */
template <class Vals>
SRE_LG_FN int32_t
sre_lso_line(const Vals &vals, uint64_t line, int64_t *value)
{
    const uint64_t val = vals.val(line, 0), raw = vals.raw(line, 0);
    *value = 0;
    if (val == 0) return SRE_LSO_NOMATCH;
    if ((raw & SRE_LG_ENTRY_UNSET) == 0 && sre_ls_number(vals, raw & SRE_LG_ENTRY_START, val - 1, value)) return SRE_LSO_NUMBER;
    *value = 0;
    return SRE_LSO_TEXT;
}

/* what one line contributes to the totals */
SRE_LG_FN sre_lso_totals_t
sre_lso_single(int32_t cls, int64_t value)
{
    sre_lso_totals_t t = sre_lso_identity();
    if (cls != SRE_LSO_NOMATCH) t.nkeyed = 1;
    if (cls == SRE_LSO_NUMBER) {
        t.nnumbered = 1;
        t.vmin = value;
        t.vmax = value;
    }
    return t;
}

SRE_LG_FN sre_lso_totals_t
sre_lso_merge(sre_lso_totals_t a, sre_lso_totals_t b)
{
    a.nkeyed += b.nkeyed;
    a.nnumbered += b.nnumbered;
    a.vmin = b.vmin < a.vmin ? b.vmin : a.vmin;
    a.vmax = b.vmax > a.vmax ? b.vmax : a.vmax;
    return a;
}

/* a workgroup's merged totals go to memory: nothing without a keyed line, the minimum and the maximum only with a number.
 * Mem: mem.add_keyed(v)  mem.add_numbered(v)  mem.min(v)  mem.max(v), atomics on the call's four words */
template <class Mem>
SRE_LG_FN void
sre_lso_flush(Mem &mem, const sre_lso_totals_t &t)
{
    if (t.nkeyed == 0) return;
    mem.add_keyed(t.nkeyed);
    if (t.nnumbered == 0) return;
    mem.add_numbered(t.nnumbered);
    mem.min(t.vmin);
    mem.max(t.vmax);
}

/* RANGE from the totals the host read */
SRE_LG_FN uint64_t
sre_lso_range(uint64_t nnumbered, int64_t vmin, int64_t vmax)
{
    return nnumbered ? (uint64_t) vmax - (uint64_t) vmin : 0;
}

/* the lines the flags select */
SRE_LG_FN uint64_t sre_lso_selected(uint64_t nlines, uint64_t nnumbered, int all) { return all ? nlines : nnumbered; }

/* the largest key among the selected lines */
SRE_LG_FN uint64_t
sre_lso_max_key(uint64_t nlines, uint64_t nnumbered, uint64_t range, int all)
{
    return all && nnumbered < nlines ? range + 1 : range;
}

/* the digit passes of a call: none when nothing is selected */
SRE_LG_FN uint32_t
sre_lso_passes(uint64_t nlines, uint64_t nnumbered, uint64_t range, int all)
{
    if (sre_lso_selected(nlines, nnumbered, all) == 0) return 0;
    return sre_lrk_passes(sre_lso_max_key(nlines, nnumbered, range, all), SRE_LSO_DIGIT_BITS);
}

/* the sort key of a line of class cls and value v */
SRE_LG_FN uint64_t
sre_lso_key(int32_t cls, int64_t v, int64_t vmin, int64_t vmax, uint64_t range, int desc, int all)
{
    if (cls == SRE_LSO_NUMBER) return desc ? (uint64_t) vmax - (uint64_t) v : (uint64_t) v - (uint64_t) vmin;
    return all ? range + 1 : SRE_LSO_DROPPED;
}

/* the digit of a key in a pass: the shift is pass * 8, up to 56, of the 64-bit key */
SRE_LG_FN uint32_t
sre_lso_digit(uint64_t key, uint32_t pass)
{
    return (uint32_t) ((key >> (pass * SRE_LSO_DIGIT_BITS)) & ((1u << SRE_LSO_DIGIT_BITS) - 1u));
}

/* the rows of the full output */
SRE_LG_FN uint64_t sre_lso_limited(uint64_t nsel, uint64_t limit) { return limit != 0 && limit < nsel ? limit : nsel; }

/* the result words from the scanned table coff[0 .. nout] (not read when nout == 0): the route's rule under the sort's name,
 * which code compiled against this header may call */
SRE_LG_FN void
sre_lso_result(const uint64_t *coff, uint64_t nout, uint64_t out_cap, uint64_t *res)
{
    sre_lr_result(coff, nout, out_cap, res);
}

/* the index row of rank r, whose line is `line` with value and class as the values pass left them */
SRE_LG_FN void
sre_lso_index_row(uint64_t line, const uint64_t *cstart, const uint64_t *coff, uint64_t r, int64_t value, int32_t cls, int64_t *row)
{
    const uint64_t o = coff[r];
    row[0] = (int64_t) line;
    row[1] = (int64_t) (cstart[r] & SRE_LG_ENTRY_START);
    row[2] = (int64_t) (coff[r + 1] - o - 1);
    row[3] = (int64_t) o;
    row[4] = cls == SRE_LSO_NUMBER ? value : 0;
    row[5] = cls;
}

#endif
