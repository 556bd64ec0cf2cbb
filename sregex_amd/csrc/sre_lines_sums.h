/*
 * sre_lines_sums.h — the rules of the line tally's sums (sre_hip_tally_sums_lines): when the text of a
 * field is a number and which, what a line contributes to the aggregate of its key, how two contributions merge, and
 * what a wave sends to memory.  The kernel (sre_hip_lines_tally.hip), the host's sre_hip_tally_number and the CPU model
 * (tests/lines_sums_sim.cpp) compile this text; nothing here touches memory except through the Text, Vals and Mem arguments.
 *
 * The NUMBER RULE.  A text is a number when it is an optional single '-' followed by 1 to SRE_LS_MAX_DIGITS bytes that
 * are all '0' .. '9', and nothing else; its value is the decimal value, negated behind '-'.  18 digits stay below 10^18,
 * inside int64 with room to spare, so no value overflows; only a sum can wrap.
 *
 * The VALUE TABLE is a second entry table of the extract's select pass (sre_lines_gather.h) over the V value groups:
 * entry e = line * V + c has val[e] = field length + 1 (0: the line is not selected) and start[e] = the field's source
 * offset under the flag bits.  Vals:
 *   vals.v                  value columns per line
 *   vals.val(line, c)       val[e]
 *   vals.raw(line, c)       start[e]
 *   vals.byte(at)           the source byte at offset `at`
 * An unselected line, an unset group (SRE_LG_ENTRY_UNSET: a line without a match under SRE_HIP_LINES_ALL has nothing
 * but those) and a text that is not a number contribute nothing.
 *
 * The AGGREGATE of a key and a column is (sum modulo 2^64, min, max, n) over the numbers of the key's lines.  All four
 * are commutative and associative, the sum because it wraps, so neither the order of the lines nor the way they are
 * bracketed shows in the result.  The identity is (0, INT64_MAX, INT64_MIN, 0): the row of a key none of whose lines
 * holds a number.
 *
 * The WAVE RULE.  A lane per line; a lane takes part when its line has a slot and the key number of the slot is below
 * `rows` = min(sums_cap, nkeys).  The wave groups its lanes by KEY NUMBER with the route's rule (sre_lr_leader, a ballot
 * on equality), one turn per distinct key held by more than one lane; per column the members' contributions are merged
 * across the lanes (sre_ls_merge, the others hold the identity) and the group's lowest lane sends the result: sre_ls_flush
 * makes at most ONE add, minimum, maximum and add, and none at all when the group holds no number.  A lane alone with
 * its key sends its own contribution the same way.  Mem:
 *   mem.add_sum(idx, v)  mem.min(idx, v)  mem.max(idx, v)  mem.add_n(idx, v)      atomics on aggregate idx = key * V + c
 */
#ifndef SRE_LINES_SUMS_H
#define SRE_LINES_SUMS_H

#include <stdint.h>
#include "sre_lines_gather.h"
#include "sre_lines_route.h"
#include "sre_lines_tally.h"

#define SRE_LS_THREADS      256u
#define SRE_LS_MAX_VALUES   8u
#define SRE_LS_MAX_DIGITS   18u
/* COPIES.  One cache line takes about 90 atomics a microsecond, whoever sends them, so the waves do not all send to the
 * caller's rows: wave w sends to copy w % copies of them, and a last pass merges the copies into the caller's rows
 * (sre_ls_merge again, so the result is the same whatever the number of copies).  As many copies as fit
 * SRE_LS_COPY_BYTES, at most SRE_LS_MAX_COPIES; one copy means the caller's rows themselves */
#define SRE_LS_MAX_COPIES   64u
#define SRE_LS_COPY_BYTES   ((uint64_t) 8 << 20)

/* the layout of sre_hip_tally_sum_t */
typedef struct {
    int64_t  sum;
    int64_t  min;
    int64_t  max;
    uint64_t n;
} sre_ls_agg_t;

SRE_LG_FN sre_ls_agg_t
sre_ls_identity(void)
{
    sre_ls_agg_t a;
    a.sum = 0;
    a.min = INT64_MAX;
    a.max = INT64_MIN;
    a.n = 0;
    return a;
}

/* the contribution of one line: the identity, or its number once */
SRE_LG_FN sre_ls_agg_t
sre_ls_single(bool is_number, int64_t value)
{
    sre_ls_agg_t a = sre_ls_identity();
    if (is_number) {
        a.sum = value;
        a.min = value;
        a.max = value;
        a.n = 1;
    }
    return a;
}

SRE_LG_FN sre_ls_agg_t
sre_ls_merge(sre_ls_agg_t a, sre_ls_agg_t b)
{
    a.sum = (int64_t) ((uint64_t) a.sum + (uint64_t) b.sum);       /* wraps */
    a.min = b.min < a.min ? b.min : a.min;
    a.max = b.max > a.max ? b.max : a.max;
    a.n += b.n;
    return a;
}

/* the number rule over the len bytes text.byte(at + j); *value is written only for a number */
template <class Text>
SRE_LG_FN bool
sre_ls_number(const Text &text, uint64_t at, uint64_t len, int64_t *value)
{
    if (len == 0 || len > SRE_LS_MAX_DIGITS + 1) return false;
    const bool     neg = text.byte(at) == '-';
    const uint32_t nd = (uint32_t) len - (neg ? 1u : 0u);
    if (nd == 0 || nd > SRE_LS_MAX_DIGITS) return false;
    uint64_t u = 0;
    for (uint32_t j = neg ? 1u : 0u; j < (uint32_t) len; j++) {
        const uint32_t d = (uint32_t) text.byte(at + j) - (uint32_t) '0';
        if (d > 9u) return false;
        u = u * 10u + d;
    }
    *value = neg ? -(int64_t) u : (int64_t) u;
    return true;
}

/* what line `line` contributes to column c */
template <class Vals>
SRE_LG_FN sre_ls_agg_t
sre_ls_line(const Vals &vals, uint64_t line, uint32_t c)
{
    const uint64_t val = vals.val(line, c), raw = vals.raw(line, c);
    int64_t        value = 0;
    const bool     is = val != 0 && (raw & SRE_LG_ENTRY_UNSET) == 0 && sre_ls_number(vals, raw & SRE_LG_ENTRY_START, val - 1, &value);
    return sre_ls_single(is, value);
}

/* does the lane of a line with this slot and (for a line with a slot) this key number take part? */
SRE_LG_FN bool
sre_ls_takes_part(uint32_t slot, uint64_t key, uint64_t rows)
{
    return slot != SRE_LT_NONE && key < rows;
}

SRE_LG_FN uint32_t
sre_ls_copies(uint64_t rows, uint32_t v)
{
    const uint64_t bytes = rows * v * 32u;
    if (bytes == 0 || bytes > SRE_LS_COPY_BYTES) return 1;
    const uint64_t fit = SRE_LS_COPY_BYTES / bytes;
    return fit > SRE_LS_MAX_COPIES ? SRE_LS_MAX_COPIES : (uint32_t) fit;
}

SRE_LG_FN uint32_t sre_ls_copy_of(uint64_t wave, uint32_t copies) { return (uint32_t) (wave % copies); }

/* the aggregate of a key's column: key * V + c */
SRE_LG_FN uint64_t sre_ls_index(uint64_t key, uint32_t v, uint32_t c) { return key * v + c; }

/* a group's merged contribution goes to memory: nothing without a number, else one access per quantity */
template <class Mem>
SRE_LG_FN void
sre_ls_flush(Mem &mem, uint64_t idx, const sre_ls_agg_t &a)
{
    if (a.n == 0) return;
    mem.add_sum(idx, a.sum);
    mem.min(idx, a.min);
    mem.max(idx, a.max);
    mem.add_n(idx, a.n);
}

#endif
