/*
 * sre_lines_distinct.h — the rules of the line distinct (sre_hip_distinct_lines): which keys
 * qualify, which lines of a key the call picks, which lane of a wave sends a slot's highest line, and what the per-line
 * arrays hold.  The kernels (sre_hip_lines_distinct.hip) and the CPU model (tests/lines_distinct_sim.cpp) compile this
 * text; nothing here touches memory except through its arguments.
 *
 * Behind the tally's insert (sre_lines_tally.h) over the key table every keyed line has its SLOT (SRE_LT_NONE: no key, or
 * a search the overflow flag stopped), and a slot has the FIRST line of its key (the table's final word) and the key's
 * COUNT.  The LAST line of a key is a third run of words, zero before: every keyed line sends its number to an atomic
 * maximum of its slot's word, so the final word is the key's highest line whatever the order of arrival, as the minimum
 * makes the first line.  A wave groups its lanes by slot first (the route's wave rule on the slot numbers: lowest
 * remaining lane, ballot of the lanes with its slot, drop them) and only the HIGHEST lane of a group sends, the group's
 * highest line: one atomic per distinct slot of a wave.
 *
 * The pick pass then reads the three runs with plain loads, behind the kernel boundary, and keeps or clears the filter's
 * per-line value: sre_ld_picks is the whole rule.
 */
#ifndef SRE_LINES_DISTINCT_H
#define SRE_LINES_DISTINCT_H

#include <stdint.h>
#include "sre_lines_tally.h"

#define SRE_LD_THREADS  256u

/* `which` (SRE_HIP_DISTINCT_*) */
enum { SRE_LD_FIRST = 0, SRE_LD_LAST = 1, SRE_LD_EVERY = 2 };

/* the arguments the C call refuses: min 0, a max below min (0: no upper bound) */
SRE_LG_FN bool
sre_ld_range_ok(uint64_t min_count, uint64_t max_count)
{
    return min_count != 0 && (max_count == 0 || max_count >= min_count);
}

/* a key of `count` lines QUALIFIES */
SRE_LG_FN bool
sre_ld_qualifies(uint64_t min_count, uint64_t max_count, uint64_t count)
{
    return min_count <= count && (max_count == 0 || count <= max_count);
}

/* is the keyed line `line` SELECTED?  first, last, count: of its key (last is read for SRE_LD_LAST only).  The line is
 * PICKED when its key qualifies and it is the line `which` names; invert selects the keyed lines that are not picked */
SRE_LG_FN bool
sre_ld_picks(int which, uint64_t min_count, uint64_t max_count, bool invert, uint64_t line, uint64_t first, uint64_t last,
             uint64_t count)
{
    const bool named = which == SRE_LD_FIRST ? line == first : which == SRE_LD_LAST ? line == last : true;
    const bool picked = named && sre_ld_qualifies(min_count, max_count, count);
    return picked != invert;
}

/* a qualifying key is counted once, at its first line */
SRE_LG_FN bool
sre_ld_counts_key(uint64_t min_count, uint64_t max_count, uint64_t line, uint64_t first, uint64_t count)
{
    return line == first && sre_ld_qualifies(min_count, max_count, count);
}

/* the last pass's wave rule: of the ballot m of a group (the lanes of one slot, m != 0) the highest lane sends */
SRE_LG_FN uint32_t
sre_ld_sender(uint64_t m)
{
    return 63u - (uint32_t) __builtin_clzll(m);
}

/* the pick pass for one line: the value the filter's scan reads (kept, or 0), *counts: the line counts a qualifying key.
 * A line without a slot reads nothing through it: Tab is asked only for a slot below the table's size.  Tab:
 *   tab.first(slot)   the table's word      tab.count(slot)   the slot's count
 *   tab.last(slot)    the third run's word (asked for SRE_LD_LAST only) */
template <class Tab>
SRE_LG_FN uint64_t
sre_ld_value(const Tab &tab, int which, uint64_t min_count, uint64_t max_count, bool invert, uint64_t line, uint32_t slot,
             uint64_t value, bool *counts)
{
    *counts = false;
    if (slot == SRE_LT_NONE) return 0;
    const uint64_t first = tab.first(slot), count = tab.count(slot);
    const uint64_t last = which == SRE_LD_LAST ? tab.last(slot) : 0;
    *counts = sre_ld_counts_key(min_count, max_count, line, first, count);
    return sre_ld_picks(which, min_count, max_count, invert, line, first, last, count) ? value : 0;
}

/* the per-line arrays: the count of the line's key, 0 without one; the key's first line, -1 without one */
template <class Tab>
SRE_LG_FN uint64_t
sre_ld_keycount(const Tab &tab, uint32_t slot)
{
    return slot == SRE_LT_NONE ? 0 : tab.count(slot);
}

template <class Tab>
SRE_LG_FN int64_t
sre_ld_keyline(const Tab &tab, uint32_t slot)
{
    return slot == SRE_LT_NONE ? -1 : (int64_t) tab.first(slot);
}

#endif
