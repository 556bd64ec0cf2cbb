/*
 * sre_lines_fold.h — the block logic of the line fold (sre_hip_fold_lines): which lines start a
 * multi-line record and which byte follows each line in the output.  The kernels (sre_hip_lines_fold.hip), the CPU model
 * (tests/lines_fold_sim.cpp) and the host check (tools/asan_fold_rule.cpp) compile this text; nothing here touches memory
 * except through its arguments.  The scans, the block words and the bitmap words are sre_lines_context.h's.
 *
 * The pass runs over the MARKED bit of every line (the filter's per-line value is not 0).  With s = 0 (a marked line
 * belongs to the line in front of it) or s = 1 (SRE_LF_NEXT: a marked line continues into the following line)
 *   nh(j)   = j == 0 || !marked(j - s)                           line j is a NATURAL HEAD
 *   h(i)    = the largest j <= i with nh(j)
 *   head(i) = max_lines ? (i - h(i)) % max_lines == 0 : h(i) == i
 * so an unmarked line k GENERATES the natural head k + s.  Both directions are scans of sre_lines_context.h over the heads
 * the lines generate: p the P word (index + 1) of the nearest natural head at or in front of a line, a forward maximum, q
 * the Q word (index) of the nearest natural head behind it, a backward minimum.  A line k of workgroup b may generate the
 * head k + 1 of workgroup b + 1 (s = 1): the words belong to the lines that generate them, so the block words of b carry
 * that head to b + 1, and nothing is read across a workgroup.
 *
 * Inside a workgroup the words are 32-bit and relative to its first line (a head index up to SRE_LC_ITEMS, a P word up to
 * SRE_LC_ITEMS + 1); what crosses workgroups is a 64-bit line index.
 */
#ifndef SRE_LINES_FOLD_H
#define SRE_LINES_FOLD_H

#include <stdint.h>
#include "sre_lines_context.h"
#include "sre_lines_gather.h"       /* SRE_LG_ENTRY_LAST */

#define SRE_LF_FN SRE_LC_FN

#define SRE_LF_NEXT     1u      /* mode: s = 1 */
/* what the pass finds out about a line */
#define SRE_LF_HEAD     1u      /* the first line of a record */
#define SRE_LF_LAST     2u      /* the last line of a record: the delimiter follows it, not the join byte */

#define SRE_LF_ROW      5u      /* words of a row of the records table */

/* the marked bits of a lane's four lines from their values: bit k for line i0 + k, none for a line at or beyond n */
SRE_LF_FN uint32_t
sre_lf_lane_bits(const uint64_t v[SRE_LC_PER_LANE], uint64_t i0, uint64_t n)
{
    uint32_t m = 0;
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) m |= (uint32_t) (i0 + k < n && v[k] != 0) << k;
    return m;
}

/* ... and from the bitmap word that holds them (i0 is a multiple of 4, so the four bits lie in one word) */
SRE_LF_FN uint32_t
sre_lf_word_bits(uint64_t word, uint64_t i0)
{
    return (uint32_t) (word >> (i0 % 64)) & 0xFu;
}

/* lines of the lane's four that lie in the buffer */
SRE_LF_FN uint32_t
sre_lf_lane_valid(uint64_t i0, uint64_t n)
{
    return i0 >= n ? 0 : n - i0 < SRE_LC_PER_LANE ? (uint32_t) (n - i0) : SRE_LC_PER_LANE;
}

/* lane t of a workgroup with the marked bits m of its nv lines: the P word of the last natural head its lines generate and
 * the Q word of the first one, relative to the workgroup */
SRE_LF_FN void
sre_lf_lane_marks(uint32_t m, uint32_t nv, uint32_t t, uint32_t s, uint32_t *last, uint32_t *first)
{
    uint32_t l = 0, f = SRE_LC_NONE32;
    for (uint32_t k = 0; k < nv; k++) {
        if ((m >> k) & 1u) continue;
        const uint32_t j = SRE_LC_PER_LANE * t + k + s;
        l = j + 1;
        if (f == SRE_LC_NONE32) f = j;
    }
    *last = l;
    *first = f;
}

/* line i whose nearest natural head at or in front of it is h: how far it lies behind the first line of its record */
SRE_LF_FN uint64_t
sre_lf_behind(uint64_t i, uint64_t h, uint64_t max_lines)
{
    const uint64_t d = i - h;
    return max_lines == 0 || d < max_lines ? d : d % max_lines;
}

/* a head at i whose nearest natural head behind it is q (q <= n; n without one): the head behind it */
SRE_LF_FN uint64_t
sre_lf_next_head(uint64_t i, uint64_t q, uint64_t max_lines)
{
    const uint64_t len = q - i;
    return max_lines != 0 && max_lines < len ? i + max_lines : q;
}

/*
 * A lane's four lines i0 .. i0 + 3 (nv of them in the buffer of n lines) with their marked bits m and mnext, the marked
 * bit of line i0 + 4 (not looked at when that line is not in the buffer).  pe: the P word of the nearest natural head that
 * the lines in front of i0 generate, 0 without one; qe: the Q word of the nearest one the lines behind i0 + 3 generate.
 * Per line: fl its SRE_LF_* bits; aux the head behind it for a head (n for the last record), else the first line of its
 * record.  Line 0 is a head whatever generates it.
 */
SRE_LF_FN void
sre_lf_lane_lines(uint64_t i0, uint64_t n, uint32_t nv, uint32_t m, uint32_t mnext, uint32_t s, uint64_t max_lines, uint64_t pe,
                  uint64_t qe, uint32_t fl[SRE_LC_PER_LANE], uint64_t aux[SRE_LC_PER_LANE])
{
    uint64_t q[SRE_LC_PER_LANE];
    for (uint32_t k = SRE_LC_PER_LANE; k-- > 0;) {
        const bool gen = k < nv && ((m >> k) & 1u) == 0;
        if (s && gen) qe = i0 + k + 1;
        q[k] = qe < n ? qe : n;
        if (!s && gen) qe = i0 + k;
    }
    if (pe == 0) pe = 1;
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
        const uint64_t i = i0 + k;
        const bool     gen = k < nv && ((m >> k) & 1u) == 0;
        fl[k] = 0;
        aux[k] = 0;
        if (!s && gen) pe = i + 1;
        if (k < nv) {
            const uint64_t r = sre_lf_behind(i, pe - 1, max_lines);
            /* line i + 1 by the same rule: a natural head when line i + 1 - s is not marked, else r + 1 lines behind */
            const uint32_t mk = s ? (m >> k) & 1u : k + 1 < SRE_LC_PER_LANE ? (m >> (k + 1)) & 1u : mnext;
            const bool     last = i + 1 == n || mk == 0 || (max_lines != 0 && r + 1 == max_lines);
            fl[k] = (r == 0 ? SRE_LF_HEAD : 0u) | (last ? SRE_LF_LAST : 0u);
            aux[k] = r == 0 ? sre_lf_next_head(i, q[k], max_lines) : i - r;
        }
        if (s && gen) pe = i + 2;
    }
}

/* the entry of line i in the gather's table (K = 1): its value and its start word */
SRE_LF_FN uint64_t
sre_lf_entry_start(uint64_t start, uint32_t fl)
{
    return start | ((fl & SRE_LF_LAST) ? SRE_LG_ENTRY_LAST : 0);
}

/* the cut of the output at out_cap over the offset table off[0 .. n]: c = the first line whose end lies beyond out_cap (n
 * when all fit), found as the filter's finish finds it ... */
SRE_LF_FN uint64_t
sre_lf_first_beyond(const uint64_t *off, uint64_t n, uint64_t out_cap)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid + 1] > out_cap) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

/* ... and the cut itself: the first line of c's record (hbits: the head bitmap, aux as sre_lf_lane_lines leaves it) */
SRE_LF_FN uint64_t
sre_lf_cut(uint64_t c, uint64_t n, const uint64_t *hbits, const uint64_t *aux)
{
    if (c >= n || ((hbits[c / 64] >> (c % 64)) & 1u)) return c;
    return aux[c];
}

/* the row of the record whose head is line i: start = the source offset of the line, next = aux[i] */
SRE_LF_FN void
sre_lf_record_row(int64_t row[SRE_LF_ROW], uint64_t i, uint64_t next, uint64_t start, const uint64_t *off)
{
    row[0] = (int64_t) i;
    row[1] = (int64_t) (next - i);
    row[2] = (int64_t) start;
    row[3] = (int64_t) (off[next] - off[i] - 1);
    row[4] = (int64_t) off[i];
}

#endif
