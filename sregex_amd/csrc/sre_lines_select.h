/*
 * sre_lines_select.h — the select rules of the line sinks: which lines of line mode and of
 * the filter are rows, and the two words val / start of every entry of the extract's and the substitute's tables, from
 * the record of a line.  The select kernels (sre_hip_lines_gather.hip), the compaction (sre_hip_lines.hip), the host
 * route of the batched API and the CPU models (tests/lines_extract_sim.cpp, tests/lines_subst_sim.cpp) compile this
 * text; nothing here touches memory except through its arguments.
 *
 * A record is rc and the ovector behind it: rec[2 + 2 g] / rec[3 + 2 g] = the span of group g relative to the line.  A
 * line is a HIT when rc != declined, an error rc included.  Nothing but a span inside its own line (0 <= a <= b <= len)
 * ever becomes an offset: every other span counts as unset, so no record can send a later pass outside the buffer.
 */
#ifndef SRE_LINES_SELECT_H
#define SRE_LINES_SELECT_H

#include <stdint.h>
#include "sre_lines_gather.h"

#define SRE_EXTRACT_MAX_FIELDS 32u
/* the chosen capture groups: field f of a row is group g[f] of the line's record */
typedef struct {
    uint32_t k;
    uint16_t g[SRE_EXTRACT_MAX_FIELDS];
} sre_extract_groups_t;

#define SRE_SUBST_MAX_PIECES  30u
#define SRE_SUBST_MAX_LITERAL 4096u
/* the parsed template: piece q is capture group g[q] of the line's record, or with g[q] < 0 the len[q] bytes at off[q]
 * of the call's literal block */
typedef struct {
    uint32_t np;
    int16_t  g[SRE_SUBST_MAX_PIECES];
    uint16_t off[SRE_SUBST_MAX_PIECES];
    uint16_t len[SRE_SUBST_MAX_PIECES];
} sre_subst_pieces_t;

/* the row rule: mode 0 selects the hits, 1 the other lines, 2 every line (line mode: 0, or 2 with `all`), whose
 * records are not read */
SRE_LG_FN bool
sre_sel_row(const int64_t *rec, int64_t declined, int mode)
{
    return mode == 2 || (rec[0] != declined) != (mode == 1);
}

/* the clamp: a span counts only inside its own line */
SRE_LG_FN bool
sre_sel_inside(int64_t a, int64_t b, uint64_t len)
{
    return a >= 0 && b >= a && (uint64_t) b <= len;
}

/* group g of a hit, inside the line: [*a, *b).  The words of a line without a hit are not read */
SRE_LG_FN bool
sre_sel_span(const int64_t *rec, bool hit, uint32_t g, uint64_t len, int64_t *a, int64_t *b)
{
    *a = hit ? rec[2 + 2 * g] : -1;
    *b = hit ? rec[3 + 2 * g] : -1;
    return sre_sel_inside(*a, *b, len);
}

/* the extract's entry f of k, group g, of the line [st, st + len): val = field length + 1 for every entry of a selected
 * line (a hit, or every line with `all`), else 0; start = the field's source offset, the line's start under UNSET for
 * an unset field, under FIRST / LAST for the first / last entry of the line */
SRE_LG_FN void
sre_sel_extract_entry(const int64_t *rec, int64_t declined, int all, uint64_t st, uint64_t len, uint32_t f, uint32_t k, uint32_t g,
                      uint64_t *val, uint64_t *start)
{
    const bool     hit = rec[0] != declined;
    /* (sre_sel_span without its branch: with no hit the two words come from the head of the record, which is read
     * anyway, so on the device the loads of g and of rc leave together and the span's load waits for nothing else) */
    const int64_t *p = hit ? rec + 2 + 2 * g : rec;
    const int64_t  x = p[0], y = p[1], a = hit ? x : -1, b = hit ? y : -1;
    const bool     set = sre_sel_inside(a, b, len);
    *val = (hit || all) ? (set ? (uint64_t) (b - a) : 0) + 1 : 0;
    *start = (set ? st + (uint64_t) a : st | SRE_LG_ENTRY_UNSET) | (f == 0 ? SRE_LG_ENTRY_FIRST : 0)
             | (f + 1 == k ? SRE_LG_ENTRY_LAST : 0);
}

/* the substitute's entry f of P = pc->np + 2.  f = 0 is the line's text in front of the match [m0, m1) = group 0,
 * f = 1 .. P - 2 the template's pieces (a literal: its length and its offset in the literal block; a group: as the
 * extract's field, without the byte behind it), f = P - 1 the text behind the match and the delimiter.  A selected line
 * without a match, or whose group 0 does not lie inside the line, is copied whole: its text is the first entry (under
 * UNSET), its pieces are empty.  Every val of an unselected line is 0 */
SRE_LG_FN void
sre_sel_subst_entry(const int64_t *rec, int64_t declined, int all, uint64_t st, uint64_t len, uint32_t f,
                    const sre_subst_pieces_t *pc, uint64_t *val, uint64_t *start)
{
    const uint32_t P = pc->np + 2;
    const bool     hit = rec[0] != declined;
    int64_t        m0, m1;
    const bool     ok = sre_sel_span(rec, hit, 0, len, &m0, &m1);
    uint64_t       v, w;
    if (f == 0) {
        v = ok ? (uint64_t) m0 : len;
        w = st | SRE_LG_ENTRY_FIRST | (ok ? 0 : SRE_LG_ENTRY_UNSET);
    } else if (f + 1 == P) {
        v = (ok ? len - (uint64_t) m1 : 0) + 1;
        w = (ok ? st + (uint64_t) m1 : st + len) | SRE_LG_ENTRY_LAST;
    } else if (pc->g[f - 1] < 0) {
        v = ok ? pc->len[f - 1] : 0;
        w = (uint64_t) pc->off[f - 1] | SRE_LG_ENTRY_LITERAL;
    } else {
        int64_t    a, b;
        const bool set = sre_sel_span(rec, ok, (uint32_t) pc->g[f - 1], len, &a, &b);
        v = set ? (uint64_t) (b - a) : 0;
        w = set ? st + (uint64_t) a : st | SRE_LG_ENTRY_UNSET;
    }
    *val = (hit || all) ? v : 0;
    *start = w;
}

#endif
