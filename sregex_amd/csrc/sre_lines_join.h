/*
 * sre_lines_join.h — the rules of the key map and of the line join (sre_hip_keyset_create_map, sre_hip_join_lines,
 * DESIGN.md §4.11.10): how the fields of a dictionary row part into key fields and value columns, and the entries a line
 * gets in the join's table.  The kernels (sre_hip_lines_keyset.hip), the gather and the index (sre_hip_lines_gather.hip)
 * and the CPU model (tests/lines_join_sim.cpp) compile this text; nothing here touches memory except through its
 * arguments.
 *
 * A KEY MAP is a key set (sre_lines_keyset.h) whose rows carry V = nfields - nkeys VALUE COLUMNS behind the nkeys key
 * fields.  A row is split once by the field rule over all nfields fields; the first nkeys entries go to the key arrays
 * (row r, field f is entry r * nkeys + f, what the insert and the probe read), the others to two arrays of their own
 * (row r, column c is entry r * V + c).  The values of a key are those of its id, the LOWEST row that carries it.
 *
 * The JOIN TABLE has P = 1 + C entries per line, C the chosen columns, e = line * P + f, in the two words of the
 * extract's table (val, start under the flag bits of sre_lines_gather.h):
 *   f = 0       the line: val = len + 1, start = the line's source offset | FIRST;
 *   f = 1 + c   column cols[c] of the line's dictionary row: val = the value's length + 1, start = the value's offset in
 *               the set's copy of the dictionary | LITERAL; a selected line WITHOUT a dictionary row has val = 1 and
 *               start = UNSET (no text: the gather reads nothing for it);
 *   the last entry carries LAST as well.
 * Every val of a line that is not selected is 0.  Every entry of a selected line takes at least one byte, the jsep or the
 * delimiter behind it, so the extract's offset scan, its whole-row cut and its count of lines apply with k = P.
 */
#ifndef SRE_LINES_JOIN_H
#define SRE_LINES_JOIN_H

#include <stdint.h>
#include "sre_lines_keyset.h"
#include "sre_lines_select.h"     /* SRE_EXTRACT_MAX_FIELDS: a row of the join table is a row of the extract's */

#define SRE_LJ_MAX_VALUES   31u         /* chosen columns of a call; P = 1 + columns <= SRE_EXTRACT_MAX_FIELDS */

/* the chosen value columns, in output order; any order, repeats allowed */
typedef struct {
    uint32_t n;
    uint8_t  col[SRE_LJ_MAX_VALUES];
} sre_lj_cols_t;

/* where entry x of nfields of a row goes: key field x of nkeys, or value column x - nkeys */
SRE_LG_FN void
sre_lj_part(const uint64_t *fstart, const uint64_t *flen, uint32_t nfields, uint32_t nkeys, uint64_t *kstart, uint64_t *klen,
            uint64_t *vstart, uint64_t *vlen)
{
    for (uint32_t x = 0; x < nfields; x++) {
        if (x < nkeys) {
            kstart[x] = fstart[x];
            klen[x] = flen[x];
        } else {
            vstart[x - nkeys] = fstart[x];
            vlen[x - nkeys] = flen[x];
        }
    }
}

/* the selection rule: the inner join takes the members, the left outer join (all) every line */
SRE_LG_FN bool
sre_lj_selected(bool keyed, int64_t id, bool all)
{
    return all || (keyed && id >= 0);
}

/* the P = 1 + c.n entries of the line [st, st + len) into val[0 .. P) and start[0 .. P).  id: the probe's answer for a
 * keyed line (a row of the dictionary, or SRE_LK_NOT_MEMBER); vstart / vlen: the map's value arrays of nvalues columns
 * per row, read only for a selected line with a row */
SRE_LG_FN void
sre_lj_entries(bool keyed, int64_t id, bool all, uint64_t st, uint64_t len, const uint64_t *vstart, const uint64_t *vlen,
               uint32_t nvalues, const sre_lj_cols_t &c, uint64_t *val, uint64_t *start)
{
    const bool sel = sre_lj_selected(keyed, id, all), row = keyed && id >= 0;
    val[0] = sel ? len + 1 : 0;
    start[0] = st | SRE_LG_ENTRY_FIRST;
    for (uint32_t x = 0; x < c.n; x++) {
        const uint64_t e = row ? (uint64_t) id * nvalues + c.col[x] : 0;
        const uint64_t last = x + 1 == c.n ? SRE_LG_ENTRY_LAST : 0;
        val[1 + x] = sel ? (row ? vlen[e] : 0) + 1 : 0;
        start[1 + x] = (row ? vstart[e] | SRE_LG_ENTRY_LITERAL : SRE_LG_ENTRY_UNSET) | last;
    }
}

#endif
