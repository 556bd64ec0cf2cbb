/*
 * sre_lines_keyset.h — the rules of the key set and of the line lookup (sre_hip_keyset_create, sre_hip_lookup_lines,
 * DESIGN.md §4.11.9): how a row of the dictionary splits into fields, when a line's key equals a row's key, the
 * read-only probe of the finished table one read at a time, and what a line's key id and filter value become.  The
 * kernels (sre_hip_lines_keyset.hip), the host hash (sre_hip_keyset_hash) and the CPU model (tests/lines_keyset_sim.cpp)
 * compile this text; nothing here touches memory except through the Bytes, Keys and Mem arguments.
 *
 * The DICTIONARY is a buffer in the row format the extract and the tally write: field 0, fsep, .., field K - 1, delim.
 * Its rows are split by the split rule of line mode (a final row without delim is a row), so row r is the bytes
 * [st, end) in front of its delimiter.  A row must hold exactly K - 1 bytes equal to fsep; they end its first K - 1
 * fields.  With K == 1 nothing is split and fsep is not looked at.  The fields of row r are entries r * K + f of two
 * arrays, fstart (offset into the dictionary) and flen.
 *
 * The KEY of a row is the tuple of its field texts, the key of a line the tuple the tally defines (sre_lines_tally.h).
 * Both are read through a Keys type (k, len(i, f), byte(i, f, j)): sre_lk_dict_keys over the dictionary's entries,
 * sre_lk_line_keys over the entry table of the extract's select pass.  sre_lt_hash gives equal tuples equal hashes
 * whichever type reads them, and sre_lk_equal compares a line against a row: every length first, then the bytes.
 *
 * The TABLE is the tally's (sre_lines_tally.h): nslots words, each SRE_LT_EMPTY or a ROW NUMBER, filled by sre_lt_step
 * over the dictionary's keys, so the final word of a key's slot is the lowest row that carries it: the key's ID.  The
 * load factor is at most 1/2 (nslots >= 2 x rows).  Behind the insert's kernel boundary the table never changes: the
 * probe reads it with plain loads and writes nothing to it.  Mem of the probe:
 *   mem.load(idx)           word idx of the table
 * One call of sre_lk_probe_step makes at most ONE such read.
 */
#ifndef SRE_LINES_KEYSET_H
#define SRE_LINES_KEYSET_H

#include <stdint.h>
#include "sre_lines_tally.h"

#define SRE_LK_THREADS      256u
#define SRE_LK_ITEMS        4u                  /* lines per lane of the probe */
#define SRE_LK_MAX_ROWS     ((uint64_t) 1 << 30)
#define SRE_LK_NO_ROW       (~(uint64_t) 0)
/* key ids of the lines that have none in the set */
#define SRE_LK_NOT_MEMBER   ((int64_t) -1)      /* the line has a key, the set does not hold it */
#define SRE_LK_NO_KEY       ((int64_t) -2)      /* the line has no match and so no key */

/* slots of the table of a dictionary of `rows` rows */
SRE_LG_FN uint64_t
sre_lk_nslots(uint64_t rows)
{
    return sre_lt_nslots(rows);
}

/* the bytes [st, end) of row r of a dictionary whose row ends are ends[0 .. rows) */
SRE_LG_FN void
sre_lk_row_span(const uint64_t *ends, uint64_t r, uint64_t *st, uint64_t *end)
{
    *st = r ? ends[r - 1] + 1 : 0;
    *end = ends[r];
}

/* the field rule: the k fields of the row [st, end) into fstart[0 .. k) and flen[0 .. k); false when the row does not
 * hold exactly k - 1 bytes equal to fsep (nothing beyond entry k - 1 is written then either).  b.byte(at): byte `at`
 * of the dictionary */
template <class Bytes>
SRE_LG_FN bool
sre_lk_row_fields(const Bytes &b, uint64_t st, uint64_t end, uint32_t k, uint32_t fsep, uint64_t *fstart, uint64_t *flen)
{
    uint64_t f = 0, at = st;
    if (k > 1) {
        for (uint64_t j = st; j < end; j++) {
            if (b.byte(j) != fsep) continue;
            if (f + 1 < k) {
                fstart[f] = at;
                flen[f] = j - at;
            }
            f++;
            at = j + 1;
        }
    }
    if (f < k) {
        fstart[f] = at;
        flen[f] = end - at;
    }
    return f + 1 == k;
}

/* the dictionary's keys: row r, field f is entry r * k + f */
struct sre_lk_dict_keys {
    const uint8_t  *buf;
    const uint64_t *fstart, *flen;
    uint32_t        k;
    SRE_LG_MEMBER bool     selected(uint64_t) const { return true; }
    SRE_LG_MEMBER uint64_t len(uint64_t row, uint32_t f) const { return flen[row * k + f]; }
    SRE_LG_MEMBER uint8_t  byte(uint64_t row, uint32_t f, uint64_t j) const { return buf[fstart[row * k + f] + j]; }
};

/* the lines' keys: the entry table of the extract's select pass over the key groups (val = field length + 1, 0: the line
 * has no match; start = the field's source offset under the flag bits of sre_lines_gather.h) */
struct sre_lk_line_keys {
    const uint8_t  *buf;
    const uint64_t *val, *start;
    uint32_t        k;
    SRE_LG_MEMBER bool     selected(uint64_t line) const { return val[line * k] != 0; }
    SRE_LG_MEMBER uint64_t len(uint64_t line, uint32_t f) const { return val[line * k + f] - 1; }
    SRE_LG_MEMBER uint8_t  byte(uint64_t line, uint32_t f, uint64_t j) const
    {
        return buf[(start[line * k + f] & SRE_LG_ENTRY_START) + j];
    }
};

/* a's key x against b's key y, field by field, lengths first (sre_lt_equal across two Keys types) */
template <class A, class B>
SRE_LG_FN bool
sre_lk_equal(const A &a, uint64_t x, const B &b, uint64_t y)
{
    for (uint32_t f = 0; f < a.k; f++) {
        if (a.len(x, f) != b.len(y, f)) return false;
    }
    for (uint32_t f = 0; f < a.k; f++) {
        const uint64_t len = a.len(x, f);
        for (uint64_t j = 0; j < len; j++) {
            if (a.byte(x, f, j) != b.byte(y, f, j)) return false;
        }
    }
    return true;
}

/* the probe of one line */
typedef struct {
    uint64_t idx;           /* the word the next read goes to */
    uint64_t probes;        /* words seen so far */
    int64_t  id;            /* done: the row number of the line's key, or SRE_LK_NOT_MEMBER */
    bool     done;
} sre_lk_probe_t;

SRE_LG_FN void
sre_lk_probe_begin(sre_lk_probe_t &P, uint64_t hash, const sre_lt_params_t &p)
{
    P.idx = sre_lt_home(hash, p);
    P.probes = 0;
    P.id = SRE_LK_NOT_MEMBER;
    P.done = false;
}

/* one step of a probe that is not done: at most one read of the table.  The walk ends at an empty word (there always
 * is one: the load factor is at most 1/2), at a word whose row has the line's key, or after nslots words */
template <class LineKeys, class DictKeys, class Mem>
SRE_LG_FN void
sre_lk_probe_step(sre_lk_probe_t &P, uint64_t line, const LineKeys &lines, const DictKeys &dict, const Mem &mem,
                  const sre_lt_params_t &p)
{
    if (P.probes == p.nslots) {
        P.done = true;
        return;
    }
    const uint64_t row = mem.load(P.idx);
    if (row == SRE_LT_EMPTY) {
        P.done = true;
    } else if (sre_lk_equal(lines, line, dict, row)) {
        P.id = (int64_t) row;
        P.done = true;
    } else {
        P.idx = (P.idx + 1) & (p.nslots - 1);
        P.probes++;
    }
}

/* the key id of a line: the probe's answer for a line with a key */
SRE_LG_FN int64_t
sre_lk_keyid(bool keyed, int64_t id)
{
    return keyed ? id : SRE_LK_NO_KEY;
}

/* the selection rule: a keyed line keeps its filter value (length + 1) when it is a member, with `invert` when it is
 * not; a line without a key is never selected */
SRE_LG_FN uint64_t
sre_lk_value(bool keyed, int64_t id, bool invert, uint64_t fval)
{
    return keyed && ((id >= 0) != invert) ? fval : 0;
}

#endif
