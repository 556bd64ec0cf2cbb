/*
 * sre_lines_sort_text.h — the rules of the line sort by text (sre_hip_sort_lines_text): the class and the
 * compared length of a line from its entry of the value table, the chunk key of a text, its descending form, the key of a
 * line without a match, the plan of the digit passes and the index row.  The kernels (sre_hip_lines_sort_text.hip), the host
 * code of the batched API and the CPU model (tests/lines_sort_text_sim.cpp) compile this text; nothing here touches memory
 * except through its arguments.  The totals, their merge and their flush, the digit of a key, the dropped key, the limit and
 * the result words are the numeric sort's (sre_lines_sort.h).
 *
 * The TEXT of a line with a match is the bytes of the ONE sort group in its first match, from entry `line` of the value
 * table (sre_lines_sums.h, V = 1); an unset group is the empty text.  The COMPARED length L is its length, or max_bytes when
 * max_bytes != 0 and the text is longer.  The values pass (sre_hip_lines_values.h) sees a line with a match as class
 * SRE_LSO_NUMBER with L as its value, any other as SRE_LSO_NOMATCH: the four totals of the call are then (keyed, keyed, minlen,
 * maxlen), INT64_MAX / INT64_MIN in the last two without a keyed line.
 *
 * CHUNKS.  The compared text is cut into chunks of SRE_LST_CHUNK = 7 bytes.  The KEY of chunk c of a text t of compared
 * length L is a 64-bit word: its top seven bytes are t[7c .. 7c + 6], big-endian, 0 past the end; its low byte is cnt =
 * clamp(L - 7c, 0, 7).  Comparing these words chunk by chunk from chunk 0 is memcmp order with a proper prefix first: a
 * padding 0 is below or equal to any byte, cnt breaks the tie between padding and a real NUL, and a text of exactly 7k bytes
 * against a longer one ties in chunk k - 1 and is decided in chunk k, by cnt 0 against at least 1.
 *
 * DIRECTION.  The descending key is SRE_LST_KMAX - key, KMAX = 0xFFFFFFFFFFFFFF07: every byte of a key is at most 0xFF and
 * cnt at most 7, so there are no borrows between bytes and each digit is mirrored on its own.  REST.  Under ALL a line without
 * a match has KMAX + 1 in chunk 0, in both directions, which is above every key of a text, and in every other chunk the key
 * of the empty chunk in the call's direction, a constant.  All ones stays SRE_LSO_DROPPED: no key.
 *
 * The SORT is LSD over the chunks, last chunk first, each chunk through the stable 8-bit digit passes of the numeric sort;
 * stability across the chunks gives the order of the texts, equal compared texts in line order, in both directions.
 *
 * The PLAN, sre_lst_plan(minlen, maxlen, rest): the (chunk, digit) passes of a call, in the order they run, from the three
 * facts the host reads; rest: ALL with at least one line without a match.  It holds every (chunk, digit) at which the keys of
 * two selected lines can differ and leaves out those at which they cannot: the byte digits of the last chunk past maxlen,
 * the cnt digit (digit 0) of a chunk in which every text has the same cnt (a chunk wholly below minlen, or minlen ==
 * maxlen) unless the rest's key stands against it, everything when maxlen == 0 without a rest, and everything without a keyed
 * line.  A rest adds all eight digits of chunk 0.  The byte at 7c + j is digit 7 - j of chunk c.  The plan's length is about
 * maxlen + maxlen / 7, LINEAR IN maxlen: max_bytes is the caller's bound on the cost.
 */
#ifndef SRE_LINES_SORT_TEXT_H
#define SRE_LINES_SORT_TEXT_H

#include <stdint.h>
#include "sre_lines_sort.h"

#define SRE_LST_CHUNK       7u
#define SRE_LST_KMAX        0xFFFFFFFFFFFFFF07ull
#define SRE_LST_REST        (SRE_LST_KMAX + 1)      /* chunk 0 of a line without a match under ALL */
#define SRE_LST_INDEX_WORDS 6u

/* one pass of the plan */
typedef struct {
    uint64_t chunk;
    uint32_t digit;
} sre_lst_pass_t;

/* the compared length of a text of len bytes */
SRE_LG_FN uint64_t sre_lst_cut(uint64_t len, uint64_t max_bytes) { return max_bytes != 0 && max_bytes < len ? max_bytes : len; }

/* the class of line `line` for the values pass, *value its compared length; vals: the value table with one column */
template <class Vals>
SRE_LG_FN int32_t
sre_lst_line(const Vals &vals, uint64_t line, uint64_t max_bytes, int64_t *value)
{
    const uint64_t val = vals.val(line, 0), raw = vals.raw(line, 0);
    *value = 0;
    if (val == 0) return SRE_LSO_NOMATCH;
    if ((raw & SRE_LG_ENTRY_UNSET) == 0) *value = (int64_t) sre_lst_cut(val - 1, max_bytes);
    return SRE_LSO_NUMBER;
}

/* cnt of chunk c of a text of compared length L */
SRE_LG_FN uint32_t
sre_lst_cnt(uint64_t L, uint64_t c)
{
    const uint64_t off = c * SRE_LST_CHUNK;
    return L <= off ? 0u : L - off >= SRE_LST_CHUNK ? SRE_LST_CHUNK : (uint32_t) (L - off);
}

/* the ascending key of chunk c of the text at `at` of compared length L; text.byte(x) is read for x in [at + 7c, at + 7c + cnt) only */
template <class Text>
SRE_LG_FN uint64_t
sre_lst_chunk_key(const Text &text, uint64_t at, uint64_t L, uint64_t c)
{
    const uint32_t cnt = sre_lst_cnt(L, c);
    const uint64_t from = at + c * SRE_LST_CHUNK;
    uint64_t       key = cnt;
    for (uint32_t j = 0; j < cnt; j++) key |= (uint64_t) text.byte(from + j) << (56u - 8u * j);
    return key;
}

/* the key in the call's direction */
SRE_LG_FN uint64_t sre_lst_dir(uint64_t key, int desc) { return desc ? SRE_LST_KMAX - key : key; }

/* chunk c of a line without a match under ALL */
SRE_LG_FN uint64_t sre_lst_rest_key(uint64_t c, int desc) { return c == 0 ? SRE_LST_REST : sre_lst_dir(0, desc); }

/* the key of chunk c of line `line`: SRE_LSO_DROPPED for a line that is not selected */
template <class Vals>
SRE_LG_FN uint64_t
sre_lst_line_key(const Vals &vals, uint64_t line, uint64_t c, uint64_t max_bytes, int desc, int all)
{
    const uint64_t val = vals.val(line, 0), raw = vals.raw(line, 0);
    if (val == 0) return all ? sre_lst_rest_key(c, desc) : SRE_LSO_DROPPED;
    const uint64_t L = (raw & SRE_LG_ENTRY_UNSET) ? 0 : sre_lst_cut(val - 1, max_bytes);
    return sre_lst_dir(sre_lst_chunk_key(vals, raw & SRE_LG_ENTRY_START, L, c), desc);
}

/* the lines the flags select */
SRE_LG_FN uint64_t sre_lst_selected(uint64_t nlines, uint64_t nkeyed, int all) { return all ? nlines : nkeyed; }

/* the plan from the facts of the one read: the passes in the order they run, last chunk first, the digits of a chunk
 * ascending.  out[0 .. min(cap, length)) is written; returns the length.  minlen > maxlen: no keyed line */
SRE_LG_FN uint64_t
sre_lst_plan(uint64_t minlen, uint64_t maxlen, int rest, sre_lst_pass_t *out, uint64_t cap)
{
    uint64_t len = 0;
    if (minlen > maxlen) return 0;
    uint64_t nchunks = maxlen / SRE_LST_CHUNK + (maxlen % SRE_LST_CHUNK != 0);
    if (rest && nchunks == 0) nchunks = 1;
    for (uint64_t c = nchunks; c-- > 0;) {
        const uint32_t lo = sre_lst_cnt(minlen, c), hi = sre_lst_cnt(maxlen, c);
        const uint32_t first_byte = rest && c == 0 ? 1u : 8u - hi;
        if (lo != hi || rest) {
            if (len < cap) out[len].chunk = c, out[len].digit = 0;
            len++;
        }
        for (uint32_t d = first_byte; d < 8u; d++, len++) {
            if (len < cap) out[len].chunk = c, out[len].digit = d;
        }
    }
    return len;
}

/* the index row of rank r, whose line is `line`: the line's four words and the field (its offset in the buffer and its FULL
 * length, not the cut one), -1, -1 for an unset group or a line without a match */
template <class Vals>
SRE_LG_FN void
sre_lst_index_row(const Vals &vals, uint64_t line, const uint64_t *cstart, const uint64_t *coff, uint64_t r, int64_t *row)
{
    const uint64_t o = coff[r], val = vals.val(line, 0), raw = vals.raw(line, 0);
    const bool     set = val != 0 && (raw & SRE_LG_ENTRY_UNSET) == 0;
    row[0] = (int64_t) line;
    row[1] = (int64_t) (cstart[r] & SRE_LG_ENTRY_START);
    row[2] = (int64_t) (coff[r + 1] - o - 1);
    row[3] = (int64_t) o;
    row[4] = set ? (int64_t) (raw & SRE_LG_ENTRY_START) : -1;
    row[5] = set ? (int64_t) (val - 1) : -1;
}

#endif
