/*
 * sre_lines_route_key.h — the rules of the line route by key (sre_hip_route_lines_by_key): the sort key
 * of a line from its dictionary id, the item a line becomes, the digit a pass looks at, the number of passes, the rank of
 * an item inside its slot, the heads of the buckets and their rows.  The kernels (sre_hip_lines_route_key.hip), the host
 * code of the batched API and the CPU model (tests/lines_route_key_sim.cpp) compile this text; nothing here touches memory
 * except through its arguments.  The slot geometry, the slot prefix and the count index are the route's (sre_lines_route.h).
 *
 * The SORT KEY of a line, from its key id (the lookup's: a dictionary row, -1 keyed but no member, -2 no key): a member's
 * id; under ALL `rows` for -1 and `rows + 1` for -2; every other line is dropped.  The largest key that can occur is
 * rows - 1, or rows + 1 under ALL, and a set has at most 2^30 rows, so a key takes 31 bits.
 *
 * The ITEM of a selected line, one word: key << 32 | line.  A buffer may therefore hold at most SRE_LRK_MAX_LINES =
 * 2^32 - 1 lines.  Items compare as (key, line): the sorted order is the output order.
 *
 * The partition is an LSD radix sort of the items by `bits` bits of the key a pass (1 .. 8), lowest digit first, each pass
 * the route's count / scan / scatter with the digit in the bucket's place:
 *   count    cnt[d * nwg + w] = items of digit d among the SRE_LR_ITEMS items of workgroup w; the exclusive scan of those
 *            words gives first[d * nwg + w], and the total behind them;
 *   scatter  rank = first[d * nwg + w] + items of digit d in the slots in front + items of digit d at lower lanes of the
 *            item's slot; the item is stored at that rank of the other array.
 * Pass 0 makes the items from the key ids in line order and drops the unselected; its total is the number of selected
 * lines.  Every pass is stable, so after the pass of the highest digit the items are sorted by (key, line).
 *
 * The rank inside a slot, two rules with the same result:
 *   SRE_LRK_RANK_BITS   `bits` ballots, one per bit of the digit: a lane keeps of each ballot the lanes that agree with its
 *                       own bit; what is left is the ballot of its digit;
 *   SRE_LRK_RANK_TURNS  the route's wave rule: one ballot per DISTINCT digit of the slot.
 * Either way a lane's rank is the set bits below it, and the lowest lane of every digit leaves the slot's count of it.
 *
 * Rank r is a HEAD when r == 0 or its key differs from rank r - 1's; the exclusive scan of the head flags numbers the
 * buckets, hrank[b] is the rank of bucket b's head and hrank[nbuckets] = nsel.
 */
#ifndef SRE_LINES_ROUTE_KEY_H
#define SRE_LINES_ROUTE_KEY_H

#include <stdint.h>
#include "sre_lines_route.h"

#define SRE_LRK_LINE_BITS   32u
#define SRE_LRK_LINE_MASK   0xFFFFFFFFull
#define SRE_LRK_MAX_LINES   0xFFFFFFFFull           /* 2^32 - 1 */
#define SRE_LRK_DROPPED     (~(uint64_t) 0)         /* the item of a line that is not selected (no key has 32 bits) */
#define SRE_LRK_MAX_BITS    8u                      /* digit width: 1 .. 8, 8 unless the knob says otherwise */

#define SRE_LRK_RANK_BITS   0
#define SRE_LRK_RANK_TURNS  1

/* the words the finish pass leaves for the host: the route's four (sre_lr_result) and three of its own */
#define SRE_LRK_RES_NSEL     SRE_LR_RES_NSEL
#define SRE_LRK_RES_NEED     SRE_LR_RES_NEED
#define SRE_LRK_RES_WRITTEN  SRE_LR_RES_WRITTEN
#define SRE_LRK_RES_BYTES    SRE_LR_RES_BYTES
#define SRE_LRK_RES_NBUCKETS (SRE_LR_RES_WORDS + 0u)
#define SRE_LRK_RES_NKEYED   (SRE_LR_RES_WORDS + 1u)
#define SRE_LRK_RES_NMEMBERS (SRE_LR_RES_WORDS + 2u)
#define SRE_LRK_RES_WORDS    (SRE_LR_RES_WORDS + 3u)

/* the sort key of a line with key id `id` against a set of `rows` rows; -1 drops the line */
SRE_LG_FN int64_t
sre_lrk_sort_key(int64_t id, uint64_t rows, int all)
{
    if (id >= 0) return (uint64_t) id < rows ? id : -1;         /* (the probe gives no id beyond the rows) */
    if (!all) return -1;
    return id == -1 ? (int64_t) rows : id == -2 ? (int64_t) rows + 1 : -1;
}

/* ... and back: the id of a key for the index and the bucket rows */
SRE_LG_FN int64_t
sre_lrk_key_id(uint64_t key, uint64_t rows)
{
    return key < rows ? (int64_t) key : key == rows ? -1 : -2;
}

SRE_LG_FN uint64_t sre_lrk_item(uint64_t key, uint64_t line) { return key << SRE_LRK_LINE_BITS | line; }
SRE_LG_FN uint64_t sre_lrk_item_key(uint64_t item) { return item >> SRE_LRK_LINE_BITS; }
SRE_LG_FN uint64_t sre_lrk_item_line(uint64_t item) { return item & SRE_LRK_LINE_MASK; }

/* the item of line i in pass 0 */
SRE_LG_FN uint64_t
sre_lrk_first_item(int64_t id, uint64_t i, uint64_t rows, int all)
{
    const int64_t k = sre_lrk_sort_key(id, rows, all);
    return k < 0 ? SRE_LRK_DROPPED : sre_lrk_item((uint64_t) k, i);
}

/* the digit width a knob value asks for */
SRE_LG_FN uint32_t sre_lrk_digit_bits(long v) { return v >= 1 && v <= (long) SRE_LRK_MAX_BITS ? (uint32_t) v : SRE_LRK_MAX_BITS; }

/* the largest sort key that can occur (0 for an empty set without ALL: nothing is selected then) */
SRE_LG_FN uint64_t sre_lrk_max_key(uint64_t rows, int all) { return all ? rows + 1 : rows ? rows - 1 : 0; }

/* the passes that sort keys up to max_key by `bits` bits each: at least one */
SRE_LG_FN uint32_t
sre_lrk_passes(uint64_t max_key, uint32_t bits)
{
    uint32_t width = 1;
    while (width < 64 && (max_key >> width) != 0) width++;
    return (width + bits - 1) / bits;
}

SRE_LG_FN uint32_t
sre_lrk_digit(uint64_t item, uint32_t pass, uint32_t bits)
{
    return (uint32_t) (sre_lrk_item_key(item) >> (pass * bits)) & ((1u << bits) - 1u);
}

/* the bit rule: of the ballot `with_bit` of the selected lanes whose digit has the bit, a lane keeps the lanes that agree
 * with its own; m starts as the ballot of the selected lanes */
SRE_LG_FN uint64_t sre_lrk_agree(uint64_t m, uint64_t with_bit, uint32_t digit, uint32_t bit)
{
    return m & (((digit >> bit) & 1u) ? with_bit : ~with_bit);
}

/* rank r of the sorted items heads a bucket */
SRE_LG_FN bool
sre_lrk_is_head(const uint64_t *items, uint64_t r)
{
    return r == 0 || sre_lrk_item_key(items[r]) != sre_lrk_item_key(items[r - 1]);
}

/* the entry of the compact table for the line [start, start + len) */
SRE_LG_FN void
sre_lrk_entry(uint64_t start, uint64_t len, uint64_t *cstart, uint64_t *cval)
{
    *cstart = sre_lr_entry_start(start);
    *cval = len + 1;
}

/* the row of bucket b from the head ranks and the scanned table coff[0 .. nsel] */
SRE_LG_FN void
sre_lrk_bucket_row(const uint64_t *items, const uint64_t *hrank, uint64_t b, const uint64_t *coff, uint64_t rows, int64_t *row)
{
    const uint64_t r0 = hrank[b], r1 = hrank[b + 1];
    row[0] = sre_lrk_key_id(sre_lrk_item_key(items[r0]), rows);
    row[1] = (int64_t) r0;
    row[2] = (int64_t) (r1 - r0);
    row[3] = (int64_t) coff[r0];
    row[4] = (int64_t) (coff[r1] - coff[r0]);
}

/* the index row of rank r */
SRE_LG_FN void
sre_lrk_index_row(const uint64_t *items, const uint64_t *cstart, const uint64_t *coff, uint64_t r, uint64_t rows, int64_t *row)
{
    const uint64_t o = coff[r];
    row[0] = (int64_t) sre_lrk_item_line(items[r]);
    row[1] = (int64_t) (cstart[r] & SRE_LG_ENTRY_START);
    row[2] = (int64_t) (coff[r + 1] - o - 1);
    row[3] = (int64_t) o;
    row[4] = sre_lrk_key_id(sre_lrk_item_key(items[r]), rows);
}

#endif
