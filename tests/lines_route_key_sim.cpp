/*
 * lines_route_key_sim.cpp — the partition of the line route by key on the CPU: every digit pass through the partition model
 * (lines_partition_sim.h) with the rules the kernels compile (sregex_amd/csrc/sre_lines_route_key.h and sre_lines_route.h):
 * the sort key, the item, the digit and either rank rule of a slot; then the compact table, the head flags, the head ranks, the bucket
 * rows, the cut and the index rows.  Every store is counted, so tests/test_lines_route_key_model.py can assert that every
 * word of every array is written exactly once per pass.  The gather over the table is the extract's model
 * (tests/lines_extract_sim.cpp), unchanged.
 */
#include "lines_partition_sim.h"
#include <string.h>

namespace {

/* a digit pass (KeyPass of sre_hip_lines_route_key.hip; keyid != NULL: pass 0 over the lines); writes[r] counts the stores
 * to dst[r] */
struct SimKeyPass {
    const int64_t  *keyid;
    const uint64_t *src;
    uint64_t        n, rows;
    int             all;
    uint32_t        pass, width;
    int             rank_rule;
    uint64_t       *dst;
    uint32_t       *writes;
    uint32_t nd() const { return 1u << width; }
    uint32_t bits() const { return width; }
    int      rule() const { return rank_rule; }
    uint64_t load(uint64_t i) const
    {
        if (i >= n) return SRE_LRK_DROPPED;
        return keyid ? sre_lrk_first_item(keyid[i], i, rows, all) : src[i];
    }
    bool     taken(uint64_t it) const { return it != SRE_LRK_DROPPED; }
    uint32_t digit(uint64_t it) const { return sre_lrk_digit(it, pass, width); }
    void     store(uint64_t r, uint64_t it, uint64_t)
    {
        dst[r] = it;
        writes[r]++;
    }
};

}  // namespace

extern "C" {

uint32_t lrksim_items(void) { return SRE_LR_ITEMS; }
uint64_t lrksim_flags(void) { return SRE_LG_ENTRY_LAST | SRE_LG_ENTRY_FIRST; }
uint64_t lrksim_start_mask(void) { return SRE_LG_ENTRY_START; }
uint64_t lrksim_max_lines(void) { return SRE_LRK_MAX_LINES; }
uint64_t lrksim_dropped(void) { return SRE_LRK_DROPPED; }

int64_t  lrksim_sort_key(int64_t id, uint64_t rows, int all) { return sre_lrk_sort_key(id, rows, all); }
int64_t  lrksim_key_id(uint64_t key, uint64_t rows) { return sre_lrk_key_id(key, rows); }
uint64_t lrksim_item(uint64_t key, uint64_t line) { return sre_lrk_item(key, line); }
uint32_t lrksim_digit_bits(long v) { return sre_lrk_digit_bits(v); }
uint64_t lrksim_max_key(uint64_t rows, int all) { return sre_lrk_max_key(rows, all); }
uint32_t lrksim_passes(uint64_t max_key, uint32_t bits) { return sre_lrk_passes(max_key, bits); }

/* one slot through a rank rule: rank[64] and c[2^bits] (zero before); returns the ballots behind the first */
uint32_t
lrksim_slot(const uint8_t *sel, const uint32_t *digit, uint32_t bits, int rule, uint32_t *rank, uint32_t *c)
{
    SimSlot s;
    for (uint32_t x = 0; x < 64; x++) {
        s.sel[x] = sel[x] != 0;
        s.digit[x] = digit[x];
    }
    const uint32_t b = s.run(rule, bits, c);
    for (uint32_t x = 0; x < 64; x++) rank[x] = s.rank[x];
    return b;
}

/* count of one pass: cnt[d * nwg + w]; writes[] counts the stores to every word of cnt.  keyid != NULL: pass 0 over the lines */
void
lrksim_count(const int64_t *keyid, const uint64_t *src, uint64_t n, uint64_t rows, int all, uint32_t pass, uint32_t bits, int rule,
             uint64_t *cnt, uint32_t *writes)
{
    const SimKeyPass p = {keyid, src, n, rows, all, pass, bits, rule, NULL, NULL};
    (void) sim_count(p, n, cnt, writes);
}

void lrksim_scan(uint64_t *v, uint64_t n) { sim_scan(v, n); }

/* scatter of one pass over the scanned counts; writes[r] counts the stores to dst[r].  Returns the stores that fell outside
 * [0, total) */
uint64_t
lrksim_scatter(const int64_t *keyid, const uint64_t *src, uint64_t n, uint64_t rows, int all, uint32_t pass, uint32_t bits, int rule,
               const uint64_t *first, uint64_t total, uint64_t *dst, uint32_t *writes)
{
    SimKeyPass p = {keyid, src, n, rows, all, pass, bits, rule, dst, writes};
    return sim_scatter(p, n, first, total);
}

/* the compact table and the head flags from the sorted items; writes[r] counts the stores to each of the three words of rank r */
void
lrksim_table(const uint64_t *items, const uint64_t *ends, uint64_t nsel, uint64_t nlines, uint64_t *cstart, uint64_t *cval,
             uint64_t *head, uint32_t *writes)
{
    for (uint64_t r = 0; r < nsel; r++) {
        const uint64_t i = sre_lrk_item_line(items[r]);
        head[r] = sre_lrk_is_head(items, r) ? 1 : 0;
        if (i >= nlines) continue;
        const uint64_t st = i == 0 ? 0 : ends[i - 1] + 1;
        sre_lrk_entry(st, ends[i] - st, cstart + r, cval + r);
        writes[r]++;
    }
}

/* the head ranks behind the scan of the flags; writes[b] counts the stores to hrank[b] */
void
lrksim_heads(const uint64_t *items, const uint64_t *hoff, uint64_t nsel, uint64_t *hrank, uint32_t *writes)
{
    for (uint64_t r = 0; r < nsel; r++) {
        const uint64_t b = hoff[r];
        if (b > r) continue;
        if (sre_lrk_is_head(items, r)) {
            hrank[b] = r;
            writes[b]++;
        }
        if (r == nsel - 1) {
            hrank[hoff[nsel]] = nsel;
            writes[hoff[nsel]]++;
        }
    }
}

void
lrksim_bucket_row(const uint64_t *items, const uint64_t *hrank, uint64_t b, const uint64_t *coff, uint64_t rows, int64_t *row)
{
    sre_lrk_bucket_row(items, hrank, b, coff, rows, row);
}

void
lrksim_index_row(const uint64_t *items, const uint64_t *cstart, const uint64_t *coff, uint64_t r, uint64_t rows, int64_t *row)
{
    sre_lrk_index_row(items, cstart, coff, r, rows, row);
}

uint64_t lrksim_cut(const uint64_t *coff, uint64_t nsel, uint64_t out_cap) { return sre_lr_cut(coff, nsel, out_cap); }

}
