/*
 * lines_route_key_sim.cpp — the partition of the line route by key on the CPU: count, scan and scatter of every digit pass
 * run workgroup by workgroup, slot by slot and lane by lane with the rules the kernels compile
 * (sregex_amd/csrc/sre_lines_route_key.h and sre_lines_route.h): the sort key, the item, the digit, the two rank rules of a
 * slot on ballots, the slot prefix and the global rank; then the compact table, the head flags, the head ranks, the bucket
 * rows, the cut and the index rows.  Every store is counted, so tests/test_lines_route_key_model.py can assert that every
 * word of every array is written exactly once per pass.  The gather over the table is the extract's model
 * (tests/lines_extract_sim.cpp), unchanged.
 */
#include "sre_lines_route_key.h"
#include <stdint.h>
#include <string.h>
#include <vector>

namespace {

/* one slot of 64 lanes in lockstep: what slot_rank of sre_hip_lines_route_key.hip does with __ballot / __shfl */
struct SimSlot {
    bool     sel[64];
    uint32_t digit[64];
    uint32_t rank[64];

    template <class Pred> uint64_t ballot(Pred pred) const
    {
        uint64_t m = 0;
        for (uint32_t x = 0; x < 64; x++) m |= (uint64_t) (pred(x) ? 1 : 0) << x;
        return m;
    }

    /* returns the ballots taken behind the first */
    uint32_t run(int rule, uint32_t bits, uint32_t *c)
    {
        uint32_t ballots = 0;
        for (uint32_t x = 0; x < 64; x++) rank[x] = 0;
        if (rule == SRE_LRK_RANK_TURNS) {
            uint64_t rem = ballot([&](uint32_t x) { return sel[x]; });
            while (rem) {
                const uint32_t lead = sre_lr_leader(rem);
                const uint32_t kd = digit[lead];
                const uint64_t m = ballot([&](uint32_t x) { return sel[x] && digit[x] == kd; });
                for (uint32_t x = 0; x < 64; x++) {
                    if (sel[x] && digit[x] == kd) rank[x] = sre_lr_rank_in(m, x);
                }
                c[kd] = sre_lr_popc(m);
                rem &= ~m;
                ballots++;
            }
            return ballots;
        }
        uint64_t m[64];
        const uint64_t all = ballot([&](uint32_t x) { return sel[x]; });
        for (uint32_t x = 0; x < 64; x++) m[x] = all;
        for (uint32_t bit = 0; bit < bits; bit++) {
            const uint64_t with_bit = ballot([&](uint32_t x) { return sel[x] && ((digit[x] >> bit) & 1u); });
            for (uint32_t x = 0; x < 64; x++) m[x] = sre_lrk_agree(m[x], with_bit, digit[x], bit);
            ballots++;
        }
        for (uint32_t x = 0; x < 64; x++) {
            const uint32_t r = sre_lr_rank_in(m[x], x);
            if (sel[x] && r == 0) c[digit[x]] = sre_lr_popc(m[x]);
            rank[x] = sel[x] ? r : 0;
        }
        return ballots;
    }
};

uint64_t
load_item(const int64_t *keyid, const uint64_t *src, uint64_t i, uint64_t n, uint64_t rows, int all)
{
    if (i >= n) return SRE_LRK_DROPPED;
    return keyid ? sre_lrk_first_item(keyid[i], i, rows, all) : src[i];
}

void
load_slot(SimSlot &s, const int64_t *keyid, const uint64_t *src, uint64_t n, uint64_t rows, int all, uint32_t pass, uint32_t bits,
          uint64_t wg, uint32_t slot)
{
    for (uint32_t x = 0; x < 64; x++) {
        const uint64_t it = load_item(keyid, src, sre_lr_line(wg, slot, x), n, rows, all);
        s.sel[x] = it != SRE_LRK_DROPPED;
        s.digit[x] = sre_lrk_digit(it, pass, bits);
    }
}

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
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    const uint32_t nd = 1u << bits;
    SimSlot        s;
    for (uint64_t w = 0; w < nwg; w++) {
        std::vector<uint32_t> c(SRE_LR_SLOTS * nd, 0);
        for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
            for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
                const uint32_t slot = sre_lr_slot(v, q);
                load_slot(s, keyid, src, n, rows, all, pass, bits, w, slot);
                (void) s.run(rule, bits, c.data() + slot * nd);
            }
        }
        for (uint32_t d = 0; d < nd; d++) {
            const uint64_t at = sre_lr_cnt_index(d, nwg, w);
            cnt[at] = sre_lr_slot_prefix(c.data() + d, nd);
            writes[at]++;
        }
    }
}

/* the scan as the filter's scan leaves it: exclusive, the total behind the last word */
void
lrksim_scan(uint64_t *v, uint64_t n)
{
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t x = v[i];
        v[i] = run;
        run += x;
    }
    v[n] = run;
}

/* scatter of one pass over the scanned counts; writes[r] counts the stores to dst[r].  Returns the stores that fell outside
 * [0, total) */
uint64_t
lrksim_scatter(const int64_t *keyid, const uint64_t *src, uint64_t n, uint64_t rows, int all, uint32_t pass, uint32_t bits, int rule,
               const uint64_t *first, uint64_t total, uint64_t *dst, uint32_t *writes)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    const uint32_t nd = 1u << bits;
    uint64_t       bad = 0;
    for (uint64_t w = 0; w < nwg; w++) {
        std::vector<uint32_t> c(SRE_LR_SLOTS * nd, 0);
        std::vector<uint32_t> rk(SRE_LR_ITEMS, 0);
        std::vector<uint64_t> gbase(nd, 0);
        SimSlot               s;
        for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
            for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
                const uint32_t slot = sre_lr_slot(v, q);
                load_slot(s, keyid, src, n, rows, all, pass, bits, w, slot);
                (void) s.run(rule, bits, c.data() + slot * nd);
                for (uint32_t x = 0; x < 64; x++) rk[slot * 64 + x] = s.rank[x];
            }
        }
        for (uint32_t d = 0; d < nd; d++) {
            (void) sre_lr_slot_prefix(c.data() + d, nd);
            gbase[d] = first[sre_lr_cnt_index(d, nwg, w)];
        }
        for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
            for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
                const uint32_t slot = sre_lr_slot(v, q);
                for (uint32_t x = 0; x < 64; x++) {
                    const uint64_t it = load_item(keyid, src, sre_lr_line(w, slot, x), n, rows, all);
                    if (it == SRE_LRK_DROPPED) continue;
                    const uint32_t d = sre_lrk_digit(it, pass, bits);
                    const uint64_t r = gbase[d] + c[slot * nd + d] + rk[slot * 64 + x];
                    if (r >= total) {
                        bad++;
                        continue;
                    }
                    dst[r] = it;
                    writes[r]++;
                }
            }
        }
    }
    return bad;
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
