/*
 * lines_route_sim.cpp — the line route's partition on the CPU: the partition model (lines_partition_sim.h) with the route's
 * pass, the key of a line as the item and its bucket as the digit under the wave rule (sregex_amd/csrc/sre_lines_route.h).
 * Every word of the compact table written is counted, so tests/test_lines_route_model.py can assert that the table is a
 * permutation written exactly once; the finish rules (the cut, the bucket totals) are the header's too.  The gather over
 * the table is the extract's model (tests/lines_extract_sim.cpp), unchanged.
 */
#include "lines_partition_sim.h"
#include <string.h>

namespace {

/* the route's pass (RoutePass of sre_hip_lines_route.hip); writes[r] counts the stores to entry r of the compact table */
struct SimRoute {
    const uint64_t *key, *ends;
    uint64_t        n;
    uint32_t        nb;
    uint64_t       *cstart, *cval, *cmeta;
    uint32_t       *writes;
    uint32_t nd() const { return nb; }
    uint32_t bits() const { return 0; }
    int      rule() const { return SRE_LRK_RANK_TURNS; }
    uint64_t load(uint64_t i) const { return i < n ? key[i] : 0; }
    bool     taken(uint64_t k) const { return sre_lr_key_selected(k) && sre_lr_key_bucket(k) < nb; }
    uint32_t digit(uint64_t k) const { return sre_lr_key_bucket(k); }
    void     store(uint64_t r, uint64_t k, uint64_t i)
    {
        const uint64_t val = sre_lr_key_val(k);
        cstart[r] = sre_lr_entry_start(ends[i] - (val - 1));
        cval[r] = val;
        cmeta[r] = sre_lr_entry_meta(sre_lr_key_bucket(k), i);
        writes[r]++;
    }
};

}  // namespace

extern "C" {

uint32_t lrsim_items(void) { return SRE_LR_ITEMS; }
uint64_t lrsim_flags(void) { return SRE_LG_ENTRY_LAST | SRE_LG_ENTRY_FIRST; }
uint64_t lrsim_start_mask(void) { return SRE_LG_ENTRY_START; }

/* the select rule: the key of a line from its rc (declined = -1 here) */
uint64_t
lrsim_key(int64_t rc, uint32_t nreg, const int32_t *map, uint64_t len)
{
    return sre_lr_key(sre_lr_bucket(rc, -1, nreg, map), len);
}

/* count: cnt[b * nwg + w].  Returns the most turns any slot's wave loop took */
uint32_t
lrsim_count(const uint64_t *key, uint64_t n, uint32_t nb, uint64_t *cnt)
{
    const SimRoute p = {key, NULL, n, nb, NULL, NULL, NULL, NULL};
    return sim_count(p, n, cnt, NULL);
}

void lrsim_scan(uint64_t *v, uint64_t n) { sim_scan(v, n); }

/* scatter over the scanned counts: the compact table; writes[r] counts the stores to entry r.  Returns the stores that
 * fell outside [0, nsel) */
uint64_t
lrsim_scatter(const uint64_t *key, const uint64_t *ends, uint64_t n, uint32_t nb, const uint64_t *first, uint64_t nsel,
              uint64_t *cstart, uint64_t *cval, uint64_t *cmeta, uint32_t *writes)
{
    SimRoute p = {key, ends, n, nb, cstart, cval, cmeta, writes};
    return sim_scatter(p, n, first, nsel);
}

uint64_t lrsim_cut(const uint64_t *coff, uint64_t nsel, uint64_t out_cap) { return sre_lr_cut(coff, nsel, out_cap); }

void
lrsim_totals(const uint64_t *first, uint64_t n, uint32_t b, const uint64_t *coff, uint64_t *nlines, uint64_t *bytes)
{
    sre_lr_bucket_totals(first, (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS, b, coff, nlines, bytes);
}

uint32_t lrsim_meta_bucket(uint64_t m) { return sre_lr_meta_bucket(m); }
uint64_t lrsim_meta_line(uint64_t m) { return sre_lr_meta_line(m); }

}
