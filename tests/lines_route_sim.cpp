/*
 * lines_route_sim.cpp — the line route's partition on the CPU: count, scan and scatter run workgroup by workgroup, slot
 * by slot and lane by lane with the rules the kernels compile (sregex_amd/csrc/sre_lines_route.h): the key, the lines a
 * wave owns, the wave rule on ballots (one turn per distinct bucket of a slot), the slot prefix and the global rank.
 * Every word of the compact table written is counted, so tests/test_lines_route_model.py can assert that the table is a
 * permutation written exactly once; the finish rules (the cut, the bucket totals) are the header's too.  The gather over
 * the table is the extract's model (tests/lines_extract_sim.cpp), unchanged.
 */
#include "sre_lines_route.h"
#include <stdint.h>
#include <string.h>
#include <vector>

namespace {

/* one slot of 64 lanes in lockstep: what wave_rank of sre_hip_lines_route.hip does with __ballot / __shfl */
struct SimWave {
    bool     sel[64];
    uint32_t bucket[64];
    uint32_t rank[64];

    uint64_t ballot(bool (*pred)(const SimWave &, uint32_t, uint32_t), uint32_t arg) const
    {
        uint64_t m = 0;
        for (uint32_t x = 0; x < 64; x++) m |= (uint64_t) (pred(*this, x, arg) ? 1 : 0) << x;
        return m;
    }
    static bool is_sel(const SimWave &w, uint32_t x, uint32_t) { return w.sel[x]; }
    static bool is_bucket(const SimWave &w, uint32_t x, uint32_t kb) { return w.sel[x] && w.bucket[x] == kb; }

    /* returns the turns of the loop */
    uint32_t run(uint32_t *c)
    {
        uint32_t turns = 0;
        for (uint32_t x = 0; x < 64; x++) rank[x] = 0;
        uint64_t rem = ballot(is_sel, 0);
        while (rem) {
            const uint32_t lead = sre_lr_leader(rem);
            const uint32_t kb = bucket[lead];
            const uint64_t m = ballot(is_bucket, kb);
            for (uint32_t x = 0; x < 64; x++) {
                if (sel[x] && bucket[x] == kb) rank[x] = sre_lr_rank_in(m, x);
            }
            c[kb] = sre_lr_popc(m);
            rem &= ~m;
            turns++;
        }
        return turns;
    }

    void load(const uint64_t *key, uint64_t n, uint32_t nb, uint64_t wg, uint32_t slot)
    {
        for (uint32_t x = 0; x < 64; x++) {
            const uint64_t i = sre_lr_line(wg, slot, x);
            const uint64_t k = i < n ? key[i] : 0;
            bucket[x] = sre_lr_key_bucket(k);
            sel[x] = sre_lr_key_selected(k) && bucket[x] < nb;
        }
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
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    uint32_t       most = 0;
    SimWave        wave;
    for (uint64_t w = 0; w < nwg; w++) {
        std::vector<uint32_t> c(SRE_LR_SLOTS * nb, 0);
        for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
            for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
                const uint32_t slot = sre_lr_slot(v, q);
                wave.load(key, n, nb, w, slot);
                const uint32_t t = wave.run(c.data() + slot * nb);
                if (t > most) most = t;
            }
        }
        for (uint32_t b = 0; b < nb; b++) cnt[sre_lr_cnt_index(b, nwg, w)] = sre_lr_slot_prefix(c.data() + b, nb);
    }
    return most;
}

/* the scan of the counts as the filter's scan leaves it: exclusive, the total behind the last word */
void
lrsim_scan(uint64_t *v, uint64_t n)
{
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t x = v[i];
        v[i] = run;
        run += x;
    }
    v[n] = run;
}

/* scatter over the scanned counts: the compact table; writes[r] counts the stores to entry r.  Returns the stores that
 * fell outside [0, nsel) */
uint64_t
lrsim_scatter(const uint64_t *key, const uint64_t *ends, uint64_t n, uint32_t nb, const uint64_t *first, uint64_t nsel,
              uint64_t *cstart, uint64_t *cval, uint64_t *cmeta, uint32_t *writes)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    uint64_t       bad = 0;
    for (uint64_t w = 0; w < nwg; w++) {
        std::vector<uint32_t> c(SRE_LR_SLOTS * nb, 0);
        std::vector<uint32_t> rk(SRE_LR_ITEMS, 0);
        std::vector<uint64_t> gbase(nb, 0);
        SimWave               wave;
        for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
            for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
                const uint32_t slot = sre_lr_slot(v, q);
                wave.load(key, n, nb, w, slot);
                (void) wave.run(c.data() + slot * nb);
                for (uint32_t x = 0; x < 64; x++) rk[slot * 64 + x] = wave.rank[x];
            }
        }
        for (uint32_t b = 0; b < nb; b++) {
            (void) sre_lr_slot_prefix(c.data() + b, nb);
            gbase[b] = first[sre_lr_cnt_index(b, nwg, w)];
        }
        for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
            for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
                const uint32_t slot = sre_lr_slot(v, q);
                for (uint32_t x = 0; x < 64; x++) {
                    const uint64_t i = sre_lr_line(w, slot, x);
                    const uint64_t k = i < n ? key[i] : 0;
                    const uint32_t b = sre_lr_key_bucket(k);
                    if (!sre_lr_key_selected(k) || b >= nb) continue;
                    const uint64_t r = gbase[b] + c[slot * nb + b] + rk[slot * 64 + x];
                    if (r >= nsel) {
                        bad++;
                        continue;
                    }
                    const uint64_t val = sre_lr_key_val(k);
                    cstart[r] = sre_lr_entry_start(ends[i] - (val - 1));
                    cval[r] = val;
                    cmeta[r] = sre_lr_entry_meta(b, i);
                    writes[r]++;
                }
            }
        }
    }
    return bad;
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
