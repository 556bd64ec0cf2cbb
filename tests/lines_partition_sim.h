/*
 * lines_partition_sim.h — the partition pass of sregex_amd/csrc/sre_hip_lines_partition.h on the CPU, for the models of the
 * line route, the line route by key and the line sort (lines_route_sim.cpp, lines_route_key_sim.cpp, lines_sort_sim.cpp):
 * one slot of 64 lanes in lockstep under either rank rule, and count, scan and scatter run workgroup by workgroup, slot by
 * slot and lane by lane with the rules the kernels compile (sre_lines_route.h, sre_lines_route_key.h).
 *
 * A model's PASS type P is the device's with the rank rule at run time: nd(), bits(), rule(), load(i), taken(item),
 * digit(item), and for the scatter store(r, item, i), which also counts the stores it makes.
 */
#ifndef LINES_PARTITION_SIM_H
#define LINES_PARTITION_SIM_H

#include "sre_lines_route_key.h"
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace {

/* one slot of 64 lanes in lockstep: what slot_rank of sre_hip_lines_rank.h does with __ballot / __shfl */
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

    /* the items of (workgroup, slot) of a pass */
    template <class P> void load(const P &p, uint64_t wg, uint32_t slot)
    {
        for (uint32_t x = 0; x < 64; x++) {
            const uint64_t it = p.load(sre_lr_line(wg, slot, x));
            sel[x] = p.taken(it);
            digit[x] = p.digit(it);
        }
    }

    /* returns the ballots taken behind the first: under SRE_LRK_RANK_TURNS the turns of the loop */
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

/* the slots of workgroup w of n items: c[slot][digit] as slot_rank leaves it, rk[slot * 64 + lane] when rk != NULL.
 * Returns the most ballots any slot took */
template <class P>
uint32_t
sim_slots(const P &p, uint64_t w, std::vector<uint32_t> &c, uint32_t *rk)
{
    const uint32_t nd = p.nd();
    uint32_t       most = 0;
    SimSlot        s;
    c.assign(SRE_LR_SLOTS * nd, 0);
    for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
        for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
            const uint32_t slot = sre_lr_slot(v, q);
            s.load(p, w, slot);
            const uint32_t b = s.run(p.rule(), p.bits(), c.data() + slot * nd);
            if (b > most) most = b;
            for (uint32_t x = 0; rk && x < 64; x++) rk[slot * 64 + x] = s.rank[x];
        }
    }
    return most;
}

/* count of a pass over n items: cnt[d * nwg + w]; writes[] (or NULL) counts the stores to every word of cnt.  Returns the
 * most ballots any slot took */
template <class P>
uint32_t
sim_count(const P &p, uint64_t n, uint64_t *cnt, uint32_t *writes)
{
    const uint64_t        nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    const uint32_t        nd = p.nd();
    uint32_t              most = 0;
    std::vector<uint32_t> c;
    for (uint64_t w = 0; w < nwg; w++) {
        const uint32_t b = sim_slots(p, w, c, NULL);
        if (b > most) most = b;
        for (uint32_t d = 0; d < nd; d++) {
            const uint64_t at = sre_lr_cnt_index(d, nwg, w);
            cnt[at] = sre_lr_slot_prefix(c.data() + d, nd);
            if (writes) writes[at]++;
        }
    }
    return most;
}

/* the scan as the filter's scan leaves it: exclusive, the total behind the last word */
inline void
sim_scan(uint64_t *v, uint64_t n)
{
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t x = v[i];
        v[i] = run;
        run += x;
    }
    v[n] = run;
}

/* scatter of a pass over the scanned counts: p.store(rank, item, i) for every taken item.  Returns the stores that fell
 * outside [0, total) */
template <class P>
uint64_t
sim_scatter(P &p, uint64_t n, const uint64_t *first, uint64_t total)
{
    const uint64_t        nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    const uint32_t        nd = p.nd();
    uint64_t              bad = 0;
    std::vector<uint32_t> c, rk(SRE_LR_ITEMS, 0);
    std::vector<uint64_t> gbase(nd, 0);
    for (uint64_t w = 0; w < nwg; w++) {
        (void) sim_slots(p, w, c, rk.data());
        for (uint32_t d = 0; d < nd; d++) {
            (void) sre_lr_slot_prefix(c.data() + d, nd);
            gbase[d] = first[sre_lr_cnt_index(d, nwg, w)];
        }
        for (uint32_t slot = 0; slot < SRE_LR_SLOTS; slot++) {
            for (uint32_t x = 0; x < 64; x++) {
                const uint64_t i = sre_lr_line(w, slot, x);
                const uint64_t it = p.load(i);
                if (!p.taken(it)) continue;
                const uint32_t d = p.digit(it);
                const uint64_t r = gbase[d] + c[slot * nd + d] + rk[slot * 64 + x];
                if (r >= total) {
                    bad++;
                    continue;
                }
                p.store(r, it, i);
            }
        }
    }
    return bad;
}

}  // namespace

#endif
