/*
 * lines_tally_sim.cpp — the line tally's insert on the CPU: every lane a state machine of the steps the kernel compiles
 * (sregex_amd/csrc/sre_lines_tally.h), one atomic access per step, run under a schedule the caller picks, so that
 * tests/test_lines_tally_model.py can put lanes to sleep between any two accesses.  A wave of 64 consecutive lines
 * groups its lines by key first (the wave rule on sre_lt_same_key; only a group's lowest lane searches) and settles when
 * its last lane is done, as the kernel's does: its selected lines, its claims, every leader's group to the count of its
 * slot.  Every access is counted.  The keep pass is the header's rule too.
 */
#include "sre_lines_tally.h"
#include <stdint.h>
#include <random>
#include <vector>

namespace {

struct SimKeys {
    const uint8_t  *buf;
    const uint64_t *val, *start;
    uint32_t        k;
    bool     selected(uint64_t line) const { return val[line * k] != 0; }
    uint64_t len(uint64_t line, uint32_t f) const { return val[line * k + f] - 1; }
    uint8_t  byte(uint64_t line, uint32_t f, uint64_t j) const { return buf[(start[line * k + f] & SRE_LG_ENTRY_START) + j]; }
};

/* one access at a time is what an atomic is */
struct SimMem {
    uint64_t *tab;
    uint64_t  nslots;
    uint64_t *cnt;
    uint64_t  tsel, tclaims, tover;
    uint64_t  ncas, nmin, nadds, bad;
    uint64_t cas(uint64_t idx, uint64_t expect, uint64_t v)
    {
        ncas++;
        if (idx >= nslots) {
            bad++;
            return 0;
        }
        const uint64_t old = tab[idx];
        if (old == expect) tab[idx] = v;
        return old;
    }
    void min(uint64_t idx, uint64_t v)
    {
        nmin++;
        if (idx >= nslots) {
            bad++;
            return;
        }
        if (v < tab[idx]) tab[idx] = v;
    }
    bool raised() { return tover != 0; }
    void add(uint32_t slot, uint64_t v)
    {
        nadds++;
        if (slot >= nslots) {
            bad++;
            return;
        }
        cnt[slot] += v;
    }
};

/* a wave's groups as sre_k_tally_insert forms them; nl: lanes of the wave that are lines.  Returns the turns */
uint32_t
group(const SimKeys &keys, uint64_t base, const bool *sel, const uint64_t *h, uint32_t nl, uint32_t *lead_of, uint32_t *size)
{
    uint64_t rem = 0;
    uint32_t turns = 0;
    for (uint32_t x = 0; x < nl; x++) {
        lead_of[x] = x;
        size[x] = 0;
        if (sel[x]) rem |= (uint64_t) 1 << x;
    }
    while (rem) {
        const uint32_t lead = sre_lr_leader(rem);
        uint64_t       m = 0;
        for (uint32_t x = 0; x < nl; x++) {
            if (((rem >> x) & 1u) != 0 && sre_lt_same_key(keys, h[x], base + x, h[lead], base + lead)) {
                m |= (uint64_t) 1 << x;
                lead_of[x] = lead;
            }
        }
        size[lead] = sre_lr_popc(m);
        rem &= ~m;
        turns++;
    }
    return turns;
}

/* what sre_k_tally_insert does behind the searches of a wave's leaders */
void
settle(const sre_lt_lane_t *L, const bool *sel, const uint32_t *lead_of, const uint32_t *size, uint32_t nl, SimMem &mem,
       const sre_lt_params_t &p, uint32_t *lslot)
{
    uint64_t msel = 0, mclaim = 0, mwrap = 0;
    for (uint32_t x = 0; x < nl; x++) {
        if (sel[x]) msel |= (uint64_t) 1 << x;
        if (L[x].claimed) mclaim |= (uint64_t) 1 << x;
        if (L[x].wrapped) mwrap |= (uint64_t) 1 << x;
    }
    bool over = mwrap != 0;
    if (msel) mem.tsel += sre_lr_popc(msel);
    if (mclaim) {
        const uint32_t mine = sre_lr_popc(mclaim);
        const uint64_t base = mem.tclaims;
        mem.tclaims += mine;
        over = over || sre_lt_claims_overflow(base, mine, p);
    }
    if (over) mem.tover = 1;
    for (uint32_t x = 0; x < nl; x++) {
        const bool leads = sel[x] && lead_of[x] == x;
        if (leads && L[x].slot != SRE_LT_NONE) mem.add(L[x].slot, size[x]);
        lslot[x] = sel[x] ? L[lead_of[x]].slot : SRE_LT_NONE;
    }
}

}  // namespace

extern "C" {

uint64_t ltsim_empty(void) { return SRE_LT_EMPTY; }
uint32_t ltsim_none(void) { return SRE_LT_NONE; }
uint64_t ltsim_nslots(uint64_t max_keys) { return sre_lt_nslots(max_keys); }
uint32_t ltsim_flag_every(void) { return SRE_LT_FLAG_EVERY; }

uint64_t
ltsim_hash(const uint8_t *buf, const uint64_t *val, const uint64_t *start, uint32_t k, uint64_t line)
{
    const SimKeys keys = {buf, val, start, k};
    return sre_lt_hash(keys, line);
}

/*
 * The whole insert over n lines of k fields.  tab: nslots words, SRE_LT_EMPTY before; cnt: nslots words, 0 before;
 * lslot: n words.  schedule:
 *   0  line order, every lane to its end before the next begins;
 *   1  random: of all lanes that are not done a random one makes one step; a wave whose lanes are all done settles at a
 *      random later time;
 *   2  as 1, but a lane that has seen an equal key (the CAS is behind it, the minimum in front) sleeps until no lane is
 *      left in its search, and the sleepers then wake in random order;
 *   3  round robin from the HIGHEST line down, one step a turn: every lane's first CAS comes before anybody's second.
 * words[0 .. 9): tsel, tclaims, tover, CAS made, minimums made, adds to the counts, accesses outside the table, steps,
 * turns of the grouping loops.
 * Returns the steps.
 */
uint64_t
ltsim_insert(const uint8_t *buf, const uint64_t *val, const uint64_t *start, uint64_t n, uint32_t k, uint64_t max_keys,
             int hash_bits, int schedule, uint64_t seed, uint64_t *tab, uint64_t *cnt, uint32_t *lslot, uint64_t *words)
{
    const SimKeys   keys = {buf, val, start, k};
    sre_lt_params_t p;
    p.nslots = sre_lt_nslots(max_keys);
    p.max_keys = max_keys;
    p.hash_mask = sre_lt_hash_mask(hash_bits);
    SimMem                     mem = {tab, p.nslots, cnt, 0, 0, 0, 0, 0, 0, 0};
    std::mt19937_64            rng(seed);
    const uint64_t             nw = (n + 63) / 64;
    std::vector<sre_lt_lane_t> L(nw * 64);
    std::vector<char>          selv(nw * 64, 0);
    std::vector<uint32_t>      left(nw, 0);      /* lanes of the wave that are not done */
    std::vector<uint64_t>      ready;            /* waves that wait to settle */
    uint64_t                   steps = 0;

    std::vector<uint32_t> lead_of(nw * 64, 0), size(nw * 64, 0);
    std::vector<uint64_t> hash(nw * 64, 0);
    uint64_t              turns = 0;
    auto lanes_of = [&](uint64_t w) { return (uint32_t) (n - w * 64 < 64 ? n - w * 64 : 64); };
    auto settle_wave = [&](uint64_t w) {
        const uint32_t nl = lanes_of(w);
        bool           sel[64];
        for (uint32_t x = 0; x < nl; x++) sel[x] = selv[w * 64 + x] != 0;
        settle(L.data() + w * 64, sel, lead_of.data() + w * 64, size.data() + w * 64, nl, mem, p, lslot + w * 64);
    };
    /* a wave begins: hashes, groups, and the searches of its leaders */
    auto begin_wave = [&](uint64_t w) {
        const uint32_t nl = lanes_of(w);
        bool           sel[64];
        for (uint32_t x = 0; x < nl; x++) {
            const uint64_t i = w * 64 + x;
            sel[x] = keys.selected(i);
            selv[i] = sel[x];
            hash[i] = sel[x] ? sre_lt_hash(keys, i) : 0;
        }
        turns += group(keys, w * 64, sel, hash.data() + w * 64, nl, lead_of.data() + w * 64, size.data() + w * 64);
        for (uint32_t x = 0; x < nl; x++) {
            const uint64_t i = w * 64 + x;
            sre_lt_begin(L[i], i, sel[x] && lead_of[i] == x, hash[i], p);
            if (!sre_lt_done(L[i])) left[w]++;
        }
    };
    auto step = [&](uint64_t i) {
        sre_lt_step(L[i], keys, mem, p);
        steps++;
        if (sre_lt_done(L[i]) && --left[i / 64] == 0) ready.push_back(i / 64);
    };

    if (schedule == 0) {
        for (uint64_t w = 0; w < nw; w++) {
            begin_wave(w);
            for (uint64_t i = w * 64; i < n && i < w * 64 + 64; i++) {
                while (!sre_lt_done(L[i])) step(i);
            }
            settle_wave(w);
        }
        ready.clear();
    } else {
        std::vector<uint64_t> live, asleep;
        for (uint64_t w = 0; w < nw; w++) {
            begin_wave(w);
            if (left[w] == 0) ready.push_back(w);
        }
        for (uint64_t i = 0; i < n; i++) {
            if (!sre_lt_done(L[i])) live.push_back(i);
        }
        if (schedule == 3) {
            while (!live.empty()) {
                std::vector<uint64_t> next;
                for (size_t q = live.size(); q-- > 0;) {
                    step(live[q]);
                    if (!sre_lt_done(L[live[q]])) next.push_back(live[q]);
                }
                live.assign(next.rbegin(), next.rend());
            }
        } else {
            while (!live.empty() || !asleep.empty()) {
                if (live.empty()) {
                    live.swap(asleep);          /* nobody searches any more: the sleepers make their minimums */
                    continue;
                }
                if (!ready.empty() && rng() % 8 == 0) {
                    const size_t q = rng() % ready.size();
                    settle_wave(ready[q]);
                    ready[q] = ready.back();
                    ready.pop_back();
                    continue;
                }
                const size_t   q = rng() % live.size();
                const uint64_t i = live[q];
                step(i);
                if (sre_lt_done(L[i])) {
                    live[q] = live.back();
                    live.pop_back();
                } else if (schedule == 2 && L[i].state == SRE_LT_LOWER) {
                    asleep.push_back(i);
                    live[q] = live.back();
                    live.pop_back();
                }
            }
        }
        /* the waves that have not settled yet, in random order */
        while (!ready.empty()) {
            const size_t q = schedule == 3 ? ready.size() - 1 : rng() % ready.size();
            settle_wave(ready[q]);
            ready[q] = ready.back();
            ready.pop_back();
        }
    }
    words[0] = mem.tsel;
    words[1] = mem.tclaims;
    words[2] = mem.tover;
    words[3] = mem.ncas;
    words[4] = mem.nmin;
    words[5] = mem.nadds;
    words[6] = mem.bad;
    words[7] = steps;
    words[8] = turns;
    return steps;
}

/* the keep pass over the n * k entries */
void
ltsim_keep(uint64_t *val, uint64_t n, uint32_t k, const uint64_t *tab, const uint32_t *lslot)
{
    for (uint64_t e = 0; e < n * k; e++) {
        const uint64_t line = e / k;
        if (!sre_lt_keeps(lslot[line], line, tab)) val[e] = 0;
    }
}

}
