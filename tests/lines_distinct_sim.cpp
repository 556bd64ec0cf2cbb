/*
 * lines_distinct_sim.cpp — the passes of the line distinct on the CPU (sregex_amd/csrc/sre_lines_distinct.h), behind the
 * tally model's insert (tests/lines_tally_sim.cpp), whose table, counts and per-line slots they take.  The `last` pass
 * groups the 64 lanes of a wave by slot as sre_k_distinct_last does, ballot by ballot, and collects one atomic maximum
 * per group, which a schedule then applies in an order of its choice; `pick` and `perline` are the header's rules over a
 * table that counts every read and refuses one outside it.
 */
#include "sre_lines_distinct.h"
#include "sre_lines_tally.h"
#include "sre_lines_route.h"
#include <stdint.h>
#include <algorithm>
#include <random>
#include <utility>
#include <vector>

namespace {

struct SimTab {
    const uint64_t *tab, *cnt, *lastrun;
    uint64_t        nslots;
    uint64_t       *reads, *bad;
    uint64_t get(const uint64_t *run, uint32_t slot) const
    {
        ++*reads;
        if (run == nullptr || slot >= nslots) {
            ++*bad;
            return 0;
        }
        return run[slot];
    }
    uint64_t first(uint32_t slot) const { return get(tab, slot); }
    uint64_t count(uint32_t slot) const { return get(cnt, slot); }
    uint64_t last(uint32_t slot) const { return get(lastrun, slot); }
};

}  // namespace

extern "C" {

uint32_t ldsim_threads(void) { return SRE_LD_THREADS; }

int
ldsim_range_ok(uint64_t min_count, uint64_t max_count)
{
    return sre_ld_range_ok(min_count, max_count);
}

int
ldsim_picks(int which, uint64_t min_count, uint64_t max_count, int invert, uint64_t line, uint64_t first, uint64_t last,
            uint64_t count)
{
    return sre_ld_picks(which, min_count, max_count, invert != 0, line, first, last, count);
}

/*
 * The last pass over n lines.  lslot: the insert's slots; lastrun: nslots words, 0 before.  schedule: 0 the atomics in
 * line order, 1 and 2 in a random order, 3 from the highest line down.  words[0 .. 4): atomics sent, turns of the
 * grouping loops, accesses outside the table, the sum over the waves of their distinct slots (what words[0] has to be).
 */
void
ldsim_last(const uint32_t *lslot, uint64_t n, uint64_t nslots, int schedule, uint64_t seed, uint64_t *lastrun, uint64_t *words)
{
    std::vector<std::pair<uint32_t, uint64_t>> sends;
    uint64_t                                   turns = 0, bad = 0, distinct = 0;
    for (uint64_t base = 0; base < n; base += 64) {
        uint32_t slot[64];
        uint64_t rem = 0;
        for (uint32_t x = 0; x < 64; x++) {
            slot[x] = base + x < n ? lslot[base + x] : SRE_LT_NONE;
            if (slot[x] != SRE_LT_NONE) rem |= (uint64_t) 1 << x;
        }
        std::vector<uint32_t> seen;
        for (uint32_t x = 0; x < 64; x++) {
            if (slot[x] != SRE_LT_NONE && std::find(seen.begin(), seen.end(), slot[x]) == seen.end()) seen.push_back(slot[x]);
        }
        distinct += seen.size();
        while (rem) {
            const uint32_t lead = sre_lr_leader(rem);
            uint64_t       m = 0;
            for (uint32_t x = 0; x < 64; x++) {
                if (((rem >> x) & 1u) != 0 && slot[x] == slot[lead]) m |= (uint64_t) 1 << x;
            }
            const uint32_t sender = sre_ld_sender(m);
            sends.push_back(std::make_pair(slot[sender], base + sender));
            rem &= ~m;
            turns++;
        }
    }
    std::mt19937_64 rng(seed);
    if (schedule == 1 || schedule == 2) std::shuffle(sends.begin(), sends.end(), rng);
    if (schedule == 3) std::reverse(sends.begin(), sends.end());
    for (const auto &s : sends) {
        if (s.first >= nslots) {
            bad++;
            continue;
        }
        if (s.second > lastrun[s.first]) lastrun[s.first] = s.second;       /* one access at a time is what an atomic is */
    }
    words[0] = sends.size();
    words[1] = turns;
    words[2] = bad;
    words[3] = distinct;
}

/*
 * The pick pass over n lines: fval[i] stays or becomes 0.  lastrun may be NULL unless which is SRE_LD_LAST.
 * words[0 .. 4): the qualifying keys, table reads, reads outside the table (or through a missing run), adds to the
 * call's word (one per workgroup with a key to count).
 */
void
ldsim_pick(const uint32_t *lslot, uint64_t n, uint64_t nslots, const uint64_t *tab, const uint64_t *cnt, const uint64_t *lastrun,
           int which, uint64_t min_count, uint64_t max_count, int invert, uint64_t *fval, uint64_t *words)
{
    uint64_t     reads = 0, bad = 0, kept = 0, adds = 0;
    const SimTab t = {tab, cnt, lastrun, nslots, &reads, &bad};
    for (uint64_t base = 0; base < n; base += SRE_LD_THREADS) {
        uint64_t a = 0;
        for (uint64_t i = base; i < n && i < base + SRE_LD_THREADS; i++) {
            bool           counts = false;
            const uint64_t before = reads;
            fval[i] = sre_ld_value(t, which, min_count, max_count, invert != 0, i, lslot[i], fval[i], &counts);
            if (lslot[i] == SRE_LT_NONE && reads != before) bad++;         /* a line without a slot read the table */
            a += counts;
        }
        if (a) adds++;
        kept += a;
    }
    words[0] = kept;
    words[1] = reads;
    words[2] = bad;
    words[3] = adds;
}

/* the per-line arrays: the first kc words of keycount and kl words of keyline; returns the reads outside the table */
uint64_t
ldsim_perline(const uint32_t *lslot, uint64_t nslots, const uint64_t *tab, const uint64_t *cnt, uint64_t *keycount, uint64_t kc,
              int64_t *keyline, uint64_t kl)
{
    uint64_t     reads = 0, bad = 0;
    const SimTab t = {tab, cnt, nullptr, nslots, &reads, &bad};
    for (uint64_t i = 0; i < kc || i < kl; i++) {
        if (i < kc) keycount[i] = sre_ld_keycount(t, lslot[i]);
        if (i < kl) keyline[i] = sre_ld_keyline(t, lslot[i]);
    }
    return bad;
}

}
