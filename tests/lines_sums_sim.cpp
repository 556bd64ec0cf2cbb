/*
 * lines_sums_sim.cpp — the sums kernel of the line tally on the CPU: the lanes of every wave do what sre_k_tally_sums
 * does with the rules it compiles (sregex_amd/csrc/sre_lines_sums.h): who takes part, the groups of a wave by key number,
 * the merge of a group's contributions over the 64 lanes, and what the group's lowest lane sends.  The waves run in the
 * order tests/test_lines_sums_model.py picks.  Every atomic goes through a Mem that applies it one at a time and logs
 * (wave, aggregate, quantity), so the test can count them per wave, address and quantity.  A wave sends to its copy of
 * the rows (sre_ls_copy_of); the copies are merged into the caller's rows at the end, as sre_k_tally_sums_merge does.
 */
#include "sre_lines_sums.h"
#include <stdint.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

namespace {

struct SimVals {
    const uint8_t  *buf;
    const uint64_t *vval, *vstart;
    uint32_t        v;
    uint64_t val(uint64_t line, uint32_t c) const { return vval[line * v + c]; }
    uint64_t raw(uint64_t line, uint32_t c) const { return vstart[line * v + c]; }
    uint8_t  byte(uint64_t at) const { return buf[at]; }
};

struct SimText {
    const uint8_t *p;
    uint8_t byte(uint64_t at) const { return p[at]; }
};

enum { Q_SUM = 0, Q_MIN = 1, Q_MAX = 2, Q_N = 3 };

struct SimMem {
    sre_ls_agg_t *sums;         /* the wave's copy */
    uint64_t      count;        /* aggregates of a copy: rows * v */
    uint64_t      wave;
    uint64_t     *log, log_cap, nlog, bad;
    bool note(uint64_t idx, uint64_t q)
    {
        if (nlog < log_cap) {
            log[3 * nlog] = wave;
            log[3 * nlog + 1] = idx;
            log[3 * nlog + 2] = q;
        }
        nlog++;
        if (idx >= count) bad++;
        return idx < count;
    }
    void add_sum(uint64_t idx, int64_t v) { if (note(idx, Q_SUM)) sums[idx].sum = (int64_t) ((uint64_t) sums[idx].sum + (uint64_t) v); }
    void min(uint64_t idx, int64_t v) { if (note(idx, Q_MIN) && v < sums[idx].min) sums[idx].min = v; }
    void max(uint64_t idx, int64_t v) { if (note(idx, Q_MAX) && v > sums[idx].max) sums[idx].max = v; }
    void add_n(uint64_t idx, uint64_t v) { if (note(idx, Q_N)) sums[idx].n += v; }
};

/* one wave of sre_k_tally_sums: lanes base .. base + 63, the lines below n.  Returns the turns of its grouping loop */
uint32_t
wave(const SimVals &vals, uint64_t base, uint64_t n, const uint32_t *lslot, const uint64_t *cnt, uint64_t rows, SimMem &mem)
{
    uint64_t key[64], members[64];
    bool     part[64];
    uint64_t rem = 0;
    uint32_t turns = 0;
    for (uint32_t x = 0; x < 64; x++) {
        const uint64_t i = base + x;
        const uint32_t slot = i < n ? lslot[i] : SRE_LT_NONE;
        key[x] = slot != SRE_LT_NONE ? cnt[slot] : 0;
        part[x] = sre_ls_takes_part(slot, key[x], rows);
        members[x] = 0;
        if (part[x]) rem |= (uint64_t) 1 << x;
    }
    while (rem) {
        const uint32_t lead = sre_lr_leader(rem);
        uint64_t       m = 0;
        for (uint32_t x = 0; x < 64; x++) {
            if (((rem >> x) & 1u) != 0 && key[x] == key[lead]) m |= (uint64_t) 1 << x;
        }
        for (uint32_t x = 0; x < 64; x++) {
            if ((m >> x) & 1u) members[x] = m;
        }
        rem &= ~m;
        turns++;
    }
    uint64_t shared = 0;
    bool     alone[64];
    for (uint32_t x = 0; x < 64; x++) {
        alone[x] = part[x] && sre_lr_popc(members[x]) == 1;
        if (part[x] && !alone[x] && sre_lr_leader(members[x]) == x) shared |= (uint64_t) 1 << x;
    }
    for (uint32_t c = 0; c < vals.v; c++) {
        sre_ls_agg_t a[64];
        for (uint32_t x = 0; x < 64; x++) a[x] = part[x] ? sre_ls_line(vals, base + x, c) : sre_ls_identity();
        for (uint32_t x = 0; x < 64; x++) {
            if (alone[x]) sre_ls_flush(mem, sre_ls_index(key[x], vals.v, c), a[x]);
        }
        for (uint64_t todo = shared; todo; todo &= todo - 1) {
            const uint32_t lead = sre_lr_leader(todo);
            const uint64_t m = members[lead];
            bool           any = false;
            for (uint32_t x = 0; x < 64; x++) any = any || (((m >> x) & 1u) != 0 && a[x].n != 0);
            if (!any) continue;
            sre_ls_agg_t g = sre_ls_identity();
            for (uint32_t x = 0; x < 64; x++) g = sre_ls_merge(g, ((m >> x) & 1u) ? a[x] : sre_ls_identity());
            sre_ls_flush(mem, sre_ls_index(key[lead], vals.v, c), g);
        }
    }
    return turns;
}

}  // namespace

extern "C" {

uint32_t lssim_none(void) { return SRE_LT_NONE; }
uint32_t lssim_max_values(void) { return SRE_LS_MAX_VALUES; }
uint32_t lssim_agg_bytes(void) { return (uint32_t) sizeof(sre_ls_agg_t); }
uint32_t lssim_copies(uint64_t rows, uint32_t v) { return sre_ls_copies(rows, v); }

/* the number rule as the kernel compiles it */
int
lssim_number(const uint8_t *text, uint64_t len, int64_t *value)
{
    const SimText t = {text};
    return sre_ls_number(t, 0, len, value) ? 1 : 0;
}

/*
 * The init and the sums kernel over n lines of v value columns.  lslot: n words; cnt: the key number of every slot; sums:
 * the caller's array, of which rows * v aggregates are written and nothing else may be touched.  copies: 0 for the
 * rule's number (sre_ls_copies), else that many; with one the waves send to the caller's array itself.
 * schedule 0: the waves in line order, 1: in random order, 2: reversed.  log: log_cap records [wave, aggregate, quantity]
 * of the atomics made.  words[0 .. 4): atomics made, atomics outside rows * v, turns of the grouping loops, copies used.
 * Returns the atomics made.
 */
uint64_t
lssim_sums(const uint8_t *buf, const uint64_t *vval, const uint64_t *vstart, uint64_t n, uint32_t v, const uint32_t *lslot,
           const uint64_t *cnt, uint64_t rows, void *sums, uint32_t copies, int schedule, uint64_t seed, uint64_t *log,
           uint64_t log_cap, uint64_t *words)
{
    const SimVals vals = {buf, vval, vstart, v};
    const uint64_t count = rows * v;
    if (copies == 0) copies = sre_ls_copies(rows, v);
    sre_ls_agg_t             *out = static_cast<sre_ls_agg_t *>(sums);
    std::vector<sre_ls_agg_t> copy(copies > 1 ? count * copies : 0);
    sre_ls_agg_t             *to = copies > 1 ? copy.data() : out;
    SimMem                    mem = {to, count, 0, log, log_cap, 0, 0};
    for (uint64_t x = 0; x < count * copies; x++) to[x] = sre_ls_identity();
    const uint64_t        nw = (n + 63) / 64;
    std::vector<uint64_t> order(nw);
    std::iota(order.begin(), order.end(), (uint64_t) 0);
    if (schedule == 1) {
        std::mt19937_64 rng(seed);
        std::shuffle(order.begin(), order.end(), rng);
    } else if (schedule == 2) {
        std::reverse(order.begin(), order.end());
    }
    uint64_t turns = 0;
    for (uint64_t w : order) {
        mem.wave = w;
        mem.sums = to + (uint64_t) sre_ls_copy_of(w, copies) * count;
        turns += wave(vals, w * 64, n, lslot, cnt, rows, mem);
    }
    for (uint64_t x = 0; copies > 1 && x < count; x++) {
        sre_ls_agg_t a = sre_ls_identity();
        for (uint32_t c = 0; c < copies; c++) a = sre_ls_merge(a, to[(uint64_t) c * count + x]);
        out[x] = a;
    }
    words[0] = mem.nlog;
    words[1] = mem.bad;
    words[2] = turns;
    words[3] = copies;
    return mem.nlog;
}

}
