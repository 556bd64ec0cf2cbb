/*
 * lines_keyset_sim.cpp — the key set and the lookup's probe on the CPU, from the text the kernels compile
 * (sregex_amd/csrc/sre_lines_keyset.h and sre_lines_tally.h): the dictionary's field rule row by row, the insert of the
 * rows with every lane a state machine of sre_lt_step, one atomic access per step under a schedule the caller picks (the
 * schedules of tests/lines_tally_sim.cpp), the hash through both Keys types, and the read-only probe one table read per
 * step, with the key id, selection and counts rule.  Every access is counted; one outside the table is counted and
 * not made.
 */
#include "sre_lines_keyset.h"
#include <stdint.h>
#include <random>
#include <vector>

namespace {

struct SimBytes {
    const uint8_t *p;
    uint8_t byte(uint64_t at) const { return p[at]; }
};

/* one access at a time is what an atomic is */
struct InsertMem {
    uint64_t *tab;
    uint64_t  nslots;
    uint64_t  ncas, nmin, bad;
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
    bool raised() { return false; }
};

struct ProbeMem {
    const uint64_t   *tab;
    uint64_t          nslots;
    mutable uint64_t  loads, bad;
    uint64_t load(uint64_t idx) const
    {
        loads++;
        if (idx >= nslots) {
            bad++;
            return SRE_LT_EMPTY;
        }
        return tab[idx];
    }
};

sre_lt_params_t
params(uint64_t nslots, int hash_bits)
{
    sre_lt_params_t p;
    p.nslots = nslots;
    p.max_keys = nslots / 2;
    p.hash_mask = sre_lt_hash_mask(hash_bits);
    return p;
}

}  // namespace

extern "C" {

uint64_t lksim_empty(void) { return SRE_LT_EMPTY; }
uint64_t lksim_no_row(void) { return SRE_LK_NO_ROW; }
uint64_t lksim_nslots(uint64_t rows) { return sre_lk_nslots(rows); }
uint64_t lksim_max_rows(void) { return SRE_LK_MAX_ROWS; }

/* the dictionary rule over row ends the caller made (the split is line mode's): the fields of every row into
 * fstart / flen (rows * k entries); returns the lowest row that breaks the field rule, SRE_LK_NO_ROW when none does */
uint64_t
lksim_fields(const uint8_t *buf, const uint64_t *ends, uint64_t rows, uint32_t k, uint32_t fsep, uint64_t *fstart, uint64_t *flen)
{
    const SimBytes b = {buf};
    uint64_t       bad = SRE_LK_NO_ROW;
    /* (from the highest row down: the lowest bad row must come out whatever the order of arrival) */
    for (uint64_t r = rows; r-- > 0;) {
        uint64_t st, end;
        sre_lk_row_span(ends, r, &st, &end);
        if (!sre_lk_row_fields(b, st, end, k, fsep, fstart + r * k, flen + r * k) && r < bad) bad = r;
    }
    return bad;
}

uint64_t
lksim_hash_row(const uint8_t *buf, const uint64_t *fstart, const uint64_t *flen, uint32_t k, uint64_t row)
{
    const sre_lk_dict_keys keys = {buf, fstart, flen, k};
    return sre_lt_hash(keys, row);
}

uint64_t
lksim_hash_line(const uint8_t *buf, const uint64_t *val, const uint64_t *start, uint32_t k, uint64_t line)
{
    const sre_lk_line_keys keys = {buf, val, start, k};
    return sre_lt_hash(keys, line);
}

/*
 * The insert of `rows` rows, every row the leader of its own search.  tab: nslots words, SRE_LT_EMPTY before.  schedule:
 *   0  row order, every lane to its end before the next begins;
 *   1  random: of all lanes that are not done a random one makes one step;
 *   2  as 1, but a lane that has seen an equal key (the CAS is behind it, the minimum in front) sleeps until no lane is
 *      left in its search, and the sleepers then wake in random order;
 *   3  round robin from the HIGHEST row down, one step a turn.
 * words[0 .. 5): claims (the distinct keys), CAS made, minimums made, accesses outside the table, steps.
 */
void
lksim_insert(const uint8_t *buf, const uint64_t *fstart, const uint64_t *flen, uint64_t rows, uint32_t k, uint64_t nslots,
             int hash_bits, int schedule, uint64_t seed, uint64_t *tab, uint64_t *words)
{
    const sre_lk_dict_keys     keys = {buf, fstart, flen, k};
    const sre_lt_params_t      p = params(nslots, hash_bits);
    InsertMem                  mem = {tab, nslots, 0, 0, 0};
    std::mt19937_64            rng(seed);
    std::vector<sre_lt_lane_t> L(rows);
    uint64_t                   steps = 0, claims = 0;
    for (uint64_t r = 0; r < rows; r++) sre_lt_begin(L[r], r, true, sre_lt_hash(keys, r), p);
    auto step = [&](uint64_t r) {
        sre_lt_step(L[r], keys, mem, p);
        steps++;
    };
    if (schedule == 0) {
        for (uint64_t r = 0; r < rows; r++) {
            while (!sre_lt_done(L[r])) step(r);
        }
    } else if (schedule == 3) {
        std::vector<uint64_t> live;
        for (uint64_t r = 0; r < rows; r++) live.push_back(r);
        while (!live.empty()) {
            std::vector<uint64_t> next;
            for (size_t q = live.size(); q-- > 0;) {
                step(live[q]);
                if (!sre_lt_done(L[live[q]])) next.push_back(live[q]);
            }
            live.assign(next.rbegin(), next.rend());
        }
    } else {
        std::vector<uint64_t> live, asleep;
        for (uint64_t r = 0; r < rows; r++) live.push_back(r);
        while (!live.empty() || !asleep.empty()) {
            if (live.empty()) {
                live.swap(asleep);
                continue;
            }
            const size_t   q = rng() % live.size();
            const uint64_t r = live[q];
            step(r);
            if (sre_lt_done(L[r])) {
                live[q] = live.back();
                live.pop_back();
            } else if (schedule == 2 && L[r].state == SRE_LT_LOWER) {
                asleep.push_back(r);
                live[q] = live.back();
                live.pop_back();
            }
        }
    }
    for (uint64_t r = 0; r < rows; r++) {
        if (L[r].claimed) claims++;
        if (L[r].wrapped || L[r].slot == SRE_LT_NONE) mem.bad++;         /* (cannot happen at load <= 1/2) */
    }
    words[0] = claims;
    words[1] = mem.ncas;
    words[2] = mem.nmin;
    words[3] = mem.bad;
    words[4] = steps;
}

/*
 * The probe pass over n lines as sre_k_keyset_probe makes it: keyid[i] for i < keyid_n, fval[i] kept or cleared.
 * words[0 .. 5): keyed lines, members, table reads, reads outside the table, the most reads one line made.
 * Returns the steps in which more than one read was made (the rule allows none).
 */
uint64_t
lksim_probe(const uint8_t *src, const uint64_t *vval, const uint64_t *vstart, uint64_t n, uint32_t k, const uint8_t *dict,
            const uint64_t *fstart, const uint64_t *flen, const uint64_t *tab, uint64_t nslots, int hash_bits, int invert,
            uint64_t *fval, int64_t *keyid, uint64_t keyid_n, uint64_t *words)
{
    const sre_lk_line_keys lines = {src, vval, vstart, k};
    const sre_lk_dict_keys rows = {dict, fstart, flen, k};
    const sre_lt_params_t  p = params(nslots, hash_bits);
    const ProbeMem         mem = {tab, nslots, 0, 0};
    uint64_t               nkeyed = 0, nmembers = 0, most = 0, twice = 0;
    for (uint64_t i = 0; i < n; i++) {
        const bool     keyed = lines.selected(i);
        sre_lk_probe_t P;
        P.id = SRE_LK_NOT_MEMBER;
        if (keyed) {
            const uint64_t before = mem.loads;
            sre_lk_probe_begin(P, sre_lt_hash(lines, i), p);
            while (!P.done) {
                const uint64_t at = mem.loads;
                sre_lk_probe_step(P, i, lines, rows, mem, p);
                if (mem.loads - at > 1) twice++;
            }
            if (mem.loads - before > most) most = mem.loads - before;
        }
        if (i < keyid_n) keyid[i] = sre_lk_keyid(keyed, P.id);
        fval[i] = sre_lk_value(keyed, P.id, invert != 0, fval[i]);
        nkeyed += keyed;
        nmembers += keyed && P.id >= 0;
    }
    words[0] = nkeyed;
    words[1] = nmembers;
    words[2] = mem.loads;
    words[3] = mem.bad;
    words[4] = most;
    return twice;
}

}
