/* tools/asan_tally_top_rule.cpp — CPU-only AddressSanitizer / UBSan run of the rules of the ordered tally
 * (sregex_amd/csrc/sre_lines_tally_top.h, what its kernels and the host code compile) through the CPU model
 * (tests/lines_tally_top_sim.cpp, compiled into this program): the first lines, the order values and their totals, every digit
 * pass over the keys, the ordered table in front of the limit, its scan, the permute and the ranks.  Every array is a heap
 * block of exactly the size the call gives it: nslots words of table and of key numbers, n slots, nkeys counts, first lines,
 * values, one-byte classes and inverse ranks, nkeys x v aggregates, n x k + 1 words of the entry table, 256 x ceil(nkeys /
 * 1024) + 1 counts, nkeys keys and 32-bit key numbers for each pair of item arrays, nrows x k starts and nrows x k + 1 values,
 * the caller's arrays at their caps, so one word read or written past any of them is reported; the key arithmetic at the
 * largest range a call may have (2^64 - 3) runs under UBSan.
 *   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -Isregex_amd/csrc tools/asan_tally_top_rule.cpp \
 *       -o /tmp/asan_tally_top && /tmp/asan_tally_top
 */
#include "../tests/lines_tally_top_sim.cpp"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

template <class T>
static T *
block(size_t n)
{
    return static_cast<T *>(calloc(n ? n : 1, sizeof(T)));      /* (n == 0: one element that nothing may need) */
}

static uint64_t rng_state = 88172645463325252ull;
static uint64_t
rnd(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "asan_tally_top_rule: %s failed at line %d\n", #cond, __LINE__);    \
            exit(1);                                                                             \
        }                                                                                        \
    } while (0)

/* dist 0: small values with ties; 1: the full 18-digit range; 2: sums at the edges of the largest range a call may have;
 * 3: no key has a number in the order column */
static int64_t
agg_value(int dist, uint64_t k, uint64_t nkeys)
{
    switch (dist) {
    case 0: return (int64_t) (rnd() % 9) - 4;
    case 1: return (int64_t) (rnd() % 1999999999999999999ull) - 999999999999999999ll;
    case 2: return k == 0 ? INT64_MAX : k == nkeys - 1 ? INT64_MIN + 2 : (int64_t) rnd();
    default: return 0;
    }
}

static uint64_t
one_case(uint64_t nkeys, int dist, int by, int desc, uint64_t limit, uint64_t cap_off)
{
    const uint32_t K = 2, V = 2, by_col = 1;
    /* the lines: every key's first line in key order, then up to two more lines of random keys, a line without a key now and then */
    std::vector<int64_t> owner;
    for (uint64_t k = 0; k < nkeys; k++) {
        owner.push_back((int64_t) k);
        for (uint64_t x = rnd() % 3; x > 0; x--) owner.push_back(rnd() % 4 == 0 ? -1 : (int64_t) (rnd() % (k + 1)));
    }
    const uint64_t n = owner.size();
    uint64_t       nslots = 1024;
    while (nslots < 2 * nkeys) nslots *= 2;
    uint64_t *tab = block<uint64_t>(nslots), *cnt = block<uint64_t>(nslots), *counts = block<uint64_t>(nkeys);
    uint32_t *lslot = block<uint32_t>(n);
    int64_t  *aggs = block<int64_t>(4 * nkeys * V);
    uint64_t *off = block<uint64_t>(n * K + 1), *start = block<uint64_t>(n * K), *ends = block<uint64_t>(n);
    for (uint64_t s = 0; s < nslots; s++) tab[s] = SRE_LT_EMPTY;
    std::vector<uint32_t> slot_of(nkeys);
    for (uint64_t k = 0; k < nkeys; k++) {
        uint32_t s = (uint32_t) (rnd() % nslots);
        while (tab[s] != SRE_LT_EMPTY) s = (s + 1) % nslots;
        tab[s] = 0;     /* (claimed; the first line below) */
        slot_of[k] = s;
        for (uint32_t c = 0; c < V; c++) {
            int64_t *g = aggs + 4 * (k * V + c);
            const bool has = dist != 3 && (c == 0 || k % 3 != 1);
            const int64_t x = agg_value(dist, k, nkeys);
            g[0] = has ? x : 0, g[1] = has ? x : INT64_MAX, g[2] = has ? x : INT64_MIN, g[3] = has ? 1 + (int64_t) (rnd() % 3) : 0;
        }
    }
    std::vector<bool> seen(nkeys, false);
    uint64_t          pos = 0, run = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t len = 3 + rnd() % 20;
        ends[i] = pos + len;
        lslot[i] = owner[i] < 0 ? SRE_LT_NONE : slot_of[owner[i]];
        bool kept = false;
        if (owner[i] >= 0) {
            counts[owner[i]]++;
            if (!seen[owner[i]]) seen[owner[i]] = kept = true, tab[slot_of[owner[i]]] = i, cnt[slot_of[owner[i]]] = (uint64_t) owner[i];
        }
        for (uint32_t f = 0; f < K; f++) {
            const uint64_t e = i * K + f, flen = f == 0 ? 1 + rnd() % 2 : rnd() % 2;
            start[e] = (pos + f) | (f == 0 ? SRE_LG_ENTRY_FIRST : 0) | (f == K - 1 ? SRE_LG_ENTRY_LAST : 0) | (f && !flen ? SRE_LG_ENTRY_UNSET : 0);
            off[e] = run;
            run += kept ? flen + 1 : 0;
        }
        pos += len + 1;
    }
    off[n * K] = run;
    /* first lines, order values, totals */
    uint64_t *first = block<uint64_t>(nkeys);
    uint32_t *fw = block<uint32_t>(nkeys), *vw = block<uint32_t>(nkeys);
    CHECK(lttsim_first(tab, lslot, cnt, n, nkeys, first, fw) == 0);
    int64_t *value = block<int64_t>(nkeys);
    int8_t  *cls = block<int8_t>(nkeys);
    uint64_t totals[4];
    uint32_t sent[4] = {0, 0, 0, 0};
    lttsim_values(counts, aggs, nkeys, V, by, by_col, value, cls, vw, totals, sent);
    const uint64_t nord = totals[1], nwg = (nkeys + SRE_LTT_KEYS - 1) / SRE_LTT_KEYS;
    const int64_t  vmin = (int64_t) totals[2], vmax = (int64_t) totals[3];
    CHECK(totals[0] == nkeys && sent[0] == nwg && sent[1] <= nwg && sent[2] == sent[1] && sent[3] == sent[1]);
    CHECK(sre_ltt_range_ok(nord, vmin, vmax));
    /* the digit passes over the keys */
    const uint32_t passes = sre_ltt_passes(nkeys, nord, vmin, vmax);
    const uint64_t ncnt = 256 * ((nkeys + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS);
    uint64_t      *key[2] = {block<uint64_t>(nkeys), block<uint64_t>(nkeys)}, *pc = block<uint64_t>(ncnt + 1);
    uint32_t      *num[2] = {block<uint32_t>(nkeys), block<uint32_t>(nkeys)}, *cw = block<uint32_t>(ncnt + 1);
    uint32_t      *kw = block<uint32_t>(nkeys), *lw = block<uint32_t>(nkeys);
    uint32_t       cur = 0;
    for (uint32_t p = 0; p < passes; p++) {
        const bool f = p == 0;
        lsosim_count(f ? value : NULL, f ? cls : NULL, key[cur], nkeys, vmin, vmax, nord, desc, 1, p, pc, cw);
        lsosim_scan(pc, ncnt);
        CHECK(pc[ncnt] == nkeys);
        const uint32_t to = f ? 0 : cur ^ 1u;
        CHECK(lsosim_scatter(f ? value : NULL, f ? cls : NULL, key[cur], num[cur], nkeys, vmin, vmax, nord, desc, 1, p, pc, nkeys, key[to],
                             num[to], kw, lw) == 0);
        cur = to;
    }
    for (uint64_t r = 1; r < nkeys; r++) {
        CHECK(key[cur][r - 1] < key[cur][r] || (key[cur][r - 1] == key[cur][r] && num[cur][r - 1] < num[cur][r]));
    }
    /* the ordered table in front of the limit, its scan, the permute at the caps, the ranks */
    const uint64_t nrows = sre_ltt_rows(nkeys, limit), nent = nrows * K;
    uint64_t      *cstart = block<uint64_t>(nent), *coff = block<uint64_t>(nent + 1);
    uint32_t      *tw = block<uint32_t>(nent);
    CHECK(lttsim_table(num[cur], first, off, start, nrows, nkeys, n, K, cstart, coff, tw) == 0);
    lsosim_scan(coff, nent);
    const uint32_t words = sre_ltt_index_words(K);
    const uint64_t crow = nrows > cap_off ? nrows - cap_off : 0, srow = nrows / 2, irow = nrows > 1 ? nrows - 1 : nrows;
    uint64_t      *oc = block<uint64_t>(crow);
    int64_t       *os = block<int64_t>(4 * V * srow), *idx = block<int64_t>(words * irow), *rank = block<int64_t>(n);
    uint32_t      *ocw = block<uint32_t>(crow), *osw = block<uint32_t>(4 * V * srow), *iw = block<uint32_t>(words * irow);
    uint32_t      *inv = block<uint32_t>(nkeys), *nw = block<uint32_t>(nkeys), *rw = block<uint32_t>(n);
    CHECK(lttsim_permute(num[cur], nkeys, counts, aggs, V, first, ends, n, cstart, coff, K, value, cls, oc, crow, ocw, os, srow, osw, idx,
                         irow, iw, inv, nw) == 0);
    lttsim_ranks(lslot, cnt, inv, n, nkeys, rank, rw);
    for (uint64_t i = 0; i < n; i++) CHECK(owner[i] < 0 ? rank[i] == -1 : num[cur][rank[i]] == (uint32_t) owner[i]);
    void *all[] = {tab, cnt, counts, lslot, aggs, off, start, ends, first, fw, vw, value, cls, key[0], key[1], pc, num[0], num[1], cw, kw, lw,
                   cstart, coff, tw, oc, os, idx, rank, ocw, osw, iw, inv, nw, rw};
    for (void *p : all) free(p);
    return passes;
}

int
main(void)
{
    const uint64_t sizes[] = {1, 63, 64, 65, 257, 1024 + 17, 2 * 1024 + 1};
    const int      bys[] = {SRE_LTT_COUNT, SRE_LTT_SUM, SRE_LTT_MIN, SRE_LTT_MAX, SRE_LTT_N};
    uint64_t       cases = 0, most = 0;
    for (uint64_t nkeys : sizes) {
        for (int dist = 0; dist < 4; dist++) {
            for (int by : bys) {
                for (int desc = 0; desc < 2; desc++) {
                    const uint64_t limit = (cases % 3 == 0) ? 0 : (cases % 3 == 1) ? 3 : nkeys + 5;
                    const uint64_t p = one_case(nkeys, dist, by, desc, limit, cases % 4);
                    most = p > most ? p : most;
                    cases++;
                }
            }
        }
    }
    /* the range rule at its edge */
    CHECK(sre_ltt_range_ok(2, INT64_MIN + 2, INT64_MAX) && !sre_ltt_range_ok(2, INT64_MIN + 1, INT64_MAX) && sre_ltt_range_ok(0, INT64_MAX, INT64_MIN));
    CHECK(most == 8);
    printf("asan_tally_top_rule: %llu cases, up to %llu passes, clean\n", (unsigned long long) cases, (unsigned long long) most);
    return 0;
}
