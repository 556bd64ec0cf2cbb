/* tools/asan_distinct_rule.cpp — CPU-only AddressSanitizer / UBSan run of the rules of the line distinct
 * (sregex_amd/csrc/sre_lines_distinct.h, what its kernels compile) through the CPU models (tests/lines_tally_sim.cpp and
 * tests/lines_distinct_sim.cpp, compiled into this program): the tally's insert over a key table under its four schedules
 * and hash masks, the last pass, the pick pass for every rule, flag and range, and the per-line arrays at their caps.  Every
 * array is a heap block of exactly the size the call gives it: n entries of the key table, nslots words for each of the
 * table's three runs, n slots, n + 1 per-line values, the caller's arrays at their caps, so one word read or written past any
 * of them is reported.
 *   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -Isregex_amd/csrc tools/asan_distinct_rule.cpp \
 *       -o /tmp/asan_distinct && /tmp/asan_distinct
 */
#include "../tests/lines_tally_sim.cpp"
#include "../tests/lines_distinct_sim.cpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
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

#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            fprintf(stderr, "asan_distinct_rule: %s failed at line %d\n", #cond, __LINE__);    \
            exit(1);                                                                            \
        }                                                                                       \
    } while (0)

static uint64_t
one_case(uint64_t n, uint64_t nkeys, int hash_bits, int schedule)
{
    /* the lines: a key number each, or none; the key's text is its decimal digits */
    std::vector<int64_t> owner(n);
    std::string          text;
    uint64_t            *val = block<uint64_t>(n), *start = block<uint64_t>(n);
    std::vector<uint64_t> first(nkeys, ~(uint64_t) 0), last(nkeys, 0), count(nkeys, 0);
    uint64_t             distinct = 0, nkeyed = 0;
    for (uint64_t i = 0; i < n; i++) {
        owner[i] = n > 1 && rnd() % 7 == 0 ? -1 : (int64_t) (rnd() % nkeys);
        start[i] = text.size() | SRE_LG_ENTRY_FIRST | SRE_LG_ENTRY_LAST;
        if (owner[i] >= 0) {
            const std::string key = std::to_string(owner[i]);
            val[i] = key.size() + 1;
            text += key;
            if (count[owner[i]]++ == 0) first[owner[i]] = i, distinct++;
            last[owner[i]] = i;
            nkeyed++;
        }
        text += "\n";
    }
    uint8_t *buf = block<uint8_t>(text.size());
    memcpy(buf, text.data(), text.size());
    const uint64_t max_keys = distinct ? distinct : 1, nslots = sre_lt_nslots(max_keys);
    uint64_t      *tab = block<uint64_t>(nslots), *cnt = block<uint64_t>(nslots), *lastrun = block<uint64_t>(nslots);
    uint32_t      *lslot = block<uint32_t>(n);
    uint64_t       words[9], lw[4], pw[4];
    for (uint64_t s = 0; s < nslots; s++) tab[s] = SRE_LT_EMPTY;
    ltsim_insert(buf, val, start, n, 1, max_keys, hash_bits, schedule, n * 31 + nkeys, tab, cnt, lslot, words);
    CHECK(words[0] == nkeyed && words[1] == distinct && words[2] == 0 && words[6] == 0);
    ldsim_last(lslot, n, nslots, schedule, n + 7, lastrun, lw);
    CHECK(lw[2] == 0 && lw[0] == lw[3] && lw[0] == lw[1]);
    uint64_t most = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (owner[i] < 0) {
            CHECK(lslot[i] == SRE_LT_NONE);
            continue;
        }
        const uint32_t s = lslot[i];
        CHECK(s < nslots && tab[s] == first[owner[i]] && lastrun[s] == last[owner[i]] && cnt[s] == count[owner[i]]);
        most = cnt[s] > most ? cnt[s] : most;
    }
    /* the per-line arrays at caps below, at and above n */
    const uint64_t caps[3] = {n / 2, n, n + 3};
    for (uint32_t x = 0; x < 3; x++) {
        const uint64_t kc = caps[x], kl = caps[(x + 1) % 3], c = kc < n ? kc : n, l = kl < n ? kl : n;
        uint64_t      *keycount = block<uint64_t>(c);
        int64_t       *keyline = block<int64_t>(l);
        CHECK(ldsim_perline(lslot, nslots, tab, cnt, keycount, c, keyline, l) == 0);
        for (uint64_t i = 0; i < c; i++) CHECK(keycount[i] == (owner[i] < 0 ? 0 : count[owner[i]]));
        for (uint64_t i = 0; i < l; i++) CHECK(keyline[i] == (owner[i] < 0 ? -1 : (int64_t) first[owner[i]]));
        free(keycount);
        free(keyline);
    }
    /* the pick pass */
    const uint64_t ranges[5][2] = {{1, 0}, {1, 1}, {2, 0}, {2, 3}, {most + 1, 0}};
    uint64_t       runs = 0;
    for (int which = SRE_LD_FIRST; which <= SRE_LD_EVERY; which++) {
        for (int invert = 0; invert < 2; invert++) {
            for (const uint64_t *r : ranges) {
                CHECK(ldsim_range_ok(r[0], r[1]));
                uint64_t *fval = block<uint64_t>(n + 1);
                for (uint64_t i = 0; i < n; i++) fval[i] = owner[i] < 0 ? 0 : 5 + i % 9;
                fval[n] = 77;
                ldsim_pick(lslot, n, nslots, tab, cnt, which == SRE_LD_LAST ? lastrun : NULL, which, r[0], r[1], invert, fval, pw);
                uint64_t kept = 0, nsel = 0;
                for (uint64_t k = 0; k < nkeys; k++) kept += count[k] != 0 && sre_ld_qualifies(r[0], r[1], count[k]);
                for (uint64_t i = 0; i < n; i++) {
                    bool sel = false;
                    if (owner[i] >= 0) {
                        const uint64_t k = (uint64_t) owner[i];
                        const bool     named = which == SRE_LD_FIRST ? i == first[k] : which == SRE_LD_LAST ? i == last[k] : true;
                        sel = (named && r[0] <= count[k] && (r[1] == 0 || count[k] <= r[1])) != (invert != 0);
                    }
                    CHECK(fval[i] == (sel ? 5 + i % 9 : 0));
                    nsel += sel;
                }
                CHECK(fval[n] == 77 && pw[0] == kept && pw[2] == 0 && pw[1] == nkeyed * (which == SRE_LD_LAST ? 3 : 2));
                CHECK(which == SRE_LD_EVERY || invert || nsel == kept);
                CHECK(r[0] != most + 1 || kept == 0);
                free(fval);
                runs++;
            }
        }
    }
    void *all[] = {val, start, buf, tab, cnt, lastrun, lslot};
    for (void *p : all) free(p);
    return runs;
}

int
main(void)
{
    const uint64_t sizes[] = {1, 63, 64, 65, 257, 1024 + 17};
    const int      bits[] = {64, 0, 1, 2};
    uint64_t       cases = 0, runs = 0;
    for (uint64_t n : sizes) {
        const uint64_t cards[] = {1, 3, n / 2 ? n / 2 : 1, n};
        for (uint64_t nkeys : cards) {
            for (int schedule = 0; schedule < 4; schedule++) {
                /* (a chain of every key behind one home slot is quadratic: the masks run at the smaller sizes) */
                for (int b : bits) {
                    if (b != 64 && n * nkeys > 70000) continue;
                    runs += one_case(n, nkeys, b, schedule);
                    cases++;
                }
            }
        }
    }
    CHECK(!ldsim_range_ok(0, 0) && !ldsim_range_ok(0, 5) && !ldsim_range_ok(3, 2) && ldsim_range_ok(1, 0) && ldsim_range_ok(2, 2));
    CHECK(sre_ld_sender(1) == 0 && sre_ld_sender(~(uint64_t) 0) == 63 && sre_ld_sender((uint64_t) 1 << 63) == 63 && sre_ld_sender(6) == 2);
    printf("asan_distinct_rule: %llu cases, %llu pick passes, clean\n", (unsigned long long) cases, (unsigned long long) runs);
    return 0;
}
