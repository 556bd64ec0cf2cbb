/* tools/asan_fold_rule.cpp — CPU-only AddressSanitizer / UBSan run of the rules of the line fold
 * (sregex_amd/csrc/sre_lines_fold.h, what its kernels compile) through the CPU model (tests/lines_fold_sim.cpp, compiled into
 * this program): marks, carry, apply, totals, the cut, the record ids and the records table, for both modes, caps on a record's
 * lines from 1 to SIZE_MAX, every order of the workgroups tried, and out_cap at and around record ends.  Every array is a heap
 * block of exactly the size the call gives it: n + 1 per-line values, n start words, n aux words, n record ids, ceil(n / 64)
 * words for each bitmap, records_cap rows, so one word read or written past any of them is reported.
 *   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -Isregex_amd/csrc tools/asan_fold_rule.cpp \
 *       -o /tmp/asan_fold && /tmp/asan_fold
 */
#include "../tests/lines_fold_sim.cpp"
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

#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            fprintf(stderr, "asan_fold_rule: %s failed at line %d\n", #cond, __LINE__);    \
            exit(1);                                                                        \
        }                                                                                   \
    } while (0)

/* one call of the model, checked against the definitions line by line */
static void
one_case(uint64_t n, uint32_t density, int next, uint64_t max_lines, int reverse, uint64_t cap_sel, uint64_t records_cap)
{
    const uint64_t        nblk = (n + SRE_LC_ITEMS - 1) / SRE_LC_ITEMS, nw = (n + 63) / 64;
    std::vector<uint8_t>  marked(n), head(n);
    std::vector<uint64_t> lens(n), off(n + 1, 0);
    uint64_t             *val = block<uint64_t>(n + 1), *start = block<uint64_t>(n), *aux = block<uint64_t>(n), *ends = block<uint64_t>(n);
    uint64_t             *mbits = block<uint64_t>(nw), *hbits = block<uint64_t>(nw), *order = block<uint64_t>(nblk);
    int64_t              *recid = block<int64_t>(n), *rows = block<int64_t>(records_cap * SRE_LF_ROW);
    uint64_t              pos = 0, h = 0, nrec = 0, nmarked = 0;
    for (uint64_t i = 0; i < n; i++) {
        marked[i] = density == 0 ? 0 : density == 100 ? 1 : rnd() % 100 < density;
        lens[i] = rnd() % 41;
        ends[i] = pos + lens[i];
        pos += lens[i] + 1;
        off[i + 1] = pos;
        val[i] = marked[i] ? lens[i] + 1 : 0;
        nmarked += marked[i];
    }
    for (uint64_t i = 0; i < n; i++) {
        const bool nh = i == 0 || !marked[i - (next ? 1 : 0)];
        h = nh ? i : h;
        head[i] = nh || (max_lines != 0 && (i - h) % max_lines == 0);
        nrec += head[i];
    }
    for (uint64_t b = 0; b < nblk; b++) order[b] = reverse ? nblk - 1 - b : b;
    /* out_cap: everything, nothing, or the end of a random line and the bytes around it */
    const uint64_t out_cap = cap_sel == 0 ? ~(uint64_t) 0 : cap_sel == 1 ? 0 : off[1 + rnd() % n] + cap_sel - 3;
    uint64_t       info[6];
    CHECK(lfsim_run(val, start, aux, ends, n, next, max_lines, order, mbits, hbits, recid, out_cap, records_cap, rows, info) == 0);
    uint64_t r = 0, longest = 0, written = 0, bytes = 0, first = 0;
    bool     open = true;
    for (uint64_t i = 0; i < n; i++) {
        if (head[i]) first = i;
        r += head[i];
        const bool last = i + 1 == n || head[i + 1];
        CHECK(val[i] == off[i] && (uint64_t) recid[i] == r - 1 && ((hbits[i / 64] >> (i % 64)) & 1u) == head[i]);
        CHECK(start[i] == ((ends[i] - lens[i]) | (last ? SRE_LG_ENTRY_LAST : 0)));
        CHECK(head[i] || aux[i] == first);
        if (last) {
            CHECK(aux[first] == i + 1);
            longest = i + 1 - first > longest ? i + 1 - first : longest;
            open = open && off[i + 1] <= out_cap;
            if (open) {
                if (written < records_cap) {
                    const int64_t *row = rows + written * SRE_LF_ROW;
                    CHECK(row[0] == (int64_t) first && row[1] == (int64_t) (i + 1 - first) && row[2] == (int64_t) (ends[first] - lens[first]));
                    CHECK(row[3] == (int64_t) (off[i + 1] - off[first] - 1) && row[4] == (int64_t) off[first]);
                }
                written++;
                bytes = off[i + 1];
            }
        }
    }
    CHECK(val[n] == off[n] && info[0] == nrec && info[1] == nmarked && info[2] == longest && info[3] == written && info[4] == bytes);
    void *all[] = {val, start, aux, ends, mbits, hbits, order, recid, rows};
    for (void *p : all) free(p);
}

int
main(void)
{
    const uint64_t sizes[] = {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 17};
    const uint32_t dens[] = {0, 3, 50, 97, 100};
    uint64_t       cases = 0;
    for (uint64_t n : sizes) {
        const uint64_t caps[] = {0, 1, 2, 255, 256, 257, 1024, 1025, n, ~(uint64_t) 0};
        for (uint32_t d : dens) {
            for (int next = 0; next < 2; next++) {
                for (uint64_t m : caps) {
                    const uint64_t sel = cases % 7;
                    one_case(n, d, next, m, (int) (cases & 1), sel, sel == 4 ? 0 : sel == 5 ? 1 : n + 2);
                    cases++;
                }
            }
        }
    }
    /* the carry over more block words than lanes */
    const uint64_t nblk = 3000;
    uint64_t      *last = block<uint64_t>(nblk), *first = block<uint64_t>(nblk);
    for (uint64_t b = 0; b < nblk; b++) {
        last[b] = b % 5 == 0 ? b * 1024 + 7 : 0;
        first[b] = b % 5 == 0 ? b * 1024 + 3 : ~(uint64_t) 0;
    }
    lfsim_carry(last, first, nblk);
    for (uint64_t b = 1; b < nblk; b++) CHECK(last[b] == (b - 1) / 5 * 5 * 1024 + 7);
    for (uint64_t b = 0; b + 5 < nblk; b++) CHECK(first[b] == (b / 5 + 1) * 5 * 1024 + 3);
    free(last);
    free(first);
    printf("asan_fold_rule: %llu cases, clean\n", (unsigned long long) cases);
    return 0;
}
