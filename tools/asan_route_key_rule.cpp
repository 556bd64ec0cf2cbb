/* tools/asan_route_key_rule.cpp — CPU-only AddressSanitizer / UBSan run of the rules of the line route by key
 * (sregex_amd/csrc/sre_lines_route_key.h, what the partition's kernels and the host code compile) through the CPU model
 * (tests/lines_route_key_sim.cpp, compiled into this program): every digit pass, the compact table, the heads, the bucket
 * rows, the index rows and the cut over the model's cases.  Every array is a heap block of exactly the size the call gives
 * it: n key ids, 2^bits x ceil(n / 1024) + 1 counts, nsel + 1 words for each item array, the values and the head ranks,
 * nsel starts, 5 words a row, so one word read or written past any of them is reported.
 *   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -Isregex_amd/csrc tools/asan_route_key_rule.cpp \
 *       -o /tmp/asan_rk && /tmp/asan_rk
 */
#include "../tests/lines_route_key_sim.cpp"
#include <stdio.h>
#include <stdlib.h>

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

/* the key id of line i: dist 0 one key, 1 round-robin, 2 distinct as far as the rows go, 3 descending, 4 random with a third
 * without a dictionary row, 5 none with one */
static int64_t
key_id(int dist, uint64_t i, uint64_t n, uint64_t rows)
{
    switch (dist) {
    case 0: return (int64_t) rows - 1;
    case 1: return (int64_t) (i % rows);
    case 2: return (int64_t) ((i * (rows / (n ? n : 1) ? rows / (n ? n : 1) : 1)) % rows);
    case 3: return (int64_t) ((n - 1 - i) % rows);
    case 4: return rnd() % 3 == 0 ? -1 - (int64_t) (rnd() & 1) : (int64_t) (rnd() % rows);
    default: return -1 - (int64_t) (rnd() & 1);
    }
}

static int
one_case(uint64_t n, uint64_t rows, uint32_t bits, int dist, int all, int rule)
{
    int            bad = 0;
    int64_t       *ids = block<int64_t>(n);
    uint64_t      *ends = block<uint64_t>(n);
    uint64_t       pos = 0, want = 0;
    for (uint64_t i = 0; i < n; i++) {
        ids[i] = key_id(dist, i, n, rows);
        if (sre_lrk_sort_key(ids[i], rows, all) >= 0) want++;
        pos += rnd() % 9;
        ends[i] = pos++;
    }
    const uint32_t nd = 1u << bits, passes = sre_lrk_passes(sre_lrk_max_key(rows, all), bits);
    uint64_t      *src = NULL, nsrc = n;
    for (uint32_t p = 0; p < passes && nsrc != 0; p++) {
        const uint64_t ncnt = nd * ((nsrc + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS);
        uint64_t      *cnt = block<uint64_t>(ncnt + 1);
        uint32_t      *cw = block<uint32_t>(ncnt + 1);
        lrksim_count(p == 0 ? ids : NULL, src, nsrc, rows, all, p, bits, rule, cnt, cw);
        lrksim_scan(cnt, ncnt);
        const uint64_t total = cnt[ncnt];
        if (total != want) bad++;
        uint64_t *dst = block<uint64_t>(total + 1);
        uint32_t *dw = block<uint32_t>(total + 1);
        if (total && lrksim_scatter(p == 0 ? ids : NULL, src, nsrc, rows, all, p, bits, rule, cnt, total, dst, dw) != 0) bad++;
        for (uint64_t r = 0; r < total; r++) bad += dw[r] != 1;
        free(cnt);
        free(cw);
        free(dw);
        free(src);
        src = dst;
        nsrc = total;
    }
    const uint64_t nsel = src ? nsrc : 0;
    for (uint64_t r = 1; r < nsel; r++) bad += src[r - 1] >= src[r];
    if (nsel) {
        uint64_t *cstart = block<uint64_t>(nsel), *coff = block<uint64_t>(nsel + 1), *head = block<uint64_t>(nsel + 1);
        uint64_t *hrank = block<uint64_t>(nsel + 1);
        uint32_t *tw = block<uint32_t>(nsel), *hw = block<uint32_t>(nsel + 1);
        lrksim_table(src, ends, nsel, n, cstart, coff, head, tw);
        lrksim_scan(head, nsel);
        lrksim_scan(coff, nsel);
        lrksim_heads(src, head, nsel, hrank, hw);
        const uint64_t nb = head[nsel];
        uint64_t       lines = 0, bytes = 0;
        for (uint64_t b = 0; b < nb; b++) {
            int64_t *row = block<int64_t>(5);
            lrksim_bucket_row(src, hrank, b, coff, rows, row);
            if ((uint64_t) row[1] != lines || (uint64_t) row[3] != bytes) bad++;
            lines += (uint64_t) row[2];
            bytes += (uint64_t) row[4];
            free(row);
        }
        if (lines != nsel || bytes != coff[nsel]) bad++;
        const uint64_t caps[4] = {coff[nsel], coff[nsel] - 1, coff[1], 0};
        for (int c = 0; c < 4; c++) {
            const uint64_t cut = lrksim_cut(coff, nsel, caps[c]);
            if (cut > nsel || coff[cut] > caps[c] || (cut < nsel && coff[cut + 1] <= caps[c])) bad++;
            for (uint64_t r = 0; r < cut; r += cut / 3 + 1) {
                int64_t *row = block<int64_t>(5);
                lrksim_index_row(src, cstart, coff, r, rows, row);
                if ((uint64_t) row[0] >= n || (uint64_t) row[3] != coff[r]) bad++;
                free(row);
            }
        }
        free(cstart);
        free(coff);
        free(head);
        free(hrank);
        free(tw);
        free(hw);
    }
    free(src);
    free(ids);
    free(ends);
    return bad;
}

int
main(void)
{
    static const uint64_t sizes[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000};
    static const uint64_t ranges[] = {1, 2, 255, 256, 257, 70000};
    static const uint32_t widths[] = {1, 4, 8};
    int                   bad = 0, cases = 0;
    for (uint64_t n : sizes) {
        for (uint64_t rows : ranges) {
            for (uint32_t bits : widths) {
                for (int dist = 0; dist < 6; dist++) {
                    for (int all = 0; all < 2; all++) {
                        bad += one_case(n, rows, bits, dist, all, (cases & 1) ? SRE_LRK_RANK_TURNS : SRE_LRK_RANK_BITS);
                        cases++;
                    }
                }
            }
        }
    }
    printf("%d cases: %s\n", cases, bad ? "FAILED" : "ok");
    return bad != 0;
}
