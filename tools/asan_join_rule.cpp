/* tools/asan_join_rule.cpp — CPU-only AddressSanitizer / UBSan run of the key map's and the line join's host-side rules
 * (sregex_amd/csrc/sre_lines_join.h, what the map's fields kernel and the join pass compile): the parting of a row's
 * fields into key fields and value columns, and the entries of a line.  Every array is a heap block of exactly the size
 * the rule may touch: the key arrays nkeys words, the value arrays nfields - nkeys, a line's entries 1 + columns, the
 * map's value arrays rows x values, so one word read or written past any of them is reported.
 *   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -Isregex_amd/csrc tools/asan_join_rule.cpp \
 *       -o /tmp/asan_jr && /tmp/asan_jr
 */
#include "sre_lines_join.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct Text {
    const uint8_t *p;
    uint8_t byte(uint64_t at) const { return p[at]; }
};

static uint64_t *
words(size_t n)
{
    return static_cast<uint64_t *>(malloc(n ? n * sizeof(uint64_t) : 1));
}

/* a row of nf fields "f0 \t f1 \t ..", field x of x bytes, parted at every nkeys */
static int
part_all(uint32_t nf)
{
    int    bad = 0;
    size_t len = 0;
    for (uint32_t x = 0; x < nf; x++) len += x + (x ? 1 : 0);
    uint8_t *row = static_cast<uint8_t *>(malloc(len ? len : 1));
    size_t   at = 0;
    for (uint32_t x = 0; x < nf; x++) {
        if (x) row[at++] = '\t';
        memset(row + at, 'a' + x % 26, x);
        at += x;
    }
    const Text t = {row};
    uint64_t  *s = words(nf), *l = words(nf);
    if (!sre_lk_row_fields(t, 0, len, nf, '\t', s, l)) bad++;
    for (uint32_t k = 1; k <= nf; k++) {
        uint64_t *ks = words(k), *kl = words(k), *vs = words(nf - k), *vl = words(nf - k);
        sre_lj_part(s, l, nf, k, ks, kl, vs, vl);
        for (uint32_t x = 0; x < nf; x++) {
            const uint64_t gs = x < k ? ks[x] : vs[x - k], gl = x < k ? kl[x] : vl[x - k];
            if (gs != s[x] || gl != x) bad++;
        }
        free(ks);
        free(kl);
        free(vs);
        free(vl);
    }
    free(s);
    free(l);
    free(row);
    return bad;
}

/* the entries of one line against a map of `rows` rows of nv columns, for every kind of line and both flags */
static int
entries_all(uint32_t nv, uint32_t ncols)
{
    int            bad = 0;
    const uint64_t rows = 3;
    uint64_t      *vstart = words(rows * nv), *vlen = words(rows * nv);
    for (uint64_t e = 0; e < rows * nv; e++) {
        vstart[e] = 100 + 7 * e;
        vlen[e] = e % 5;
    }
    sre_lj_cols_t c;
    memset(&c, 0, sizeof(c));
    c.n = ncols;
    for (uint32_t x = 0; x < ncols; x++) c.col[x] = (uint8_t) ((x * 5 + 3) % nv);       /* any order, repeats */
    const uint32_t P = 1 + ncols;
    for (int all = 0; all < 2; all++) {
        for (int kind = 0; kind < 3; kind++) {          /* a member of the last row, a keyed line that is none, no key */
            const bool     keyed = kind != 2;
            const int64_t  id = kind == 0 ? (int64_t) rows - 1 : SRE_LK_NOT_MEMBER;
            const bool     sel = all || kind == 0;
            uint64_t      *val = words(P), *start = words(P);
            sre_lj_entries(keyed, id, all != 0, 4096, 17, kind == 0 ? vstart : NULL, kind == 0 ? vlen : NULL, nv, c, val, start);
            if (sre_lj_selected(keyed, id, all != 0) != sel) bad++;
            if (val[0] != (sel ? 18u : 0u) || start[0] != (4096 | SRE_LG_ENTRY_FIRST)) bad++;
            for (uint32_t x = 0; x < ncols; x++) {
                const uint64_t e = (rows - 1) * nv + c.col[x], last = x + 1 == ncols ? SRE_LG_ENTRY_LAST : 0;
                const uint64_t wv = !sel ? 0 : kind == 0 ? vlen[e] + 1 : 1;
                const uint64_t ws = (kind == 0 ? vstart[e] | SRE_LG_ENTRY_LITERAL : SRE_LG_ENTRY_UNSET) | last;
                if (val[1 + x] != wv || start[1 + x] != ws) bad++;
            }
            free(val);
            free(start);
        }
    }
    free(vstart);
    free(vlen);
    return bad;
}

int
main(void)
{
    int bad = 0;
    for (uint32_t nf = 1; nf <= SRE_EXTRACT_MAX_FIELDS; nf++) bad += part_all(nf);
    for (uint32_t nv = 1; nv <= SRE_LJ_MAX_VALUES; nv++) {
        for (uint32_t ncols = 1; ncols <= SRE_LJ_MAX_VALUES; ncols++) bad += entries_all(nv, ncols);
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
