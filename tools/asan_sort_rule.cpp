/* tools/asan_sort_rule.cpp — CPU-only AddressSanitizer / UBSan run of the rules of the line sort
 * (sregex_amd/csrc/sre_lines_sort.h, what the sort's kernels and the host code compile) through the CPU model
 * (tests/lines_sort_sim.cpp, compiled into this program): the values pass, every digit pass, the compact table in front of the
 * limit, the result words, the cut and the index rows over the model's cases.  Every array is a heap block of exactly the size
 * the call gives it: the buffer's bytes, n entries of the value table, n values and n one-byte classes, 256 x ceil(n / 1024) + 1
 * counts, nsel keys and nsel 32-bit lines for each pair of item arrays, nout starts and nout + 1 values, 6 words a row, so one
 * word read or written past any of them is reported; the key arithmetic at +-(10^18 - 1) runs under UBSan.
 *   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -Isregex_amd/csrc tools/asan_sort_rule.cpp \
 *       -o /tmp/asan_sort && /tmp/asan_sort
 */
#include "../tests/lines_sort_sim.cpp"
#include <stdio.h>
#include <stdlib.h>
#include <string>

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

static const int64_t BIG = 999999999999999999ll;

/* the sort field of line i: dist 0 one value, 1 status codes, 2 16 bits, 3 bits 32 .. 39 only, 4 the top digit of an 8-pass
 * range, 5 the full range with both extremes, 6 descending, 7 a third not numbered, 8 none numbered.  "" with *kind = 0: no
 * match; *kind = 1: an unset group; *kind = 2: the text */
static std::string
field(int dist, uint64_t i, uint64_t n, int *kind)
{
    *kind = 2;
    switch (dist) {
    case 0: return "-42";
    case 1: return std::to_string(200 + rnd() % 400);
    case 2: return std::to_string(rnd() % 65536);
    case 3: return std::to_string(777 + ((rnd() % 256) << 32));
    case 4: return std::to_string((rnd() % 8) << 56);
    case 5: return std::to_string(i == 0 ? BIG : i == 1 ? -BIG : (int64_t) (rnd() % (2 * (uint64_t) BIG + 1)) - BIG);
    case 6: return std::to_string(n - i);
    case 7: {
        static const char *junk[] = {"+1", "1 ", "-", "", "1234567890123456789", "12a"};
        const uint64_t     r = rnd() % 9;
        if (r == 0) *kind = 0;
        if (r == 1) *kind = 1;
        if (r == 2) return junk[rnd() % 6];
        return r == 3 ? "-0" : r == 4 ? "007" : std::to_string((int64_t) (rnd() % 600) - 300);
    }
    default: *kind = (int) (rnd() % 3); return "abc";
    }
}

static int
one_case(uint64_t n, int dist, int desc, int all)
{
    int         bad = 0;
    std::string text;
    uint64_t   *ends = block<uint64_t>(n), *vval = block<uint64_t>(n), *vstart = block<uint64_t>(n);
    for (uint64_t i = 0; i < n; i++) {
        int               kind;
        const std::string f = field(dist, i, n, &kind);
        const uint64_t    st = text.size(), pad = rnd() % 5;
        text.append(pad, 'x');
        const uint64_t at = text.size();
        text += f;
        text.append(rnd() % 3, ' ');
        ends[i] = text.size();
        text += '\n';
        const uint64_t flags = SRE_LG_ENTRY_FIRST | SRE_LG_ENTRY_LAST;
        vval[i] = kind == 0 ? 0 : kind == 1 ? 1 : f.size() + 1;
        vstart[i] = (kind == 2 ? at : st | SRE_LG_ENTRY_UNSET) | flags;
    }
    /* the buffer as a block of exactly its bytes */
    uint8_t *buf = block<uint8_t>(text.size());
    memcpy(buf, text.data(), text.size());
    int64_t  *value = block<int64_t>(n);
    int8_t   *cls = block<int8_t>(n);
    uint32_t *vw = block<uint32_t>(n), *cw = block<uint32_t>(n), *sent = block<uint32_t>(4);
    uint64_t *totals = block<uint64_t>(4);
    if (lsosim_values(buf, text.size(), vval, vstart, n, value, cls, vw, cw, totals, sent) != 0) bad++;
    for (uint64_t i = 0; i < n; i++) bad += vw[i] != 1 || cw[i] != 1;
    const uint64_t nnum = totals[1];
    const int64_t  vmin = (int64_t) totals[2], vmax = (int64_t) totals[3];
    const uint64_t range = sre_lso_range(nnum, vmin, vmax), nsel = sre_lso_selected(n, nnum, all);
    const uint32_t passes = sre_lso_passes(n, nnum, range, all);
    if ((nsel == 0) != (passes == 0) || passes > SRE_LSO_MAX_PASSES) bad++;
    uint64_t *src = NULL, nsrc = n;
    uint32_t *sline = NULL;
    for (uint32_t p = 0; p < passes; p++) {
        const uint64_t ncnt = 256 * ((nsrc + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS);
        uint64_t      *cnt = block<uint64_t>(ncnt + 1);
        uint32_t      *cntw = block<uint32_t>(ncnt + 1);
        lsosim_count(p == 0 ? value : NULL, p == 0 ? cls : NULL, src, nsrc, vmin, vmax, nnum, desc, all, p, cnt, cntw);
        lsosim_scan(cnt, ncnt);
        const uint64_t total = cnt[ncnt];
        if (total != nsel) bad++;
        uint64_t *dkey = block<uint64_t>(total);
        uint32_t *dline = block<uint32_t>(total), *kw = block<uint32_t>(total), *lw = block<uint32_t>(total);
        if (lsosim_scatter(p == 0 ? value : NULL, p == 0 ? cls : NULL, src, sline, nsrc, vmin, vmax, nnum, desc, all, p, cnt, total, dkey,
                           dline, kw, lw) != 0)
        {
            bad++;
        }
        for (uint64_t r = 0; r < total; r++) bad += kw[r] != 1 || lw[r] != 1;
        free(cnt);
        free(cntw);
        free(kw);
        free(lw);
        free(src);
        free(sline);
        src = dkey;
        sline = dline;
        nsrc = total;
    }
    for (uint64_t r = 1; r < nsel; r++) bad += src[r - 1] > src[r] || (src[r - 1] == src[r] && sline[r - 1] >= sline[r]);
    const uint64_t limits[4] = {0, 1, nsel / 2 + 1, nsel + 7};
    for (int l = 0; l < 4 && nsel; l++) {
        const uint64_t nout = sre_lso_limited(nsel, limits[l]);
        uint64_t      *cstart = block<uint64_t>(nout), *coff = block<uint64_t>(nout + 1), *res = block<uint64_t>(SRE_LSO_RES_WORDS);
        uint32_t      *tw = block<uint32_t>(nout);
        lsosim_table(sline, ends, nout, n, cstart, coff, tw);
        lsosim_scan(coff, nout);
        const uint64_t caps[4] = {coff[nout], coff[nout] - 1, coff[1], 0};
        for (int c = 0; c < 4; c++) {
            lsosim_result(coff, nout, caps[c], res);
            const uint64_t cut = res[SRE_LSO_RES_WRITTEN];
            if (res[SRE_LSO_RES_NSEL] != nout || cut > nout || coff[cut] > caps[c] || (cut < nout && coff[cut + 1] <= caps[c])) bad++;
            for (uint64_t r = 0; r < cut; r += cut / 3 + 1) {
                int64_t *row = block<int64_t>(SRE_LSO_INDEX_WORDS);
                lsosim_index_row(sline[r], cstart, coff, r, value[sline[r]], cls[sline[r]], row);
                if ((uint64_t) row[0] >= n || (uint64_t) row[3] != coff[r] || row[5] != cls[sline[r]]) bad++;
                free(row);
            }
        }
        free(cstart);
        free(coff);
        free(res);
        free(tw);
    }
    free(src);
    free(sline);
    free(buf);
    free(value);
    free(cls);
    free(vw);
    free(cw);
    free(sent);
    free(totals);
    free(ends);
    free(vval);
    free(vstart);
    return bad;
}

int
main(void)
{
    static const uint64_t sizes[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000};
    int                   bad = 0, cases = 0;
    for (uint64_t n : sizes) {
        for (int dist = 0; dist < 9; dist++) {
            for (int desc = 0; desc < 2; desc++) {
                for (int all = 0; all < 2; all++) {
                    bad += one_case(n, dist, desc, all);
                    cases++;
                }
            }
        }
    }
    printf("%d cases: %s\n", cases, bad ? "FAILED" : "ok");
    return bad != 0;
}
