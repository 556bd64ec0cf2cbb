/* tools/asan_sort_text_rule.cpp — CPU-only AddressSanitizer / UBSan run of the rules of the line sort by text
 * (sregex_amd/csrc/sre_lines_sort_text.h, what the sort's kernels and the host code compile) through the CPU model
 * (tests/lines_sort_text_sim.cpp, compiled into this program): the values pass, the plan, the keys of every chunk, the pass that
 * makes the items and every later digit pass, then the compact table in front of the limit, the result words, the cut and the
 * index rows.  Every array is a heap block of exactly the size the call gives it: the buffer's bytes (the last field ends on
 * the buffer's last byte in the cases without a final delimiter), n entries of the value table, n lengths and n one-byte
 * classes, n keys of the lines, 256 x ceil(n / 1024) + 1 counts, nsel keys and nsel 32-bit lines for each pair of item arrays
 * (the model allocates those), nout starts and nout + 1 values, 6 words a row, so one byte or word read or written past any of
 * them is reported; the key arithmetic (KMAX - key, the shifts of the chunk bytes) runs under UBSan.
 *   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -Isregex_amd/csrc -Itests \
 *       tools/asan_sort_text_rule.cpp -o /tmp/asan_sort_text && /tmp/asan_sort_text
 */
#include "../tests/lines_sort_text_sim.cpp"
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
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

/* the sort field of line i: dist 0 one text, 1 all empty, 2 lengths 0 - 16 over four bytes, 3 a shared first chunk, 4 two shared
 * chunks, 5 the prefix chain, 6 lengths 0 - 40, 7 a third without a match or unset, 8 none keyed.  *kind = 0: no match; 1: an
 * unset group; 2: the text */
static std::string
field(int dist, uint64_t i, int *kind)
{
    static const char alphabet[4] = {'\0', 'a', 'b', '\xff'};
    std::string       t;
    *kind = 2;
    switch (dist) {
    case 0: return "same-text";
    case 1: return "";
    case 2:
    case 7:
        if (dist == 7 && rnd() % 3 == 0) *kind = (int) (rnd() % 2);
        for (uint64_t k = rnd() % 17; k > 0; k--) t += alphabet[rnd() % 4];
        return *kind == 2 ? t : "";
    case 3:
    case 4:
        t.assign(dist == 3 ? 7 : 14, 'P');
        for (uint64_t k = 1 + rnd() % 6; k > 0; k--) t += alphabet[1 + rnd() % 3];
        return t;
    case 5: return std::string((i * 7) % 21, 'x');
    case 6:
        for (uint64_t k = rnd() % 41; k > 0; k--) t += (char) ('a' + rnd() % 3);
        return t;
    default: *kind = (int) (rnd() % 2); return "";
    }
}

static int
one_case(uint64_t n, int dist, int desc, int all, uint64_t max_bytes, int final_delim)
{
    int                      bad = 0;
    std::string              text;
    std::vector<std::string> cut(n);
    std::vector<int>         kinds(n);
    uint64_t                *ends = block<uint64_t>(n), *vval = block<uint64_t>(n), *vstart = block<uint64_t>(n);
    for (uint64_t i = 0; i < n; i++) {
        int               kind;
        const std::string f = field(dist, i, &kind);
        const uint64_t    st = text.size(), pad = rnd() % 5;
        text.append(pad, 'x');
        const uint64_t at = text.size();
        text += f;
        if (i + 1 < n || final_delim) text.append(rnd() % 3, ' ');
        ends[i] = text.size();
        if (i + 1 < n || final_delim) text += '\n';
        const uint64_t flags = SRE_LG_ENTRY_FIRST | SRE_LG_ENTRY_LAST;
        vval[i] = kind == 0 ? 0 : kind == 1 ? 1 : f.size() + 1;
        vstart[i] = (kind == 2 ? at : st | SRE_LG_ENTRY_UNSET) | flags;
        kinds[i] = kind;
        cut[i] = kind == 2 ? f.substr(0, max_bytes ? max_bytes : std::string::npos) : "";
    }
    /* the buffer as a block of exactly its bytes */
    uint8_t *buf = block<uint8_t>(text.size());
    memcpy(buf, text.data(), text.size());
    uint32_t *lines = block<uint32_t>(n);
    uint64_t *info = block<uint64_t>(5);
    if (lstsim_sort(buf, text.size(), vval, vstart, n, max_bytes, desc, all, lines, info) != 0) bad++;
    /* the order: unsigned bytes, a proper prefix first, ties in line order, the rest behind */
    std::vector<uint32_t> want;
    for (uint64_t i = 0; i < n; i++) {
        if (kinds[i] != 0) want.push_back((uint32_t) i);
    }
    const uint64_t nkeyed = want.size();
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) {
        const int c = memcmp(cut[a].data(), cut[b].data(), std::min(cut[a].size(), cut[b].size()));
        const bool less = c != 0 ? c < 0 : cut[a].size() < cut[b].size(), more = c != 0 ? c > 0 : cut[a].size() > cut[b].size();
        return desc ? more : less;
    });
    for (uint64_t i = 0; all && i < n; i++) {
        if (kinds[i] == 0) want.push_back((uint32_t) i);
    }
    const uint64_t nsel = want.size();
    if (info[0] != nkeyed || info[1] != nsel) bad++;
    for (uint64_t r = 0; r < nsel; r++) bad += lines[r] != want[r];
    const uint64_t limits[4] = {0, 1, nsel / 2 + 1, nsel + 7};
    for (int l = 0; l < 4 && nsel; l++) {
        const uint64_t nout = sre_lso_limited(nsel, limits[l]);
        uint64_t      *cstart = block<uint64_t>(nout), *coff = block<uint64_t>(nout + 1), *res = block<uint64_t>(SRE_LSO_RES_WORDS);
        uint32_t      *tw = block<uint32_t>(nout);
        lsosim_table(lines, ends, nout, n, cstart, coff, tw);
        lsosim_scan(coff, nout);
        const uint64_t caps[4] = {coff[nout], coff[nout] - 1, coff[1], 0};
        for (int c = 0; c < 4; c++) {
            lsosim_result(coff, nout, caps[c], res);
            const uint64_t cutat = res[SRE_LSO_RES_WRITTEN];
            if (res[SRE_LSO_RES_NSEL] != nout || cutat > nout || coff[cutat] > caps[c] || (cutat < nout && coff[cutat + 1] <= caps[c])) bad++;
            for (uint64_t r = 0; r < cutat; r += cutat / 3 + 1) {
                int64_t *row = block<int64_t>(SRE_LST_INDEX_WORDS);
                if (lstsim_index_row(buf, text.size(), vval, vstart, lines[r], cstart, coff, r, row) != 0) bad++;
                const bool set = kinds[lines[r]] == 2;
                if ((uint64_t) row[0] != lines[r] || (uint64_t) row[3] != coff[r] || (row[4] < 0) != !set || (row[5] < 0) != !set) bad++;
                if (set && (uint64_t) row[5] + 1 != vval[lines[r]]) bad++;
                free(row);
            }
        }
        free(cstart);
        free(coff);
        free(res);
        free(tw);
    }
    free(lines);
    free(info);
    free(buf);
    free(ends);
    free(vval);
    free(vstart);
    return bad;
}

int
main(void)
{
    static const uint64_t sizes[] = {0, 1, 64, 65, 1025, 2500};
    static const uint64_t cuts[] = {0, 1, 7, 8};
    int                   bad = 0, cases = 0;
    for (uint64_t n : sizes) {
        for (int dist = 0; dist < 9; dist++) {
            for (int desc = 0; desc < 2; desc++) {
                for (int all = 0; all < 2; all++) {
                    const uint64_t max_bytes = cuts[(n + dist + desc) % 4];
                    bad += one_case(n, dist, desc, all, max_bytes, (dist + all) % 2);
                    cases++;
                }
            }
        }
    }
    printf("%d cases: %s\n", cases, bad ? "FAILED" : "ok");
    return bad != 0;
}
