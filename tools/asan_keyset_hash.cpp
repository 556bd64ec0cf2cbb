/* tools/asan_keyset_hash.cpp — CPU-only AddressSanitizer / UBSan run of the key set's host hash: the field rule and the
 * tally's hash over a row (sregex_amd/csrc/sre_lines_keyset.h, sre_lines_tally.h, what sre_hip_keyset_hash, the field
 * kernel and the insert compile).  Every row sits at the very end of a heap block of exactly its length, so one byte read
 * past `len` is reported, and the two field arrays have exactly K entries, so a row with too many separators that wrote
 * one more would be reported too.
 *   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -Isregex_amd/csrc tools/asan_keyset_hash.cpp \
 *       -o /tmp/asan_kh && /tmp/asan_kh
 */
#include "sre_lines_keyset.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct Text {
    const uint8_t *p;
    uint8_t byte(uint64_t at) const { return p[at]; }
};

/* the hash of the row as sre_hip_keyset_hash computes it; *ok: the row holds k fields */
static uint64_t
row_hash(const char *s, size_t len, uint32_t k, uint32_t fsep, bool *ok)
{
    uint8_t  *heap = static_cast<uint8_t *>(malloc(len ? len : 1));
    uint64_t *fstart = static_cast<uint64_t *>(malloc(k * sizeof(uint64_t)));
    uint64_t *flen = static_cast<uint64_t *>(malloc(k * sizeof(uint64_t)));
    memcpy(heap, s, len);
    const Text t = {heap};
    uint64_t   h = 0;
    *ok = sre_lk_row_fields(t, 0, len, k, fsep, fstart, flen);
    if (*ok) {
        const sre_lk_dict_keys keys = {heap, fstart, flen, k};
        h = sre_lt_hash(keys, 0);
        if (!sre_lk_equal(keys, 0, keys, 0)) h = 0;
    }
    free(flen);
    free(fstart);
    free(heap);
    return h;
}

static int
check(const char *s, size_t len, uint32_t k, bool want)
{
    bool           ok;
    const uint64_t h = row_hash(s, len, k, '\t', &ok);
    if (ok != want || (want && h == 0)) {
        printf("FAIL %.*s k=%u: %d\n", (int) len, s, k, (int) ok);
        return 1;
    }
    return 0;
}

int
main(void)
{
    int  bad = 0;
    bool ok;
    bad += check("", 0, 1, true) + check("a", 1, 1, true) + check("a\tb", 3, 1, true) + check("a\tb", 3, 2, true);
    bad += check("a", 1, 2, false) + check("a\tb\tc", 5, 2, false) + check("\t", 1, 2, true) + check("\t\t\t\t", 4, 2, false);
    bad += check("", 0, 2, false) + check("a\tb\tc", 5, 3, true) + check("\t\t", 2, 3, true);
    /* ("ab", "c") and ("a", "bc") */
    if (row_hash("ab\tc", 4, 2, '\t', &ok) == row_hash("a\tbc", 4, 2, '\t', &ok)) bad += 1;
    /* every number of separators against every K up to 32, over rows of every length up to 40 */
    char buf[64];
    for (size_t len = 0; len <= 40; len++) {
        for (size_t nsep = 0; nsep <= len; nsep++) {
            memset(buf, 'x', sizeof(buf));
            for (size_t j = 0; j < nsep; j++) buf[(j * 7) % len] = '\t';
            size_t real = 0;
            for (size_t j = 0; j < len; j++) real += buf[j] == '\t';
            for (uint32_t k = 1; k <= 32; k++) bad += check(buf, len, k, k == 1 || real + 1 == k);
        }
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
