/* tools/asan_tally_number.cpp — CPU-only AddressSanitizer / UBSan run of the number rule of the tally's sums
 * (sregex_amd/csrc/sre_lines_sums.h, what sre_hip_tally_number and sre_k_tally_sums compile): every text sits at the very
 * end of a heap block of exactly its length, so one byte read past `len` is reported.
 *   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -Isregex_amd/csrc tools/asan_tally_number.cpp \
 *       -o /tmp/asan_tn && /tmp/asan_tn
 */
#include "sre_lines_sums.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct Text {
    const uint8_t *p;
    uint8_t byte(uint64_t at) const { return p[at]; }
};

static int
check(const char *s, size_t len, bool want, int64_t value)
{
    uint8_t *heap = static_cast<uint8_t *>(malloc(len ? len : 1));
    memcpy(heap, s, len);
    const Text t = {heap};
    int64_t    got = -4242;
    const bool is = sre_ls_number(t, 0, len, &got);
    free(heap);
    if (is != want || got != (want ? value : -4242)) {
        printf("FAIL %.*s: %d %lld\n", (int) len, s, (int) is, (long long) got);
        return 1;
    }
    return 0;
}

int
main(void)
{
    int bad = 0;
    bad += check("0", 1, true, 0) + check("-0", 2, true, 0) + check("007", 3, true, 7);
    bad += check("999999999999999999", 18, true, 999999999999999999ll) + check("-999999999999999999", 19, true, -999999999999999999ll);
    bad += check("", 0, false, 0) + check("-", 1, false, 0) + check("--1", 3, false, 0) + check("+1", 2, false, 0);
    bad += check("1 ", 2, false, 0) + check(" 1", 2, false, 0) + check("12a", 3, false, 0) + check("1-", 2, false, 0);
    bad += check("1111111111111111111", 19, false, 0) + check("-1111111111111111111", 20, false, 0);
    bad += check("999999999999999999\0", 19, false, 0);
    /* every length up to 24 of digits, with and without the sign, and with one byte of every value at every place */
    char buf[32];
    for (size_t len = 1; len <= 24; len++) {
        for (int neg = 0; neg < 2; neg++) {
            memset(buf, '7', sizeof(buf));
            if (neg) buf[0] = '-';
            const size_t nd = len - (size_t) neg;
            int64_t      v = 0;
            for (size_t j = 0; j < nd && nd <= 18; j++) v = v * 10 + 7;
            bad += check(buf, len, nd >= 1 && nd <= 18, neg ? -v : v);
            for (size_t at = 0; at < len; at++) {
                for (int b = 0; b < 256; b++) {
                    if ((b >= '0' && b <= '9') || (at == 0 && b == '-')) continue;
                    const char keep = buf[at];
                    buf[at] = (char) b;
                    bad += check(buf, len, false, 0);
                    buf[at] = keep;
                }
            }
        }
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
