/*
 * scan_split_sim.cpp — the split walk's rule (sregex_amd/csrc/sre_scan_split.h, which sre_k_scan's common round mirrors
 * line by line) against the serial walk, on random small fast tables.  Stand-alone: no GPU, no library.
 *
 *   scan_split_sim SEED CASES   ->  "ok cases=.. hit=.. miss=.. slow=.. slow_later=.. counted=.."   exit status 0
 *                                   or the first case that differs, exit status 1
 *
 * A table is what the kernel keeps in LDS: rows of 256 entries [count : 8][flags : 8][byte address of the next row : 16]
 * from byte address BASE on, a trap row behind them whose entries all point back into it with the SLOW flag, SLOW
 * entries of ordinary rows pointing there too, count bytes on some entries (none in the trap row).  An index string
 * is one round: N byte offsets into a row (index * 4), N = 8, 16, 32 or 64 as for 1, 2, 4 and 8 class bits.  Quiet
 * tables (most entries of a row point back to it, as in a stable stretch) make the guess hit, busy ones make it miss.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sre_scan_split.h"

namespace {

constexpr uint32_t ROW_BYTES = 1024, BASE = 512;     /* (the kernel's table does not start at LDS address 0 either) */

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
};

struct Table {
    uint32_t              nrows;        /* ordinary rows; row nrows is the trap row */
    std::vector<uint32_t> e;
    uint32_t row_addr(uint32_t r) const { return BASE + r * ROW_BYTES; }
    uint32_t at(uint32_t t, uint32_t ix4) const { return e[((t & SRE_SPLIT_ROW_MASK) - BASE + ix4) / 4]; }
};

Table
make_table(Rng &g, uint32_t nsym, uint32_t quiet_pct, uint32_t slow_pm, uint32_t cnt_pct)
{
    Table T;
    T.nrows = 1 + g.below(6);
    T.e.assign((T.nrows + 1) * 256, 0);
    const uint32_t trap = T.row_addr(T.nrows) | SRE_SPLIT_SLOW;
    for (uint32_t r = 0; r <= T.nrows; r++) {
        for (uint32_t x = 0; x < 256; x++) {
            uint32_t v = trap;
            if (r < T.nrows && x < nsym && g.below(1000) >= slow_pm) {
                const uint32_t to = g.below(100) < quiet_pct ? r : g.below(T.nrows);
                v = T.row_addr(to) | (g.below(100) < cnt_pct ? (1 + g.below(3)) << SRE_SPLIT_CNT_SHIFT : 0u)
                    | (g.below(8) == 0 ? 1u << 17 : 0u);        /* (another flag bit the rule must carry along) */
            }
            T.e[r * 256 + x] = v;
        }
    }
    return T;
}

template <int K>
int
check(const Table &T, const std::vector<uint32_t> &ix, uint32_t t0, const sre_split_result &want, bool *miss)
{
    auto look = [&](uint32_t t, int j) { return T.at(t, ix[j]); };
    const sre_split_result got = sre_split_walk<K, true>(t0, (int) ix.size(), look);
    const sre_split_result nocount = sre_split_walk<K, false>(t0, (int) ix.size(), look);
    *miss = got.miss;
    return got.t == want.t && got.cnt == want.cnt && nocount.t == want.t && nocount.cnt == 0;
}

}

int
main(int argc, char **argv)
{
    Rng g{argc > 1 ? strtoull(argv[1], nullptr, 0) : 1};
    const long cases = argc > 2 ? atol(argv[2]) : 20000;
    long hit = 0, missed = 0, slow = 0, slow_later = 0, counted = 0;
    for (long c = 0; c < cases; c++) {
        const uint32_t nsym = 2 + g.below(15);
        const uint32_t quiet = g.below(3) == 0 ? 30 + g.below(50) : 90 + g.below(11);
        const Table T = make_table(g, nsym, quiet, g.below(2) ? g.below(30) : 0, g.below(2) ? g.below(40) : 0);
        const int N = 8 << g.below(4);
        std::vector<uint32_t> ix(N);
        /* sometimes one symbol for the whole round but one place: an event at a chosen offset */
        const bool flat = g.below(2) == 0;
        const uint32_t s0 = g.below(nsym), at = g.below(N);
        for (int j = 0; j < N; j++) ix[j] = 4 * (flat && (uint32_t) j != at ? s0 : g.below(nsym + (g.below(50) == 0)));
        const uint32_t t0 = T.row_addr(g.below(T.nrows)) | (g.below(4) == 0 ? 3u << SRE_SPLIT_CNT_SHIFT : 0u);
        /* the serial walk */
        sre_split_result want;
        want.t = t0;
        want.cnt = 0;
        int first_slow = -1;
        for (int j = 0; j < N; j++) {
            want.t = T.at(want.t, ix[j]);
            want.cnt += want.t >> SRE_SPLIT_CNT_SHIFT;
            if (first_slow < 0 && (want.t & SRE_SPLIT_SLOW)) first_slow = j;
        }
        bool m2 = false, m4 = false;
        if (!check<1>(T, ix, t0, want, &m2) || m2 || !check<2>(T, ix, t0, want, &m2) || !check<4>(T, ix, t0, want, &m4)) {
            printf("DIFFERS case %ld N %d t0 %#x want t %#x cnt %u\n", c, N, t0, want.t, want.cnt);
            return 1;
        }
        hit += !m4;
        missed += m4;
        slow += first_slow >= 0 && first_slow < N / 4;
        slow_later += first_slow >= N / 4;
        counted += want.cnt != 0 && first_slow < 0;
    }
    printf("ok cases=%ld hit=%ld miss=%ld slow=%ld slow_later=%ld counted=%ld\n", cases, hit, missed, slow, slow_later, counted);
    return 0;
}
