/*
 * sre_scan_split.h — the rule of the speculative split walk of sre_k_scan's common round, in plain C++.
 *
 * A round is N dependent fast-table lookups.  Walked as K sub-chains of N / K lookups, step by step side by side,
 * the K reads of a step are independent and overlap in LDS.  Chain 0 starts where the serial walk starts; chains
 * 1 .. K-1 start from the GUESS that the lane is still in the row it entered the round in (a stable stretch, any
 * quiet stream).  A chain's result counts only if the chain in front of it counts and ended in the guessed row; the
 * first chain that does not count and all behind it are walked again serially.  Entries that leave the fast path
 * (SLOW) point to the trap row, whose entries all point back to it, and no round starts there: a chain that met one
 * ends in another row than the guessed one, and a round that ends SLOW stays SLOW whatever is walked behind it.
 *
 * The kernel (sre_hip_scan.hip, "the split walk") mirrors sre_split_walk line by line with its SDWA forms in place
 * of look(); tests/scan_split_sim.cpp checks this text against the serial walk.  Change both together.
 *
 * An entry is [count : 8][flags : 8][byte address of the next row : 16], as in the kernel's LDS copy.
 */
#ifndef SRE_SCAN_SPLIT_H
#define SRE_SCAN_SPLIT_H

#include <stdint.h>

#define SRE_SPLIT_ROW_MASK 0xffffu          /* the next row's address */
#define SRE_SPLIT_SLOW (1u << 16)           /* the entry leaves the fast path (it points into the trap row) */
#define SRE_SPLIT_CNT_SHIFT 24

struct sre_split_result {
    uint32_t t;         /* the round's last entry */
    uint32_t cnt;       /* sum of the count bytes of the round's entries */
    bool     miss;      /* some chain did not count: the caller's throttle */
};

/* look(t, j): the entry that index j of the round selects in the row entry t points to */
template <bool COUNT, typename Look>
static inline void
sre_split_serial(uint32_t &t, uint32_t &cnt, int j0, int j1, Look look)
{
    for (int j = j0; j < j1; j++) {
        t = look(t, j);
        if (COUNT) cnt += t >> SRE_SPLIT_CNT_SHIFT;
    }
}

template <int K, bool COUNT, typename Look>
static inline sre_split_result
sre_split_walk(uint32_t t, int N, Look look)
{
    const int      L = N / K;                           /* lookups per chain */
    const uint32_t t0 = t;                              /* the guess: the round's own entry row (low half) */
    uint32_t       tc[K], cc[K];
    for (int c = 0; c < K; c++) {
        tc[c] = t0;
        cc[c] = 0;
    }
    for (int j = 0; j < L; j++) {
        for (int c = 0; c < K; c++) tc[c] = look(tc[c], c * L + j);
        if (COUNT) {
            for (int c = 0; c < K; c++) cc[c] += tc[c] >> SRE_SPLIT_CNT_SHIFT;
        }
    }
    /* every guess hit iff every chain but the last ended in row t0 (a SLOW entry points to the trap row, where no
     * round starts: the row's address says it all) */
    sre_split_result r;
    uint32_t         off = 0;
    r.t = tc[K - 1];
    r.cnt = 0;
    for (int c = 0; c < K - 1; c++) off |= tc[c] ^ t0;
    for (int c = 0; c < K; c++) r.cnt += cc[c];
    r.miss = (off & SRE_SPLIT_ROW_MASK) != 0;
    if (r.miss) {
        /* chain c counts iff chain c - 1 counts and ended in row t0 */
        int nv = 1;                                     /* chains that count */
        r.t = tc[0];
        r.cnt = cc[0];
        for (int c = 1; c < K; c++) {
            if (nv == c && ((r.t ^ t0) & SRE_SPLIT_ROW_MASK) == 0) {
                r.t = tc[c];
                r.cnt += cc[c];
                nv = c + 1;
            }
        }
        /* the first chain that does not count and all behind it, from the end of the chain in front; a SLOW end stays
         * SLOW whatever follows (the trap row): nothing to walk */
        if (!(r.t & SRE_SPLIT_SLOW)) {
            for (int c = 1; c < K; c++) {
                if (nv <= c) sre_split_serial<COUNT>(r.t, r.cnt, c * L, (c + 1) * L, look);
            }
        }
    }
    return r;
}

#endif
