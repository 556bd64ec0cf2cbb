/*
 * lines_context_sim.cpp — the context pass of the line filter on the CPU: marks, carry and apply run workgroup by
 * workgroup with the kernels' geometry (1024 lines per workgroup, 256 lanes of 4 lines, waves of 64; one workgroup of
 * 1024 lanes for the carry) and the block logic the kernels compile (sregex_amd/csrc/sre_lines_context.h): the
 * per-lane combine, the scans step by step as the shuffles make them, the selection rule, the bitmap word, the counts.
 * apply works IN PLACE on val and in any order of the workgroups; every access to val outside the workgroup's own
 * lines is counted and not made, so tests/test_lines_context_model.py can assert the in-place rule.
 */
#include "sre_lines_context.h"
#include <stdint.h>
#include <vector>

namespace {

/* val as workgroup b of apply may see it */
struct BlockVal {
    uint64_t *val;              /* val[0] is line org */
    uint64_t  org, n, lo, hi;   /* the workgroup's lines [lo, hi) */
    uint64_t  bad;

    uint64_t load(uint64_t i)
    {
        if (i < lo || i >= hi || i >= n) {
            bad++;
            return 0;
        }
        return val[i - org];
    }
    void store(uint64_t i, uint64_t v)
    {
        if (i < lo || i >= hi || i >= n) bad++;
        else val[i - org] = v;
    }
};

/* the workgroup's scans over its lanes' words, as sre_k_context_marks and sre_k_context_apply start */
void
block_words(BlockVal &bv, uint64_t base, uint64_t v[][SRE_LC_PER_LANE], uint32_t *p, uint32_t *q, uint32_t *ptot, uint32_t *qtot)
{
    for (uint32_t t = 0; t < SRE_LC_THREADS; t++) {
        for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
            const uint64_t i = base + SRE_LC_PER_LANE * t + k;
            v[t][k] = i < bv.n ? bv.load(i) : 0;
        }
        sre_lc_lane_marks(v[t], t, &p[t], &q[t]);
    }
    sre_lc_block_scan(p, q, SRE_LC_WAVES, ptot, qtot);
}

/* sre_k_context_apply of one workgroup whose first line is `base`: the lines' bits into fl[0 .. 1024), and through the
 * optional arguments what the kernel writes */
void
apply_block(BlockVal &bv, const uint64_t *ends, uint64_t base, uint64_t pin, uint64_t qin, uint64_t before, uint64_t after,
            uint32_t *fl, uint64_t *bits, uint64_t *nmatched, uint64_t *ngroups)
{
    static uint64_t v[SRE_LC_THREADS][SRE_LC_PER_LANE];
    uint32_t        p[SRE_LC_THREADS], q[SRE_LC_THREADS], ptot, qtot;
    block_words(bv, base, v, p, q, &ptot, &qtot);
    for (uint32_t t = 0; t < SRE_LC_THREADS; t++) {
        const uint64_t q0 = base + SRE_LC_PER_LANE * t;
        sre_lc_lane_lines(q0, bv.n, v[t], sre_lc_p_global(base, p[t], pin), sre_lc_q_global(base, q[t], qin), before, after,
                          fl + SRE_LC_PER_LANE * t);
    }
    uint64_t m = 0, g = 0;
    for (uint32_t w = 0; w < SRE_LC_WAVES; w++) {
        uint64_t bm[SRE_LC_PER_LANE] = {0}, bc[SRE_LC_PER_LANE] = {0}, bg[SRE_LC_PER_LANE] = {0};
        for (uint32_t l = 0; l < SRE_LC_WAVE; l++) {
            const uint32_t t = w * SRE_LC_WAVE + l;
            for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
                const uint32_t f = fl[SRE_LC_PER_LANE * t + k];
                const uint64_t i = base + SRE_LC_PER_LANE * t + k;
                if ((f & SRE_LC_CONTEXT) && ends) bv.store(i, ends[i] - (i ? ends[i - 1] + 1 : 0) + 1);
                bm[k] |= (uint64_t) (v[t][k] != 0) << l;
                bc[k] |= (uint64_t) ((f & SRE_LC_CONTEXT) != 0) << l;
                bg[k] |= (uint64_t) ((f & SRE_LC_GROUP) != 0) << l;
            }
        }
        for (uint32_t l = 0; bits && l < SRE_LC_WAVE * SRE_LC_PER_LANE / 64; l++) {
            const uint64_t word = base / 64 + (SRE_LC_WAVE * SRE_LC_PER_LANE / 64) * w + l;
            if (word < (bv.n + 63) / 64) bits[word] = sre_lc_bitmap_word(bc, l);
        }
        m += sre_lc_count(bm);
        g += sre_lc_count(bg);
    }
    if (nmatched) *nmatched += m;
    if (ngroups) *ngroups += g;
}

/* sre_k_context_carry: 1024 lanes, a contiguous run of the block words each */
void
carry(uint64_t *last, uint64_t *first, uint64_t nblk)
{
    uint64_t       p[SRE_LC_CARRY_LANES], q[SRE_LC_CARRY_LANES], ptot, qtot;
    const uint64_t per = (nblk + SRE_LC_CARRY_LANES - 1) / SRE_LC_CARRY_LANES;
    for (uint64_t t = 0; t < SRE_LC_CARRY_LANES; t++) {
        const uint64_t lo = t * per < nblk ? t * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
        sre_lc_run_marks(last, first, lo, hi, &p[t], &q[t]);
    }
    sre_lc_block_scan(p, q, SRE_LC_CARRY_LANES / SRE_LC_WAVE, &ptot, &qtot);
    for (uint64_t t = 0; t < SRE_LC_CARRY_LANES; t++) {
        const uint64_t lo = t * per < nblk ? t * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
        sre_lc_run_carry(last, first, lo, hi, p[t], q[t]);
    }
}

}  // namespace

extern "C" uint32_t lcsim_items(void) { return SRE_LC_ITEMS; }

/*
 * The whole pass over val[0 .. n) and ends[0 .. n): val in place, bits[0 .. ceil(n / 64)), counts[0] = matched lines,
 * counts[1] = groups.  order[0 .. nblk) is the order in which apply takes the workgroups (any permutation gives the same:
 * no workgroup reads what another one writes).  Returns the accesses of apply to val outside the workgroup's lines.
 */
extern "C" uint64_t
lcsim_run(uint64_t *val, const uint64_t *ends, uint64_t n, uint64_t before, uint64_t after, const uint64_t *order, uint64_t *bits,
          uint64_t *counts)
{
    const uint64_t        nblk = (n + SRE_LC_ITEMS - 1) / SRE_LC_ITEMS;
    std::vector<uint64_t> last(nblk), first(nblk);
    static uint64_t       v[SRE_LC_THREADS][SRE_LC_PER_LANE];
    uint64_t              bad = 0;
    for (uint64_t b = 0; b < nblk; b++) {
        const uint64_t base = b * SRE_LC_ITEMS;
        BlockVal       bv = {val, 0, n, base, base + SRE_LC_ITEMS, 0};
        uint32_t       p[SRE_LC_THREADS], q[SRE_LC_THREADS], ptot, qtot;
        block_words(bv, base, v, p, q, &ptot, &qtot);
        last[b] = sre_lc_p_global(base, ptot, 0);
        first[b] = sre_lc_q_global(base, qtot, SRE_LC_NONE);
        bad += bv.bad;
    }
    carry(last.data(), first.data(), nblk);
    counts[0] = counts[1] = 0;
    std::vector<uint32_t> fl(SRE_LC_ITEMS);
    for (uint64_t x = 0; x < nblk; x++) {
        const uint64_t b = order[x], base = b * SRE_LC_ITEMS;
        BlockVal       bv = {val, 0, n, base, base + SRE_LC_ITEMS, 0};
        apply_block(bv, ends, base, last[b], first[b], before, after, fl.data(), bits, &counts[0], &counts[1]);
        bad += bv.bad;
    }
    return bad;
}

/* the carry alone over given block words (synthetic line indices of any size) */
extern "C" void
lcsim_carry(uint64_t *last, uint64_t *first, uint64_t nblk)
{
    carry(last, first, nblk);
}

/* apply of ONE workgroup whose first line is `base` (any multiple of 1024, beyond 2^32 too) of a buffer of n lines, with
 * the carries pin / qin: v[0 .. 1024) its values (not written), fl[0 .. 1024) the lines' SRE_LC_* bits */
extern "C" void
lcsim_block(uint64_t *v, uint64_t base, uint64_t n, uint64_t pin, uint64_t qin, uint64_t before, uint64_t after, uint32_t *fl)
{
    BlockVal bv = {v, base, n, base, base + SRE_LC_ITEMS, 0};
    apply_block(bv, nullptr, base, pin, qin, before, after, fl, nullptr, nullptr, nullptr);
}
