/*
 * lines_fold_sim.cpp — the fold pass of the line fold (sre_hip_fold_lines) on the CPU: marks, carry, apply, totals, finish,
 * record ids and records run workgroup by workgroup with the kernels' geometry (1024 lines per workgroup, 256 lanes of 4
 * lines, waves of 64; one workgroup of 1024 lanes for the carry) and the block logic the kernels compile
 * (sregex_amd/csrc/sre_lines_fold.h over sre_lines_context.h): the per-lane combine, the scans step by step as the shuffles
 * make them, the head rule, the bitmap words, the cut, the rows.  apply works IN PLACE on val and in any order of the
 * workgroups; every access of marks and apply to val, start and aux outside the workgroup's own lines, and every read of
 * val by apply at all, is counted and not made, so tests/test_lines_fold_model.py can assert the in-place rule.
 */
#include "sre_lines_fold.h"
#include <stdint.h>
#include <vector>

namespace {

/* a per-line array as workgroup [lo, hi) may see it; word 0 is line org */
struct BlockArr {
    uint64_t *a;
    uint64_t  org, n, lo, hi;
    uint64_t *bad;

    uint64_t load(uint64_t i)
    {
        if (i < lo || i >= hi || i >= n) {
            ++*bad;
            return 0;
        }
        return a[i - org];
    }
    void store(uint64_t i, uint64_t v)
    {
        if (i < lo || i >= hi || i >= n) ++*bad;
        else a[i - org] = v;
    }
};

/* a wave's four bitmap words from the bit of every line of its 64 lanes */
void
wave_words(const uint32_t *bit, uint32_t w, uint64_t out[4], uint32_t *count)
{
    uint64_t b[SRE_LC_PER_LANE] = {0};
    for (uint32_t l = 0; l < SRE_LC_WAVE; l++) {
        for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) b[k] |= (uint64_t) bit[SRE_LC_PER_LANE * (w * SRE_LC_WAVE + l) + k] << l;
    }
    for (uint32_t l = 0; l < 4; l++) out[l] = sre_lc_bitmap_word(b, l);
    *count = sre_lc_count(b);
}

/* (word 0 of bits holds line worg) */
void
store_words(uint64_t *bits, uint64_t worg, const uint32_t *bit, uint64_t base, uint64_t n, uint64_t *total)
{
    for (uint32_t w = 0; w < SRE_LC_WAVES; w++) {
        uint64_t words[4];
        uint32_t c;
        wave_words(bit, w, words, &c);
        for (uint32_t l = 0; l < 4; l++) {
            const uint64_t word = base / 64 + 4 * w + l;
            if (bits && word < (n + 63) / 64) bits[word - worg / 64] = words[l];
        }
        if (total) *total += c;
    }
}

/* sre_k_fold_marks of the workgroup whose first line is base */
void
marks_block(BlockArr &val, uint64_t base, uint64_t n, uint32_t s, uint64_t *mbits, uint64_t worg, uint64_t *last, uint64_t *first)
{
    uint32_t p[SRE_LC_THREADS], q[SRE_LC_THREADS], ptot, qtot, bit[SRE_LC_ITEMS];
    for (uint32_t t = 0; t < SRE_LC_THREADS; t++) {
        const uint64_t q0 = base + SRE_LC_PER_LANE * t;
        uint64_t       v[SRE_LC_PER_LANE];
        for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) v[k] = q0 + k < n ? val.load(q0 + k) : 0;
        const uint32_t m = sre_lf_lane_bits(v, q0, n);
        for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) bit[SRE_LC_PER_LANE * t + k] = (m >> k) & 1u;
        sre_lf_lane_marks(m, sre_lf_lane_valid(q0, n), t, s, &p[t], &q[t]);
    }
    store_words(mbits, worg, bit, base, n, nullptr);
    sre_lc_block_scan(p, q, SRE_LC_WAVES, &ptot, &qtot);
    *last = sre_lc_p_global(base, ptot, 0);
    *first = sre_lc_q_global(base, qtot, SRE_LC_NONE);
}

/* sre_k_fold_carry */
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

/* the marked bits of lane t's lines and of the line behind them, from the bitmap whose word 0 holds line worg */
void
lane_bits(const uint64_t *mbits, uint64_t worg, uint64_t q0, uint64_t n, uint32_t *m, uint32_t *mnext)
{
    const uint64_t nx = q0 + SRE_LC_PER_LANE;
    *m = sre_lf_lane_valid(q0, n) ? sre_lf_word_bits(mbits[(q0 - worg) / 64], q0) : 0;
    *mnext = nx < n ? (uint32_t) (mbits[(nx - worg) / 64] >> (nx % 64)) & 1u : 0;
}

/* sre_k_fold_apply of the workgroup whose first line is base: fl / ax its lines' bits and aux words; through the optional
 * arguments what the kernel writes */
void
apply_block(const uint64_t *mbits, uint64_t worg, uint64_t base, uint64_t n, uint32_t s, uint64_t max_lines, uint64_t hin,
            uint64_t qin, uint32_t *fl, uint64_t *ax, const uint64_t *ends, BlockArr *val, BlockArr *start, BlockArr *aux,
            uint64_t *hbits, uint64_t *counts)
{
    uint32_t p[SRE_LC_THREADS], q[SRE_LC_THREADS], ptot, qtot, m[SRE_LC_THREADS], mn[SRE_LC_THREADS];
    for (uint32_t t = 0; t < SRE_LC_THREADS; t++) {
        const uint64_t q0 = base + SRE_LC_PER_LANE * t;
        lane_bits(mbits, worg, q0, n, &m[t], &mn[t]);
        sre_lf_lane_marks(m[t], sre_lf_lane_valid(q0, n), t, s, &p[t], &q[t]);
    }
    sre_lc_block_scan(p, q, SRE_LC_WAVES, &ptot, &qtot);
    uint32_t hbit[SRE_LC_ITEMS], mbit[SRE_LC_ITEMS];
    uint64_t longest = 0;
    for (uint32_t t = 0; t < SRE_LC_THREADS; t++) {
        const uint64_t q0 = base + SRE_LC_PER_LANE * t;
        const uint32_t nv = sre_lf_lane_valid(q0, n);
        sre_lf_lane_lines(q0, n, nv, m[t], mn[t], s, max_lines, sre_lc_p_global(base, p[t], hin), sre_lc_q_global(base, q[t], qin),
                          fl + SRE_LC_PER_LANE * t, ax + SRE_LC_PER_LANE * t);
        for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
            const uint32_t x = SRE_LC_PER_LANE * t + k;
            const uint64_t i = q0 + k;
            hbit[x] = (fl[x] & SRE_LF_HEAD) != 0;
            mbit[x] = (m[t] >> k) & 1u;
            if (k >= nv) continue;
            if (hbit[x] && ax[x] - i > longest) longest = ax[x] - i;
            if (ends) {
                const uint64_t st = i ? ends[i - 1] + 1 : 0;
                val->store(i, ends[i] - st + 1);
                start->store(i, sre_lf_entry_start(st, fl[x]));
                aux->store(i, ax[x]);
            }
        }
    }
    if (counts) {
        counts[0] = counts[1] = 0;
        store_words(hbits, 0, hbit, base, n, &counts[0]);
        store_words(nullptr, 0, mbit, base, n, &counts[1]);
        counts[2] = longest;
    }
}

}  // namespace

extern "C" uint32_t lfsim_items(void) { return SRE_LC_ITEMS; }
extern "C" uint64_t lfsim_flag_last(void) { return SRE_LG_ENTRY_LAST; }

/*
 * The whole call behind the per-line values.  val[0 .. n] holds the values (not 0: marked) and comes back as the offset table
 * off[0 .. n]; start, aux, recid: n words; mbits, hbits: ceil(n / 64) words; order[0 .. nblk): the order in which apply takes
 * the workgroups.  info: nrecords, nmarked, longest, fwritten, fbytes, the cut line.  rows: records_cap rows of five words.
 * Returns the accesses outside a workgroup's own lines, and the reads of val by apply.
 */
extern "C" uint64_t
lfsim_run(uint64_t *val, uint64_t *start, uint64_t *aux, const uint64_t *ends, uint64_t n, int next, uint64_t max_lines,
          const uint64_t *order, uint64_t *mbits, uint64_t *hbits, int64_t *recid, uint64_t out_cap, uint64_t records_cap, int64_t *rows,
          uint64_t *info)
{
    const uint64_t        nblk = (n + SRE_LC_ITEMS - 1) / SRE_LC_ITEMS;
    const uint32_t        s = next ? 1u : 0u;
    std::vector<uint64_t> hin(nblk), qin(nblk), blkh(nblk), blkm(nblk), blkl(nblk);
    uint64_t              bad = 0;
    for (uint64_t b = 0; b < nblk; b++) {
        const uint64_t base = b * SRE_LC_ITEMS;
        BlockArr       v = {val, 0, n, base, base + SRE_LC_ITEMS, &bad};
        marks_block(v, base, n, s, mbits, 0, &hin[b], &qin[b]);
    }
    carry(hin.data(), qin.data(), nblk);
    std::vector<uint32_t> fl(SRE_LC_ITEMS);
    std::vector<uint64_t> ax(SRE_LC_ITEMS);
    for (uint64_t x = 0; x < nblk; x++) {
        const uint64_t b = order[x], base = b * SRE_LC_ITEMS;
        BlockArr       v = {val, 0, n, base, base + SRE_LC_ITEMS, &bad}, st = {start, 0, n, base, base + SRE_LC_ITEMS, &bad},
                 au = {aux, 0, n, base, base + SRE_LC_ITEMS, &bad};
        uint64_t counts[3];
        apply_block(mbits, 0, base, n, s, max_lines, hin[b], qin[b], fl.data(), ax.data(), ends, &v, &st, &au, hbits, counts);
        blkh[b] = counts[0];
        blkm[b] = counts[1];
        blkl[b] = counts[2];
    }
    /* totals */
    uint64_t th = 0, tm = 0, tl = 0;
    for (uint64_t b = 0; b < nblk; b++) {
        const uint64_t h = blkh[b];
        blkh[b] = th;
        th += h;
        tm += blkm[b];
        tl = blkl[b] > tl ? blkl[b] : tl;
    }
    /* the scan of the entry table */
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t v = val[i];
        val[i] = run;
        run += v;
    }
    val[n] = run;
    /* finish */
    const uint64_t cut = sre_lf_cut(sre_lf_first_beyond(val, n, out_cap), n, hbits, aux);
    uint64_t       written = th;
    if (cut != n) {
        const uint64_t b = cut / SRE_LC_ITEMS;
        written = blkh[b];
        for (uint64_t j = b * SRE_LC_ITEMS; j < cut; j++) written += (hbits[j / 64] >> (j % 64)) & 1u;
    }
    /* record ids and records, lane by lane */
    const uint64_t limit = records_cap < written ? records_cap : written;
    for (uint64_t b = 0; b < nblk; b++) {
        uint64_t r = blkh[b];
        for (uint32_t t = 0; t < SRE_LC_THREADS; t++) {
            const uint64_t q0 = b * SRE_LC_ITEMS + SRE_LC_PER_LANE * t;
            const uint32_t h = sre_lf_lane_valid(q0, n) ? sre_lf_word_bits(hbits[q0 / 64], q0) : 0;
            for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
                if ((h >> k) & 1u) {
                    if (r < limit) sre_lf_record_row(rows + r * SRE_LF_ROW, q0 + k, aux[q0 + k], q0 + k ? ends[q0 + k - 1] + 1 : 0, val);
                    r++;
                }
                if (q0 + k < n) recid[q0 + k] = (int64_t) r - 1;
            }
        }
    }
    info[0] = th;
    info[1] = tm;
    info[2] = tl;
    info[3] = written;
    info[4] = val[cut];
    info[5] = cut;
    return bad;
}

/* the carry alone over given block words (synthetic line indices of any size) */
extern "C" void
lfsim_carry(uint64_t *last, uint64_t *first, uint64_t nblk)
{
    carry(last, first, nblk);
}

/* marks of ONE workgroup whose first line is `base` (any multiple of 1024, beyond 2^32 too) of a buffer of n lines: v[0 ..
 * 1024) its values; words[0 .. 16) its bitmap words, out[0 .. 2) its block words */
extern "C" uint64_t
lfsim_marks_block(uint64_t *v, uint64_t base, uint64_t n, int next, uint64_t *words, uint64_t *out)
{
    uint64_t              bad = 0;
    BlockArr              a = {v, base, n, base, base + SRE_LC_ITEMS, &bad};
    for (uint64_t w = 0; w < 16; w++) words[w] = 0;
    marks_block(a, base, n, next ? 1u : 0u, words, base, &out[0], &out[1]);
    return bad;
}

/* apply of ONE such workgroup with the carries hin / qin: words[0 .. 17) the bitmap words of its lines and of the line behind
 * them; fl[0 .. 1024) the lines' SRE_LF_* bits, ax[0 .. 1024) their aux words, counts[0 .. 3) heads, marked lines, longest */
extern "C" void
lfsim_apply_block(const uint64_t *words, uint64_t base, uint64_t n, int next, uint64_t max_lines, uint64_t hin, uint64_t qin,
                  uint32_t *fl, uint64_t *ax, uint64_t *counts)
{
    apply_block(words, base, base, n, next ? 1u : 0u, max_lines, hin, qin, fl, ax, nullptr, nullptr, nullptr, nullptr, nullptr, counts);
}
