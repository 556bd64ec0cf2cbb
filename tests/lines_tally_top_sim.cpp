/*
 * lines_tally_top_sim.cpp — the ordered tally on the CPU: the first lines, the order values and their totals, the ordered
 * table, the permute and the ranks, lane by lane as the kernels of sregex_amd/csrc/sre_hip_lines_tally_top.hip run them, with
 * the rules they compile (sre_lines_tally_top.h).  The digit passes between the order values and the ordered table are the
 * line sort's model (lines_sort_sim.cpp, through lines_partition_sim.h), included here unchanged and run over the keys with
 * all = 1.  Every store and every atomic is counted, so tests/test_lines_tally_top_model.py can assert that every word of
 * every array is written exactly once and nothing beyond the caps.  The gather over the ordered table is the extract's model
 * (tests/lines_extract_sim.cpp), unchanged.  tools/asan_tally_top_rule.cpp includes this file.
 */
#include "sre_lines_tally_top.h"
#include "lines_sort_sim.cpp"

extern "C" {

uint32_t lttsim_keys(void) { return SRE_LTT_KEYS; }
uint64_t lttsim_max_range(void) { return SRE_LTT_MAX_RANGE; }
uint32_t lttsim_none(void) { return SRE_LT_NONE; }
uint64_t lttsim_first_flag(void) { return SRE_LG_ENTRY_FIRST; }
uint64_t lttsim_last_flag(void) { return SRE_LG_ENTRY_LAST; }
uint32_t lttsim_index_words(uint32_t k) { return sre_ltt_index_words(k); }
int      lttsim_by_ok(int by, uint64_t by_col, uint64_t v) { return sre_ltt_by_ok(by, by_col, v) ? 1 : 0; }
int      lttsim_range_ok(uint64_t nordered, int64_t vmin, int64_t vmax) { return sre_ltt_range_ok(nordered, vmin, vmax) ? 1 : 0; }
uint64_t lttsim_rows(uint64_t nkeys, uint64_t limit) { return sre_ltt_rows(nkeys, limit); }
uint32_t lttsim_passes(uint64_t nkeys, uint64_t nordered, int64_t vmin, int64_t vmax) { return sre_ltt_passes(nkeys, nordered, vmin, vmax); }

/* the class of a key; *value its order value.  agg: the four words of the column's aggregate */
int32_t
lttsim_order(int by, uint64_t count, const int64_t *agg, int64_t *value)
{
    sre_ls_agg_t a;
    a.sum = agg[0], a.min = agg[1], a.max = agg[2], a.n = (uint64_t) agg[3];
    return sre_ltt_order(by, count, &a, value);
}

/* first lines, a lane per line; fw[key] counts the stores to first[key].  Returns the stores outside [0, nkeys) */
uint64_t
lttsim_first(const uint64_t *tab, const uint32_t *lslot, const uint64_t *cnt, uint64_t n, uint64_t nkeys, uint64_t *first, uint32_t *fw)
{
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t slot = lslot[i];
        if (!sre_lt_keeps(slot, i, tab)) continue;
        const uint64_t key = cnt[slot];
        if (key >= nkeys) {
            bad++;
            continue;
        }
        first[key] = i, fw[key]++;
    }
    return bad;
}

/* the order-values pass over nkeys keys, the walk of sim_values (lines_sort_sim.cpp): value[k], cls[k] (vw[k] counts the stores
 * to both), totals[4] with the identities first, sent[4] the atomics each word received.  aggs: nkeys * v aggregates of four
 * words */
void
lttsim_values(const uint64_t *counts, const int64_t *aggs, uint64_t nkeys, uint32_t v, int by, uint32_t by_col, int64_t *value,
              int8_t *cls, uint32_t *vw, uint64_t *totals, uint32_t *sent)
{
    sim_values(nkeys, value, cls, totals, sent, [&](uint64_t k, int64_t *x) {
        sre_ls_agg_t a = sre_ls_identity();
        if (by != SRE_LTT_COUNT) {
            const int64_t *g = aggs + 4 * (k * v + by_col);
            a.sum = g[0], a.min = g[1], a.max = g[2], a.n = (uint64_t) g[3];
        }
        vw[k]++;
        return sre_ltt_order(by, counts[k], &a, x);
    });
}

/* the ordered table, a lane per entry of the first nrows ranks; tw[x] counts the stores to the two words of entry x.  Returns
 * the entries whose key or first line was out of range */
uint64_t
lttsim_table(const uint32_t *keys, const uint64_t *first, const uint64_t *off, const uint64_t *start, uint64_t nrows, uint64_t nkeys,
             uint64_t n, uint32_t k, uint64_t *cstart, uint64_t *cval, uint32_t *tw)
{
    uint64_t bad = 0;
    for (uint64_t x = 0; x < nrows * k; x++) {
        const uint64_t r = x / k, f = x - r * k, key = keys[r];
        const uint64_t line = key < nkeys ? first[key] : n;
        if (line >= n) {
            bad++;
            continue;
        }
        sre_ltt_entry(off, start, line * k + f, cstart + x, cval + x);
        tw[x]++;
    }
    return bad;
}

/* the permute, a lane per rank: cw / sw / iw / nw count the stores to every WORD of ocounts / osums / index / inv */
uint64_t
lttsim_permute(const uint32_t *keys, uint64_t nkeys, const uint64_t *counts, const int64_t *aggs, uint32_t v, const uint64_t *first,
               const uint64_t *ends, uint64_t n, const uint64_t *cstart, const uint64_t *coff, uint32_t k, const int64_t *value,
               const int8_t *cls, uint64_t *ocounts, uint64_t counts_rows, uint32_t *cw, int64_t *osums, uint64_t sums_rows, uint32_t *sw,
               int64_t *index, uint64_t index_rows, uint32_t *iw, uint32_t *inv, uint32_t *nw)
{
    uint64_t       bad = 0;
    const uint32_t words = sre_ltt_index_words(k);
    for (uint64_t r = 0; r < nkeys; r++) {
        const uint64_t key = keys[r];
        if (key >= nkeys) {
            bad++;
            continue;
        }
        inv[key] = (uint32_t) r, nw[key]++;
        if (r < counts_rows) ocounts[r] = counts[key], cw[r]++;
        if (r < sums_rows) {
            for (uint32_t c = 0; c < 4 * v; c++) osums[4 * r * v + c] = aggs[4 * key * v + c], sw[4 * r * v + c]++;
        }
        if (r < index_rows) {
            const uint64_t line = first[key];
            if (line >= n) {
                bad++;
                continue;
            }
            const uint64_t st = line == 0 ? 0 : ends[line - 1] + 1;
            sre_ltt_index_row(line, st, ends[line] - st, cstart, coff, r, k, key, cls[key] == SRE_LSO_NUMBER ? value[key] : 0,
                              index + r * words);
            for (uint32_t c = 0; c < words; c++) iw[r * words + c]++;
        }
    }
    return bad;
}

/* the ranks of the lines, a lane per line i < m; rw[i] counts the stores */
void
lttsim_ranks(const uint32_t *lslot, const uint64_t *cnt, const uint32_t *inv, uint64_t m, uint64_t nkeys, int64_t *rank, uint32_t *rw)
{
    for (uint64_t i = 0; i < m; i++) {
        const uint32_t slot = lslot[i];
        int64_t        r = -1;
        if (slot != SRE_LT_NONE) {
            const uint64_t key = cnt[slot];
            if (key < nkeys) r = (int64_t) inv[key];
        }
        rank[i] = r, rw[i]++;
    }
}

}
