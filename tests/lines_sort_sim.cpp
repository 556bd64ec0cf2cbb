/*
 * lines_sort_sim.cpp — the line sort on the CPU: the values pass, then every digit pass through the partition model
 * (lines_partition_sim.h), with the rules the kernels compile (sregex_amd/csrc/sre_lines_sort.h, sre_lines_route_key.h,
 * sre_lines_route.h, sre_lines_sums.h): the class and the value of a line, the totals a workgroup sends, the sort key and
 * the digit; then the compact table, the result words and the index rows.  Every store and every atomic is counted, so tests/test_lines_sort_model.py
 * can assert that every word of every array is written exactly once per pass.  The gather over the table is the extract's
 * model (tests/lines_extract_sim.cpp), unchanged.  tools/asan_sort_rule.cpp includes this file.
 */
#include "sre_lines_sort.h"
#include "lines_partition_sim.h"
#include <string.h>

namespace {

/* the value table of the one sort group over host memory: every access checked against the sizes the caller gave */
struct SimVals {
    const uint8_t  *buf;
    uint64_t        len;
    const uint64_t *vval, *vstart;
    uint64_t       *bad;
    uint64_t val(uint64_t line, uint32_t) const { return vval[line]; }
    uint64_t raw(uint64_t line, uint32_t) const { return vstart[line]; }
    uint8_t  byte(uint64_t at) const
    {
        if (at >= len) {
            (*bad)++;
            return 0;
        }
        return buf[at];
    }
};

/* the four words of the call and the atomics sent to each */
struct SimMem {
    uint64_t *w;
    uint32_t *sent;
    void add_keyed(uint64_t v) { w[0] += v, sent[0]++; }
    void add_numbered(uint64_t v) { w[1] += v, sent[1]++; }
    void min(int64_t v)
    {
        if (v < (int64_t) w[2]) w[2] = (uint64_t) v;
        sent[2]++;
    }
    void max(int64_t v)
    {
        if (v > (int64_t) w[3]) w[3] = (uint64_t) v;
        sent[3]++;
    }
};

/* what every digit pass knows of the call (SortKeys of sre_hip_lines_sort.hip) */
struct SimKeys {
    int64_t  vmin, vmax;
    uint64_t range;
    int      desc, all;
};

SimKeys
sim_keys(int64_t vmin, int64_t vmax, uint64_t nnumbered, int desc, int all)
{
    SimKeys k;
    k.vmin = vmin;
    k.vmax = vmax;
    k.range = sre_lso_range(nnumbered, vmin, vmax);
    k.desc = desc;
    k.all = all;
    return k;
}

/* a digit pass (SortPass of sre_hip_lines_sort.hip; value != NULL: pass 0 over the lines); kw[r] / lw[r] count the stores to
 * dkey[r] / dline[r] */
struct SimSortPass {
    const int64_t  *value;
    const int8_t   *cls;
    const uint64_t *src;
    const uint32_t *sline;
    uint64_t        n;
    SimKeys         k;
    uint32_t        pass;
    uint64_t       *dkey;
    uint32_t       *dline, *kw, *lw;
    uint32_t nd() const { return 1u << SRE_LSO_DIGIT_BITS; }
    uint32_t bits() const { return SRE_LSO_DIGIT_BITS; }
    int      rule() const { return SRE_LRK_RANK_BITS; }
    uint64_t load(uint64_t i) const
    {
        if (i >= n) return SRE_LSO_DROPPED;
        return value ? sre_lso_key(cls[i], value[i], k.vmin, k.vmax, k.range, k.desc, k.all) : src[i];
    }
    bool     taken(uint64_t key) const { return key != SRE_LSO_DROPPED; }
    uint32_t digit(uint64_t key) const { return sre_lso_digit(key, pass); }
    void     store(uint64_t r, uint64_t key, uint64_t i)
    {
        dkey[r] = key, kw[r]++;
        dline[r] = value ? (uint32_t) i : sline[i], lw[r]++;
    }
};

/* the values pass (sre_k_values of sre_hip_lines_values.h) over n items, workgroup by workgroup, wave by wave, lane by lane:
 * value[i] and cls[i] of every item, totals[4] with the identities first, sent[4] the atomics each word received.
 * classify(i, &v): the class of item i, v its value; it counts the stores to value[i] and cls[i] */
template <class Classify>
void
sim_values(uint64_t n, int64_t *value, int8_t *cls, uint64_t *totals, uint32_t *sent, Classify classify)
{
    const sre_lso_totals_t id = sre_lso_identity();
    SimMem                 mem = {totals, sent};
    totals[0] = id.nkeyed, totals[1] = id.nnumbered, totals[2] = (uint64_t) id.vmin, totals[3] = (uint64_t) id.vmax;
    const uint64_t nwg = (n + SRE_LSO_LINES - 1) / SRE_LSO_LINES;
    for (uint64_t w = 0; w < nwg; w++) {
        sre_lso_totals_t part[SRE_LSO_THREADS / 64u];
        for (uint32_t wave = 0; wave < SRE_LSO_THREADS / 64u; wave++) {
            sre_lso_totals_t t = sre_lso_identity();
            for (uint32_t lane = 0; lane < 64; lane++) {
                for (uint32_t j = 0; j < SRE_LSO_PER_LANE; j++) {
                    const uint64_t i = w * SRE_LSO_LINES + j * SRE_LSO_THREADS + wave * 64u + lane;
                    if (i >= n) continue;
                    int64_t       v;
                    const int32_t c = classify(i, &v);
                    value[i] = v;
                    cls[i] = (int8_t) c;
                    t = sre_lso_merge(t, sre_lso_single(c, v));
                }
            }
            part[wave] = t;
        }
        sre_lso_totals_t t = part[0];
        for (uint32_t wave = 1; wave < SRE_LSO_THREADS / 64u; wave++) t = sre_lso_merge(t, part[wave]);
        sre_lso_flush(mem, t);
    }
}

}  // namespace

extern "C" {

uint32_t lsosim_items(void) { return SRE_LR_ITEMS; }
uint32_t lsosim_values_lines(void) { return SRE_LSO_LINES; }
uint64_t lsosim_flags(void) { return SRE_LG_ENTRY_LAST | SRE_LG_ENTRY_FIRST; }
uint64_t lsosim_start_mask(void) { return SRE_LG_ENTRY_START; }
uint64_t lsosim_unset(void) { return SRE_LG_ENTRY_UNSET; }
uint64_t lsosim_dropped(void) { return SRE_LSO_DROPPED; }

uint64_t lsosim_range(uint64_t nnum, int64_t vmin, int64_t vmax) { return sre_lso_range(nnum, vmin, vmax); }
uint64_t lsosim_selected(uint64_t n, uint64_t nnum, int all) { return sre_lso_selected(n, nnum, all); }
uint64_t lsosim_max_key(uint64_t n, uint64_t nnum, uint64_t range, int all) { return sre_lso_max_key(n, nnum, range, all); }
uint32_t lsosim_passes(uint64_t n, uint64_t nnum, uint64_t range, int all) { return sre_lso_passes(n, nnum, range, all); }
uint64_t lsosim_limited(uint64_t nsel, uint64_t limit) { return sre_lso_limited(nsel, limit); }
uint32_t lsosim_digit(uint64_t key, uint32_t pass) { return sre_lso_digit(key, pass); }

uint64_t
lsosim_key(int32_t cls, int64_t v, int64_t vmin, int64_t vmax, uint64_t nnum, int desc, int all)
{
    return sre_lso_key(cls, v, vmin, vmax, sre_lso_range(nnum, vmin, vmax), desc, all);
}

/* the values pass over the value table of n lines: value[i], cls[i] (vw[i], cw[i] count the stores), totals[4] with the
 * identities first, sent[4] the atomics each word received.  Returns the source bytes read outside [0, len) */
uint64_t
lsosim_values(const uint8_t *buf, uint64_t len, const uint64_t *vval, const uint64_t *vstart, uint64_t n, int64_t *value, int8_t *cls,
              uint32_t *vw, uint32_t *cw, uint64_t *totals, uint32_t *sent)
{
    uint64_t      bad = 0;
    const SimVals vals = {buf, len, vval, vstart, &bad};
    sim_values(n, value, cls, totals, sent, [&](uint64_t i, int64_t *v) {
        vw[i]++, cw[i]++;
        return sre_lso_line(vals, i, v);
    });
    return bad;
}

/* count of one pass: cnt[d * nwg + w]; writes[] counts the stores to every word of cnt.  value != NULL: pass 0 over the lines */
void
lsosim_count(const int64_t *value, const int8_t *cls, const uint64_t *src, uint64_t n, int64_t vmin, int64_t vmax, uint64_t nnum,
             int desc, int all, uint32_t pass, uint64_t *cnt, uint32_t *writes)
{
    const SimSortPass p = {value, cls, src, NULL, n, sim_keys(vmin, vmax, nnum, desc, all), pass, NULL, NULL, NULL, NULL};
    (void) sim_count(p, n, cnt, writes);
}

void lsosim_scan(uint64_t *v, uint64_t n) { sim_scan(v, n); }

/* scatter of one pass over the scanned counts; kw[r] / lw[r] count the stores to dkey[r] / dline[r].  Returns the stores that
 * fell outside [0, total) */
uint64_t
lsosim_scatter(const int64_t *value, const int8_t *cls, const uint64_t *src, const uint32_t *sline, uint64_t n, int64_t vmin,
               int64_t vmax, uint64_t nnum, int desc, int all, uint32_t pass, const uint64_t *first, uint64_t total, uint64_t *dkey,
               uint32_t *dline, uint32_t *kw, uint32_t *lw)
{
    SimSortPass p = {value, cls, src, sline, n, sim_keys(vmin, vmax, nnum, desc, all), pass, dkey, dline, kw, lw};
    return sim_scatter(p, n, first, total);
}

/* the compact table of the first nout ranks; writes[r] counts the stores to the two words of rank r */
void
lsosim_table(const uint32_t *lines, const uint64_t *ends, uint64_t nout, uint64_t nlines, uint64_t *cstart, uint64_t *cval,
             uint32_t *writes)
{
    for (uint64_t r = 0; r < nout; r++) {
        const uint64_t i = lines[r];
        if (i >= nlines) continue;
        const uint64_t st = i == 0 ? 0 : ends[i - 1] + 1;
        sre_lrk_entry(st, ends[i] - st, cstart + r, cval + r);
        writes[r]++;
    }
}

void lsosim_result(const uint64_t *coff, uint64_t nout, uint64_t out_cap, uint64_t *res) { sre_lr_result(coff, nout, out_cap, res); }

void
lsosim_index_row(uint64_t line, const uint64_t *cstart, const uint64_t *coff, uint64_t r, int64_t value, int32_t cls, int64_t *row)
{
    sre_lso_index_row(line, cstart, coff, r, value, cls, row);
}

}
