/*
 * lines_sort_sim.cpp — the line sort on the CPU: the values pass, then count, scan and scatter of every digit pass run
 * workgroup by workgroup, slot by slot and lane by lane with the rules the kernels compile (sregex_amd/csrc/sre_lines_sort.h,
 * sre_lines_route_key.h, sre_lines_route.h, sre_lines_sums.h): the class and the value of a line, the totals a workgroup
 * sends, the sort key, the digit, the rank rule of a slot on ballots, the slot prefix and the global rank; then the compact
 * table, the result words and the index rows.  Every store and every atomic is counted, so tests/test_lines_sort_model.py
 * can assert that every word of every array is written exactly once per pass.  The gather over the table is the extract's
 * model (tests/lines_extract_sim.cpp), unchanged.  tools/asan_sort_rule.cpp includes this file.
 */
#include "sre_lines_sort.h"
#include <stdint.h>
#include <string.h>
#include <vector>

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

/* one slot of 64 lanes in lockstep: what slot_rank<SRE_LRK_RANK_BITS> of sre_hip_lines_rank.h does with __ballot */
struct SimSlot {
    bool     sel[64];
    uint32_t digit[64];
    uint32_t rank[64];

    template <class Pred> uint64_t ballot(Pred pred) const
    {
        uint64_t m = 0;
        for (uint32_t x = 0; x < 64; x++) m |= (uint64_t) (pred(x) ? 1 : 0) << x;
        return m;
    }

    void run(uint32_t *c)
    {
        uint64_t       m[64];
        const uint64_t all = ballot([&](uint32_t x) { return sel[x]; });
        for (uint32_t x = 0; x < 64; x++) m[x] = all;
        for (uint32_t bit = 0; bit < SRE_LSO_DIGIT_BITS; bit++) {
            const uint64_t with_bit = ballot([&](uint32_t x) { return sel[x] && ((digit[x] >> bit) & 1u); });
            for (uint32_t x = 0; x < 64; x++) m[x] = sre_lrk_agree(m[x], with_bit, digit[x], bit);
        }
        for (uint32_t x = 0; x < 64; x++) {
            const uint32_t r = sre_lr_rank_in(m[x], x);
            if (sel[x] && r == 0) c[digit[x]] = sre_lr_popc(m[x]);
            rank[x] = sel[x] ? r : 0;
        }
    }
};

/* what every digit pass knows of the call (SortKeys of sre_hip_lines_sort.hip) */
struct SimKeys {
    int64_t  vmin, vmax;
    uint64_t range;
    int      desc, all;
};

uint64_t
load_key(const int64_t *value, const int8_t *cls, const uint64_t *src, uint64_t i, uint64_t n, const SimKeys &k)
{
    if (i >= n) return SRE_LSO_DROPPED;
    return value ? sre_lso_key(cls[i], value[i], k.vmin, k.vmax, k.range, k.desc, k.all) : src[i];
}

void
load_slot(SimSlot &s, const int64_t *value, const int8_t *cls, const uint64_t *src, uint64_t n, const SimKeys &k, uint32_t pass,
          uint64_t wg, uint32_t slot)
{
    for (uint32_t x = 0; x < 64; x++) {
        const uint64_t key = load_key(value, cls, src, sre_lr_line(wg, slot, x), n, k);
        s.sel[x] = key != SRE_LSO_DROPPED;
        s.digit[x] = sre_lso_digit(key, pass);
    }
}

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
    uint64_t               bad = 0;
    const SimVals          vals = {buf, len, vval, vstart, &bad};
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
                    const int32_t c = sre_lso_line(vals, i, &v);
                    value[i] = v, vw[i]++;
                    cls[i] = (int8_t) c, cw[i]++;
                    t = sre_lso_merge(t, sre_lso_single(c, v));
                }
            }
            part[wave] = t;
        }
        sre_lso_totals_t t = part[0];
        for (uint32_t wave = 1; wave < SRE_LSO_THREADS / 64u; wave++) t = sre_lso_merge(t, part[wave]);
        sre_lso_flush(mem, t);
    }
    return bad;
}

/* count of one pass: cnt[d * nwg + w]; writes[] counts the stores to every word of cnt.  value != NULL: pass 0 over the lines */
void
lsosim_count(const int64_t *value, const int8_t *cls, const uint64_t *src, uint64_t n, int64_t vmin, int64_t vmax, uint64_t nnum,
             int desc, int all, uint32_t pass, uint64_t *cnt, uint32_t *writes)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    const uint32_t nd = 1u << SRE_LSO_DIGIT_BITS;
    const SimKeys  k = sim_keys(vmin, vmax, nnum, desc, all);
    SimSlot        s;
    for (uint64_t w = 0; w < nwg; w++) {
        std::vector<uint32_t> c(SRE_LR_SLOTS * nd, 0);
        for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
            for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
                const uint32_t slot = sre_lr_slot(v, q);
                load_slot(s, value, cls, src, n, k, pass, w, slot);
                s.run(c.data() + slot * nd);
            }
        }
        for (uint32_t d = 0; d < nd; d++) {
            const uint64_t at = sre_lr_cnt_index(d, nwg, w);
            cnt[at] = sre_lr_slot_prefix(c.data() + d, nd);
            writes[at]++;
        }
    }
}

/* the scan as the filter's scan leaves it: exclusive, the total behind the last word */
void
lsosim_scan(uint64_t *v, uint64_t n)
{
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t x = v[i];
        v[i] = run;
        run += x;
    }
    v[n] = run;
}

/* scatter of one pass over the scanned counts; kw[r] / lw[r] count the stores to dkey[r] / dline[r].  Returns the stores that
 * fell outside [0, total) */
uint64_t
lsosim_scatter(const int64_t *value, const int8_t *cls, const uint64_t *src, const uint32_t *sline, uint64_t n, int64_t vmin,
               int64_t vmax, uint64_t nnum, int desc, int all, uint32_t pass, const uint64_t *first, uint64_t total, uint64_t *dkey,
               uint32_t *dline, uint32_t *kw, uint32_t *lw)
{
    const uint64_t nwg = (n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS;
    const uint32_t nd = 1u << SRE_LSO_DIGIT_BITS;
    const SimKeys  k = sim_keys(vmin, vmax, nnum, desc, all);
    uint64_t       bad = 0;
    for (uint64_t w = 0; w < nwg; w++) {
        std::vector<uint32_t> c(SRE_LR_SLOTS * nd, 0);
        std::vector<uint32_t> rk(SRE_LR_ITEMS, 0);
        std::vector<uint64_t> gbase(nd, 0);
        SimSlot               s;
        for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
            for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
                const uint32_t slot = sre_lr_slot(v, q);
                load_slot(s, value, cls, src, n, k, pass, w, slot);
                s.run(c.data() + slot * nd);
                for (uint32_t x = 0; x < 64; x++) rk[slot * 64 + x] = s.rank[x];
            }
        }
        for (uint32_t d = 0; d < nd; d++) {
            (void) sre_lr_slot_prefix(c.data() + d, nd);
            gbase[d] = first[sre_lr_cnt_index(d, nwg, w)];
        }
        for (uint32_t v = 0; v < SRE_LR_WAVES; v++) {
            for (uint32_t q = 0; q < SRE_LR_ROUNDS; q++) {
                const uint32_t slot = sre_lr_slot(v, q);
                for (uint32_t x = 0; x < 64; x++) {
                    const uint64_t i = sre_lr_line(w, slot, x);
                    const uint64_t key = load_key(value, cls, src, i, n, k);
                    if (key == SRE_LSO_DROPPED) continue;
                    const uint32_t d = sre_lso_digit(key, pass);
                    const uint64_t r = gbase[d] + c[slot * nd + d] + rk[slot * 64 + x];
                    if (r >= total) {
                        bad++;
                        continue;
                    }
                    dkey[r] = key, kw[r]++;
                    dline[r] = value ? (uint32_t) i : sline[i], lw[r]++;
                }
            }
        }
    }
    return bad;
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

void lsosim_result(const uint64_t *coff, uint64_t nout, uint64_t out_cap, uint64_t *res) { sre_lso_result(coff, nout, out_cap, res); }

void
lsosim_index_row(uint64_t line, const uint64_t *cstart, const uint64_t *coff, uint64_t r, int64_t value, int32_t cls, int64_t *row)
{
    sre_lso_index_row(line, cstart, coff, r, value, cls, row);
}

}
