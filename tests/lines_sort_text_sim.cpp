/*
 * lines_sort_text_sim.cpp — the line sort by text on the CPU: the values pass, the keys of a chunk, the pass that makes the
 * items and every later digit pass through the partition model (lines_partition_sim.h), with the rules the kernels compile
 * (sregex_amd/csrc/sre_lines_sort_text.h and what it builds on): the compared length, the chunk key, its descending form, the
 * rest's key and the plan.  The values pass, the later digit passes, the compact table and the result words are the numeric
 * sort's model (lines_sort_sim.cpp, compiled into this file).  Every store is counted, so tests/test_lines_sort_text_model.py
 * can assert that every word of every array is written exactly once per pass, and every byte of the buffer is read through a
 * check against its length.  tools/asan_sort_text_rule.cpp includes this file.
 */
#include "sre_lines_sort_text.h"
#include "lines_sort_sim.cpp"
#include <vector>

namespace {

/* a text in host memory, for the key rule alone */
struct SimText {
    const uint8_t *t;
    uint64_t       len;
    uint64_t      *bad;
    uint8_t byte(uint64_t at) const
    {
        if (at >= len) {
            (*bad)++;
            return 0;
        }
        return t[at];
    }
};

/* the pass that makes the items (TextFirstPass of sre_hip_lines_sort_text.hip) */
struct SimTextFirst {
    const uint64_t *src;
    uint64_t        n;
    uint32_t        pass;
    uint64_t       *dkey;
    uint32_t       *dline, *kw, *lw;
    uint32_t nd() const { return 1u << SRE_LSO_DIGIT_BITS; }
    uint32_t bits() const { return SRE_LSO_DIGIT_BITS; }
    int      rule() const { return SRE_LRK_RANK_BITS; }
    uint64_t load(uint64_t i) const { return i < n ? src[i] : SRE_LSO_DROPPED; }
    bool     taken(uint64_t key) const { return key != SRE_LSO_DROPPED; }
    uint32_t digit(uint64_t key) const { return sre_lso_digit(key, pass); }
    void     store(uint64_t r, uint64_t key, uint64_t i)
    {
        dkey[r] = key, kw[r]++;
        dline[r] = (uint32_t) i, lw[r]++;
    }
};

}  // namespace

extern "C" {

uint64_t lstsim_kmax(void) { return SRE_LST_KMAX; }
uint64_t lstsim_rest(void) { return SRE_LST_REST; }
uint32_t lstsim_chunk(void) { return SRE_LST_CHUNK; }
uint64_t lstsim_cut(uint64_t len, uint64_t max_bytes) { return sre_lst_cut(len, max_bytes); }
uint64_t lstsim_dir(uint64_t key, int desc) { return sre_lst_dir(key, desc); }
uint64_t lstsim_rest_key(uint64_t c, int desc) { return sre_lst_rest_key(c, desc); }

/* the ascending key of chunk c of the first L bytes of t (len bytes); *bad counts the bytes read outside [0, len) */
uint64_t
lstsim_chunk_key(const uint8_t *t, uint64_t len, uint64_t L, uint64_t c, uint64_t *bad)
{
    const SimText text = {t, len, bad};
    return sre_lst_chunk_key(text, 0, L, c);
}

/* pairs[2 i], pairs[2 i + 1] = chunk, digit of pass i < min(cap, length); returns the length */
uint64_t
lstsim_plan(uint64_t minlen, uint64_t maxlen, int rest, uint64_t *pairs, uint64_t cap)
{
    const uint64_t              len = sre_lst_plan(minlen, maxlen, rest, NULL, 0), take = len < cap ? len : cap;
    std::vector<sre_lst_pass_t> plan(take);
    (void) sre_lst_plan(minlen, maxlen, rest, plan.data(), take);
    for (uint64_t i = 0; i < take; i++) pairs[2 * i] = plan[i].chunk, pairs[2 * i + 1] = plan[i].digit;
    return len;
}

/* the values pass over the value table of n lines: value[i] the compared length, cls[i] (vw[i], cw[i] count the stores),
 * totals[4] with the identities first, sent[4] the atomics each word received */
uint64_t
lstsim_values(const uint8_t *buf, uint64_t len, const uint64_t *vval, const uint64_t *vstart, uint64_t n, uint64_t max_bytes,
              int64_t *value, int8_t *cls, uint32_t *vw, uint32_t *cw, uint64_t *totals, uint32_t *sent)
{
    uint64_t      bad = 0;
    const SimVals vals = {buf, len, vval, vstart, &bad};
    sim_values(n, value, cls, totals, sent, [&](uint64_t i, int64_t *v) {
        vw[i]++, cw[i]++;
        return sre_lst_line(vals, i, max_bytes, v);
    });
    return bad;
}

/* the keys of chunk `chunk` (sre_k_sort_text_keys): lines == NULL: of the nitems == n lines; otherwise of the items' lines.
 * kw[i] counts the stores to keys[i].  Returns the source bytes read outside [0, len) plus the lines outside [0, n) */
uint64_t
lstsim_keys(const uint8_t *buf, uint64_t len, const uint64_t *vval, const uint64_t *vstart, uint64_t n, uint64_t max_bytes,
            const uint32_t *lines, uint64_t nitems, uint64_t chunk, int desc, int all, uint64_t *keys, uint32_t *kw)
{
    uint64_t      bad = 0;
    const SimVals vals = {buf, len, vval, vstart, &bad};
    for (uint64_t i = 0; i < nitems; i++) {
        const uint64_t line = lines ? lines[i] : i;
        if (line >= n) {
            bad++;
            continue;
        }
        keys[i] = sre_lst_line_key(vals, line, chunk, max_bytes, desc, all);
        kw[i]++;
    }
    return bad;
}

/* count of the pass that makes the items, over the keys of the n lines */
void
lstsim_first_count(const uint64_t *lkeys, uint64_t n, uint32_t pass, uint64_t *cnt, uint32_t *writes)
{
    const SimTextFirst p = {lkeys, n, pass, NULL, NULL, NULL, NULL};
    (void) sim_count(p, n, cnt, writes);
}

/* its scatter over the scanned counts.  Returns the stores that fell outside [0, total) */
uint64_t
lstsim_first_scatter(const uint64_t *lkeys, uint64_t n, uint32_t pass, const uint64_t *first, uint64_t total, uint64_t *dkey,
                     uint32_t *dline, uint32_t *kw, uint32_t *lw)
{
    SimTextFirst p = {lkeys, n, pass, dkey, dline, kw, lw};
    return sim_scatter(p, n, first, total);
}

/* the index row of rank r */
uint64_t
lstsim_index_row(const uint8_t *buf, uint64_t len, const uint64_t *vval, const uint64_t *vstart, uint64_t line, const uint64_t *cstart,
                 const uint64_t *coff, uint64_t r, int64_t *row)
{
    uint64_t      bad = 0;
    const SimVals vals = {buf, len, vval, vstart, &bad};
    sre_lst_index_row(vals, line, cstart, coff, r, row);
    return bad;
}

/* The whole sort as the host drives it behind its one read (sort_text_passes of sre_hip_batch.cpp), every array a heap block
 * of exactly the call's size: the values pass, the plan, per chunk the keys and the digit passes.  out_lines[0 .. nsel) the
 * lines of the sorted items; info[0 .. 5) = nkeyed, nsel, minlen, maxlen, the plan's length.  Returns what went wrong: bytes
 * read outside the buffer, stores outside an array, words written not exactly once in a pass, totals that disagree */
uint64_t
lstsim_sort(const uint8_t *buf, uint64_t len, const uint64_t *vval, const uint64_t *vstart, uint64_t n, uint64_t max_bytes, int desc,
            int all, uint32_t *out_lines, uint64_t *info)
{
    uint64_t              bad = 0;
    std::vector<int64_t>  value(n);
    std::vector<int8_t>   cls(n);
    std::vector<uint32_t> vw(n, 0), cw(n, 0);
    uint64_t              totals[4];
    uint32_t              sent[4] = {0, 0, 0, 0};
    bad += lstsim_values(buf, len, vval, vstart, n, max_bytes, value.data(), cls.data(), vw.data(), cw.data(), totals, sent);
    for (uint64_t i = 0; i < n; i++) bad += vw[i] != 1 || cw[i] != 1;
    const uint64_t nkeyed = totals[0];
    bad += totals[1] != nkeyed;
    const uint64_t minlen = nkeyed ? totals[2] : ~(uint64_t) 0, maxlen = nkeyed ? totals[3] : 0;
    const uint64_t nsel = sre_lst_selected(n, nkeyed, all);
    const int      rest = all && nkeyed < n;
    std::vector<sre_lst_pass_t> plan(sre_lst_plan(minlen, maxlen, rest, NULL, 0));
    (void) sre_lst_plan(minlen, maxlen, rest, plan.data(), plan.size());
    info[0] = nkeyed, info[1] = nsel, info[2] = minlen, info[3] = maxlen, info[4] = plan.size();
    if (nsel == 0) return bad;
    std::vector<sre_lst_pass_t> run = plan;
    if (run.empty()) run.push_back(sre_lst_pass_t{0, 0});
    std::vector<uint64_t> key[2];
    std::vector<uint32_t> line[2];
    int                   cur = -1;
    for (size_t at = 0; at < run.size();) {
        const uint64_t chunk = run[at].chunk;
        size_t         to = at;
        while (to < run.size() && run[to].chunk == chunk) to++;
        if (cur < 0) {
            /* the keys of the lines, where the compared lengths were; the first digit makes the items */
            std::vector<uint64_t> lkeys(n);
            std::vector<uint32_t> kw(n, 0);
            bad += lstsim_keys(buf, len, vval, vstart, n, max_bytes, NULL, n, chunk, desc, all, lkeys.data(), kw.data());
            for (uint64_t i = 0; i < n; i++) bad += kw[i] != 1;
            const uint64_t        ncnt = 256 * ((n + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS);
            std::vector<uint64_t> cnt(ncnt + 1);
            std::vector<uint32_t> cntw(ncnt + 1, 0);
            lstsim_first_count(lkeys.data(), n, run[at].digit, cnt.data(), cntw.data());
            for (uint64_t x = 0; x < ncnt; x++) bad += cntw[x] != 1;
            sim_scan(cnt.data(), ncnt);
            bad += cnt[ncnt] != nsel;
            key[0].assign(nsel, 0), line[0].assign(nsel, 0);
            std::vector<uint32_t> skw(nsel, 0), slw(nsel, 0);
            bad += lstsim_first_scatter(lkeys.data(), n, run[at].digit, cnt.data(), nsel, key[0].data(), line[0].data(), skw.data(),
                                        slw.data());
            for (uint64_t r = 0; r < nsel; r++) bad += skw[r] != 1 || slw[r] != 1;
            cur = 0;
            at++;
        } else {
            std::vector<uint32_t> kw(nsel, 0);
            bad += lstsim_keys(buf, len, vval, vstart, n, max_bytes, line[cur].data(), nsel, chunk, desc, all, key[cur].data(), kw.data());
            for (uint64_t r = 0; r < nsel; r++) bad += kw[r] != 1;
        }
        for (; at < to; at++, cur ^= 1) {
            const uint64_t        ncnt = 256 * ((nsel + SRE_LR_ITEMS - 1) / SRE_LR_ITEMS);
            std::vector<uint64_t> cnt(ncnt + 1);
            std::vector<uint32_t> cntw(ncnt + 1, 0), skw(nsel, 0), slw(nsel, 0);
            lsosim_count(NULL, NULL, key[cur].data(), nsel, 0, 0, 0, desc, all, run[at].digit, cnt.data(), cntw.data());
            for (uint64_t x = 0; x < ncnt; x++) bad += cntw[x] != 1;
            sim_scan(cnt.data(), ncnt);
            bad += cnt[ncnt] != nsel;
            key[cur ^ 1].assign(nsel, 0), line[cur ^ 1].assign(nsel, 0);
            bad += lsosim_scatter(NULL, NULL, key[cur].data(), line[cur].data(), nsel, 0, 0, 0, desc, all, run[at].digit, cnt.data(), nsel,
                                  key[cur ^ 1].data(), line[cur ^ 1].data(), skw.data(), slw.data());
            for (uint64_t r = 0; r < nsel; r++) bad += skw[r] != 1 || slw[r] != 1;
        }
    }
    for (uint64_t r = 0; r < nsel; r++) out_lines[r] = line[cur][r];
    return bad;
}

}
