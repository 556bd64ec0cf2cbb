/*
 * lines_join_sim.cpp — the key map and the line join on the CPU, from the text the kernels compile
 * (sregex_amd/csrc/sre_lines_join.h, sre_lines_keyset.h and the join table of sre_lines_gather.h): the split of a map's
 * rows into key fields and value columns, the join pass line by line as sre_k_keyset_join makes it (the probe of the
 * finished table, the key id, the entries of the line), and the gather over the join table, tile by tile with the
 * kernel's table slices and its LDS window rule, over host copies of the three extents: the source and the output,
 * multiples of 16 bytes, and the map's copy of the dictionary, its text and 16 bytes.  Every byte read and written is
 * counted; an access outside an extent is counted and not made.
 */
#include "sre_lines_join.h"
#include "sre_lines_gather.h"
#include "sre_lines_select.h"     /* SRE_EXTRACT_MAX_FIELDS */
#include <stdint.h>
#include <string.h>
#include <vector>

namespace {

struct SimBytes {
    const uint8_t *p;
    uint8_t byte(uint64_t at) const { return p[at]; }
};

struct InsertMem {
    uint64_t *tab;
    uint64_t  nslots, bad;
    uint64_t cas(uint64_t idx, uint64_t expect, uint64_t v)
    {
        if (idx >= nslots) {
            bad++;
            return 0;
        }
        const uint64_t old = tab[idx];
        if (old == expect) tab[idx] = v;
        return old;
    }
    void min(uint64_t idx, uint64_t v)
    {
        if (idx >= nslots) bad++;
        else if (v < tab[idx]) tab[idx] = v;
    }
    bool raised() { return false; }
};

struct ProbeMem {
    const uint64_t  *tab;
    uint64_t         nslots;
    mutable uint64_t bad;
    uint64_t load(uint64_t idx) const
    {
        if (idx >= nslots) {
            bad++;
            return SRE_LT_EMPTY;
        }
        return tab[idx];
    }
};

sre_lt_params_t
params(uint64_t nslots, int hash_bits)
{
    sre_lt_params_t p;
    p.nslots = nslots;
    p.max_keys = nslots / 2;
    p.hash_mask = sre_lt_hash_mask(hash_bits);
    return p;
}

/* the extents of the gather: src S-space bytes [0, src_len) and dst P-space bytes [0, dst_len), multiples of 16; lit the
 * dictionary's copy, lit_len = its text + 16 */
struct SimMem {
    const uint8_t *src;
    uint64_t       src_len;
    const uint8_t *lit;
    uint64_t       lit_len;
    uint8_t       *dst;
    uint64_t       dst_len;
    uint32_t      *reads, *lit_reads, *writes;
    uint64_t       bad;

    sre_lg_u128 get(const uint8_t *base, uint64_t len, uint32_t *count, uint64_t s, bool aligned)
    {
        uint8_t b[16];
        memset(b, 0, sizeof(b));
        if ((aligned && (s & 15u)) || s + 16 > len || s + 16 < s) {
            bad++;
        } else {
            memcpy(b, base + s, 16);
            for (int k = 0; k < 16; k++) count[s + k]++;
        }
        sre_lg_u128 v;
        memcpy(&v.lo, b, 8);
        memcpy(&v.hi, b + 8, 8);
        return v;
    }
    sre_lg_u128 load(uint64_t q) { return get(src, src_len, reads, q * 16, true); }
    sre_lg_u128 loadu(uint64_t s) { return get(src, src_len, reads, s, false); }
    sre_lg_u128 lit_load(uint64_t q) { return get(lit, lit_len, lit_reads, q * 16, true); }
    sre_lg_u128 lit_loadu(uint64_t s) { return get(lit, lit_len, lit_reads, s, false); }
    void store_bytes(uint64_t c, sre_lg_u128 v, uint32_t first, uint32_t count)
    {
        uint8_t b[16];
        memcpy(b, &v.lo, 8);
        memcpy(b + 8, &v.hi, 8);
        for (uint32_t k = first; k < first + count; k++) {
            const uint64_t p = c * 16 + k;
            if (k >= 16 || p >= dst_len) {
                bad++;
                continue;
            }
            dst[p] = b[k];
            writes[p]++;
        }
    }
    void store(uint64_t c, sre_lg_u128 v) { store_bytes(c, v, 0, 16); }
};

}  // namespace

extern "C" {

uint32_t ljsim_window(void) { return SRE_LG_WINDOW; }
uint32_t ljsim_max_values(void) { return SRE_LJ_MAX_VALUES; }
uint64_t ljsim_flag_last(void) { return SRE_LG_ENTRY_LAST; }
uint64_t ljsim_flag_unset(void) { return SRE_LG_ENTRY_UNSET; }
uint64_t ljsim_flag_first(void) { return SRE_LG_ENTRY_FIRST; }
uint64_t ljsim_flag_literal(void) { return SRE_LG_ENTRY_LITERAL; }
uint64_t ljsim_nslots(uint64_t rows) { return sre_lk_nslots(rows); }

/* the map's fields over row ends the caller made, as sre_k_keymap_fields: key fields into fstart / flen (rows * k), value
 * columns into vstart / vlen (rows * (nf - k)); returns the lowest row that breaks the field rule, SRE_LK_NO_ROW without */
uint64_t
ljsim_fields(const uint8_t *buf, const uint64_t *ends, uint64_t rows, uint32_t nf, uint32_t k, uint32_t fsep, uint64_t *fstart,
             uint64_t *flen, uint64_t *vstart, uint64_t *vlen)
{
    const SimBytes b = {buf};
    uint64_t       bad = SRE_LK_NO_ROW;
    for (uint64_t r = rows; r-- > 0;) {
        uint64_t st, end, s[SRE_EXTRACT_MAX_FIELDS], l[SRE_EXTRACT_MAX_FIELDS];
        sre_lk_row_span(ends, r, &st, &end);
        if (!sre_lk_row_fields(b, st, end, nf, fsep, s, l)) {
            if (r < bad) bad = r;
            continue;
        }
        sre_lj_part(s, l, nf, k, fstart + r * k, flen + r * k, vstart + r * (nf - k), vlen + r * (nf - k));
    }
    return bad;
}

/* the table of the rows' keys, from the HIGHEST row down (the lowest row of a key must end in its slot whatever the order);
 * tab: nslots words, SRE_LT_EMPTY before.  Returns the accesses outside the table */
uint64_t
ljsim_insert(const uint8_t *buf, const uint64_t *fstart, const uint64_t *flen, uint64_t rows, uint32_t k, uint64_t nslots,
             int hash_bits, uint64_t *tab)
{
    const sre_lk_dict_keys keys = {buf, fstart, flen, k};
    const sre_lt_params_t  p = params(nslots, hash_bits);
    InsertMem              mem = {tab, nslots, 0};
    for (uint64_t r = rows; r-- > 0;) {
        sre_lt_lane_t L;
        sre_lt_begin(L, r, true, sre_lt_hash(keys, r), p);
        while (!sre_lt_done(L)) sre_lt_step(L, keys, mem, p);
    }
    return mem.bad;
}

/* the join pass over n lines as sre_k_keyset_join makes it: own[i], keyid[i] for i < keyid_n, and the P = 1 + ncols
 * entries of every line in val / start (n * P words).  words[0 .. 3): keyed lines, members, reads outside the table */
void
ljsim_join(const uint8_t *src, const uint64_t *vval, const uint64_t *vstart, const uint64_t *ends, uint64_t n, uint32_t k,
           const uint8_t *dict, const uint64_t *fstart, const uint64_t *flen, const uint64_t *mstart, const uint64_t *mlen,
           uint32_t nvalues, const uint64_t *tab, uint64_t nslots, int hash_bits, const uint32_t *cols, uint32_t ncols, int all,
           uint64_t *val, uint64_t *start, int64_t *own, int64_t *keyid, uint64_t keyid_n, uint64_t *words)
{
    const sre_lk_line_keys lines = {src, vval, vstart, k};
    const sre_lk_dict_keys rows = {dict, fstart, flen, k};
    const sre_lt_params_t  p = params(nslots, hash_bits);
    const ProbeMem         mem = {tab, nslots, 0};
    sre_lj_cols_t          c;
    const uint32_t         P = 1 + ncols;
    memset(&c, 0, sizeof(c));
    c.n = ncols;
    for (uint32_t x = 0; x < ncols; x++) c.col[x] = (uint8_t) cols[x];
    words[0] = words[1] = 0;
    for (uint64_t i = 0; i < n; i++) {
        const bool     keyed = lines.selected(i);
        sre_lk_probe_t R;
        R.id = SRE_LK_NOT_MEMBER;
        if (keyed) {
            sre_lk_probe_begin(R, sre_lt_hash(lines, i), p);
            while (!R.done) sre_lk_probe_step(R, i, lines, rows, mem, p);
        }
        const int64_t  id = sre_lk_keyid(keyed, R.id);
        const uint64_t st = i ? ends[i - 1] + 1 : 0;
        own[i] = id;
        if (i < keyid_n) keyid[i] = id;
        sre_lj_entries(keyed, R.id, all != 0, st, ends[i] - st, mstart, mlen, nvalues, c, val + i * P, start + i * P);
        words[0] += keyed;
        words[1] += keyed && R.id >= 0;
    }
    words[2] = mem.bad;
}

/* the cut: the first of n lines of p entries whose row ends beyond out_cap */
uint64_t ljsim_cut(const uint64_t *off, uint64_t n, uint64_t p, uint64_t out_cap) { return sre_lg_row_cut(off, n, p, out_cap); }

/* the whole gather.  off[0 .. nent], starts[0 .. nent - 1] as the runtime holds them.  *windowed / *global = tiles that
 * took the LDS window / the global table.  Returns the accesses outside the extents. */
uint64_t
ljsim_gather(const uint64_t *off, const uint64_t *starts, uint64_t nent, uint64_t out_bytes, uint32_t src_head, uint32_t dst_head,
             uint32_t delim, uint32_t jsep, const uint8_t *src, uint64_t src_len, const uint8_t *lit, uint64_t lit_len,
             uint8_t *dst, uint64_t dst_len, uint32_t *reads, uint32_t *lit_reads, uint32_t *writes, uint64_t *windowed,
             uint64_t *global)
{
    sre_lg_geom_t g;
    g.nlines = nent;
    g.out_bytes = out_bytes;
    g.src_head = src_head;
    g.dst_head = dst_head;
    g.delim = delim;
    g.fsep = jsep;
    SimMem                mem = {src, src_len, lit, lit_len, dst, dst_len, reads, lit_reads, writes, 0};
    const sre_lg_tab_join tab = {off, starts, 0};
    const uint64_t        nchunks = sre_lg_nchunks(g);
    const uint64_t        ntiles = (nchunks + SRE_LG_TILE_CHUNKS - 1) / SRE_LG_TILE_CHUNKS;
    *windowed = *global = 0;
    for (uint64_t t = 0; t < ntiles; t++) {
        uint64_t la, lb;
        if (!sre_lg_tile_slice(tab, g, t, &la, &lb)) {
            mem.bad++;          /* the kernel launches no tile without bytes */
            continue;
        }
        const uint64_t        cnt = lb - la + 1;
        std::vector<uint64_t> w_off, w_start;
        if (cnt <= SRE_LG_WINDOW) {
            for (uint64_t x = 0; x <= cnt; x++) w_off.push_back(off[la + x]);
            for (uint64_t x = 0; x < cnt; x++) w_start.push_back(tab.raw(la + x));
            ++*windowed;
        } else {
            ++*global;
        }
        const sre_lg_tab_join win = {w_off.data(), w_start.data(), la};
        /* in the order of the kernel's lanes and steps */
        for (uint32_t k = 0; k < SRE_LG_CHUNKS; k++) {
            for (uint32_t x = 0; x < SRE_LG_THREADS; x++) {
                const uint64_t c = t * SRE_LG_TILE_CHUNKS + (uint64_t) k * SRE_LG_THREADS + x;
                if (c >= nchunks) continue;
                if (cnt <= SRE_LG_WINDOW) sre_lg_chunk(win, g, c, la, lb, mem);
                else sre_lg_chunk(tab, g, c, la, lb, mem);
            }
        }
    }
    return mem.bad;
}

}
