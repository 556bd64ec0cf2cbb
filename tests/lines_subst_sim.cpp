/*
 * lines_subst_sim.cpp — the line substitute's gather on the CPU: every output chunk walked with the chunk logic the
 * kernel compiles (sregex_amd/csrc/sre_lines_gather.h) over the PIECE table (sre_lg_tab_pieces), tile by tile with
 * the kernel's table slices and its LDS window rule, over host copies of the three 16-byte aligned extents: the
 * source, the literal block and the output.  Every source and literal byte read and every output byte written is
 * counted, so tests/test_lines_subst_model.py can assert where the kernel may touch memory.  The cut at a line
 * boundary is the header's; the lines in front of it are counted as the kernels count them, by last entries.  The select
 * rule that fills the piece table from the lines' records (sregex_amd/csrc/sre_lines_select.h) is exported as the kernel
 * and the host route call it.
 */
#include "sre_lines_gather.h"
#include "sre_lines_select.h"
#include <stdint.h>
#include <string.h>
#include <vector>

namespace {

/* the aligned extents: src holds S-space bytes [0, src_len), lit the literal block [0, lit_len), dst P-space bytes
 * [0, dst_len), all multiples of 16 as the kernel sees them; an access outside them is counted and not made */
struct SimMem {
    const uint8_t *src;
    uint64_t       src_len;
    const uint8_t *lit;
    uint64_t       lit_len;
    uint8_t       *dst;
    uint64_t       dst_len;
    uint32_t      *reads;       /* per source byte */
    uint32_t      *lit_reads;   /* per byte of the literal block */
    uint32_t      *writes;      /* per output byte */
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

uint32_t lssim_window(void) { return SRE_LG_WINDOW; }
uint64_t lssim_flag_last(void) { return SRE_LG_ENTRY_LAST; }
uint64_t lssim_flag_unset(void) { return SRE_LG_ENTRY_UNSET; }
uint64_t lssim_flag_first(void) { return SRE_LG_ENTRY_FIRST; }
uint64_t lssim_flag_literal(void) { return SRE_LG_ENTRY_LITERAL; }

/* the cut: the first of n lines of p entries whose row ends beyond out_cap */
uint64_t lssim_cut(const uint64_t *off, uint64_t n, uint64_t p, uint64_t out_cap) { return sre_lg_row_cut(off, n, p, out_cap); }

/* the selected lines among the first `lines`: the last entries (e % p == p - 1) that take a byte, the predicate of
 * the substitute's sums, finish and index passes */
uint64_t
lssim_count(const uint64_t *off, uint64_t p, uint64_t lines)
{
    uint64_t k = 0;
    for (uint64_t j = 0; j < lines * p; j++) k += (j % p == p - 1 && off[j + 1] > off[j]) ? 1 : 0;
    return k;
}

/* the select rule over n lines: line i has the record recs[i * slots ..] and the extent [st[i], st[i] + len[i]); piece q of
 * the np of the template is group pg[q], or with pg[q] < 0 the plen[q] bytes at poff[q] of the literal block.  val /
 * start: n * (np + 2) words, entry i * (np + 2) + f as sre_k_subst_select writes it.  -1: more pieces than a template has */
int
lssim_select(const int64_t *recs, uint32_t slots, uint64_t n, int64_t declined, int all, const uint64_t *st, const uint64_t *len,
             const int32_t *pg, const uint32_t *poff, const uint32_t *plen, uint32_t np, uint64_t *val, uint64_t *start)
{
    sre_subst_pieces_t pc;
    if (np > SRE_SUBST_MAX_PIECES) return -1;
    memset(&pc, 0, sizeof(pc));
    pc.np = np;
    for (uint32_t q = 0; q < np; q++) {
        pc.g[q] = (int16_t) pg[q];
        pc.off[q] = (uint16_t) poff[q];
        pc.len[q] = (uint16_t) plen[q];
    }
    const uint32_t P = np + 2;
    for (uint64_t i = 0; i < n; i++) {
        for (uint32_t f = 0; f < P; f++) {
            sre_sel_subst_entry(recs + i * slots, declined, all, st[i], len[i], f, &pc, val + i * P + f, start + i * P + f);
        }
    }
    return 0;
}

/* the whole gather.  off[0 .. nent], starts[0 .. nent - 1] as the runtime holds them.  *windowed / *global = tiles
 * that took the LDS window / the global table.  Returns the accesses outside the extents. */
uint64_t
lssim_gather(const uint64_t *off, const uint64_t *starts, uint64_t nent, uint64_t out_bytes, uint32_t src_head, uint32_t dst_head,
             uint32_t delim, const uint8_t *src, uint64_t src_len, const uint8_t *lit, uint64_t lit_len, uint8_t *dst,
             uint64_t dst_len, uint32_t *reads, uint32_t *lit_reads, uint32_t *writes, uint64_t *windowed, uint64_t *global)
{
    sre_lg_geom_t g;
    g.nlines = nent;
    g.out_bytes = out_bytes;
    g.src_head = src_head;
    g.dst_head = dst_head;
    g.delim = delim;
    g.fsep = delim;
    SimMem                  mem = {src, src_len, lit, lit_len, dst, dst_len, reads, lit_reads, writes, 0};
    const sre_lg_tab_pieces tab = {off, starts, 0};
    const uint64_t          nchunks = sre_lg_nchunks(g);
    const uint64_t          ntiles = (nchunks + SRE_LG_TILE_CHUNKS - 1) / SRE_LG_TILE_CHUNKS;
    *windowed = *global = 0;
    for (uint64_t t = 0; t < ntiles; t++) {
        uint64_t la, lb;
        if (!sre_lg_tile_slice(tab, g, t, &la, &lb)) {
            mem.bad++;          /* the kernel launches no tile without bytes */
            continue;
        }
        const uint64_t cnt = lb - la + 1;
        std::vector<uint64_t> w_off, w_start;
        if (cnt <= SRE_LG_WINDOW) {
            for (uint64_t x = 0; x <= cnt; x++) w_off.push_back(off[la + x]);
            for (uint64_t x = 0; x < cnt; x++) w_start.push_back(tab.raw(la + x));
            ++*windowed;
        } else {
            ++*global;
        }
        const sre_lg_tab_pieces win = {w_off.data(), w_start.data(), la};
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
