/*
 * lines_extract_sim.cpp — the line extract's gather on the CPU: every output chunk walked with the chunk logic the
 * kernel compiles (sregex_amd/csrc/sre_lines_gather.h) over the ENTRY table (sre_lg_tab_fields), tile by tile with
 * the kernel's table slices and its LDS window rule, over host copies of the two 16-byte aligned extents.  Every
 * source byte read and every output byte written is counted, so tests/test_lines_extract_model.py can assert where
 * the kernel may touch memory.  The cut at a line boundary is the header's too.  The select rule that fills the entry
 * table from the lines' records (sregex_amd/csrc/sre_lines_select.h) is exported as the kernel and the host route call it.
 */
#include "sre_lines_gather.h"
#include "sre_lines_select.h"
#include <stdint.h>
#include <string.h>
#include <vector>

namespace {

/* the aligned extents: src holds S-space bytes [0, src_len), dst P-space bytes [0, dst_len), both multiples of
 * 16 as the kernel sees them; an access outside them is counted and not made */
struct SimMem {
    const uint8_t *src;
    uint64_t       src_len;
    uint8_t       *dst;
    uint64_t       dst_len;
    uint32_t      *reads;       /* per source byte */
    uint32_t      *writes;      /* per output byte */
    uint64_t       bad;

    sre_lg_u128 get(uint64_t s, bool aligned)
    {
        uint8_t b[16];
        memset(b, 0, sizeof(b));
        if ((aligned && (s & 15u)) || s + 16 > src_len || s + 16 < s) {
            bad++;
        } else {
            memcpy(b, src + s, 16);
            for (int k = 0; k < 16; k++) reads[s + k]++;
        }
        sre_lg_u128 v;
        memcpy(&v.lo, b, 8);
        memcpy(&v.hi, b + 8, 8);
        return v;
    }
    sre_lg_u128 load(uint64_t q) { return get(q * 16, true); }
    sre_lg_u128 loadu(uint64_t s) { return get(s, false); }
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

uint32_t lesim_window(void) { return SRE_LG_WINDOW; }
uint64_t lesim_flag_last(void) { return SRE_LG_ENTRY_LAST; }
uint64_t lesim_flag_unset(void) { return SRE_LG_ENTRY_UNSET; }
uint64_t lesim_flag_first(void) { return SRE_LG_ENTRY_FIRST; }

/* the cut: the first of n lines of k fields whose row ends beyond out_cap */
uint64_t lesim_cut(const uint64_t *off, uint64_t n, uint64_t k, uint64_t out_cap) { return sre_lg_row_cut(off, n, k, out_cap); }

/* the select rule over n lines: line i has the record recs[i * slots ..] and the extent [st[i], st[i] + len[i]); field f of
 * the k of a row is group groups[f].  val / start: n * k words, entry i * k + f as sre_k_extract_select writes it */
void
lesim_select(const int64_t *recs, uint32_t slots, uint64_t n, int64_t declined, int all, const uint64_t *st, const uint64_t *len,
             const uint32_t *groups, uint32_t k, uint64_t *val, uint64_t *start)
{
    for (uint64_t i = 0; i < n; i++) {
        for (uint32_t f = 0; f < k; f++) {
            sre_sel_extract_entry(recs + i * slots, declined, all, st[i], len[i], f, k, groups[f], val + i * k + f, start + i * k + f);
        }
    }
}

/* the whole gather.  off[0 .. nent], starts[0 .. nent - 1] as the runtime holds them.  *windowed / *global = tiles
 * that took the LDS window / the global table.  Returns the accesses outside the extents. */
uint64_t
lesim_gather(const uint64_t *off, const uint64_t *starts, uint64_t nent, uint64_t out_bytes, uint32_t src_head, uint32_t dst_head,
             uint32_t delim, uint32_t fsep, const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_len, uint32_t *reads,
             uint32_t *writes, uint64_t *windowed, uint64_t *global)
{
    sre_lg_geom_t g;
    g.nlines = nent;
    g.out_bytes = out_bytes;
    g.src_head = src_head;
    g.dst_head = dst_head;
    g.delim = delim;
    g.fsep = fsep;
    SimMem                  mem = {src, src_len, dst, dst_len, reads, writes, 0};
    const sre_lg_tab_fields tab = {off, starts, 0};
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
        const sre_lg_tab_fields win = {w_off.data(), w_start.data(), la};
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
