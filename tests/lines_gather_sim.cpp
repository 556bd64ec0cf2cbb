/*
 * lines_gather_sim.cpp — the line filter's gather on the CPU: every output chunk walked with the chunk logic the
 * kernel compiles (sregex_amd/csrc/sre_lines_gather.h), tile by tile with the kernel's table slices and its LDS
 * window rule, over host copies of the two 16-byte aligned extents.  Every source byte read and every output
 * byte written is counted, so tests/test_lines_gather_model.py can assert where the kernel may touch memory.
 */
#include "sre_lines_gather.h"
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

/* the plan of one chunk as rows [kind (0 text, 1 delimiter), S, d, cnt] */
struct PlanSink {
    uint64_t *rows;
    uint32_t  cap, n;
    void text(uint64_t s, uint32_t d, uint32_t cnt) { put(0, s, d, cnt); }
    void delim(uint32_t d) { put(1, 0, d, 1); }
    void put(uint64_t kind, uint64_t s, uint64_t d, uint64_t cnt)
    {
        if (n < cap) {
            rows[4 * n] = kind;
            rows[4 * n + 1] = s;
            rows[4 * n + 2] = d;
            rows[4 * n + 3] = cnt;
        }
        n++;
    }
};

}  // namespace

extern "C" {

uint32_t lgsim_tile_chunks(void) { return SRE_LG_TILE_CHUNKS; }
uint32_t lgsim_window(void) { return SRE_LG_WINDOW; }

/* the whole gather.  off[0 .. n], ends[0 .. n - 1] as the runtime holds them.  *windowed / *global = tiles that
 * took the LDS window / the global table.  Returns the accesses outside the extents. */
uint64_t
lgsim_gather(const uint64_t *off, const uint64_t *ends, uint64_t n, uint64_t out_bytes, uint32_t src_head, uint32_t dst_head,
             uint32_t delim, const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_len, uint32_t *reads,
             uint32_t *writes, uint64_t *windowed, uint64_t *global)
{
    sre_lg_geom_t g;
    g.nlines = n;
    g.out_bytes = out_bytes;
    g.src_head = src_head;
    g.dst_head = dst_head;
    g.delim = delim;
    SimMem                  mem = {src, src_len, dst, dst_len, reads, writes, 0};
    const sre_lg_tab_global tab = {off, ends};
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
            for (uint64_t x = 0; x < cnt; x++) w_start.push_back(tab.start(la + x));
            ++*windowed;
        } else {
            ++*global;
        }
        const sre_lg_tab_window win = {w_off.data(), w_start.data(), la};
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

/* the plan of chunk c alone, no data touched: rows of 4 words, at most cap of them; returns their number, and
 * the chunk's owned bytes in first_count[0 .. 1] and its tile's slice in first_count[2 .. 3] */
uint32_t
lgsim_plan(const uint64_t *off, const uint64_t *ends, uint64_t n, uint64_t out_bytes, uint32_t src_head, uint32_t dst_head,
           uint64_t c, uint64_t *rows, uint32_t cap, uint64_t *first_count)
{
    sre_lg_geom_t g;
    g.nlines = n;
    g.out_bytes = out_bytes;
    g.src_head = src_head;
    g.dst_head = dst_head;
    g.delim = 0;
    const sre_lg_tab_global tab = {off, ends};
    PlanSink                sink = {rows, cap, 0};
    uint64_t                la = 0, lb = 0;
    uint32_t                first = 0, count = 0;
    if (!sre_lg_tile_slice(tab, g, c / SRE_LG_TILE_CHUNKS, &la, &lb)) return 0;
    if (!sre_lg_walk(tab, g, c, la, lb, sink, &first, &count)) return 0;
    first_count[0] = first;
    first_count[1] = count;
    first_count[2] = la;
    first_count[3] = lb;
    return sink.n;
}

}
