/*
 * sre_lines_gather.h — the chunk logic of the line filter's gather (sre_hip_filter_lines):
 * which lines cover a 16-byte chunk of the output, which source bytes go where in it and where the
 * delimiters fall.  The gather kernel (sre_hip_lines_gather.hip) and the CPU model (tests/lines_gather_sim.cpp)
 * compile this text; nothing here touches memory except through the Tab and Mem arguments.
 *
 * The table is the OFFSET TABLE of the call: off[i], i = 0 .. nlines, the exclusive prefix sum of the per-line
 * values (len + 1 for a selected line, 0 for the others), so off[nlines] = need_bytes.  It is monotone, a line
 * is selected iff off[i + 1] > off[i], and the line that holds output byte o is the LAST i with off[i] <= o.
 * A line's text starts at start(i) in the source; its delimiter is output byte off[i + 1] - 1.
 *
 * Two position spaces, both counted from a 16-byte aligned address so that chunk q is bytes [16q, 16q + 16):
 *   P = dst_head + output offset   (dst_head = d_out % 16),  output chunk c covers P in [16c, 16c + 16)
 *   S = src_head + source offset   (src_head = d_buf % 16),  source block q covers S in [16q, 16q + 16)
 * All offsets are 64-bit.
 *
 * Line extract (sre_hip_extract_lines) gathers with the same logic over a table of ENTRIES
 * e = line * K + f, field f of the K chosen capture groups of a line: off[] is the prefix sum of (field length + 1)
 * of the selected lines' entries, the text of an entry starts at its word of the call's starts array, and the
 * byte behind it is the field separator, or the delimiter behind the last field of a line (sre_lg_tab_fields).
 *
 * Line substitute (sre_hip_substitute_lines) gathers over a table of PIECES e = line * P + f: the
 * line's text in front of its first match, the pieces of the template, the text behind the match.  The pieces of a
 * row abut: only the last entry of a line has a byte behind it (the delimiter), the text of every other entry runs to
 * off[e + 1]; an entry may take no byte at all and is then never visited.  The text of a literal piece comes from the
 * call's LITERAL BLOCK, a second 16-byte aligned extent (sre_lg_tab_pieces).
 *
 * Line join (sre_hip_join_lines) gathers over a table of entries e = line * P + f: the line's text,
 * then P - 1 values of the line's dictionary row.  Every entry has a byte behind it as the extract's fields have (the
 * join separator, or the delimiter behind the last), and the text of a value comes from the key map's copy of its
 * dictionary, the second extent in the literal block's place (sre_lg_tab_join).
 */
#ifndef SRE_LINES_GATHER_H
#define SRE_LINES_GATHER_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRE_LG_FN __host__ __device__ static inline
#define SRE_LG_MEMBER __host__ __device__ inline
#else
#define SRE_LG_FN static inline
#define SRE_LG_MEMBER inline
#endif

/* a workgroup of SRE_LG_THREADS lanes owns one tile of SRE_LG_TILE_CHUNKS output chunks; lane x, step k takes
 * chunk k * SRE_LG_THREADS + x of the tile.  A tile whose slice of the table has at most SRE_LG_WINDOW lines
 * keeps the slice in LDS; a longer slice (many empty or unselected lines) is searched in the global table */
#define SRE_LG_THREADS      256u
#define SRE_LG_CHUNKS       4u
#define SRE_LG_TILE_CHUNKS  (SRE_LG_THREADS * SRE_LG_CHUNKS)       /* 16 KiB of output */
#define SRE_LG_WINDOW       1024u

typedef struct {
    uint64_t lo, hi;            /* bytes 0..7 and 8..15 of a chunk, little endian */
} sre_lg_u128;

typedef struct sre_lg_geom_t {
    uint64_t nlines;
    uint64_t out_bytes;         /* bytes the call writes: whole lines only */
    uint32_t src_head;          /* d_buf % 16 */
    uint32_t dst_head;          /* d_out % 16 */
    uint32_t delim;
    uint32_t fsep = 0;          /* line extract only: the byte behind a field that is not the last of its line */
} sre_lg_geom_t;

/* v moved down / up by k bytes (k >= 16 gives 0), and the mask of the first n bytes */
SRE_LG_FN sre_lg_u128
sre_lg_shr(sre_lg_u128 v, uint32_t k)
{
    if (k >= 16) { v.lo = 0; v.hi = 0; return v; }
    if (k >= 8) { v.lo = v.hi; v.hi = 0; k -= 8; }
    if (k) {
        v.lo = (v.lo >> (8 * k)) | (v.hi << (64 - 8 * k));
        v.hi >>= 8 * k;
    }
    return v;
}

SRE_LG_FN sre_lg_u128
sre_lg_shl(sre_lg_u128 v, uint32_t k)
{
    if (k >= 16) { v.lo = 0; v.hi = 0; return v; }
    if (k >= 8) { v.hi = v.lo; v.lo = 0; k -= 8; }
    if (k) {
        v.hi = (v.hi << (8 * k)) | (v.lo >> (64 - 8 * k));
        v.lo <<= 8 * k;
    }
    return v;
}

SRE_LG_FN sre_lg_u128
sre_lg_mask(uint32_t n)
{
    sre_lg_u128 m;
    m.lo = n >= 8 ? ~(uint64_t) 0 : n ? ~(uint64_t) 0 >> (64 - 8 * n) : 0;
    m.hi = n >= 16 ? ~(uint64_t) 0 : n > 8 ? ~(uint64_t) 0 >> (64 - 8 * (n - 8)) : 0;
    return m;
}

/* the table in global memory: off[0 .. nlines] and the line ends of the split (a line starts one past the
 * end in front of it) */
struct sre_lg_tab_global {
    const uint64_t *offs;
    const uint64_t *ends;
    SRE_LG_MEMBER uint64_t off(uint64_t i) const { return offs[i]; }
    SRE_LG_MEMBER uint64_t start(uint64_t i) const { return i ? ends[i - 1] + 1 : 0; }
    SRE_LG_MEMBER bool     trails(uint64_t) const { return true; }
    template <class Sink> SRE_LG_MEMBER void text(Sink &sink, uint64_t i, uint64_t at, uint32_t head, uint32_t d, uint32_t cnt) const
    {
        sink.text((uint64_t) head + start(i) + at, d, cnt);
    }
    template <class Sink> SRE_LG_MEMBER void end(Sink &sink, uint64_t, uint32_t d) const { sink.delim(d); }
};

/* a window of it: lines base .. base + count - 1, offs[0 .. count] and starts[0 .. count - 1] */
struct sre_lg_tab_window {
    const uint64_t *offs;
    const uint64_t *starts;
    uint64_t        base;
    SRE_LG_MEMBER uint64_t off(uint64_t i) const { return offs[i - base]; }
    SRE_LG_MEMBER uint64_t start(uint64_t i) const { return starts[i - base]; }
    SRE_LG_MEMBER bool     trails(uint64_t) const { return true; }
    template <class Sink> SRE_LG_MEMBER void text(Sink &sink, uint64_t i, uint64_t at, uint32_t head, uint32_t d, uint32_t cnt) const
    {
        sink.text((uint64_t) head + start(i) + at, d, cnt);
    }
    template <class Sink> SRE_LG_MEMBER void end(Sink &sink, uint64_t, uint32_t d) const { sink.delim(d); }
};

/* the entry table of the line extract, whole (base 0, global memory) or a window of it (entries base .. , LDS):
 * offs as above, starts[e] = the source offset of the entry's text with flag bits on top.  The flags spare the
 * gather a division by K per entry and tell the index an unset field from an empty one */
#define SRE_LG_ENTRY_LAST   (1ull << 63)        /* the last field of its line: the delimiter follows, not fsep */
#define SRE_LG_ENTRY_UNSET  (1ull << 62)        /* the group is unset (index rows only) */
#define SRE_LG_ENTRY_FIRST  (1ull << 61)        /* the first field of its line (index rows only) */
#define SRE_LG_ENTRY_START  (SRE_LG_ENTRY_FIRST - 1)

struct sre_lg_tab_fields {
    const uint64_t *offs;
    const uint64_t *starts;
    uint64_t        base;
    SRE_LG_MEMBER uint64_t off(uint64_t e) const { return offs[e - base]; }
    SRE_LG_MEMBER uint64_t raw(uint64_t e) const { return starts[e - base]; }
    SRE_LG_MEMBER uint64_t start(uint64_t e) const { return starts[e - base] & SRE_LG_ENTRY_START; }
    SRE_LG_MEMBER bool     trails(uint64_t) const { return true; }
    template <class Sink> SRE_LG_MEMBER void text(Sink &sink, uint64_t e, uint64_t at, uint32_t head, uint32_t d, uint32_t cnt) const
    {
        sink.text((uint64_t) head + start(e) + at, d, cnt);
    }
    template <class Sink> SRE_LG_MEMBER void end(Sink &sink, uint64_t e, uint32_t d) const
    {
        if (starts[e - base] & SRE_LG_ENTRY_LAST) sink.delim(d);
        else sink.sep(d);
    }
};

/* the piece table of the line substitute, whole (base 0, global memory) or a window of it (LDS): entries
 * e = line * P + f, f = 0 the line's text in front of the match (FIRST), f = 1 .. P - 2 the template's pieces,
 * f = P - 1 the text behind the match (LAST; its value counts the delimiter too, so the last entry of a selected line
 * always takes a byte).  One more flag below the three: the text of a LITERAL entry starts at its offset in the
 * literal block, not in the source.  UNSET on a piece: the group is unset; on the FIRST entry: the line has no match
 * and is copied whole (index rows only).  Only the LAST entry has a byte behind its text */
#define SRE_LG_ENTRY_LITERAL    (1ull << 60)
#define SRE_LG_PIECE_START      (SRE_LG_ENTRY_LITERAL - 1)

struct sre_lg_tab_pieces {
    const uint64_t *offs;
    const uint64_t *starts;
    uint64_t        base;
    SRE_LG_MEMBER uint64_t off(uint64_t e) const { return offs[e - base]; }
    SRE_LG_MEMBER uint64_t raw(uint64_t e) const { return starts[e - base]; }
    SRE_LG_MEMBER uint64_t start(uint64_t e) const { return starts[e - base] & SRE_LG_PIECE_START; }
    SRE_LG_MEMBER bool     trails(uint64_t e) const { return (starts[e - base] & SRE_LG_ENTRY_LAST) != 0; }
    template <class Sink> SRE_LG_MEMBER void text(Sink &sink, uint64_t e, uint64_t at, uint32_t head, uint32_t d, uint32_t cnt) const
    {
        const uint64_t w = starts[e - base];
        if (w & SRE_LG_ENTRY_LITERAL) sink.literal((w & SRE_LG_PIECE_START) + at, d, cnt);
        else sink.text((uint64_t) head + (w & SRE_LG_PIECE_START) + at, d, cnt);
    }
    template <class Sink> SRE_LG_MEMBER void end(Sink &sink, uint64_t, uint32_t d) const { sink.delim(d); }
};

/* the entry table of the line join (sre_hip_join_lines, sre_lines_join.h), whole (base 0, global memory) or a window of it
 * (LDS): entries e = line * P + f, f = 0 the line's text from the source (FIRST), f = 1 .. P - 1 a value from the key
 * map's copy of the dictionary (LITERAL: the offset is one into that copy, the call's second extent) or nothing at all
 * (UNSET: a line without a dictionary row).  Every entry trails a byte as the extract's fields do: the delimiter behind
 * the LAST entry, the join separator (the geometry's fsep) behind every other */
struct sre_lg_tab_join {
    const uint64_t *offs;
    const uint64_t *starts;
    uint64_t        base;
    SRE_LG_MEMBER uint64_t off(uint64_t e) const { return offs[e - base]; }
    SRE_LG_MEMBER uint64_t raw(uint64_t e) const { return starts[e - base]; }
    SRE_LG_MEMBER uint64_t start(uint64_t e) const { return starts[e - base] & SRE_LG_PIECE_START; }
    SRE_LG_MEMBER bool     trails(uint64_t) const { return true; }
    template <class Sink> SRE_LG_MEMBER void text(Sink &sink, uint64_t e, uint64_t at, uint32_t head, uint32_t d, uint32_t cnt) const
    {
        const uint64_t w = starts[e - base];
        if (w & SRE_LG_ENTRY_LITERAL) sink.literal((w & SRE_LG_PIECE_START) + at, d, cnt);
        else sink.text((uint64_t) head + (w & SRE_LG_PIECE_START) + at, d, cnt);
    }
    template <class Sink> SRE_LG_MEMBER void end(Sink &sink, uint64_t e, uint32_t d) const
    {
        if (starts[e - base] & SRE_LG_ENTRY_LAST) sink.delim(d);
        else sink.sep(d);
    }
};

/* the last i of [lo, hi] with off(i) <= o; the caller knows off(lo) <= o */
template <class Tab>
SRE_LG_FN uint64_t
sre_lg_find(const Tab &tab, uint64_t o, uint64_t lo, uint64_t hi)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (tab.off(mid) <= o) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/* the cut of the line extract's output at out_cap: the first line i of n (n when all fit) whose row ends beyond
 * it, off[(i + 1) k] > out_cap, so that off[i k] bytes are written and every row is whole */
SRE_LG_FN uint64_t
sre_lg_row_cut(const uint64_t *off, uint64_t n, uint64_t k, uint64_t out_cap)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[(mid + 1) * k] > out_cap) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

/* output chunks of the call, and the output bytes [*o_lo, *o_hi) of chunks [c0, c1) (empty: false) */
SRE_LG_FN uint64_t
sre_lg_nchunks(const sre_lg_geom_t &g)
{
    return g.out_bytes ? ((uint64_t) g.dst_head + g.out_bytes + 15) / 16 : 0;
}

SRE_LG_FN bool
sre_lg_span(const sre_lg_geom_t &g, uint64_t c0, uint64_t c1, uint64_t *o_lo, uint64_t *o_hi)
{
    const uint64_t end = (uint64_t) g.dst_head + g.out_bytes;
    uint64_t       p = c0 * 16, q = c1 * 16;
    if (p < g.dst_head) p = g.dst_head;
    if (q > end) q = end;
    if (p >= q) return false;
    *o_lo = p - g.dst_head;
    *o_hi = q - g.dst_head;
    return true;
}

/* the slice of the table a tile needs: the lines of its first and of its last output byte.  Every chunk of the
 * tile is then searched in [*la, *lb], and the walk reads off(i) up to i = *lb + 1 */
template <class Tab>
SRE_LG_FN bool
sre_lg_tile_slice(const Tab &tab, const sre_lg_geom_t &g, uint64_t tile, uint64_t *la, uint64_t *lb)
{
    uint64_t o_lo, o_hi;
    if (!sre_lg_span(g, tile * SRE_LG_TILE_CHUNKS, (tile + 1) * SRE_LG_TILE_CHUNKS, &o_lo, &o_hi)) return false;
    *la = sre_lg_find(tab, o_lo, 0, g.nlines - 1);
    *lb = sre_lg_find(tab, o_hi - 1, *la, g.nlines - 1);
    return true;
}

/*
 * The plan of output chunk c, searched in the lines [lo, hi] (a tile's slice): the pieces in output order,
 *   sink.text(S, d, cnt)   cnt source bytes from position S go to bytes d .. d + cnt - 1 of the chunk
 *   sink.delim(d)          byte d of the chunk is the delimiter
 *   sink.sep(d)            ... the field separator (the entry table of the line extract only)
 *   sink.literal(L, d, cnt) cnt bytes from offset L of the literal block (the piece table of the line substitute only)
 * and the chunk's bytes [*first, *first + *count) are the ones the call owns (all 16 except in the first and
 * the last chunk of the output).  Every selected line takes at least its delimiter byte, so a chunk meets at
 * most 16 lines and the loop runs at most 16 times; stepping to the next selected line is one look at the
 * table when the next line is selected and a search otherwise, never a walk over the lines in between.
 *
 * The table says how an entry ends: tab.trails(i) is true when one byte follows the entry's text (tab.end emits it),
 * and the text is then output bytes [off(i), off(i + 1) - 1); otherwise the text runs to off(i + 1).  The tables of
 * the filter and the extract answer true for every entry at compile time.  An entry that takes no byte is never
 * visited, the step to the next entry that takes bytes skips it, so every visited entry still takes at least one
 * byte of the chunk.
 */
template <class Tab, class Sink>
SRE_LG_FN bool
sre_lg_walk(const Tab &tab, const sre_lg_geom_t &g, uint64_t c, uint64_t lo, uint64_t hi, Sink &sink, uint32_t *first,
            uint32_t *count)
{
    uint64_t o, o_hi;
    if (!sre_lg_span(g, c, c + 1, &o, &o_hi)) return false;
    const uint64_t p0 = c * 16;                     /* P of the chunk's byte 0 */
    *first = (uint32_t) (o + g.dst_head - p0);
    *count = (uint32_t) (o_hi - o);
    uint64_t i = sre_lg_find(tab, o, lo, hi);
    for (;;) {
        const uint64_t b = tab.off(i), e = tab.off(i + 1);      /* the line is output bytes [b, e), e - 1 its delimiter */
        const bool     tr = tab.trails(i);
        const uint64_t t_lim = tr ? e - 1 : e;
        const uint64_t t_end = o_hi < t_lim ? o_hi : t_lim;
        if (o < t_end) {
            tab.text(sink, i, o - b, g.src_head, (uint32_t) (o + g.dst_head - p0), (uint32_t) (t_end - o));
            o = t_end;
        }
        if (tr && o < o_hi) {
            tab.end(sink, i, (uint32_t) (o + g.dst_head - p0));
            o++;
        }
        if (o >= o_hi) break;
        /* o = off(i + 1): the next selected line is i + 1, or lies behind a run of lines that take no byte */
        i = tab.off(i + 2) > o ? i + 1 : sre_lg_find(tab, o, i + 1, hi);
    }
    return true;
}

/*
 * The sink that builds the chunk in registers.  Mem gives 16-byte loads only:
 *   mem.load(q)    source block q (aligned)
 *   mem.loadu(S)   the 16 bytes from source position S (any alignment)
 * A piece of 16 bytes (the common case: the chunk lies inside one line) is one unaligned load of bytes that
 * are all text of the line.  A shorter piece comes from the one or two aligned blocks that hold its bytes,
 * funnelled into place; those blocks lie inside the 16-byte aligned extent of the source buffer because they
 * hold bytes of it.
 *
 * The text of a literal piece comes the same way from the literal block, through mem.lit_load(q) and
 * mem.lit_loadu(L): the block starts at a 16-byte aligned address and is padded to a multiple of 16 bytes, so the
 * aligned blocks that hold bytes of a literal lie inside it.
 */
template <class Mem>
struct sre_lg_assembler {
    Mem        &mem;
    uint32_t    delim_byte, sep_byte;
    sre_lg_u128 acc;

    SRE_LG_MEMBER sre_lg_assembler(Mem &m, uint32_t d, uint32_t s) : mem(m), delim_byte(d), sep_byte(s) { acc.lo = 0; acc.hi = 0; }

    template <bool LIT> SRE_LG_MEMBER sre_lg_u128 block(uint64_t q)
    {
        if constexpr (LIT) return mem.lit_load(q);
        else return mem.load(q);
    }
    template <bool LIT> SRE_LG_MEMBER sre_lg_u128 blocku(uint64_t s)
    {
        if constexpr (LIT) return mem.lit_loadu(s);
        else return mem.loadu(s);
    }

    SRE_LG_MEMBER void text(uint64_t s, uint32_t d, uint32_t cnt) { put<false>(s, d, cnt); }
    SRE_LG_MEMBER void literal(uint64_t s, uint32_t d, uint32_t cnt) { put<true>(s, d, cnt); }

    template <bool LIT> SRE_LG_MEMBER void put(uint64_t s, uint32_t d, uint32_t cnt)
    {
        if (cnt == 16) {
            acc = blocku<LIT>(s);
            return;
        }
        const uint64_t q = s >> 4;
        const uint32_t sh = (uint32_t) (s & 15u);
        sre_lg_u128    v = sre_lg_shr(block<LIT>(q), sh);
        if (sh + cnt > 16) {
            const sre_lg_u128 w = sre_lg_shl(block<LIT>(q + 1), 16 - sh);
            v.lo |= w.lo;
            v.hi |= w.hi;
        }
        const sre_lg_u128 m = sre_lg_mask(cnt);
        v.lo &= m.lo;
        v.hi &= m.hi;
        v = sre_lg_shl(v, d);
        acc.lo |= v.lo;
        acc.hi |= v.hi;
    }

    SRE_LG_MEMBER void byte(uint32_t b, uint32_t d)
    {
        sre_lg_u128 v;
        v.lo = b & 0xFFu;
        v.hi = 0;
        v = sre_lg_shl(v, d);
        acc.lo |= v.lo;
        acc.hi |= v.hi;
    }
    SRE_LG_MEMBER void delim(uint32_t d) { byte(delim_byte, d); }
    SRE_LG_MEMBER void sep(uint32_t d) { byte(sep_byte, d); }
};

/* one output chunk: plan, assemble, store.  mem.store(c, v) writes the aligned chunk whole, mem.store_bytes(c,
 * v, first, count) the bytes [first, first + count) of it (the first and the last chunk of the output only) */
template <class Tab, class Mem>
SRE_LG_FN void
sre_lg_chunk(const Tab &tab, const sre_lg_geom_t &g, uint64_t c, uint64_t lo, uint64_t hi, Mem &mem)
{
    sre_lg_assembler<Mem> as(mem, g.delim, g.fsep);
    uint32_t              first, count;
    if (!sre_lg_walk(tab, g, c, lo, hi, as, &first, &count)) return;
    if (count == 16) mem.store(c, as.acc);
    else mem.store_bytes(c, as.acc, first, count);
}

#endif
