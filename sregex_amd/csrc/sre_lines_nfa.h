/*
 * sre_lines_nfa.h — one SHORT LINE on the bit-parallel NFA tier (line mode): ONE
 * text of the set step for the short-line kernel (sre_hip_lines_nfa.hip sre_k_lines_nfa) and for the
 * CPU model (tests/lines_nfa_sim.cpp).
 *
 * A line is a whole stream: it enters with the fresh initial set, the byte in front of its offset 0
 * counts as the start of the stream (never the delimiter), and behind its last byte comes the end of
 * input.  So a lane needs no warm-up, no summary and no chain check — it walks its line from the
 * initial set and stops at the first step that reaches MATCH.
 *
 * The step is the set kernels' (sre_hip_nfa.hip sre_k_nfa / sre_k_nfa_sa) for the four table shapes
 * of the 64-bit forms, on 64-bit words whatever the program's width:
 *
 *   look-ahead forms first list the continuations of the assertions that hold between the byte in
 *   front and this one:      S |= expand[(prev kind * 4 + kind) << xshift | assertion bits of S]
 *   plain slices:            t = S & (accept[b] | MATCH);  S' = (t & MATCH) | OR_k tab[k][byte k of t]
 *   shift-and:               t = S & accept[b]
 *                            S' = ((t & shift_src) << 1) | (t & self) | seed | OR_q tab[q][hot byte q of t]
 *   event:                   (t & ev_t) | (S' & ev_s)    ev_t: the `evacc` forms' MATCH sources,
 *                                                        ev_s: the MATCH bits of every other form
 */
#ifndef SRE_LINES_NFA_H
#define SRE_LINES_NFA_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRE_LNFA_FN __host__ __device__ static inline
#else
#define SRE_LNFA_FN static inline
#endif

#define SRE_LNFA_KIND_EDGE 3u       /* sre_nfa.h SRE_NFA_KIND_EDGE: start of the stream / end of input */

/* the tables as the step reads them: LDS in the kernel, host memory in the model */
typedef struct {
    uint32_t sa, la;                /* the shape: shift-and (else plain slices), look-ahead assertions */
    uint32_t ntab;                  /* plain: follow slices that hold consuming threads; shift-and: lookups (0..3) */
    uint32_t hot[3];                /* shift-and: bit offset in t of the byte that indexes lookup q */
    uint32_t xshift, ashift;        /* look-ahead: log2 of the entries of one expansion context; bit offset of the
                                       assertion bits in the set */
    uint64_t amask;                 /* ... and their mask behind the shift */
    uint64_t init;                  /* the fresh initial set (SRE_DFA_INIT_START) */
    uint64_t sticky;                /* plain: the MATCH bits, accepted by every byte and listing themselves */
    uint64_t seed, self, shift_src; /* shift-and (shift_src: all ones when the form is not `masked`) */
    uint64_t shmask, wmask;         /* shift-and: bits a shift may produce (no carry: not bit 32); bits of the form's width */
    uint64_t ev_t, ev_s;
    const uint64_t *accept;         /* [256] */
    const uint64_t *tab;            /* [ntab][256] */
    const uint64_t *expand;         /* [16 << xshift], la only */
    const uint8_t  *kind;           /* [256] sre_nfa.h SRE_NFA_KIND_* (| SRE_NFA_LEADING), la only */
} sre_lnfa_t;

/* a lane's walk of one line */
typedef struct {
    uint64_t S;
    uint32_t prevk;                 /* la: kind of the byte in front */
    int64_t  ev;                    /* position of the first step that reached MATCH (the line's length: at the
                                       end of input), -1 none */
} sre_lnfa_lane_t;

SRE_LNFA_FN void
sre_lnfa_begin(const sre_lnfa_t &T, sre_lnfa_lane_t &L)
{
    L.S = T.init;
    L.prevk = SRE_LNFA_KIND_EDGE;
    L.ev = -1;
}

SRE_LNFA_FN uint64_t
sre_lnfa_expand(const sre_lnfa_t &T, uint64_t S, uint32_t prevk, uint32_t ck)
{
    const uint64_t a = (S >> T.ashift) & T.amask;
    /* (no assertion listed: nothing to expand — the set kernels skip the lookup by a ballot) */
    if (a) S |= T.expand[((uint64_t) (prevk * 4u + ck) << T.xshift) + a];
    return S;
}

/* the byte at position pos of the line; returns nonzero when its step reached MATCH (L.ev = pos) */
SRE_LNFA_FN int
sre_lnfa_byte(const sre_lnfa_t &T, sre_lnfa_lane_t &L, uint32_t byte, int64_t pos)
{
    uint64_t S = L.S;
    if (T.la) {
        const uint32_t ck = T.kind[byte] & 3u;
        S = sre_lnfa_expand(T, S, L.prevk, ck);
        L.prevk = ck;
    }
    uint64_t t, S1;
    if (T.sa) {
        t = S & T.accept[byte];
        uint64_t e = T.seed;
        /* (at most three lookups, written out: a loop over hot[] would index the table struct by a variable
         * and keep the kernel's copy of it in memory) */
        if (T.ntab > 0) e |= T.tab[(uint32_t) ((t >> T.hot[0]) & 0xffu)];
        if (T.ntab > 1) e |= T.tab[256u + (uint32_t) ((t >> T.hot[1]) & 0xffu)];
        if (T.ntab > 2) e |= T.tab[512u + (uint32_t) ((t >> T.hot[2]) & 0xffu)];
        S1 = ((((t & T.shift_src) << 1) & T.shmask) | (t & T.self) | e) & T.wmask;
    } else {
        t = S & (T.accept[byte] | T.sticky);
        S1 = t & T.sticky;
        for (uint32_t k = 0; k < T.ntab; k++) S1 |= T.tab[k * 256u + (uint32_t) ((t >> (8u * k)) & 0xffu)];
    }
    L.S = S1;
    if ((t & T.ev_t) | (S1 & T.ev_s)) {
        L.ev = pos;
        return 1;
    }
    return 0;
}

/* behind the last byte of a line of n bytes that held no event: the extra iteration at end of input
 * (the set kernels' `last_seg && !no_eof`) — assertions that hold in front of the end list their
 * continuations, a MATCH among them is an event at n */
SRE_LNFA_FN void
sre_lnfa_end(const sre_lnfa_t &T, sre_lnfa_lane_t &L, int64_t n)
{
    if (!T.la) return;
    L.S = sre_lnfa_expand(T, L.S, L.prevk, SRE_LNFA_KIND_EDGE);
    if (L.S & T.ev_s) L.ev = n;
}

/* the scalar part of the tables of a shift-and form; w64 .. shift_src as sre_nfa_sa_t / sre_nfa_sa_tables_t
 * name them, hot_byte[q] = the byte of the mask that indexes lookup q, assert_byte = the one that holds the
 * assertion bits, xshift = log2 of the entries of one expansion context */
SRE_LNFA_FN void
sre_lnfa_set_sa(sre_lnfa_t &T, uint32_t w64, uint32_t carry, uint32_t masked, uint32_t evacc, uint32_t nlut,
                const uint32_t *hot_byte, uint64_t init0, uint64_t seed, uint64_t self, uint64_t shift_src,
                uint64_t match_bits, uint64_t msrc, uint32_t nassert, uint32_t assert_byte, uint32_t xshift)
{
    T.sa = 1;
    T.la = nassert != 0;
    T.ntab = nlut;
    T.hot[0] = nlut > 0 ? 8u * hot_byte[0] : 0u;
    T.hot[1] = nlut > 1 ? 8u * hot_byte[1] : 0u;
    T.hot[2] = nlut > 2 ? 8u * hot_byte[2] : 0u;
    T.xshift = xshift;
    T.ashift = 8u * assert_byte;
    T.amask = xshift >= 8 ? 0xffull : (1ull << xshift) - 1;
    T.init = init0;
    T.sticky = 0;
    T.seed = seed;
    T.self = self;
    T.shift_src = masked ? shift_src : ~0ull;
    T.shmask = (w64 && carry) ? ~0ull : ~(1ull << 32);
    T.wmask = w64 ? ~0ull : 0xffffffffull;
    T.ev_t = evacc ? msrc : 0;
    T.ev_s = evacc ? 0 : match_bits;
}

/* ... of a plain form of nslices byte slices (with assertions the last one holds their bits and no consuming thread) */
SRE_LNFA_FN void
sre_lnfa_set_plain(sre_lnfa_t &T, uint32_t nslices, uint32_t nassert, uint64_t init0, uint64_t match_bits)
{
    T.sa = 0;
    T.la = nassert != 0;
    T.ntab = nassert ? nslices - 1 : nslices;
    T.hot[0] = T.hot[1] = T.hot[2] = 0;
    T.xshift = 8;
    T.ashift = nassert ? 8u * (nslices - 1) : 0u;
    T.amask = 0xffull;
    T.init = init0;
    T.sticky = match_bits;
    T.seed = T.self = T.shift_src = 0;
    T.shmask = T.wmask = ~0ull;
    T.ev_t = 0;
    T.ev_s = match_bits;
}

#endif
