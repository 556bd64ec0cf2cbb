/*
 * sre_lines_context.h — the block logic of the line filter's context pass (sre_hip_filter_lines_context, DESIGN.md
 * §4.11.5): which lines lie within `before` lines in front of a matched line or `after` lines behind one.  The kernels
 * (sre_hip_lines_context.hip) and the CPU model (tests/lines_context_sim.cpp) compile this text; nothing here touches
 * memory except through its arguments.
 *
 * The pass runs over the filter's per-line values val[0 .. n): line i is MATCHED when val[i] > 0.  For every line
 *   p(i) = the nearest matched line at or in front of i,   q(i) = the nearest matched line at or behind i,
 * and line i is SELECTED when i - p(i) <= after or q(i) - i <= before (a matched line is its own p and q).  Both are
 * scans: p a forward maximum, q a backward minimum, so the cost per line does not depend on before and after.
 *
 * Encodings.  A "P word" is a line index + 1, 0 when there is no such line (the identity of the maximum); a "Q word" is
 * a line index, all ones when there is none (the identity of the minimum).  Inside a workgroup of SRE_LC_ITEMS lines
 * both are 32-bit and relative to the workgroup's first line; the words that cross workgroups (the block words of the
 * marks and carry kernels) and everything compared with before / after are 64-bit line indices.  Distances are
 * differences of indices that are known to be ordered, so nothing overflows for any before / after up to SIZE_MAX.
 *
 * Geometry: a workgroup of SRE_LC_THREADS lanes owns SRE_LC_ITEMS consecutive lines, lane t the lines 4t .. 4t + 3 of
 * them; a wave of 64 lanes therefore owns 256 consecutive lines, four 64-bit words of the context bitmap.
 */
#ifndef SRE_LINES_CONTEXT_H
#define SRE_LINES_CONTEXT_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRE_LC_FN __host__ __device__ static inline
#else
#define SRE_LC_FN static inline
#endif

#define SRE_LC_ITEMS        1024u
#define SRE_LC_THREADS      256u
#define SRE_LC_PER_LANE     4u
#define SRE_LC_WAVE         64u
#define SRE_LC_WAVES        (SRE_LC_THREADS / SRE_LC_WAVE)
#define SRE_LC_CARRY_LANES  1024u                   /* the one workgroup of the carry kernel */

#define SRE_LC_NONE32       0xFFFFFFFFu             /* Q word, workgroup-relative: no matched line */
#define SRE_LC_NONE         (~(uint64_t) 0)         /* Q word: no matched line */

/* what the pass finds out about a line; the first two are bits 0 and 1 of word [4] of an index row */
#define SRE_LC_CONTEXT      1u                      /* selected, not matched itself */
#define SRE_LC_GROUP        2u                      /* selected, and line 0 or its predecessor is not selected */
#define SRE_LC_SELECTED     4u

/* ---- the per-lane combine ---- */

/* a lane's four values: the P word of its last matched line and the Q word of its first one, relative to the
 * workgroup (t = the lane's number in it) */
SRE_LC_FN void
sre_lc_lane_marks(const uint64_t v[SRE_LC_PER_LANE], uint32_t t, uint32_t *last, uint32_t *first)
{
    uint32_t l = 0, f = SRE_LC_NONE32;
    for (uint32_t q = 0; q < SRE_LC_PER_LANE; q++) {
        if (v[q] == 0) continue;
        l = SRE_LC_PER_LANE * t + q + 1;
        if (f == SRE_LC_NONE32) f = SRE_LC_PER_LANE * t + q;
    }
    *last = l;
    *first = f;
}

/* ---- the scans ---- */

/* one step of a wave's scan at distance d: x is the lane's word, y the word of lane - d (forward: the maximum of P
 * words) or of lane + d (backward: the minimum of Q words); a lane without such a neighbour keeps its word */
template <class T>
SRE_LC_FN T
sre_lc_fwd(T x, T y, uint32_t lane, uint32_t d)
{
    return lane >= d && y > x ? y : x;
}

template <class T>
SRE_LC_FN T
sre_lc_bwd(T x, T y, uint32_t lane, uint32_t d)
{
    return lane + d < SRE_LC_WAVE && y < x ? y : x;
}

/* what the waves in front of wave w (forward) or behind it (backward) hand it, from the nw waves' totals */
template <class T>
SRE_LC_FN T
sre_lc_waves_fwd(const T *wtot, uint32_t nw, uint32_t w)
{
    T r = 0;
    for (uint32_t i = 0; i < nw; i++) r = i < w && wtot[i] > r ? wtot[i] : r;
    return r;
}

template <class T>
SRE_LC_FN T
sre_lc_waves_bwd(const T *wtot, uint32_t nw, uint32_t w)
{
    T r = (T) ~(T) 0;
    for (uint32_t i = 0; i < nw; i++) r = i > w && wtot[i] < r ? wtot[i] : r;
    return r;
}

/* The scans as functions over an array, for the CPU model: x[0 .. 64) are the words of a wave's lanes, and every step
 * reads what the shuffle of the kernel reads (lane - d, lane + d; a lane without that neighbour gets its own word).
 * They come back EXCLUSIVE (lane l: the lanes in front of l, resp. behind it), the wave's total in *total. */
template <class T>
SRE_LC_FN void
sre_lc_wave_scan_fwd(T *x, T *total)
{
    T y[SRE_LC_WAVE], own = x[SRE_LC_WAVE - 1];
    for (uint32_t l = SRE_LC_WAVE; l-- > 1;) x[l] = x[l - 1];
    x[0] = 0;
    for (uint32_t d = 1; d < SRE_LC_WAVE; d <<= 1) {
        for (uint32_t l = 0; l < SRE_LC_WAVE; l++) y[l] = x[l >= d ? l - d : l];
        for (uint32_t l = 0; l < SRE_LC_WAVE; l++) x[l] = sre_lc_fwd(x[l], y[l], l, d);
    }
    *total = x[SRE_LC_WAVE - 1] > own ? x[SRE_LC_WAVE - 1] : own;
}

template <class T>
SRE_LC_FN void
sre_lc_wave_scan_bwd(T *x, T *total)
{
    T y[SRE_LC_WAVE], own = x[0];
    for (uint32_t l = 0; l + 1 < SRE_LC_WAVE; l++) x[l] = x[l + 1];
    x[SRE_LC_WAVE - 1] = (T) ~(T) 0;
    for (uint32_t d = 1; d < SRE_LC_WAVE; d <<= 1) {
        for (uint32_t l = 0; l < SRE_LC_WAVE; l++) y[l] = x[l + d < SRE_LC_WAVE ? l + d : l];
        for (uint32_t l = 0; l < SRE_LC_WAVE; l++) x[l] = sre_lc_bwd(x[l], y[l], l, d);
    }
    *total = x[0] < own ? x[0] : own;
}

/* ... and of a workgroup of nw waves: p[0 .. 64 nw) the lanes' P words, q their Q words; both come back exclusive
 * over the whole workgroup, the workgroup's totals in *ptot and *qtot */
template <class T>
SRE_LC_FN void
sre_lc_block_scan(T *p, T *q, uint32_t nw, T *ptot, T *qtot)
{
    T wp[SRE_LC_CARRY_LANES / SRE_LC_WAVE], wq[SRE_LC_CARRY_LANES / SRE_LC_WAVE];
    for (uint32_t w = 0; w < nw; w++) {
        sre_lc_wave_scan_fwd(p + w * SRE_LC_WAVE, &wp[w]);
        sre_lc_wave_scan_bwd(q + w * SRE_LC_WAVE, &wq[w]);
    }
    for (uint32_t w = 0; w < nw; w++) {
        const T pin = sre_lc_waves_fwd(wp, nw, w), qin = sre_lc_waves_bwd(wq, nw, w);
        for (uint32_t l = 0; l < SRE_LC_WAVE; l++) {
            T &a = p[w * SRE_LC_WAVE + l], &b = q[w * SRE_LC_WAVE + l];
            a = pin > a ? pin : a;
            b = qin < b ? qin : b;
        }
    }
    *ptot = sre_lc_waves_fwd(wp, nw, nw);
    T qt = wq[0];
    for (uint32_t w = 1; w < nw; w++) qt = wq[w] < qt ? wq[w] : qt;
    *qtot = qt;
}

/* workgroup-relative words to line indices: `base` is the workgroup's first line, pin / qin what the carry kernel
 * handed the workgroup */
SRE_LC_FN uint64_t
sre_lc_p_global(uint64_t base, uint32_t rel, uint64_t pin)
{
    return rel ? base + rel : pin;
}

SRE_LC_FN uint64_t
sre_lc_q_global(uint64_t base, uint32_t rel, uint64_t qin)
{
    return rel != SRE_LC_NONE32 ? base + rel : qin;
}

/* ---- the carry over the block words ---- */

/* A lane of the carry kernel owns the block words [lo, hi).  Its P and Q words for the workgroup's scan ... */
SRE_LC_FN void
sre_lc_run_marks(const uint64_t *last, const uint64_t *first, uint64_t lo, uint64_t hi, uint64_t *p, uint64_t *q)
{
    uint64_t a = 0, b = SRE_LC_NONE;
    for (uint64_t i = lo; i < hi; i++) {
        a = last[i] > a ? last[i] : a;
        b = first[i] < b ? first[i] : b;
    }
    *p = a;
    *q = b;
}

/* ... and, with the exclusive words pin / qin the scan gave it, its block words in place: last[b] becomes p_in of
 * block b, the nearest matched line in front of the block, first[b] becomes q_in, the nearest one behind it */
SRE_LC_FN void
sre_lc_run_carry(uint64_t *last, uint64_t *first, uint64_t lo, uint64_t hi, uint64_t pin, uint64_t qin)
{
    for (uint64_t i = lo; i < hi; i++) {
        const uint64_t x = last[i];
        last[i] = pin;
        pin = x > pin ? x : pin;
    }
    for (uint64_t i = hi; i-- > lo;) {
        const uint64_t x = first[i];
        first[i] = qin;
        qin = x < qin ? x : qin;
    }
}

/* ---- the selection rule ---- */

/* line i with p = the P word of the nearest matched line at or in front of it (p <= i + 1) and q = the Q word of the
 * nearest one at or behind it (q >= i) */
SRE_LC_FN bool
sre_lc_selected(uint64_t i, uint64_t p, uint64_t q, uint64_t before, uint64_t after)
{
    return (p != 0 && i - (p - 1) <= after) || (q != SRE_LC_NONE && q - i <= before);
}

/* line i of n, matched or not, with pe = the P word of the nearest matched line IN FRONT of it and q as above: the
 * SRE_LC_* bits of the line.  Its predecessor is judged by the same rule: p(i - 1) = pe, and q(i - 1) = q unless line
 * i - 1 is matched itself, and then pe says so. */
SRE_LC_FN uint32_t
sre_lc_line(uint64_t i, uint64_t n, bool matched, uint64_t pe, uint64_t q, uint64_t before, uint64_t after)
{
    if (i >= n || !sre_lc_selected(i, matched ? i + 1 : pe, q, before, after)) return 0;
    const bool pred = i != 0 && sre_lc_selected(i - 1, pe, q, before, after);
    return SRE_LC_SELECTED | (matched ? 0 : SRE_LC_CONTEXT) | (pred ? 0 : SRE_LC_GROUP);
}

/* a lane's four lines i0 .. i0 + 3 with values v: pe = the P word of the nearest matched line in front of i0, qe the Q
 * word of the nearest one behind i0 + 3 */
SRE_LC_FN void
sre_lc_lane_lines(uint64_t i0, uint64_t n, const uint64_t v[SRE_LC_PER_LANE], uint64_t pe, uint64_t qe, uint64_t before,
                  uint64_t after, uint32_t fl[SRE_LC_PER_LANE])
{
    uint64_t q[SRE_LC_PER_LANE];
    for (uint32_t k = SRE_LC_PER_LANE; k-- > 0;) {
        qe = v[k] ? i0 + k : qe;
        q[k] = qe;
    }
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) {
        fl[k] = sre_lc_line(i0 + k, n, v[k] != 0, pe, q[k], before, after);
        pe = v[k] ? i0 + k + 1 : pe;
    }
}

/* ---- the bitmap word and the counts ---- */

/* the 16 low bits of x spread to every fourth bit */
SRE_LC_FN uint64_t
sre_lc_spread4(uint64_t x)
{
    x &= 0xFFFFull;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

/* b[k] = the wave's ballot of a bit of line k of every lane (bit l: lane l, the wave's line 4 l + k).  Word w of the
 * four bitmap words of the wave's 256 lines: bit j = the wave's line 64 w + j, the lanes 16 w .. 16 w + 15 */
SRE_LC_FN uint64_t
sre_lc_bitmap_word(const uint64_t b[SRE_LC_PER_LANE], uint32_t w)
{
    uint64_t r = 0;
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) r |= sre_lc_spread4(b[k] >> (16 * w)) << k;
    return r;
}

/* lines of the wave with the bit */
SRE_LC_FN uint32_t
sre_lc_count(const uint64_t b[SRE_LC_PER_LANE])
{
    uint32_t r = 0;
    for (uint32_t k = 0; k < SRE_LC_PER_LANE; k++) r += (uint32_t) __builtin_popcountll(b[k]);
    return r;
}

#endif
