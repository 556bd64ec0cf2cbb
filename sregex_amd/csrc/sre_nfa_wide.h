/*
 * sre_nfa_wide.h — the WIDE bit-parallel form of a compiled program: the set of live threads in
 * W = 1, 2 or 4 64-bit words (64, 128 or 256 bits), for programs the 64-bit builder (sre_nfa.h)
 * declines for width alone.  The semantics are those of sre_nfa.h (exact sets for Thompson; for Pike
 * exact up to the first MATCH event, with a CLEAN position in front of it; look-ahead assertions by
 * the expansion tables); only the width and the table form are new.
 *
 * The form is the shift-and form of sre_nfa.h carried across words, always masked, MATCH as event
 * sources (`evacc`):
 *
 *      S  |= expand[prev kind * 4 + cur kind][assertion bits of S]     (look-ahead programs)
 *      ev |= S & match                                                  (an expansion listed MATCH)
 *      t   = S & accept[byte];   ev |= t & msrc                         (a consumed byte reaches MATCH)
 *      S'  = ((t & shift_src) << 1) | (t & self) | seed | OR_k lut[k][byte hot[k] of t]
 *
 * The shift carries from one word into the next.  Bits are counted AFTER equivalent threads are merged
 * (the two arms of `(?:a|b)` are one bit), so W is often smaller than prog->nthreads / 64.  When no
 * layout of the chains needs few enough lookups, every byte of the mask that holds a thread is a lookup
 * and nothing shifts: the plain slices of sre_nfa.h, the correctness baseline (16 lookups at 128 bits).
 * The lookup tables, the accept table and the expansion table live in LDS; a form whose tables do not
 * fit the budget (SRE_NFA_WIDE_LDS_BUDGET, with the staging tile) is declined.
 */
#ifndef SRE_NFA_WIDE_H
#define SRE_NFA_WIDE_H

#include "sre_program.h"
#include "sre_nfa.h"

#define SRE_NFA_WIDE_MAX_WORDS 4u
#define SRE_NFA_WIDE_MAX_LUT   16u
/* LDS of a workgroup the tables and the staging tile may take (160 KiB per CU, MI355X: the most one
 * workgroup may have) */
#define SRE_NFA_WIDE_LDS_BUDGET (160u * 1024u)
/* what the kernel's staging tile and row descriptors take beside the tables (sre_hip_nfa_wide.hip) */
#define SRE_NFA_WIDE_TILE_LDS   (256u * (64u + 16u) + 256u * 16u)

/* the lookup count a kernel variant is compiled for (0, 1, 2, 4, 8, 16); the slots beyond the form's own
 * read a table of zeros */
static inline uint32_t
sre_nfa_wide_round_lut(uint32_t nlut)
{
    return nlut == 0 ? 0u : nlut <= 1 ? 1u : nlut <= 2 ? 2u : nlut <= 4 ? 4u : nlut <= 8 ? 8u : 16u;
}

/* the kernel's whole LDS for a form (all of it dynamic): staging tile and row descriptors | accept [256][W] |
 * byte kinds [256] x 4 B | zero table [256][W] (only when the variant has more slots than the form has
 * lookups) | lookups [nlut][256][W] | expansion [16][1 << nassert][W].  The builder admits a form by this
 * number and the launcher asks for it: one formula for both. */
static inline size_t
sre_nfa_wide_lds(uint32_t W, uint32_t nlut, uint32_t nassert)
{
    const size_t e = (size_t) W * 8u;
    return (size_t) SRE_NFA_WIDE_TILE_LDS + 256u * e + 256u * 4u + (sre_nfa_wide_round_lut(nlut) > nlut ? 256u * e : 0u)
           + (size_t) nlut * 256u * e + (nassert ? ((size_t) 16u << nassert) * e : 0u);
}

/* build options (tests force every variant) */
#define SRE_NFA_WIDE_NO_MERGE      1u      /* keep equivalent threads apart */
#define SRE_NFA_WIDE_EXPLICIT_ANY  2u      /* the ".*?" thread as a bit, not the implicit seed */
#define SRE_NFA_WIDE_PLAIN         4u      /* no shift: every byte that holds a thread is a lookup */
#define SRE_NFA_WIDE_MIN_W2        8u      /* at least 128 bits */
#define SRE_NFA_WIDE_MIN_W4       16u      /* 256 bits */

#ifdef __cplusplus
#include <vector>

struct sre_nfa_wide_s {
    uint32_t W;                 /* 64-bit words per set: 1, 2 or 4 */
    uint32_t nbits;             /* highest bit in use + 1 */
    uint32_t raw_bits;          /* threads + newline twins + assertions, before merging */
    uint32_t plain;             /* 1: the plain slices (nothing shifts) */
    uint32_t nlut;              /* <= SRE_NFA_WIDE_MAX_LUT */
    uint32_t hot[SRE_NFA_WIDE_MAX_LUT];     /* byte of the mask (0 .. 8W - 1) that indexes lut[k] */
    uint32_t nassert;           /* look-ahead assertions: bits 0 .. nassert - 1 of word 0 */
    uint32_t implicit_any;      /* the ".*?" thread is the seed, not a bit */
    uint64_t init[3][4];        /* SRE_DFA_INIT_* -> initial set */
    uint64_t seed[4], any_bits[4], match_bits[4], msrc[4], valid[4], self[4], shift_src[4];
    uint64_t accept[256][4];
    std::vector<uint64_t> lut;      /* [nlut][256][W] */
    std::vector<uint64_t> expand;   /* [16 contexts][1 << nassert][W] */
    uint8_t  kind[256];             /* per input byte: SRE_NFA_KIND_* | SRE_NFA_LEADING (sre_nfa.h) */
    size_t   lds_bytes;             /* tables + staging tile of the kernel */
};
typedef struct sre_nfa_wide_s sre_nfa_wide_t;

extern "C" {
#else
typedef struct sre_nfa_wide_s sre_nfa_wide_t;
#endif

/* NULL + *why when the program has no wide form: more than 256 bits after merging, tables beyond the
 * LDS budget, or what sre_nfa_build also declines for (more than 8 look-ahead assertions, one inside a
 * loop, a nullable regex, more than 4096 instructions) */
sre_nfa_wide_t *sre_nfa_wide_build(const sre_program_t *prog, unsigned options, const char **why);
void sre_nfa_wide_free(sre_nfa_wide_t *w);

#ifdef __cplusplus
}
#endif
#endif
