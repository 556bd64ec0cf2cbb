/*
 * tests/nfa_wide_sim.cpp — TEST-ONLY host model of the wide bit-parallel NFA scanner.
 *
 * Walks the tables of sregex_amd/csrc/sre_nfa_wide.cpp sequentially over a buffer, W 64-bit words per
 * set, the way the device kernel (sre_hip_nfa_wide.hip) does per lane, and reports the first MATCH event
 * and the last clean position in front of it.  Compiled by tests/test_nfa_wide_model.py into
 * tests/_build/; not part of, nor linked into, the product library.
 */
#include "sre_nfa_wide.h"
#include <string.h>
#include <stdint.h>

namespace {

struct Set {
    uint64_t w[4];
};

/* the look-ahead expansion at a position: prev / cur = kinds of the bytes around it */
inline void
expand(const sre_nfa_wide_t *a, Set &S, uint32_t prev, uint32_t cur)
{
    if (!a->nassert) return;
    const uint64_t idx = S.w[0] & ((1ull << a->nassert) - 1);
    const size_t   per = (size_t) 1 << a->nassert;
    for (uint32_t i = 0; i < a->W; i++) S.w[i] |= a->expand[((size_t) (prev * 4 + cur) * per + idx) * a->W + i];
}

/* one consuming step; returns t (the threads that consumed the byte) */
inline Set
step(const sre_nfa_wide_t *a, Set &S, unsigned byte)
{
    Set t, r;
    for (uint32_t i = 0; i < 4; i++) {
        t.w[i] = i < a->W ? S.w[i] & a->accept[byte][i] : 0;
        r.w[i] = 0;
    }
    for (uint32_t i = 0; i < a->W; i++) {
        const uint64_t ts = t.w[i] & a->shift_src[i];
        const uint64_t below = i ? (t.w[i - 1] & a->shift_src[i - 1]) >> 63 : 0;
        r.w[i] = (ts << 1) | below | (t.w[i] & a->self[i]) | a->seed[i];
    }
    for (uint32_t k = 0; k < a->nlut; k++) {
        const uint32_t x = (uint32_t) (t.w[a->hot[k] >> 3] >> (8 * (a->hot[k] & 7))) & 0xffu;
        for (uint32_t i = 0; i < a->W; i++) r.w[i] |= a->lut[((size_t) k * 256 + x) * a->W + i];
    }
    S = r;
    return t;
}

inline bool
meets(const sre_nfa_wide_t *a, const Set &S, const uint64_t *m)
{
    uint64_t v = 0;
    for (uint32_t i = 0; i < a->W; i++) v |= S.w[i] & m[i];
    return v != 0;
}

}  // namespace

extern "C" {

void *wsim_build(const sre_program_t *prog, unsigned options, const char **why) { return sre_nfa_wide_build(prog, options, why); }
void wsim_free(void *h) { sre_nfa_wide_free(static_cast<sre_nfa_wide_t *>(h)); }

/* info = W, nbits, raw_bits, plain, nlut, nassert, implicit_any, lds bytes */
void wsim_info(void *h, int64_t *info)
{
    const sre_nfa_wide_t *a = static_cast<sre_nfa_wide_t *>(h);
    info[0] = a->W; info[1] = a->nbits; info[2] = a->raw_bits; info[3] = a->plain;
    info[4] = a->nlut; info[5] = a->nassert; info[6] = a->implicit_any; info[7] = (int64_t) a->lds_bytes;
}

void wsim_valid(void *h, uint64_t *out)
{
    const sre_nfa_wide_t *a = static_cast<sre_nfa_wide_t *>(h);
    for (int i = 0; i < 4; i++) out[i] = a->valid[i];
}

/* out[0] = first event step (-1 none), out[1] = last clean position <= it (every position checked),
 * out[2] = how the event came: 0 a consumed byte (MATCH listed at out[0] + 1), 1 a look-ahead expansion (at out[0]) */
void wsim_run(void *h, const uint8_t *data, int64_t n, int variant, int64_t *out)
{
    const sre_nfa_wide_t *a = static_cast<sre_nfa_wide_t *>(h);
    Set S;
    memcpy(S.w, a->init[variant], sizeof(S.w));
    int64_t  clean = 0, ev = -1, how = -1;
    uint32_t prev = SRE_NFA_KIND_EDGE;
    uint64_t nany[4];
    for (int i = 0; i < 4; i++) nany[i] = ~a->any_bits[i];
    for (int64_t p = 0; p <= n; p++) {
        const uint32_t cur = p < n ? (a->kind[data[p]] & 3u) : (uint32_t) SRE_NFA_KIND_EDGE;
        expand(a, S, prev, cur);
        if (meets(a, S, a->match_bits)) {
            ev = p;
            how = 1;
            break;
        }
        if (p == n) break;
        const Set t = step(a, S, data[p]);
        if (meets(a, t, a->msrc)) {
            ev = p;
            how = 0;
            break;
        }
        if (!meets(a, t, nany)) clean = p + 1;
        prev = cur;
    }
    out[0] = ev;
    out[1] = clean;
    out[2] = how;
}

/* the set after walking the bytes from `in` (events ignored, as the exact-entry pass walks);
 * prev = the kind of the byte in front of the first one */
void wsim_walk_set(void *h, const uint64_t *in, const uint8_t *data, int64_t n, uint32_t prev, uint64_t *out)
{
    const sre_nfa_wide_t *a = static_cast<sre_nfa_wide_t *>(h);
    Set S;
    memcpy(S.w, in, sizeof(S.w));
    for (int64_t p = 0; p < n; p++) {
        const uint32_t cur = a->kind[data[p]] & 3u;
        expand(a, S, prev, cur);
        step(a, S, data[p]);
        prev = cur;
    }
    for (uint32_t i = 0; i < 4; i++) out[i] = i < a->W ? S.w[i] & a->valid[i] : 0;
}

}  // extern "C"
