/*
 * tests/streams_nfa_sim.cpp — TEST-ONLY host model of a stream of a stream set on the bit-parallel NFA
 * tier: the rule of one call (sregex_amd/csrc/sre_streams_nfa.h, the text the device tail compiles)
 * around a sequential walk of the thread set over the chunk — by the plain slices, the shift-and form or
 * the wide form, stepped as tests/nfa_sim.cpp and tests/nfa_wide_sim.cpp step them.  Compiled by
 * tests/test_streams_nfa_model.py into tests/_build/; not part of, nor linked into, the product library.
 */
#include "sre_nfa.h"
#include "sre_nfa_wide.h"
#include "sre_streams_nfa.h"
#include <string.h>
#include <stdint.h>

namespace {

enum { KIND_PLAIN = 0, KIND_SA = 1, KIND_WIDE = 2 };

struct Form {
    int             kind;
    sre_nfa_t      *nfa;
    sre_nfa_wide_t *wide;
};

inline uint32_t
words(const Form *f)
{
    return f->kind == KIND_WIDE ? f->wide->W : 1u;
}

/* The walk of one chunk from the set S: the position of the first step that reaches MATCH (-1: none),
 * S = the set behind the last byte (as the kernels store it: valid bits only). */
int64_t
walk(const Form *f, uint64_t *S, const uint8_t *data, int64_t n)
{
    if (f->kind == KIND_PLAIN) {
        const sre_nfa_t *a = f->nfa;
        for (int64_t p = 0; p < n; p++) {
            const uint64_t t = S[0] & a->accept[data[p]];
            uint64_t       r = 0;
            for (uint32_t k = 0; k < a->nslices; k++) r |= a->follow[(size_t) k * 256 + ((t >> (8 * k)) & 0xff)];
            S[0] = r;
            if (r & a->match_bits) return p;
        }
        return -1;
    }
    if (f->kind == KIND_SA) {
        const sre_nfa_sa_t *a = f->nfa->sa;
        for (int64_t p = 0; p < n; p++) {
            const uint64_t t = S[0] & a->accept[data[p]];
            const uint64_t ts = a->masked ? t & a->shift_src : t;
            uint64_t       sh;
            if (!a->w64) sh = (uint64_t) (uint32_t) ((uint32_t) ts << 1);
            else if (a->carry) sh = ts << 1;
            else sh = ((uint64_t) (uint32_t) ((uint32_t) (ts >> 32) << 1) << 32) | (uint32_t) ((uint32_t) ts << 1);
            uint64_t r = sh | (t & a->self) | a->seed;
            for (uint32_t k = 0; k < a->nlut; k++) r |= a->lut[(size_t) k * 256 + ((t >> (8 * a->hot[k])) & 0xff)];
            S[0] = r;
            if (a->evacc ? (t & a->msrc) != 0 : (r & a->match_bits) != 0) return p;
        }
        S[0] &= a->valid;
        return -1;
    }
    const sre_nfa_wide_t *a = f->wide;
    for (int64_t p = 0; p < n; p++) {
        uint64_t t[4], r[4], ev = 0;
        for (uint32_t i = 0; i < a->W; i++) t[i] = S[i] & a->accept[data[p]][i];
        for (uint32_t i = 0; i < a->W; i++) {
            const uint64_t ts = t[i] & a->shift_src[i];
            const uint64_t below = i ? (t[i - 1] & a->shift_src[i - 1]) >> 63 : 0;
            r[i] = (ts << 1) | below | (t[i] & a->self[i]) | a->seed[i];
            ev |= t[i] & a->msrc[i];
        }
        for (uint32_t k = 0; k < a->nlut; k++) {
            const uint32_t x = (uint32_t) (t[a->hot[k] >> 3] >> (8 * (a->hot[k] & 7))) & 0xffu;
            for (uint32_t i = 0; i < a->W; i++) r[i] |= a->lut[((size_t) k * 256 + x) * a->W + i];
        }
        for (uint32_t i = 0; i < a->W; i++) S[i] = r[i];
        if (ev) return p;
    }
    for (uint32_t i = 0; i < a->W; i++) S[i] &= a->valid[i];
    return -1;
}

}  // namespace

extern "C" {

/* kind 0: the plain slices, 1: the shift-and form under `options` (SRE_NFA_SA_*), 2: the wide form under
 * `options` (sre_nfa_wide.h).  NULL + *why when the program has no such form or has look-ahead assertions. */
void *snsim_build(const sre_program_t *prog, int kind, unsigned options, const char **why)
{
    static const char *dummy;
    if (why == NULL) why = &dummy;
    *why = NULL;
    Form *f = new Form();
    f->kind = kind;
    if (kind == KIND_WIDE) {
        f->wide = sre_nfa_wide_build(prog, options, why);
        if (f->wide && f->wide->nassert) {
            *why = "look-ahead assertions";
            sre_nfa_wide_free(f->wide);
            f->wide = NULL;
        }
    } else {
        f->nfa = sre_nfa_build2(prog, kind == KIND_PLAIN ? (unsigned) SRE_NFA_SA_OFF : options, why);
        if (f->nfa && (f->nfa->nassert || (kind == KIND_SA && f->nfa->sa == NULL))) {
            *why = f->nfa->nassert ? "look-ahead assertions" : "no shift-and form";
            sre_nfa_free(f->nfa);
            f->nfa = NULL;
        }
    }
    if (f->nfa == NULL && f->wide == NULL) {
        delete f;
        return NULL;
    }
    return f;
}

void snsim_free(void *h)
{
    Form *f = static_cast<Form *>(h);
    sre_nfa_free(f->nfa);
    sre_nfa_wide_free(f->wide);
    delete f;
}

int snsim_words(void *h) { return (int) words(static_cast<Form *>(h)); }

/* One call on the context row[0 .. 1 + W) (zeros: a fresh stream).  out[0] = rc, out[1] = state
 * (SRE_SNFA_OPEN ..), out[2] = bytes of the chunk the call looked at. */
void snsim_call(void *h, uint64_t *row, const uint8_t *data, int64_t len, int eof, int fed, int64_t *out)
{
    const Form    *f = static_cast<Form *>(h);
    const uint32_t W = words(f);
    uint64_t       S[4] = {0, 0, 0, 0};
    int64_t        ev = -1, looked = 0;
    bool           empty = true;
    if (sre_streams_nfa_scans(row[0], fed)) {
        for (uint32_t i = 0; i < W; i++) {
            if (row[0] & SRE_SNFA_STARTED) S[i] = row[1 + i];
            else S[i] = f->kind == KIND_WIDE ? f->wide->init[0][i] : f->kind == KIND_SA ? f->nfa->sa->init[0] : f->nfa->init[0];
        }
        ev = walk(f, S, data, len);
        looked = ev >= 0 ? ev + 1 : len;
        for (uint32_t i = 0; i < W; i++) empty = empty && S[i] == 0;
    }
    const sre_snfa_step_t r = sre_streams_nfa_rule(row[0], fed, (uint64_t) len, eof, ev, empty);
    if (!r.keep_set) {
        for (uint32_t i = 0; i < W; i++) row[1 + i] = S[i];
    }
    row[0] = r.flags;
    out[0] = r.rc;
    out[1] = r.state;
    out[2] = looked;
}

}  // extern "C"
