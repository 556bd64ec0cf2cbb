/*
 * tests/lines_nfa_sim.cpp — TEST-ONLY host model of the short-line kernel of line mode on the NFA tier
 * (sregex_amd/csrc/sre_hip_lines_nfa.hip): the step of sre_lines_nfa.h — the text the kernel compiles —
 * walked over single lines, on the host tables of sre_nfa.cpp.  Compiled by tests/test_lines_nfa_model.py
 * into tests/_build/; not part of, nor linked into, the product library.
 */
#include "sre_nfa.h"
#include "sre_lines_nfa.h"
#include <stdint.h>
#include <vector>

namespace {

struct LineSim {
    sre_nfa_t            *nfa;
    sre_lnfa_t            form[2];      /* 0: plain slices, 1: shift-and */
    bool                  has[2];
    std::vector<uint64_t> follow;       /* padded to nslices x 256, as the device copy is */
};

}  // namespace

extern "C" {

void *lnsim_build(const sre_program_t *prog, unsigned sa_options, const char **why)
{
    sre_nfa_t *n = sre_nfa_build2(prog, sa_options, why);
    if (n == NULL) return NULL;
    LineSim *s = new LineSim();
    s->nfa = n;
    s->has[0] = true;
    s->has[1] = n->sa != NULL;
    /* the plain form: its assertion bits are the last byte slice (sre_hip_nfa.hip sre_k_nfa) */
    if (n->nassert && n->assert_slice != n->nslices - 1) {
        *why = "assertion slice is not the last one";
        sre_nfa_free(n);
        delete s;
        return NULL;
    }
    s->follow.assign((size_t) n->nslices * 256, 0);
    for (size_t i = 0; i < n->follow.size() && i < s->follow.size(); i++) s->follow[i] = n->follow[i];
    sre_lnfa_t &p = s->form[0];
    sre_lnfa_set_plain(p, n->nslices, n->nassert, n->init[0], n->match_bits);
    p.accept = n->accept;
    p.tab = s->follow.data();
    p.expand = n->expand.data();
    p.kind = n->kind;
    if (n->sa) {
        const sre_nfa_sa_t *a = n->sa;
        sre_lnfa_t         &q = s->form[1];
        /* the host table is indexed by the whole assertion byte: 256 entries a context */
        sre_lnfa_set_sa(q, a->w64, a->carry, a->masked, a->evacc, a->nlut, a->hot, a->init[0], a->seed, a->self, a->shift_src,
                        a->match_bits, a->msrc, a->nassert, a->assert_byte, 8);
        q.accept = a->accept;
        q.tab = a->lut.data();
        q.expand = a->expand.data();
        q.kind = n->kind;
    }
    return s;
}

void lnsim_free(void *h)
{
    LineSim *s = static_cast<LineSim *>(h);
    sre_nfa_free(s->nfa);
    delete s;
}

void *lnsim_nfa(void *h) { return static_cast<LineSim *>(h)->nfa; }

/* -1: the program has no such form; else bit 0 shift-and, bit 1 look-ahead, bit 2 events from the consumed set */
int lnsim_shape(void *h, int form)
{
    const LineSim *s = static_cast<LineSim *>(h);
    if (!s->has[form]) return -1;
    const sre_lnfa_t &t = s->form[form];
    return (t.sa ? 1 : 0) | (t.la ? 2 : 0) | (t.ev_t ? 4 : 0);
}

/* one line as the kernel's lane walks it: the position of the first event, -1 none */
int64_t lnsim_walk(void *h, int form, const uint8_t *data, int64_t n)
{
    const LineSim    *s = static_cast<LineSim *>(h);
    const sre_lnfa_t &t = s->form[form];
    sre_lnfa_lane_t   L;
    sre_lnfa_begin(t, L);
    for (int64_t p = 0; p < n; p++) {
        if (sre_lnfa_byte(t, L, data[p], p)) return L.ev;
    }
    sre_lnfa_end(t, L, n);
    return L.ev;
}

}
