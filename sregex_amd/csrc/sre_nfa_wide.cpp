/*
 * sre_nfa_wide.cpp — builds the wide bit-parallel form described in sre_nfa_wide.h.
 *
 * The rules are those of sre_nfa_build2 (sre_nfa.cpp): the closure mirrors sre_vm_pike.c:756-942 on
 * sets, a thread that can consume '\n' and whose closure differs with ^ true gets a newline twin, the
 * look-ahead assertions wait in the list and are decided by the expansion tables, the ".*?" thread is
 * the implicit seed, equivalent threads are merged.  Only the width (sets of any size, placed in up to
 * 256 bits) and the table form are new; the 64-bit form and its builder are left as they are.
 */
#include "sre_nfa_wide.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <set>

namespace {

/* a set of bits of any size */
struct Bits {
    std::vector<uint64_t> w;
    Bits() {}
    explicit Bits(size_t nbits) : w((nbits + 63) / 64, 0) {}
    void set(size_t i) { w[i >> 6] |= 1ull << (i & 63); }
    bool get(size_t i) const { return (i >> 6) < w.size() && ((w[i >> 6] >> (i & 63)) & 1); }
    bool any() const
    {
        for (uint64_t v : w) {
            if (v) return true;
        }
        return false;
    }
    bool meets(const Bits &o) const
    {
        for (size_t i = 0; i < w.size() && i < o.w.size(); i++) {
            if (w[i] & o.w[i]) return true;
        }
        return false;
    }
    Bits &operator|=(const Bits &o)
    {
        for (size_t i = 0; i < w.size() && i < o.w.size(); i++) w[i] |= o.w[i];
        return *this;
    }
    Bits minus(const Bits &o) const
    {
        Bits r = *this;
        for (size_t i = 0; i < r.w.size() && i < o.w.size(); i++) r.w[i] &= ~o.w[i];
        return r;
    }
};

struct WideBuilder {
    const sre_program_t *prog;

    bool consumes(const sre_insn_t &in, unsigned c) const
    {
        switch (in.opcode) {
        case SRE_OP_CHAR:  return c == in.ch;
        case SRE_OP_ANY:   return true;
        case SRE_OP_IN:    return sre_in_ranges(&prog->ranges[in.x], in.nranges, c) != 0;
        case SRE_OP_NOTIN: return sre_in_ranges(&prog->ranges[in.x], in.nranges, c) == 0;
        default:           return false;
        }
    }

    /* list-able instructions reachable from pc0 through epsilon edges (as sre_nfa.cpp) */
    void closure(uint32_t pc0, bool a_ok, bool caret_ok, std::set<uint32_t> &out) const
    {
        std::vector<uint32_t> stack(1, pc0);
        std::vector<uint8_t>  seen(prog->len + 1, 0);
        while (!stack.empty()) {
            uint32_t pc = stack.back();
            stack.pop_back();
            while (pc < prog->len && !seen[pc]) {
                seen[pc] = 1;
                const sre_insn_t &in = prog->insns[pc];
                if (in.opcode == SRE_OP_JMP) {
                    pc = in.x;
                } else if (in.opcode == SRE_OP_SPLIT) {
                    stack.push_back(in.y);
                    pc = in.x;
                } else if (in.opcode == SRE_OP_SAVE) {
                    pc++;
                } else if (in.opcode == SRE_OP_ASSERT && !(in.ch & SRE_ASSERT_LOOKAHEAD)) {
                    if (!(in.ch == SRE_ASSERT_BIG_A ? a_ok : caret_ok)) break;     /* :839-864 */
                    pc++;
                } else {
                    out.insert(pc);
                    break;
                }
            }
        }
    }
};

/* a merged thread of the wide form */
struct Node {
    Bits     fol;           /* successors over node ids (self excluded) */
    bool     self, to_match, is_any, is_assert, is_match;
    uint64_t acc[4];        /* bytes it consumes */
    int      next, prev;    /* the node one bit above / below (a link the shift serves) */
};

}  // namespace

extern "C" void
sre_nfa_wide_free(sre_nfa_wide_t *w)
{
    delete w;
}

extern "C" sre_nfa_wide_t *
sre_nfa_wide_build(const sre_program_t *prog, unsigned options, const char **why)
{
    static const char *dummy;
    if (why == NULL) why = &dummy;
    *why = NULL;
    if (prog->lookahead_asserts > 8) {
        *why = "more than 8 look-ahead assertions ($ \\z \\b \\B)";
        return NULL;
    }
    if (prog->len > 4096) {
        *why = "more than 4096 instructions";
        return NULL;
    }
    WideBuilder b;
    b.prog = prog;

    /* ---- pc-level follow sets, without and with ^ true (sre_nfa.cpp) */
    std::vector<std::set<uint32_t>> fol[2];
    fol[0].resize(prog->len);
    fol[1].resize(prog->len);
    std::vector<uint32_t> listable, asserts;
    for (uint32_t pc = 0; pc < prog->len; pc++) {
        const sre_insn_t &in = prog->insns[pc];
        switch (in.opcode) {
        case SRE_OP_CHAR: case SRE_OP_IN: case SRE_OP_NOTIN: case SRE_OP_ANY:
            b.closure(pc + 1, false, false, fol[0][pc]);
            b.closure(pc + 1, false, true, fol[1][pc]);
            listable.push_back(pc);
            break;
        case SRE_OP_MATCH:
            listable.push_back(pc);
            break;
        case SRE_OP_ASSERT:
            if (in.ch & SRE_ASSERT_LOOKAHEAD) asserts.push_back(pc);
            break;
        default:
            break;
        }
    }
    /* a look-ahead assertion inside a loop keeps the exact VM (sre_nfa.cpp) */
    for (uint32_t a : asserts) {
        std::vector<uint8_t>  seen(prog->len + 1, 0);
        std::vector<uint32_t> stack(1, a + 1);
        while (!stack.empty()) {
            const uint32_t pc = stack.back();
            stack.pop_back();
            if (pc >= prog->len || seen[pc]) continue;
            seen[pc] = 1;
            if (pc == a) {
                *why = "a look-ahead assertion inside a loop (the VM's generation tags decide what its splice lists)";
                return NULL;
            }
            const sre_insn_t &in = prog->insns[pc];
            if (in.opcode == SRE_OP_MATCH) continue;
            if (in.opcode == SRE_OP_JMP) {
                stack.push_back(in.x);
            } else if (in.opcode == SRE_OP_SPLIT) {
                stack.push_back(in.x);
                stack.push_back(in.y);
            } else {
                stack.push_back(pc + 1);
            }
        }
    }

    /* ---- the plain numbering ("raw" bits): pc 1 first, then program order with newline twins, then
     * the assertions */
    std::vector<int>      bit_of(prog->len, -1), twin_of(prog->len, -1);
    std::vector<uint32_t> bit_pc;
    auto needs_twin = [&](uint32_t pc) {
        const sre_insn_t &in = prog->insns[pc];
        if (in.opcode == SRE_OP_MATCH || !b.consumes(in, '\n') || fol[0][pc] == fol[1][pc]) return false;
        for (unsigned c = 0; c < 256; c++) {
            if (c != '\n' && b.consumes(in, c)) return true;
        }
        return false;
    };
    auto assign = [&](uint32_t pc) {
        if (bit_of[pc] >= 0) return;
        bit_of[pc] = (int) bit_pc.size();
        bit_pc.push_back(pc);
        if (needs_twin(pc)) {
            twin_of[pc] = (int) bit_pc.size();
            bit_pc.push_back(pc);
        }
    };
    if (prog->len > 1 && prog->insns[1].opcode == SRE_OP_ANY) assign(1);
    for (uint32_t pc : listable) assign(pc);
    const uint32_t nassert = (uint32_t) asserts.size();
    for (uint32_t pc : asserts) {
        bit_of[pc] = (int) bit_pc.size();
        bit_pc.push_back(pc);
    }
    const size_t nraw = bit_pc.size();
    auto mask_of = [&](const std::set<uint32_t> &pcs) {
        Bits m(nraw);
        for (uint32_t pc : pcs) {
            m.set((size_t) bit_of[pc]);
            if (twin_of[pc] >= 0) m.set((size_t) twin_of[pc]);
        }
        return m;
    };
    Bits any_raw(nraw), match_raw(nraw), assert_raw(nraw);
    if (bit_of.size() > 1 && bit_of[1] >= 0) {
        any_raw.set((size_t) bit_of[1]);
        if (twin_of[1] >= 0) any_raw.set((size_t) twin_of[1]);
    }
    for (uint32_t pc : asserts) assert_raw.set((size_t) bit_of[pc]);
    std::vector<Bits>     fbit(nraw, Bits(nraw));
    std::vector<uint64_t> A(nraw * 4, 0);      /* bytes each raw bit consumes */
    for (uint32_t pc : listable) {
        const sre_insn_t &in = prog->insns[pc];
        if (in.opcode == SRE_OP_MATCH) {
            match_raw.set((size_t) bit_of[pc]);
            continue;
        }
        bool only_nl = b.consumes(in, '\n');
        for (unsigned c = 0; c < 256; c++) {
            if (!b.consumes(in, c)) continue;
            if (c != '\n') only_nl = false;
            const int bit = (twin_of[pc] >= 0 && c == '\n') ? twin_of[pc] : bit_of[pc];
            A[(size_t) bit * 4 + (c >> 6)] |= 1ull << (c & 63);
        }
        fbit[bit_of[pc]] = mask_of(fol[only_nl ? 1 : 0][pc]);
        if (twin_of[pc] >= 0) fbit[twin_of[pc]] = mask_of(fol[1][pc]);
    }
    Bits init_raw[3];
    for (int v = 0; v < 3; v++) {
        std::set<uint32_t> s;
        b.closure(0, v == 0, v != 2, s);
        init_raw[v] = mask_of(s);
    }
    if (init_raw[0].meets(match_raw)) {
        *why = "nullable regex: the first match event is at offset 0, nothing to skip";
        return NULL;
    }

    sre_nfa_wide_t *n = new sre_nfa_wide_t();
    n->raw_bits = (uint32_t) nraw;
    n->nassert = nassert;
    for (unsigned c = 0; c < 256; c++) {
        uint8_t k = sre_isword(c) ? SRE_NFA_KIND_WORD : c == '\n' ? SRE_NFA_KIND_NL : SRE_NFA_KIND_OTHER;
        bool    lead = false;
        if (prog->leading_byte != -1) lead = (int) c == prog->leading_byte;
        for (uint32_t i = 0; !lead && prog->leading_byte == -1 && i < prog->nleading; i++) {
            lead = b.consumes(prog->insns[prog->leading_insns[i]], c);
        }
        n->kind[c] = (uint8_t) (k | (lead ? SRE_NFA_LEADING : 0u));
    }
    /* ---- the expansion of every assertion per context, transitively closed (sre_nfa.cpp) */
    std::vector<Bits> xraw((size_t) 16 * nassert, Bits(nraw));
    for (uint32_t prev = 0; prev < 4 && nassert; prev++) {
        for (uint32_t cur = 0; cur < 4; cur++) {
            const bool prev_word = prev == SRE_NFA_KIND_WORD, cur_word = cur == SRE_NFA_KIND_WORD;
            const bool at_start = prev == SRE_NFA_KIND_EDGE, at_end = cur == SRE_NFA_KIND_EDGE;
            auto holds = [&](uint8_t ch) {
                switch (ch) {                                   /* :450-497 */
                case SRE_ASSERT_SMALL_Z: return at_end;
                case SRE_ASSERT_DOLLAR:  return at_end || cur == SRE_NFA_KIND_NL;
                case SRE_ASSERT_SMALL_B: return prev_word != cur_word;
                case SRE_ASSERT_BIG_B:   return prev_word == cur_word;
                default:                 return false;
                }
            };
            for (uint32_t i = 0; i < nassert; i++) {
                if (!holds(prog->insns[asserts[i]].ch)) continue;
                std::set<uint32_t> acc, todo, done;
                todo.insert(asserts[i]);
                while (!todo.empty()) {
                    const uint32_t a = *todo.begin();
                    todo.erase(todo.begin());
                    if (!done.insert(a).second) continue;
                    std::set<uint32_t> cl;
                    b.closure(a + 1, at_start, at_start || prev == SRE_NFA_KIND_NL, cl);     /* :506-526 */
                    for (uint32_t pc : cl) {
                        acc.insert(pc);
                        const sre_insn_t &in = prog->insns[pc];
                        if (in.opcode == SRE_OP_ASSERT && holds(in.ch)) todo.insert(pc);
                    }
                }
                xraw[(size_t) (prev * 4 + cur) * nassert + i] = mask_of(acc);
            }
        }
    }

    /* ---- the ".*?" thread stays implicit when it is one bit, always listed, lists itself and not MATCH */
    int  any_bit = -1;
    int  nany = 0;
    for (size_t i = 0; i < nraw; i++) {
        if (any_raw.get(i)) {
            if (any_bit < 0) any_bit = (int) i;
            nany++;
        }
    }
    bool implicit_any = nany == 1 && !(options & SRE_NFA_WIDE_EXPLICIT_ANY);
    if (implicit_any) {
        for (int v = 0; v < 3; v++) implicit_any = implicit_any && init_raw[v].get((size_t) any_bit);
        implicit_any = implicit_any && fbit[any_bit].get((size_t) any_bit) && !fbit[any_bit].meets(match_raw);
        for (unsigned c = 0; c < 256; c++) implicit_any = implicit_any && ((A[(size_t) any_bit * 4 + (c >> 6)] >> (c & 63)) & 1);
    }
    n->implicit_any = implicit_any;

    /* ---- classes of equivalent threads: same follow set, same MATCH reach, listed by the same sets.  Merging
     * two such threads changes no other pair's equality (their columns are equal), so one grouping is the
     * fixed point of the 64-bit builder's pairwise loop. */
    std::vector<Bits> roots = {init_raw[0], init_raw[1], init_raw[2]};
    if (implicit_any) roots.push_back(fbit[any_bit]);
    for (const Bits &x : xraw) roots.push_back(x);
    std::vector<uint8_t> live(nraw, 0);
    for (size_t i = 0; i < nraw; i++) live[i] = !match_raw.get(i) && !(implicit_any && (int) i == any_bit);
    std::vector<int> rep(nraw, -1);
    {
        std::map<std::vector<uint64_t>, int> cls;
        for (size_t i = 0; i < nraw; i++) {
            if (!live[i]) continue;
            if ((options & SRE_NFA_WIDE_NO_MERGE) || any_raw.get(i) || assert_raw.get(i)) {
                rep[i] = (int) i;
                continue;
            }
            std::vector<uint64_t> key = fbit[i].minus(match_raw).w;
            key.push_back(fbit[i].meets(match_raw) ? 1 : 0);
            Bits col(nraw + roots.size());
            for (size_t k = 0; k < nraw; k++) {
                if (fbit[k].get(i)) col.set(k);
            }
            for (size_t r = 0; r < roots.size(); r++) {
                if (roots[r].get(i)) col.set(nraw + r);
            }
            key.insert(key.end(), col.w.begin(), col.w.end());
            auto it = cls.find(key);
            if (it == cls.end()) {
                cls[key] = (int) i;
                rep[i] = (int) i;
            } else {
                rep[i] = it->second;
            }
        }
    }

    /* ---- nodes: the assertions first (bits 0 .. of word 0), then every class */
    std::vector<Node> nd;
    std::vector<int>  node_of(nraw, -1);
    auto new_node = [&]() {
        Node x;
        x.self = x.to_match = x.is_any = x.is_assert = x.is_match = false;
        memset(x.acc, 0, sizeof(x.acc));
        x.next = x.prev = -1;
        nd.push_back(x);
        return (int) nd.size() - 1;
    };
    for (size_t i = 0; i < nraw; i++) {
        if (live[i] && assert_raw.get(i)) {
            node_of[i] = new_node();
            nd[node_of[i]].is_assert = true;
        }
    }
    for (size_t i = 0; i < nraw; i++) {
        if (!live[i] || assert_raw.get(i)) continue;
        if (rep[i] == (int) i) {
            node_of[i] = new_node();
            nd[node_of[i]].is_any = any_raw.get(i);
            nd[node_of[i]].to_match = fbit[i].meets(match_raw);
        }
    }
    for (size_t i = 0; i < nraw; i++) {
        if (live[i] && rep[i] != (int) i && rep[i] >= 0) node_of[i] = node_of[rep[i]];
        if (live[i] && node_of[i] >= 0) {
            for (int q = 0; q < 4; q++) nd[node_of[i]].acc[q] |= A[i * 4 + q];
        }
    }
    /* an expansion that lists MATCH is an event at its position: one bit that no byte accepts */
    bool exp_match = false;
    for (const Bits &x : xraw) exp_match = exp_match || x.meets(match_raw);
    int match_node = -1;
    if (exp_match) {
        match_node = new_node();
        nd[match_node].is_match = true;
    }
    const size_t nn = nd.size();
    if (nn > 64 * SRE_NFA_WIDE_MAX_WORDS) {
        *why = "more than 256 thread bits after merging (threads, newline twins, assertions)";
        delete n;
        return NULL;
    }
    auto to_nodes = [&](const Bits &raw) {
        Bits m(nn);
        for (size_t i = 0; i < nraw; i++) {
            if (raw.get(i) && live[i] && node_of[i] >= 0) m.set((size_t) node_of[i]);
        }
        if (match_node >= 0 && raw.meets(match_raw)) m.set((size_t) match_node);
        return m;
    };
    for (size_t i = 0; i < nraw; i++) {
        if (!live[i] || rep[i] != (int) i) continue;
        const int v = node_of[i];
        Bits f = to_nodes(fbit[i].minus(match_raw));
        nd[v].self = f.get((size_t) v);
        if (nd[v].self) f.w[(size_t) v >> 6] &= ~(1ull << (v & 63));
        nd[v].fol = f;
    }
    for (size_t v = 0; v < nn; v++) {
        if (nd[v].fol.w.empty()) nd[v].fol = Bits(nn);
    }

    /* ---- links: a thread with ONE successor first (it then needs no lookup at all) */
    const bool plain = (options & SRE_NFA_WIDE_PLAIN) != 0;
    auto reaches = [&](int from, int target) {
        for (int k = from; k >= 0; k = nd[k].next) {
            if (k == target) return true;
        }
        return false;
    };
    auto popc = [](const Bits &x) {
        int c = 0;
        for (uint64_t v : x.w) c += __builtin_popcountll(v);
        return c;
    };
    for (int pass = 0; pass < 2 && !plain; pass++) {
        for (size_t v = 0; v < nn; v++) {
            if (nd[v].next >= 0 || !nd[v].fol.any()) continue;
            if (pass == 0 && popc(nd[v].fol) != 1) continue;
            for (size_t w = 0; w < nn; w++) {
                if (!nd[v].fol.get(w) || nd[w].prev >= 0 || nd[w].is_assert || nd[w].is_match || reaches((int) w, (int) v)) continue;
                nd[v].next = (int) w;
                nd[w].prev = (int) v;
                break;
            }
        }
    }
    std::vector<uint8_t> is_src(nn, 0);
    for (size_t v = 0; v < nn; v++) {
        Bits rest = nd[v].fol;
        if (nd[v].next >= 0) rest.w[(size_t) nd[v].next >> 6] &= ~(1ull << (nd[v].next & 63));
        is_src[v] = rest.any();
    }
    std::vector<std::vector<int>> chains;
    for (size_t v = 0; v < nn; v++) {
        if (nd[v].prev >= 0 || nd[v].is_assert) continue;
        std::vector<int> c;
        for (int k = (int) v; k >= 0; k = nd[k].next) c.push_back(k);
        chains.push_back(c);
    }

    /* ---- placement: the assertions at bits 0 .., then the chains one behind the other (the shift
     * carries across words, so a chain may straddle them); the order is searched for the fewest bytes
     * that hold a source */
    const size_t     nc = chains.size();
    std::vector<int> best_pos;
    uint32_t         best_hot = 0;
    int              best_n = 1 << 30;
    {
        std::vector<size_t> order(nc);
        std::vector<int>    nsrc(nc, 0);
        for (size_t i = 0; i < nc; i++) {
            order[i] = i;
            for (int v : chains[i]) nsrc[i] += is_src[v];
        }
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t c) {
            if ((nsrc[a] > 0) != (nsrc[c] > 0)) return nsrc[a] > 0;
            return (uint64_t) nsrc[a] * chains[c].size() > (uint64_t) nsrc[c] * chains[a].size();
        });
        uint64_t rng = 0x9e3779b97f4a7c15ull;
        auto     rnd = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
        for (int attempt = 0; attempt < 300; attempt++) {
            if (attempt) {
                const int swaps = attempt < 150 ? 1 + (int) (rnd() % 3) : (int) nc;
                for (int k = 0; k < swaps && nc > 1; k++) std::swap(order[rnd() % nc], order[rnd() % nc]);
            }
            std::vector<int> pos(nn, -1);
            uint32_t         at = 0;
            for (size_t v = 0; v < nn; v++) {
                if (nd[v].is_assert) pos[v] = (int) at++;
            }
            for (size_t ci = 0; ci < nc; ci++) {
                for (int v : chains[order[ci]]) pos[v] = (int) at++;
            }
            uint32_t hot = 0;
            for (size_t v = 0; v < nn; v++) {
                if (is_src[v]) hot |= 1u << (pos[v] >> 3);
            }
            const int nh = __builtin_popcount(hot);
            if (nh < best_n) {
                best_n = nh;
                best_hot = hot;
                best_pos = pos;
            }
            if (nh <= 1 || plain) break;
        }
    }
    uint32_t W = nn <= 64 ? 1u : nn <= 128 ? 2u : 4u;
    if ((options & SRE_NFA_WIDE_MIN_W2) && W < 2) W = 2;
    if (options & SRE_NFA_WIDE_MIN_W4) W = 4;
    n->W = W;
    n->nbits = (uint32_t) nn;
    n->plain = plain;
    n->nlut = (uint32_t) best_n;
    if (n->nlut > SRE_NFA_WIDE_MAX_LUT || sre_nfa_wide_lds(W, n->nlut, nassert) > SRE_NFA_WIDE_LDS_BUDGET) {
        *why = "the wide form's lookup tables do not fit the LDS budget (too many bytes of the mask hold threads "
               "the shift does not serve)";
        delete n;
        return NULL;
    }
    n->lds_bytes = sre_nfa_wide_lds(W, n->nlut, nassert);
    uint32_t k = 0;
    for (uint32_t by = 0; by < 32; by++) {
        if (best_hot & (1u << by)) n->hot[k++] = by;
    }
    for (; k < SRE_NFA_WIDE_MAX_LUT; k++) n->hot[k] = 0;

    /* ---- tables */
    const std::vector<int> &pos = best_pos;
    auto setb = [](uint64_t *m, int bit) { m[bit >> 6] |= 1ull << (bit & 63); };
    auto bits_of = [&](const Bits &nodes, uint64_t *m) {
        for (size_t v = 0; v < nn; v++) {
            if (nodes.get(v)) setb(m, pos[v]);
        }
    };
    memset(n->init, 0, sizeof(n->init));
    memset(n->seed, 0, sizeof(n->seed));
    memset(n->any_bits, 0, sizeof(n->any_bits));
    memset(n->match_bits, 0, sizeof(n->match_bits));
    memset(n->msrc, 0, sizeof(n->msrc));
    memset(n->valid, 0, sizeof(n->valid));
    memset(n->self, 0, sizeof(n->self));
    memset(n->shift_src, 0, sizeof(n->shift_src));
    memset(n->accept, 0, sizeof(n->accept));
    for (int v = 0; v < 3; v++) bits_of(to_nodes(init_raw[v]), n->init[v]);
    if (implicit_any) bits_of(to_nodes(fbit[any_bit].minus(match_raw)), n->seed);
    for (size_t v = 0; v < nn; v++) {
        const int p = pos[v];
        setb(n->valid, p);
        if (nd[v].self) setb(n->self, p);
        if (nd[v].next >= 0) setb(n->shift_src, p);
        if (nd[v].is_any) setb(n->any_bits, p);
        if (nd[v].is_match) setb(n->match_bits, p);
        if (nd[v].to_match) setb(n->msrc, p);
        for (unsigned c = 0; c < 256; c++) {
            if ((nd[v].acc[c >> 6] >> (c & 63)) & 1) setb(n->accept[c], p);
        }
    }
    n->lut.assign((size_t) n->nlut * 256 * W, 0);
    for (uint32_t q = 0; q < n->nlut; q++) {
        for (size_t v = 0; v < nn; v++) {
            if ((uint32_t) (pos[v] >> 3) != n->hot[q] || !is_src[v]) continue;
            Bits rest = nd[v].fol;
            if (nd[v].next >= 0) rest.w[(size_t) nd[v].next >> 6] &= ~(1ull << (nd[v].next & 63));
            uint64_t m[4] = {0, 0, 0, 0};
            bits_of(rest, m);
            for (uint32_t x = 0; x < 256; x++) {
                if (!((x >> (pos[v] & 7)) & 1)) continue;
                for (uint32_t i = 0; i < W; i++) n->lut[((size_t) q * 256 + x) * W + i] |= m[i];
            }
        }
    }
    if (nassert) {
        const size_t per = (size_t) 1 << nassert;
        n->expand.assign(16 * per * W, 0);
        for (uint32_t ctx = 0; ctx < 16; ctx++) {
            for (uint32_t j = 0; j < nassert; j++) {
                uint64_t m[4] = {0, 0, 0, 0};
                bits_of(to_nodes(xraw[(size_t) ctx * nassert + j]), m);
                /* assertion j of the program sits at bit pos[node of it] (< nassert) */
                const int ab = pos[node_of[bit_of[asserts[j]]]];
                for (size_t x = 0; x < per; x++) {
                    if (!((x >> ab) & 1)) continue;
                    for (uint32_t i = 0; i < W; i++) n->expand[((size_t) ctx * per + x) * W + i] |= m[i];
                }
            }
        }
    }
    return n;
}
