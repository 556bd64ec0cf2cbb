/*
 * sre_lines_tally.h — the rules of the line tally (sre_hip_tally_lines): the hash of a line's key,
 * when two lines have the same key, the insert of a line into the table of keys one atomic at a time, and what a wave
 * adds to the counts.  The kernels (sre_hip_lines_tally.hip) and the CPU model (tests/lines_tally_sim.cpp) compile this
 * text; nothing here touches memory except through the Keys and Mem arguments.
 *
 * The KEY of a selected line is the tuple of its K field texts as the extract's select pass left them: entry
 * e = line * K + f has val[e] = field length + 1 (0: the line is not selected) and start[e] = the field's source offset
 * under the flag bits of sre_lines_gather.h.  Keys:
 *   keys.k                  fields per line
 *   keys.selected(line)     val[line * K] != 0
 *   keys.len(line, f)       val[e] - 1
 *   keys.byte(line, f, j)   byte j of the field
 * Two lines have the same key when every field has the same length and the same bytes; the hash mixes every length in,
 * so ("ab", "c") and ("a", "bc") differ in their hashes as a rule and in the comparison always.
 *
 * The TABLE has nslots words (a power of two).  A word is SRE_LT_EMPTY or a LINE NUMBER: the line that currently stands
 * for the key of that slot.  The fields of every line were written before the insert began, so whoever reads a word
 * compares against a line of the slot's key, whichever line that is at the time.  A word only ever goes from EMPTY to
 * a line and from a line to a lower line of the same key: a slot never empties and never changes its key, so a key
 * cannot land in two slots, and the final word is the key's lowest line whatever the order of arrival.  Mem:
 *   mem.cas(idx, expect, v) atomic compare-and-swap of word idx, returns what the word held
 *   mem.min(idx, v)         atomic minimum into word idx
 *   mem.raised()            atomic load of the overflow flag
 * One call of sre_lt_step makes at most ONE of these accesses and at most one look at the flag, so a model can
 * interleave lanes at every point at which the hardware can.
 *
 * Only one lane per key of a WAVE goes to the table.  The 64 lines of a wave are grouped first by the route's wave rule
 * (sre_lines_route.h) on the keys: lowest remaining lane, ballot of the lanes with its key (sre_lt_same_key: the hashes,
 * then the fields), drop them; one turn per distinct key of the wave.  The lowest lane of a group LEADS it: it holds the
 * group's lowest line, searches the table for all of them and hands them its slot.  A buffer in which every line has
 * the same key then sends one lane per wave to the one word, not a million.
 *
 * After its search a leader knows its slot (SRE_LT_NONE: stopped on overflow) and whether it CLAIMED it (its CAS found
 * EMPTY).  The wave then settles: one add of its selected lines, one returning add of its claims (the flag goes up
 * when the claims pass max_keys, sre_lt_claims_overflow), and per leader ONE add of its group's size to the count of
 * its slot: an add per distinct slot of the wave, since the keys of two leaders of a wave differ.
 */
#ifndef SRE_LINES_TALLY_H
#define SRE_LINES_TALLY_H

#include <stdint.h>
#include "sre_lines_gather.h"
#include "sre_lines_route.h"

#define SRE_LT_THREADS      256u
#define SRE_LT_EMPTY        (~(uint64_t) 0)
#define SRE_LT_NONE         (~(uint32_t) 0)
#define SRE_LT_MIN_SLOTS    1024u
#define SRE_LT_MAX_KEYS     ((uint64_t) 1 << 30)
/* a lane looks at the overflow flag before its first probe and then every SRE_LT_FLAG_EVERY probes */
#define SRE_LT_FLAG_EVERY   32u

typedef struct {
    uint64_t nslots;        /* power of two, >= 2 * max_keys, >= SRE_LT_MIN_SLOTS */
    uint64_t max_keys;
    uint64_t hash_mask;     /* all ones; SRE_HIP_TALLY_HASH_BITS = n leaves the low n bits (test knob) */
} sre_lt_params_t;

/* slots of a table for max_keys keys: load factor at most 1/2 */
SRE_LG_FN uint64_t
sre_lt_nslots(uint64_t max_keys)
{
    uint64_t s = SRE_LT_MIN_SLOTS;
    while (s < 2 * max_keys) s <<= 1;
    return s;
}

SRE_LG_FN uint64_t
sre_lt_hash_mask(int bits)
{
    return bits >= 64 ? ~(uint64_t) 0 : bits <= 0 ? 0 : (((uint64_t) 1 << bits) - 1);
}

SRE_LG_FN uint64_t
sre_lt_mix(uint64_t h)
{
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 29;
    return h;
}

/* the hash of a line's key: per field its length mixed in, then its bytes (FNV-1a steps), mixed once more at the end */
template <class Keys>
SRE_LG_FN uint64_t
sre_lt_hash(const Keys &keys, uint64_t line)
{
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint32_t f = 0; f < keys.k; f++) {
        const uint64_t len = keys.len(line, f);
        h = sre_lt_mix(h ^ (len + 0x9E3779B97F4A7C15ull));
        for (uint64_t j = 0; j < len; j++) h = (h ^ keys.byte(line, f, j)) * 0x100000001B3ull;
    }
    return sre_lt_mix(h);
}

/* field by field, lengths first */
template <class Keys>
SRE_LG_FN bool
sre_lt_equal(const Keys &keys, uint64_t a, uint64_t b)
{
    for (uint32_t f = 0; f < keys.k; f++) {
        if (keys.len(a, f) != keys.len(b, f)) return false;
    }
    for (uint32_t f = 0; f < keys.k; f++) {
        const uint64_t len = keys.len(a, f);
        for (uint64_t j = 0; j < len; j++) {
            if (keys.byte(a, f, j) != keys.byte(b, f, j)) return false;
        }
    }
    return true;
}

/* where the search of a hash begins */
SRE_LG_FN uint64_t
sre_lt_home(uint64_t hash, const sre_lt_params_t &p)
{
    return (hash & p.hash_mask) & (p.nslots - 1);
}

enum { SRE_LT_PROBE = 0, SRE_LT_LOWER = 1, SRE_LT_DONE = 2 };

typedef struct {
    uint64_t line;
    uint64_t idx;           /* the word the next access goes to */
    uint64_t probes;        /* words seen so far */
    uint32_t state;
    uint32_t slot;          /* DONE: the line's slot, or SRE_LT_NONE */
    bool     claimed;       /* DONE: this lane's CAS took the slot from EMPTY */
    bool     wrapped;       /* DONE: the search went round the table (the wave raises the flag) */
} sre_lt_lane_t;

/* the wave rule's test: does the line (hash h) belong to the group of the leading line (hash lead_h)? */
template <class Keys>
SRE_LG_FN bool
sre_lt_same_key(const Keys &keys, uint64_t h, uint64_t line, uint64_t lead_h, uint64_t lead_line)
{
    return h == lead_h && (line == lead_line || sre_lt_equal(keys, line, lead_line));
}

/* a lane begins: only the leader of a group searches; every other lane is done at once, without a slot of its own */
SRE_LG_FN void
sre_lt_begin(sre_lt_lane_t &L, uint64_t line, bool leads, uint64_t hash, const sre_lt_params_t &p)
{
    L.line = line;
    L.probes = 0;
    L.claimed = false;
    L.wrapped = false;
    L.slot = SRE_LT_NONE;
    L.idx = leads ? sre_lt_home(hash, p) : 0;
    L.state = leads ? SRE_LT_PROBE : SRE_LT_DONE;
}

SRE_LG_FN bool sre_lt_done(const sre_lt_lane_t &L) { return L.state == SRE_LT_DONE; }

/* one step of a lane that is not done: at most one access to the table */
template <class Keys, class Mem>
SRE_LG_FN void
sre_lt_step(sre_lt_lane_t &L, const Keys &keys, Mem &mem, const sre_lt_params_t &p)
{
    if (L.state == SRE_LT_LOWER) {
        /* the slot holds a higher line of this key, or did when the CAS looked */
        mem.min(L.idx, L.line);
        L.slot = (uint32_t) L.idx;
        L.state = SRE_LT_DONE;
        return;
    }
    if (L.probes % SRE_LT_FLAG_EVERY == 0 && mem.raised()) {
        L.state = SRE_LT_DONE;          /* the call has overflowed: nothing of it will be delivered */
        return;
    }
    if (L.probes == p.nslots) {
        L.wrapped = true;               /* every word holds another key */
        L.state = SRE_LT_DONE;
        return;
    }
    const uint64_t old = mem.cas(L.idx, SRE_LT_EMPTY, L.line);
    if (old == SRE_LT_EMPTY) {
        L.claimed = true;
        L.slot = (uint32_t) L.idx;
        L.state = SRE_LT_DONE;
    } else if (sre_lt_equal(keys, L.line, old)) {
        /* the word only falls: below this line already, it stays there and no minimum is needed */
        if (old < L.line) {
            L.slot = (uint32_t) L.idx;
            L.state = SRE_LT_DONE;
        } else {
            L.state = SRE_LT_LOWER;
        }
    } else {
        L.idx = (L.idx + 1) & (p.nslots - 1);
        L.probes++;
    }
}

/* the wave's claims: `base` claims were made before this wave's `mine`; true when the flag has to go up */
SRE_LG_FN bool
sre_lt_claims_overflow(uint64_t base, uint32_t mine, const sre_lt_params_t &p)
{
    return base + mine > p.max_keys;
}

/* keep: an entry of a line with a slot stays selected only when the line is the slot's final word */
SRE_LG_FN bool
sre_lt_keeps(uint32_t slot, uint64_t line, const uint64_t *tab)
{
    return slot != SRE_LT_NONE && tab[slot] == line;
}

#endif
