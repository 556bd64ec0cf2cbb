/*
 * scan_record_sim.cpp — the pack / load rule of a scan lane's record (sregex_amd/csrc/sre_scan_record.h) on the CPU:
 * for random records, records that are plain, and records that differ from a plain one in exactly one field,
 *   - load(pack(x)) gives x back field by field, whatever stale bytes the summary buffer holds behind a plain digest;
 *   - a record is called plain only if the record rebuilt from its digest equals it, and then nothing is stored;
 *   - the digest's bits are what the chain check reads of a record.
 * usage: scan_record_sim SEED CASES      prints "ok cases=N plain=P one_field=F full=U", exit status 1 on a mismatch
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sre_scan_record.h"

static std::mt19937_64 rng;

static uint32_t r32() { return (uint32_t) rng(); }
static int64_t  rpos() { return (rng() & 3) == 0 ? -1 : (int64_t) (rng() % (1ull << 33)); }

static sre_seg_summary_t
random_record(uint32_t seg_len)
{
    sre_seg_summary_t x;
    x.s_in = (rng() & 15) == 0 ? 0xffffffffu : r32() % 62;
    x.s_out = (rng() & 1) ? x.s_in : r32() % 62;
    x.flags = r32() & 63u;
    x.pad = 0;
    x.pe_state = r32() % 62; x.pe_sym = r32() % 17;
    x.pe_pos = rpos(); x.pe_sp = rpos();
    x.lm_state = r32() % 62; x.lm_sym = r32() % 17;
    x.lm_pos = rpos(); x.lm_sp = rpos();
    x.lm_apos = rpos(); x.pe_apos = rpos();
    x.lm_astate = r32() % 62; x.pe_astate = r32() % 62;
    x.term_pos = rpos();
    x.count = (int64_t) (rng() % 3);
    x.cur_sp = rpos();
    x.in_pe_pos = rpos();
    x.in_pe_state = r32() % 62; x.in_pe_sym = r32() % 17;
    x.stable_until = (rng() & 1) ? seg_len : (r32() % (seg_len + 1)) & ~63u;
    x.stable_from = (rng() & 1) ? 0 : (r32() % (seg_len + 1)) & ~63u;
    return x;
}

/* field f of x, as a 64-bit value, and its setter: the list a test of "one field at a time" walks */
enum { NFIELDS = 24 };
static void
bump(sre_seg_summary_t &x, int f)
{
    switch (f) {
    case 0: x.s_out ^= 1u; break;               /* (s_in is what the plain record is built from: s_out differs instead) */
    case 1: x.s_out = x.s_in + 1; break;
    case 2: x.flags ^= 1u << (rng() % 6); break;
    case 3: x.pad = 1 + r32() % 7; break;
    case 4: x.pe_state = 1 + r32() % 61; break;
    case 5: x.pe_sym = 1 + r32() % 16; break;
    case 6: x.pe_pos = (int64_t) (rng() % 1000); break;
    case 7: x.pe_sp = (int64_t) (rng() % 1000); break;
    case 8: x.lm_state = 1 + r32() % 61; break;
    case 9: x.lm_sym = 1 + r32() % 16; break;
    case 10: x.lm_pos = (int64_t) (rng() % 1000); break;
    case 11: x.lm_sp = (int64_t) (rng() % 1000); break;
    case 12: x.lm_apos = (int64_t) (rng() % 1000); break;
    case 13: x.pe_apos = (int64_t) (rng() % 1000); break;
    case 14: x.lm_astate = 1 + r32() % 61; break;
    case 15: x.pe_astate = 1 + r32() % 61; break;
    case 16: x.term_pos = (int64_t) (rng() % 1000); break;
    case 17: x.count = 1 + (int64_t) (rng() % 2); break;
    case 18: x.cur_sp = (int64_t) (rng() % 1000); break;
    case 19: x.in_pe_pos = (int64_t) (rng() % 1000); break;
    case 20: x.in_pe_state = 1 + r32() % 61; break;
    case 21: x.in_pe_sym = 1 + r32() % 16; break;
    case 22: x.stable_until -= 64; break;
    case 23: x.stable_from += 64; break;
    }
}

static int
fail(const char *what, uint64_t i, int f)
{
    printf("MISMATCH %s case=%llu field=%d\n", what, (unsigned long long) i, f);
    return 1;
}

int
main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const uint64_t cases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 300000;
    rng.seed(seed);
    static const uint32_t LENS[3] = {64, 256, 16896};
    const uint64_t        NSEG = 257;
    uint64_t              nplain = 0, none = 0, nfull = 0;
    /* a summary buffer and its digests, as a scanner reuses them: stale records stay behind plain digests */
    std::vector<sre_seg_summary_t> sum(NSEG);
    std::vector<sre_seg_digest_t>  dig(NSEG);
    for (uint64_t g = 0; g < NSEG; g++) {
        sum[g] = random_record(256);
        dig[g].s_in = dig[g].s_out = dig[g].count = 0;
        dig[g].bits = SRE_DIGEST_FULL;
    }
    for (uint64_t i = 0; i < cases; i++) {
        const uint32_t    seg_len = LENS[rng() % 3];
        const uint64_t    g = rng() % NSEG;
        const int         kind = (int) (rng() % 4);     /* 0 random, 1 plain, 2 / 3 plain but for one field */
        int               f = -1;
        sre_seg_summary_t x;
        if (kind == 0) {
            x = random_record(seg_len);
        } else {
            x = sre_scan_record_plain((rng() & 31) == 0 ? 0xffffffffu : r32() % 62, seg_len);
            if (kind >= 2) {
                f = (int) (rng() % NFIELDS);
                bump(x, f);
            }
        }
        /* what the scan kernel does at the end of a lane */
        bool                   plain;
        const sre_seg_digest_t d = sre_scan_record_pack(x, seg_len, &plain);
        dig[g] = d;
        if (!plain) sum[g] = x;
        /* plain exactly when the record rebuilt from the digest alone equals x, bit for bit */
        const sre_seg_summary_t rebuilt = sre_scan_record_plain(d.s_in, seg_len);
        const bool              same = memcmp(&rebuilt, &x, sizeof(x)) == 0;
        if (plain != same) return fail("plain", i, f);
        if (plain != !(d.bits & SRE_DIGEST_FULL)) return fail("full-bit", i, f);
        if (kind == 1 && !plain) return fail("plain-record-not-plain", i, f);
        if (kind >= 2 && plain) return fail("one-field-record-plain", i, f);
        /* the round trip, field by field */
        const sre_seg_summary_t y = sre_scan_record_load(dig.data(), sum.data(), g, seg_len);
        if (!sre_scan_record_equal(x, y) || memcmp(&x, &y, sizeof(x)) != 0) return fail("load", i, f);
        /* ... and without digests every record is read where it is stored */
        if (!plain) {
            const sre_seg_summary_t z = sre_scan_record_load(nullptr, sum.data(), g, seg_len);
            if (memcmp(&x, &z, sizeof(x)) != 0) return fail("load-no-digest", i, f);
        }
        /* what the chain check reads */
        const uint32_t want = ((x.flags & SRE_SUM_TERM) ? SRE_DIGEST_TERM : 0u) | ((x.flags & SRE_SUM_LASTEV) ? SRE_DIGEST_LASTEV : 0u)
                              | (x.cur_sp >= 0 ? SRE_DIGEST_SP : 0u) | ((x.flags & SRE_SUM_STABLE) ? 0u : SRE_DIGEST_UNSTABLE);
        if ((d.bits & ~SRE_DIGEST_FULL) != want || d.s_in != x.s_in || d.s_out != x.s_out || d.count != (uint32_t) x.count) {
            return fail("digest", i, f);
        }
        nplain += plain;
        none += kind >= 2;
        nfull += !plain;
    }
    printf("ok cases=%llu plain=%llu one_field=%llu full=%llu\n", (unsigned long long) cases, (unsigned long long) nplain,
           (unsigned long long) none, (unsigned long long) nfull);
    return 0;
}
