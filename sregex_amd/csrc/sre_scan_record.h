/*
 * sre_scan_record.h — the ONE rule by which a FIRST / Thompson scan lane's record (sre_seg_summary_t, 136 bytes)
 * is kept as a digest (sre_seg_digest_t, 16 bytes) and read back.
 *
 * Most segments of a long stream are PLAIN: the automaton sat in one state through all of it, nothing
 * happened, and the whole record follows from the entry state and the segment length.  The scan kernel
 * writes the digest of every segment (coalesced) and the record itself only where it is not plain; the
 * grid-wide chain check reads digests only, and every other reader goes through sre_scan_record_load().
 * The summary buffer is reused from call to call: behind a digest without SRE_DIGEST_FULL, sum[g] holds
 * whatever an earlier call left there and is never read.
 *
 * Host and device (the CPU test tests/scan_record_sim.cpp runs the same functions).
 */
#ifndef SRE_SCAN_RECORD_H
#define SRE_SCAN_RECORD_H

#include <stddef.h>
#include <stdint.h>

/* what one lane learnt about its segment */
typedef struct {
    uint32_t s_in;          /* state assumed at the segment start (after warm-up) */
    uint32_t s_out;         /* state at the segment end */
    uint32_t flags;         /* SRE_SUM_* */
    uint32_t pad;
    /* SRE_SUM_PENDING: the search in flight at the segment end holds a match */
    uint32_t pe_state, pe_sym;      /* state before the event's transition, its symbol */
    int64_t  pe_pos, pe_sp;         /* event position; start of its search (-1 unknown) */
    /* SRE_SUM_LASTEV: FIRST: last match event seen here; COUNT: last completed match */
    uint32_t lm_state, lm_sym;
    int64_t  lm_pos, lm_sp;
    /* a known state shortly before that event (start of its 64-byte round), so
     * the capture walker need not replay the segment: -1 if none */
    int64_t  lm_apos, pe_apos;
    uint32_t lm_astate, pe_astate;
    int64_t  term_pos;      /* position where the scan of this stream ended, -1 none */
    int64_t  count;         /* COUNT: searches completed with a match in this segment */
    int64_t  cur_sp;        /* start of the search in flight at the segment end, -1 unknown */
    /* COUNT, SRE_SUM_IN_PENDING: the pending match the lane believed it ENTERED with (from its
     * warm-up, or the exact carry).  Equal entry states do not imply equal pending events, so the
     * chain check compares this with the predecessor's pe_* as well. */
    int64_t  in_pe_pos;
    uint32_t in_pe_state, in_pe_sym;
    /* FIRST: the byte steps [0, stable_until) of the segment, counted from its start, were
     * STABLE steps of the entry state s_in, and so were the steps [stable_from, length) of
     * the exit state s_out (whole 64-byte rounds; stable_until == length: the whole segment,
     * flag SRE_SUM_STABLE). */
    uint32_t stable_until, stable_from;
} sre_seg_summary_t;

/* bits: SRE_DIGEST_* below (as verify_one_stream keeps them); count: the record's, FIRST / Thompson: 0 or 1 */
typedef struct sre_seg_digest_s {
    uint32_t s_in, s_out, bits, count;
} sre_seg_digest_t;

#define SRE_SUM_PENDING   1u
#define SRE_SUM_TERM      2u   /* the scan of this stream ended inside this segment */
#define SRE_SUM_LASTEV    4u
#define SRE_SUM_ERROR     8u   /* COUNT: ... and the iteration ended with SRE_ERROR */
#define SRE_SUM_IN_PENDING 16u /* COUNT: the lane entered its segment holding a pending match (in_pe_*) */
#define SRE_SUM_STABLE    32u  /* every byte step of the segment was a STABLE step of s_in == s_out */

#ifdef __HIPCC__
#define SRE_RECORD_FN static __host__ __device__ inline
#else
#define SRE_RECORD_FN static inline
#endif

/* sre_seg_digest_t.bits, as the chain check keeps them (verify_one_stream; bit 0 is its own "link broken") */
#define SRE_DIGEST_TERM      2u     /* SRE_SUM_TERM */
#define SRE_DIGEST_LASTEV    4u     /* SRE_SUM_LASTEV */
#define SRE_DIGEST_SP        8u     /* cur_sp >= 0 */
#define SRE_DIGEST_UNSTABLE  16u    /* not SRE_SUM_STABLE */
#define SRE_DIGEST_FULL      32u    /* the record is not plain: sum[g] holds it */

/* the comparison below names every field: a new one has to be added there (and to the plain record) */
static_assert(sizeof(sre_seg_summary_t) == 136, "sre_seg_summary_t changed: update sre_scan_record_plain / _equal");

/* the plain record of a segment of seg_len bytes entered in state s_in */
SRE_RECORD_FN sre_seg_summary_t
sre_scan_record_plain(uint32_t s_in, uint32_t seg_len)
{
    sre_seg_summary_t r;
    r.s_in = s_in;
    r.s_out = s_in;
    r.flags = SRE_SUM_STABLE;
    r.pad = 0;
    r.pe_state = r.pe_sym = 0;
    r.pe_pos = r.pe_sp = -1;
    r.lm_state = r.lm_sym = 0;
    r.lm_pos = r.lm_sp = -1;
    r.lm_apos = r.pe_apos = -1;
    r.lm_astate = r.pe_astate = 0;
    r.term_pos = -1;
    r.count = 0;
    r.cur_sp = -1;
    r.in_pe_pos = -1;
    r.in_pe_state = r.in_pe_sym = 0;
    r.stable_until = seg_len;       /* the entry state's stable stretch is the whole segment ... */
    r.stable_from = 0;              /* ... and so is the exit state's (the lane entered its shadow row in its first round) */
    return r;
}

SRE_RECORD_FN bool
sre_scan_record_equal(const sre_seg_summary_t &a, const sre_seg_summary_t &b)
{
    return a.s_in == b.s_in && a.s_out == b.s_out && a.flags == b.flags && a.pad == b.pad
           && a.pe_state == b.pe_state && a.pe_sym == b.pe_sym && a.pe_pos == b.pe_pos && a.pe_sp == b.pe_sp
           && a.lm_state == b.lm_state && a.lm_sym == b.lm_sym && a.lm_pos == b.lm_pos && a.lm_sp == b.lm_sp
           && a.lm_apos == b.lm_apos && a.pe_apos == b.pe_apos && a.lm_astate == b.lm_astate && a.pe_astate == b.pe_astate
           && a.term_pos == b.term_pos && a.count == b.count && a.cur_sp == b.cur_sp
           && a.in_pe_pos == b.in_pe_pos && a.in_pe_state == b.in_pe_state && a.in_pe_sym == b.in_pe_sym
           && a.stable_until == b.stable_until && a.stable_from == b.stable_from;
}

/* the digest of record x of a segment of seg_len bytes; *plain: x is exactly what the digest alone gives back
 * (then SRE_DIGEST_FULL is clear and x need not be stored) */
SRE_RECORD_FN sre_seg_digest_t
sre_scan_record_pack(const sre_seg_summary_t &x, uint32_t seg_len, bool *plain)
{
    sre_seg_digest_t d;
    d.s_in = x.s_in;
    d.s_out = x.s_out;
    d.bits = ((x.flags & SRE_SUM_TERM) ? SRE_DIGEST_TERM : 0u) | ((x.flags & SRE_SUM_LASTEV) ? SRE_DIGEST_LASTEV : 0u)
             | (x.cur_sp >= 0 ? SRE_DIGEST_SP : 0u) | ((x.flags & SRE_SUM_STABLE) ? 0u : SRE_DIGEST_UNSTABLE);
    d.count = (uint32_t) x.count;
    *plain = sre_scan_record_equal(x, sre_scan_record_plain(x.s_in, seg_len));
    if (!*plain) d.bits |= SRE_DIGEST_FULL;
    return d;
}

/* the record of segment g: from the digest where that is all there is, else sum[g] (dig == NULL: no digests,
 * every record is stored).  seg_len: the length of a segment that is not its stream's last (a last segment is
 * never plain). */
SRE_RECORD_FN sre_seg_summary_t
sre_scan_record_load(const sre_seg_digest_t *dig, const sre_seg_summary_t *sum, uint64_t g, uint32_t seg_len)
{
    if (dig != NULL) {
        const sre_seg_digest_t d = dig[g];
        if (!(d.bits & SRE_DIGEST_FULL)) return sre_scan_record_plain(d.s_in, seg_len);
    }
    return sum[g];
}

#ifdef __HIPCC__
/* a summary array as its readers index it: records[k] is the record of segment k, wherever it is kept */
struct sre_scan_records_t {
    const sre_seg_summary_t *sum;
    const sre_seg_digest_t  *dig;
    uint32_t                 seg_len;
    __host__ __device__ inline sre_seg_summary_t operator[](uint64_t k) const
    {
        return sre_scan_record_load(dig, sum, k, seg_len);
    }
    /* the records from segment `first` on (one stream's) */
    __host__ __device__ inline sre_scan_records_t operator+(uint64_t first) const
    {
        return sre_scan_records_t{sum + first, dig != NULL ? dig + first : NULL, seg_len};
    }
};
#endif

#endif
