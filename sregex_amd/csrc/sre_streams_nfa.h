/*
 * sre_streams_nfa.h — what one call means to one stream of a stream set on the bit-parallel NFA
 * tier (sre_hip_streams_create_engine): ONE text for the device tail
 * (sre_hip_streams.hip sre_k_streams_nfa_tail) and for the CPU model (tests/streams_nfa_sim.cpp).
 *
 * A Thompson context of a program without look-ahead assertions is its thread set
 * (sre_vm_thompson.c:273-345: ^ goes by the byte just consumed, \A holds for the thread added in the
 * first call only), so a stream's context row is
 *      [0]      SRE_SNFA_* flags | closing rc << 32
 *      [1 .. W] the thread set in front of the next byte, in the numbering of the set's kernel
 * and a zero-filled row is a fresh context.  A MATCH that is listed at the position not yet run is a
 * FLAG, not a bit of the set: the shift-and forms that accumulate events (sre_nfa.h `evacc`) have
 * no MATCH bit.
 */
#ifndef SRE_STREAMS_NFA_H
#define SRE_STREAMS_NFA_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRE_SNFA_FN __host__ __device__ static inline
#else
#define SRE_SNFA_FN static inline
#endif

#define SRE_SNFA_STARTED  1u    /* an earlier call answered SRE_AGAIN: the set words are the context */
#define SRE_SNFA_PENDING  2u    /* the last byte fed listed MATCH: the next position that runs meets it */
#define SRE_SNFA_CLOSED   4u    /* a call gave the final answer (bits 32..63: that rc) */

#define SRE_SNFA_RC_OK        0
#define SRE_SNFA_RC_AGAIN     (-2)
#define SRE_SNFA_RC_DECLINED  (-5)

/* record states, as sre_hip_streams.h SRE_SSTATE_* */
#define SRE_SNFA_OPEN        0
#define SRE_SNFA_NOW_CLOSED  1
#define SRE_SNFA_WAS_CLOSED  2
#define SRE_SNFA_NOT_FED     3

typedef struct {
    int64_t  rc;        /* undefined for SRE_SNFA_NOT_FED */
    int32_t  state;     /* SRE_SNFA_OPEN .. SRE_SNFA_NOT_FED */
    int32_t  keep_set;  /* 1: the row's set words stay as they are, 0: they become the call's exit set */
    uint64_t flags;     /* the row's flag word behind the call */
} sre_snfa_step_t;

/* does the call scan bytes of this stream (does it take segments of the pass)? */
SRE_SNFA_FN int
sre_streams_nfa_scans(uint64_t flags, int fed)
{
    return fed && (flags & (SRE_SNFA_CLOSED | SRE_SNFA_PENDING)) == 0;
}

/*
 * One call.  flags: the row's flag word in front of it; fed / len / eof: what the caller handed in;
 * ev: the position in the chunk of the first step that reached MATCH (-1: none; only looked at when
 * sre_streams_nfa_scans()); exit_empty: the exit set is empty.
 *
 * A slot that is not fed answers SRE_SNFA_NOT_FED whatever its row holds (the table-driven set's
 * contract); then, in this order (sre_vm_thompson.c:88-258):
 *   closed before the call          -> WAS_CLOSED, the closing rc again, nothing read
 *   MATCH pending                   -> a call that runs a position (len > 0 or eof) meets it: OK, closed;
 *                                      len == 0 without eof runs none (:88): AGAIN, still pending
 *   0 <= ev < len - 1               -> MATCH is popped at ev + 1 < len: OK, closed
 *   ev == len - 1                   -> with eof the extra iteration meets it (:233-235): OK, closed;
 *                                      else AGAIN, pending
 *   no event                        -> DECLINED with eof (closed), else AGAIN.  An empty set stays
 *                                      empty and answers the same (:92-94), so exit_empty decides nothing.
 */
SRE_SNFA_FN sre_snfa_step_t
sre_streams_nfa_rule(uint64_t flags, int fed, uint64_t len, int eof, int64_t ev, int exit_empty)
{
    sre_snfa_step_t r;
    r.rc = 0;
    r.keep_set = 1;
    r.flags = flags;
    (void) exit_empty;
    if (!fed) {
        r.state = SRE_SNFA_NOT_FED;
        return r;
    }
    if (flags & SRE_SNFA_CLOSED) {
        r.state = SRE_SNFA_WAS_CLOSED;
        r.rc = (int64_t) (int32_t) (uint32_t) (flags >> 32);
        return r;
    }
    int closes = 0;
    r.rc = SRE_SNFA_RC_AGAIN;
    if (flags & SRE_SNFA_PENDING) {
        if (len > 0 || eof) {
            r.rc = SRE_SNFA_RC_OK;
            closes = 1;
        }
    } else if (ev >= 0 && (uint64_t) ev + 1 < len) {
        r.rc = SRE_SNFA_RC_OK;
        closes = 1;
    } else if (ev >= 0) {
        if (eof) {
            r.rc = SRE_SNFA_RC_OK;
            closes = 1;
        } else {
            r.flags |= SRE_SNFA_PENDING;
        }
    } else {
        r.keep_set = 0;
        if (eof) {
            r.rc = SRE_SNFA_RC_DECLINED;
            closes = 1;
        }
    }
    r.flags |= SRE_SNFA_STARTED;
    if (closes) r.flags = (r.flags & 0xffffffffull) | SRE_SNFA_CLOSED | ((uint64_t) (uint32_t) (int32_t) r.rc << 32);
    r.state = closes ? SRE_SNFA_NOW_CLOSED : SRE_SNFA_OPEN;
    return r;
}

#endif
