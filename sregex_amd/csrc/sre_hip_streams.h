/*
 * sre_hip_streams.h — stream sets (sre_hip_streams_*): many streams of one program whose
 * contexts live in HBM between calls and are advanced together, chunk by chunk
 * (sre_hip_streams.hip; the batched tail kernel sits beside the single-stream one in
 * sre_hip_scan.hip, whose device code it shares).  DESIGN.md §4.13.
 */
#ifndef SRE_HIP_STREAMS_H
#define SRE_HIP_STREAMS_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sre_hip_scan.h"
#include "sre_hip_nfa.h"

/*
 * One context row, in 64-bit words — what sre_stream_ctx_t holds for the compat path plus what
 * sre_vm_pike_ctx_t keeps on the host for its chunk route, sized from the program:
 *   [0] automaton state (low 32 bits) | has_pending (high 32 bits)
 *   [1] pending regex id
 *   [2] processed_bytes
 *   [3] SRE_SFL_* flags
 *   [4 ..]                      pending vector, nslots words
 *   [4 + nslots ..]             capture vectors of the carried list, max_threads x nslots
 *   [4 + nslots * (1 + T) ..]   the tail kernel's second set of those rows
 * row_words = 4 + nslots * (1 + 2 * max_threads); Thompson carries the state alone (nslots = 0).
 * A zero-filled row is a fresh context.
 */
#define SRE_SROW_STATE      0
#define SRE_SROW_REGEX      1
#define SRE_SROW_PROCESSED  2
#define SRE_SROW_FLAGS      3
#define SRE_SROW_HDR        4

#define SRE_SFL_NEWLINE  1u     /* seen_newline / seen_word of the reference's context (sre_vm_pike.c:586-601) */
#define SRE_SFL_WORD     2u
#define SRE_SFL_STARTED  4u     /* the search is under way: an earlier call answered SRE_AGAIN */
#define SRE_SFL_CLOSED   8u     /* a call gave the final answer; the row waits for sre_hip_streams_reset */

/* record of a stream: [rc, state, has_pending, pending[2], ovector] */
#define SRE_SREC_HDR        5
#define SRE_SSTATE_OPEN     0
#define SRE_SSTATE_CLOSED   1
#define SRE_SSTATE_WAS_CLOSED 2
#define SRE_SSTATE_NOT_FED  3

#define SRE_STREAMS_TAIL_THREADS  64u       /* one wave stages the tables, its lane 0 walks */
#define SRE_STREAMS_TAIL_GRID     2048u     /* workgroups of the tail kernel: beyond that they take their streams in turn */

typedef struct {
    uint32_t row_words, nslots, max_threads;
    uint32_t rec_slots, ovec_slots;
} sre_streams_layout_t;

/* device words of one call; they travel to the host in front of the records */
typedef struct {
    uint64_t seg;           /* segment size of the call */
    uint64_t nsegs;         /* segments of all fed, open streams */
    uint64_t nactive;       /* ... how many those are */
    uint64_t bytes;         /* ... and their bytes */
    uint64_t unsettled;     /* streams the tail kernel found unverified (fix-up rounds wanted) */
    uint64_t pad[3];
} sre_streams_info_t;

/* what the host hands in per stream and call: three words */
typedef struct {
    uint64_t ptr;           /* device pointer of the chunk */
    uint64_t len;
    uint64_t flags;         /* SRE_SFEED_* */
} sre_streams_feed_t;
#define SRE_SFEED_FED  1u
#define SRE_SFEED_EOF  2u

#ifdef __cplusplus
extern "C" {
#endif
/* fresh contexts for rows idx[0..n) (d_idx == NULL: rows 0..n) */
hipError_t sre_launch_streams_reset(int64_t *d_rows, uint32_t row_words, const uint64_t *d_idx, uint64_t n,
    hipStream_t stream);
/* The call's geometry and per-stream entries from the feed words and the context rows, by one
 * workgroup: ptrs / lens / seg_first (n + 1 entries; a stream that is not fed or closed has no
 * segments), sentry (SRE_SENTRY_*: a fresh stream enters with init0, one under way with
 * rekind[4 * state + flags] — d_rekind == NULL: the state itself), the state slot of every
 * record, *d_info.  seg_fixed == 0: sre_scan_auto_segment over the bytes fed. */
hipError_t sre_launch_streams_prologue(const sre_streams_feed_t *d_feed, uint32_t n, const int64_t *d_rows,
    sre_streams_layout_t layout, const uint8_t *d_rekind, uint32_t init0, uint64_t seg_fixed, uint64_t resident,
    uint64_t seg_cap, const uint8_t **d_ptrs, uint64_t *d_lens, uint64_t *d_seg_first, uint32_t *d_sentry,
    int64_t *d_recs, sre_streams_info_t *d_info, hipStream_t stream);
/* sre_hip_scan.hip: the tail of every fed stream (only_unsettled: of those marked
 * SRE_STREAM_UNSETTLED by the first call); d_scratch: grid x (seg_bytes + 16) entries,
 * d_tailres: grid entries */
hipError_t sre_launch_streams_tail(const sre_scan_tables_t *d_tab, sre_scan_tables_t h_tab, sre_scan_geom_t geom,
    const sre_seg_summary_t *d_sum, const sre_stream_status_t *d_status, uint16_t *d_scratch, int64_t *d_rows,
    sre_streams_layout_t layout, sre_stream_result_t *d_tailres, int64_t *d_recs, sre_streams_info_t *d_info,
    uint32_t grid, int only_unsettled, hipStream_t stream);

/* ---- the bit-parallel NFA tier (sre_hip_streams_create_engine): rows of 1 + W words, sre_streams_nfa.h */
typedef struct { uint64_t w[4]; } sre_streams_nfa_init_t;      /* the initial set of a fresh stream */
/* As sre_launch_streams_prologue: ptrs / lens / seg_first of the streams that scan bytes in this call
 * (sre_streams_nfa_scans), d_sflags (SRE_SFLAG_NO_EOF unless the stream's chunk is its last), d_eset
 * [n][W]: the set every stream enters with; the records — and rows — of the streams the call
 * decides without a byte; *d_info */
hipError_t sre_launch_streams_nfa_prologue(const sre_streams_feed_t *d_feed, uint32_t n, int64_t *d_rows, uint32_t W,
    sre_streams_nfa_init_t init0, uint32_t rec_slots, uint64_t seg_fixed, uint64_t resident, uint64_t seg_cap,
    const uint8_t **d_ptrs, uint64_t *d_lens, uint64_t *d_seg_first, uint8_t *d_sflags, uint64_t *d_eset,
    int64_t *d_recs, sre_streams_info_t *d_info, hipStream_t stream);
/* d_lo[s] = first wrong segment of stream s or -1 (verified), *d_pending = streams that are not */
hipError_t sre_launch_streams_nfa_lo(const sre_nfa_status_t *d_status, uint32_t n, int64_t *d_lo, uint64_t *d_pending,
    hipStream_t stream);
/* the tail of every stream that scanned (only_unsettled: of those the first tail left for the fix-up
 * rounds): row, record, d_info->unsettled; d_wsets: the wide kernel's [nsegs][2][W] sets, NULL: W == 1
 * and the exit sets are d_sum[].s_out */
hipError_t sre_launch_streams_nfa_tail(const sre_streams_feed_t *d_feed, uint32_t n, int64_t *d_rows, uint32_t W,
    const uint64_t *d_seg_first, const sre_nfa_status_t *d_status, const sre_nfa_summary_t *d_sum, const uint64_t *d_wsets,
    uint32_t rec_slots, int64_t *d_recs, sre_streams_info_t *d_info, int only_unsettled, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
