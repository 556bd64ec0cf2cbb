/*
 * sre_hip_nfa_wide.h — device tables and launchers of the wide bit-parallel NFA scanner
 * (sre_hip_nfa_wide.hip; host form: sre_nfa_wide.h).  Summaries, status words and records are those of
 * the 64-bit tier (sre_hip_nfa.h); the sets themselves travel in arrays of W words per segment.
 */
#ifndef SRE_HIP_NFA_WIDE_H
#define SRE_HIP_NFA_WIDE_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sre_hip_nfa.h"

typedef struct {
    uint32_t W, nlut, nassert, pad;
    uint32_t hot[16];               /* byte of the mask that indexes lut[k] */
    uint64_t init[3][4];
    uint64_t seed[4], any_bits[4], match_bits[4], msrc[4], valid[4], self[4], shift_src[4];
    const uint64_t *accept;         /* [256][W]                   device */
    const uint64_t *lut;            /* [nlut][256][W]             device (NULL when nlut == 0) */
    const uint64_t *expand;         /* [16][1 << nassert][W]      device (look-ahead programs) */
    const uint8_t  *kind;           /* [256]                      device (sre_nfa.h SRE_NFA_KIND_*) */
} sre_nfa_wide_tables_t;

#ifdef __cplusplus
extern "C" {
#endif
/* LDS of a workgroup of the scan kernel (tables, padded lookups, staging) */
size_t sre_nfa_wide_kernel_lds(const sre_nfa_wide_tables_t *t);
int sre_nfa_wide_blocks_per_cu(const sre_nfa_wide_tables_t *t);
const char *sre_nfa_wide_kernel_name(const sre_nfa_wide_tables_t *t, char *buf, size_t n);
/* one pass of sre_k_nfa_wide over segments [lo[s], ...) of every stream (lo == NULL: all, speculative entry
 * sets from a 128-byte warm-up); d_sets: [nsegs][2][W] entry and exit sets, d_belief: [nsegs][W];
 * d_entry: [nstreams][W] per-stream entry sets (stream sets), NULL: the tables' initial sets */
hipError_t sre_launch_nfa_wide_scan(sre_nfa_wide_tables_t tab, sre_scan_geom_t geom, sre_nfa_summary_t *d_sum,
    uint64_t *d_sets, const int64_t *d_lo, const uint64_t *d_belief, const uint8_t *d_bvalid, const uint64_t *d_entry,
    hipStream_t stream);
/* the chain check on W-word sets, then the 64-bit tier's clean-position reduction and status / records */
hipError_t sre_launch_nfa_wide_verify(int mode, uint32_t W, sre_scan_geom_t geom, const sre_nfa_summary_t *d_sum,
    const uint64_t *d_sets, void *d_acc, sre_nfa_status_t *d_status, uint64_t *d_belief, uint8_t *d_bvalid,
    int64_t *d_records, uint32_t ovec_slots, const int64_t *d_lo, hipStream_t stream);
/* exact entry sets (a program that never forgets): d_mat holds 64W x W words per segment of the batch */
size_t sre_nfa_wide_matrix_bytes(uint32_t W, uint64_t nsegs);
hipError_t sre_launch_nfa_wide_exact_entries(sre_nfa_wide_tables_t tab, sre_scan_geom_t geom,
    const sre_nfa_summary_t *d_sum, const uint64_t *d_sets, const int64_t *d_lo, uint64_t *d_mat, uint64_t *d_belief,
    uint8_t *d_bvalid, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
