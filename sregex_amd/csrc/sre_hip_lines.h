/*
 * sre_hip_lines.h — line mode (sre_hip_scan_lines): the delimiter split of one device
 * buffer, the per-batch geometry the scan kernels read, the settle counters and the
 * compaction of the reported rows (sre_hip_lines.hip).  DESIGN.md §4.11.
 */
#ifndef SRE_HIP_LINES_H
#define SRE_HIP_LINES_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sre_hip_scan.h"
#include "sre_hip_nfa.h"
#include "sre_lines_nfa.h"
#include "sre_lines_select.h"     /* sre_extract_groups_t, sre_subst_pieces_t and the select rules */
#include "sre_lines_join.h"       /* sre_lj_cols_t */

/* split: a workgroup of SRE_LINES_THREADS lanes owns one tile of 16-byte aligned chunks, each lane
 * loads SRE_LINES_CHUNKS chunks of it (lane x, step k: chunk k * SRE_LINES_THREADS + x of the tile).
 * Tiles are counted from the 16-byte aligned address at or below the buffer: tile t starts at
 * buffer offset t * SRE_LINES_TILE_BYTES - (d_buf % 16). */
#define SRE_LINES_THREADS     256u
#define SRE_LINES_CHUNKS      16u
#define SRE_LINES_TILE_BYTES  (SRE_LINES_THREADS * SRE_LINES_CHUNKS * 16u)     /* 64 KiB */
/* geometry and compaction passes: items (lines) per workgroup, 4 per lane */
#define SRE_LINES_ITEMS       1024u
/* lines per batch (SRE_HIP_LINES_BATCH overrides), and the most capture-walker scratch a batch may
 * take: lines x (segment + 16) x 2 B — 1 Mi lines of 96 B take 570 MB at 256-byte segments */
#define SRE_LINES_BATCH       (1u << 20)
#define SRE_LINES_WALK_MAX (1ull << 30)
/* NFA tier: the most per-segment working set (summaries, beliefs, the wide kernel's sets) a batch may take, and
 * the longest line the short-line kernel takes by default (SRE_HIP_LINES_SHORT_MAX overrides; 0: off) */
#define SRE_LINES_NFA_WORK_MAX  (1ull << 30)
#define SRE_LINES_SHORT_MAX     512u

/* device words of one line-mode call; the host reads them in small copies */
typedef struct {
    uint64_t nlines;        /* split: lines in the buffer */
    uint64_t i1;            /* batch: first line behind it */
    uint64_t bytes;         /* batch: bytes of its lines */
    uint64_t seg;           /* batch: segment size */
    uint64_t nsegs;         /* batch: segments */
    uint64_t reported;      /* running count of reported lines, all batches so far */
    uint64_t pending;       /* settle: streams of the batch whose status is not done */
    uint64_t maps;          /* settle: streams that asked for lineage maps (need_maps) */
    uint64_t nshort;        /* batch, NFA tier: lines the short-line kernel takes (they have no segment) */
    /* the line filter (sre_hip_filter_lines): the four words the host reads before the gather */
    uint64_t fsel;          /* lines selected */
    uint64_t fneed;         /* bytes all of them take */
    uint64_t fwritten;      /* selected lines that fit out_cap whole */
    uint64_t fbytes;        /* bytes of those */
    /* the filter with context (sre_hip_filter_lines_context): two more words, read with the four */
    uint64_t cmatched;      /* lines the match rule selects (with context only; without, fsel says it) */
    uint64_t cgroups;       /* maximal runs of adjacent selected lines */
    /* the line tally (sre_hip_tally_lines): three more words, read with the four (zeroed in front of the insert) */
    uint64_t tsel;          /* lines that have a key */
    uint64_t tclaims;       /* slots of the table claimed */
    uint64_t tover;         /* not 0: more than max_keys distinct keys, or the table is full */
    /* the line distinct (sre_hip_distinct_lines): the tally's three and one more word, read with the four (zeroed with them) */
    uint64_t dkept;         /* distinct keys whose count is within the call's range */
    /* the line lookup (sre_hip_lookup_lines): two more words, read with the four (zeroed in front of the probe) */
    uint64_t knkeyed;       /* lines that have a key */
    uint64_t knmembers;     /* of those, lines whose key is in the set */
    /* the line sort (sre_hip_sort_lines): four words of its own, set by the values pass and read in one copy */
    uint64_t skeyed;        /* lines that have a match */
    uint64_t snumbered;     /* of those, lines whose sort field is a number */
    uint64_t svmin;         /* the least of those numbers, an int64_t (INT64_MAX without one) */
    uint64_t svmax;         /* the greatest, an int64_t (INT64_MIN without one) */
    /* the line fold (sre_hip_fold_lines): three more words, read with the four; fwritten counts records there */
    uint64_t gnrec;         /* records: the heads */
    uint64_t gmarked;       /* marked lines */
    uint64_t glongest;      /* lines of the longest record */
} sre_lines_info_t;

#ifdef __cplusplus
extern "C" {
#endif
/* split pass 1 + tile scan: info->nlines.  ends / tiles sized by the caller: ntiles =
 * ceil((d_buf % 16 + len) / SRE_LINES_TILE_BYTES) entries of tiles */
hipError_t sre_launch_lines_count(const void *d_buf, uint64_t len, uint32_t delim, uint64_t *d_tiles,
    sre_lines_info_t *d_info, hipStream_t stream);
/* split pass 2: ends[i] = offset of line i's delimiter (len for a final line without one) */
hipError_t sre_launch_lines_write(const void *d_buf, uint64_t len, uint32_t delim, const uint64_t *d_tiles,
    uint64_t *d_ends, hipStream_t stream);
/* the batch from line i0: at most bmax lines whose capture-walker buffer (see SRE_LINES_WALK_MAX) fits, its
 * segment size (seg_fixed, else sre_scan_auto_segment(bytes, resident, seg_cap)) and the arrays
 * sre_scan_geom_t reads (ptrs / lens / seg_first, nmax + 1 entries); info->i1, bytes, seg, nsegs */
hipError_t sre_launch_lines_geometry(const void *d_buf, const uint64_t *d_ends, uint64_t nlines, uint64_t i0,
    uint64_t nmax, uint64_t scratch_max, uint64_t seg_fixed, uint64_t resident, uint64_t seg_cap,
    const uint8_t **d_ptrs, uint64_t *d_lens, uint64_t *d_seg_first, uint64_t *d_blk,
    sre_lines_info_t *d_info, hipStream_t stream);
/* the same for the NFA tier.  Lines shorter than short_lim bytes get NO segment (the short-line kernel takes
 * them; 0: none does, an empty line then keeps its one segment); the batch is the longest of at most nmax lines
 * whose segments' working set fits: (bytes / seg + lines) * seg_cost <= work_max, a single line always does.
 * The segment size goes by the bytes of all the batch's lines.  info->i1, bytes, seg, nsegs, nshort */
hipError_t sre_launch_lines_geometry_nfa(const void *d_buf, const uint64_t *d_ends, uint64_t nlines, uint64_t i0,
    uint64_t nmax, uint64_t short_lim, uint64_t work_max, uint64_t seg_cost, uint64_t seg_fixed, uint64_t resident,
    uint64_t seg_cap, const uint8_t **d_ptrs, uint64_t *d_lens, uint64_t *d_seg_first, uint64_t *d_blk,
    sre_lines_info_t *d_info, hipStream_t stream);
/* info->pending / info->maps of the batch's n status words (zeroed first) */
hipError_t sre_launch_lines_settle(const sre_stream_status_t *d_status, uint32_t n, sre_lines_info_t *d_info,
    hipStream_t stream);
/* ordered compaction of the batch (lines i0 .. i0 + info->i1 - i0) behind info->reported: rows
 * [line, start, len, record] with index < cap go to d_rows */
hipError_t sre_launch_lines_compact(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0,
    int all, const uint64_t *d_ends, uint64_t *d_blk, sre_lines_info_t *d_info, int64_t *d_rows, uint64_t cap,
    hipStream_t stream);
/* the short-line kernel (sre_hip_lines_nfa.hip): the tables of a 64-bit form as its step reads them
 * (sre_lines_nfa.h; device pointers inside) ... */
sre_lnfa_t sre_lines_nfa_tables_plain(const sre_nfa_tables_t *p);
sre_lnfa_t sre_lines_nfa_tables_sa(const sre_nfa_sa_tables_t *a);
/* ... and one lane per line of the batch (lines i0 .. i0 + nb): a line shorter than short_lim bytes gets its
 * status block, its record (as the chain check writes them: Pike records with an event wait for the window
 * kernel) and lo = 0 when the window kernel has to run over it, else -1; a longer line gets lo = -1 only */
hipError_t sre_launch_lines_nfa(sre_lnfa_t tab, const void *d_buf, const uint64_t *d_ends, uint64_t i0, uint32_t nb,
    uint32_t short_lim, int thompson, sre_nfa_status_t *d_status, int64_t *d_records, uint32_t ovec_slots,
    int64_t *d_lo, hipStream_t stream);
/* ---- the line filter (sre_hip_lines_gather.hip) ---- */
/* select pass of the batch (lines i0 .. info->i1, at most nmax): d_val[i] = len + 1 of a row of sre_sel_row, else 0 */
hipError_t sre_launch_filter_select(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0, int mode,
    const uint64_t *d_ends, const sre_lines_info_t *d_info, uint64_t *d_val, hipStream_t stream);
/* d_val[0 .. n) becomes the offset table off[0 .. n] in place (n + 1 words); d_blk: 2 x ceil(n / SRE_LINES_ITEMS)
 * words, the second half keeps the selected lines in front of each workgroup for the index; info->fsel, fneed,
 * fwritten, fbytes */
hipError_t sre_launch_filter_offsets(uint64_t *d_val, uint64_t n, uint64_t *d_blk, uint64_t out_cap,
    sre_lines_info_t *d_info, hipStream_t stream);
/* the gather: output bytes [0, out_bytes) of the selected lines and their delimiters to d_out */
hipError_t sre_launch_lines_gather(const void *d_buf, void *d_out, const uint64_t *d_off, const uint64_t *d_ends,
    uint64_t nlines, uint64_t out_bytes, uint32_t delim, hipStream_t stream);
/* rows [line, start, len, output offset] of the first min(index_cap, info->fwritten) written lines */
hipError_t sre_launch_filter_index(const uint64_t *d_off, const uint64_t *d_ends, uint64_t n, const uint64_t *d_blk,
    const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index, hipStream_t stream);
/* ---- the filter's context lines (sre_hip_lines_context.hip) ---- */
/* between the last select pass and sre_launch_filter_offsets: every line within `after` lines behind a line with
 * d_val[i] > 0 or `before` lines in front of one gets d_val[i] = len + 1 too (marks, carry, apply: a cost per line that
 * does not depend on before / after).  d_bits: ceil(n / 64) words, bit i set for such a context-only line; d_blk:
 * 4 x ceil(n / SRE_LINES_ITEMS) words of its own (nothing of it is read afterwards); info->cmatched, cgroups */
hipError_t sre_launch_context_select(uint64_t *d_val, const uint64_t *d_ends, uint64_t n, uint64_t before, uint64_t after,
    uint64_t *d_bits, uint64_t *d_blk, sre_lines_info_t *d_info, hipStream_t stream);
/* the call without context, behind sre_launch_filter_offsets: info->cgroups from the offset table (and cmatched = 0:
 * info->fsel is the count); d_blk: ceil(n / SRE_LINES_ITEMS) words of its own */
hipError_t sre_launch_context_runs(const uint64_t *d_off, uint64_t n, uint64_t *d_blk, sre_lines_info_t *d_info,
    hipStream_t stream);
/* sre_launch_filter_index with rows of FIVE words: [4] bit 0 = context-only (from d_bits; NULL: no line is), bit 1 =
 * first line of a group.  d_blk: the words of sre_launch_filter_offsets */
hipError_t sre_launch_context_index(const uint64_t *d_off, const uint64_t *d_ends, uint64_t n, const uint64_t *d_blk,
    const uint64_t *d_bits, const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index, hipStream_t stream);
/* ---- the line fold (sre_hip_lines_fold.hip, sre_lines_fold.h) ---- */
/* between the last select pass and sre_launch_extract_offsets with k = 1 (marks, carry, apply, totals): line i is marked when
 * d_val[i] > 0, and a marked line belongs to the record of the line in front of it, with `next` to the one behind it;
 * max_lines caps the lines of a record (0: no cap).  Afterwards d_val / d_start are the extract's entry table with one entry a
 * line: d_val[i] = len + 1, d_start[i] the line's source offset under SRE_LG_ENTRY_LAST where the delimiter follows the line
 * (n words each).  d_bits: 2 x ceil(n / 64) words (the marked lines, the heads); d_aux: n words (a head: the head behind it,
 * any other line: the first line of its record); d_blk: 5 x ceil(n / SRE_LINES_ITEMS) words of its own, the third run the
 * heads in front of each workgroup; info->gnrec, gmarked, glongest */
hipError_t sre_launch_fold_select(uint64_t *d_val, uint64_t *d_start, const uint64_t *d_ends, uint64_t n, int next,
    uint64_t max_lines, uint64_t *d_bits, uint64_t *d_aux, uint64_t *d_blk, sre_lines_info_t *d_info, hipStream_t stream);
/* behind sre_launch_extract_offsets: the cut at out_cap moved back to the first line of its record; info->fbytes, and
 * info->fwritten = the records in front of the cut */
hipError_t sre_launch_fold_finish(const uint64_t *d_off, uint64_t n, const uint64_t *d_bits, const uint64_t *d_aux,
    const uint64_t *d_blk, uint64_t out_cap, sre_lines_info_t *d_info, hipStream_t stream);
/* d_recid[i] = the record of line i for i < min(recid_cap, n); rows [first line, lines, source offset, bytes without the final
 * delimiter, output offset] of the first min(records_cap, info->fwritten) records (nwritten: that word as the host read it).
 * Nothing is launched for a capacity of 0 */
hipError_t sre_launch_fold_tables(const uint64_t *d_off, const uint64_t *d_ends, uint64_t n, const uint64_t *d_bits,
    const uint64_t *d_aux, const uint64_t *d_blk, const sre_lines_info_t *d_info, int64_t *d_recid, uint64_t recid_cap,
    int64_t *d_records, uint64_t records_cap, uint64_t nwritten, hipStream_t stream);
/* ---- the line extract (sre_hip_lines_gather.hip) ---- */
/* select pass of the batch over its entries e = line * k + f: d_val[e] and d_start[e] as sre_sel_extract_entry gives
 * them.  A batch may have at most 2^32 - 1 entries */
hipError_t sre_launch_extract_select(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0, int all,
    const sre_extract_groups_t *groups, const uint64_t *d_ends, const sre_lines_info_t *d_info, uint64_t *d_val,
    uint64_t *d_start, hipStream_t stream);
/* sre_launch_filter_offsets over the n * k entries (n * k + 1 words; d_blk: 2 x ceil(n * k / SRE_LINES_ITEMS)), the
 * cut made at a line boundary; info->fsel and fwritten count lines */
hipError_t sre_launch_extract_offsets(uint64_t *d_val, uint64_t n, uint32_t k, uint64_t *d_blk, uint64_t out_cap,
    sre_lines_info_t *d_info, hipStream_t stream);
/* the gather over the entry table: output bytes [0, out_bytes) of the rows to d_out */
hipError_t sre_launch_extract_gather(const void *d_buf, void *d_out, const uint64_t *d_off, const uint64_t *d_start,
    uint64_t nentries, uint64_t out_bytes, uint32_t delim, uint32_t fsep, hipStream_t stream);
/* rows [line, start, len, output offset, (field offset, field length) x k] of the first min(index_cap,
 * info->fwritten) written rows; an unset field is (-1, -1) */
hipError_t sre_launch_extract_index(const uint64_t *d_off, const uint64_t *d_start, const uint64_t *d_ends, uint64_t n,
    uint32_t k, const uint64_t *d_blk, const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index,
    hipStream_t stream);
/* ---- the line substitute (sre_hip_lines_gather.hip) ---- */
/* select pass of the batch over its entries e = line * p + f, p = np + 2: d_val[e] and d_start[e] as
 * sre_sel_subst_entry gives them.  A batch may have at most 2^32 - 1 entries */
hipError_t sre_launch_subst_select(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0, int all,
    const sre_subst_pieces_t *pieces, const uint64_t *d_ends, const sre_lines_info_t *d_info, uint64_t *d_val,
    uint64_t *d_start, hipStream_t stream);
/* sre_launch_extract_offsets over the n * p entries, lines counted by their last entries (the others may be empty);
 * info->fsel and fwritten count lines */
hipError_t sre_launch_subst_offsets(uint64_t *d_val, uint64_t n, uint32_t p, uint64_t *d_blk, uint64_t out_cap,
    sre_lines_info_t *d_info, hipStream_t stream);
/* the gather over the piece table: output bytes [0, out_bytes) of the rows to d_out.  d_lit: the literal block, 16-byte
 * aligned and a multiple of 16 bytes */
hipError_t sre_launch_subst_gather(const void *d_buf, void *d_out, const uint64_t *d_off, const uint64_t *d_start,
    const void *d_lit, uint64_t nentries, uint64_t out_bytes, uint32_t delim, hipStream_t stream);
/* rows [line, start, len, output offset of the row, match offset, match length, output offset of the replacement, its
 * length] of the first min(index_cap, info->fwritten) written rows; a line without a match has -1 in the last four */
hipError_t sre_launch_subst_index(const uint64_t *d_off, const uint64_t *d_start, const uint64_t *d_ends, uint64_t n,
    uint32_t p, const uint64_t *d_blk, const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index,
    hipStream_t stream);
/* ---- the line route (sre_hip_lines_route.hip, sre_lines_route.h) ---- */
/* select pass of the batch (lines i0 .. info->i1, at most nmax): d_key[i] = bucket << 56 | (len + 1), the bucket
 * d_map[rc] of the regex that matched (d_map[nreg] without a match), or 0 where the map says -1; d_map: nreg + 1 words */
hipError_t sre_launch_route_select(const int64_t *d_records, uint32_t slots, uint64_t nmax, uint64_t i0, uint32_t nreg,
    const int32_t *d_map, const uint64_t *d_ends, const sre_lines_info_t *d_info, uint64_t *d_key, hipStream_t stream);
/* d_cnt[b * nwg + w] = lines of bucket b among the SRE_LINES_ITEMS lines of workgroup w, nwg = ceil(n / SRE_LINES_ITEMS);
 * sre_launch_filter_offsets over those nbuckets * nwg words (+ 1) then makes them the first ranks */
hipError_t sre_launch_route_count(const uint64_t *d_key, uint64_t n, uint32_t nbuckets, uint64_t *d_cnt, hipStream_t stream);
/* the compact table from the scanned counts: entry r of nsel = d_first[nbuckets * nwg] is the line of rank r in the
 * bucket-major, line-ordered output: d_cstart[r] its source offset under SRE_LG_ENTRY_LAST | FIRST, d_cval[r] = len + 1,
 * d_cmeta[r] = bucket << 56 | line */
hipError_t sre_launch_route_scatter(const uint64_t *d_key, const uint64_t *d_ends, uint64_t n, uint32_t nbuckets,
    const uint64_t *d_first, uint64_t nsel, uint64_t *d_cstart, uint64_t *d_cval, uint64_t *d_cmeta, hipStream_t stream);
/* behind sre_launch_filter_offsets over d_cval (d_coff[0 .. nsel]; not read when nsel == 0): d_res[0 .. 4) = nsel, the
 * bytes of all rows, the rows that fit out_cap whole, their bytes; then [lines, bytes] of each bucket */
hipError_t sre_launch_route_finish(const uint64_t *d_first, uint64_t n, uint32_t nbuckets, const uint64_t *d_coff, uint64_t nsel,
    uint64_t out_cap, uint64_t *d_res, hipStream_t stream);
/* rows [line, start, len, output offset, bucket] of the first min(index_cap, d_res[2]) ranks; nrows: that number */
hipError_t sre_launch_route_index(const uint64_t *d_coff, const uint64_t *d_cstart, const uint64_t *d_cmeta,
    const uint64_t *d_res, uint64_t nrows, uint64_t index_cap, int64_t *d_index, hipStream_t stream);
/* ---- the line tally (sre_hip_lines_tally.hip, sre_lines_tally.h) ---- */
/* between the extract's last select pass and sre_launch_extract_offsets.  insert, a lane per line: a selected line
 * (d_val[line * k] != 0) finds or claims the slot of its key in d_tab (nslots words, all SRE_LT_EMPTY before) and leaves
 * the slot in d_lslot[line], SRE_LT_NONE for the others; d_cnt[slot] (zero before) += the lines of the slot, one add per
 * distinct slot of a wave; info->tsel, tclaims, tover (zero before).  keep, a lane per entry: d_val[e] = 0 for every
 * entry of a line that is not the final word of its slot, so the table selects the first line of every key */
hipError_t sre_launch_tally_insert(const void *d_buf, uint64_t *d_val, const uint64_t *d_start, uint64_t n, uint32_t k,
    uint64_t nslots, uint64_t max_keys, uint64_t hash_mask, uint64_t *d_tab, uint64_t *d_cnt, uint32_t *d_lslot,
    sre_lines_info_t *d_info, hipStream_t stream);
/* behind sre_launch_extract_offsets (d_off, and d_blk as it left them): the rank r of every kept line among the kept
 * lines is the number of its key: d_counts[r] = d_cnt[slot] for r < counts_cap, then d_cnt[slot] = r; and, in a second
 * kernel, d_keyid[i] = d_cnt[d_lslot[i]] for i < min(keyid_cap, n), -1 for a line without a slot */
hipError_t sre_launch_tally_ranks(const uint64_t *d_off, const uint64_t *d_start, uint64_t n, uint32_t k, const uint64_t *d_blk,
    const uint32_t *d_lslot, uint64_t *d_cnt, uint64_t *d_counts, uint64_t counts_cap, int64_t *d_keyid, uint64_t keyid_cap,
    hipStream_t stream);
/* ---- the tally's sums (sre_hip_lines_tally.hip, sre_lines_sums.h) ---- */
/* the first kernel of sre_launch_tally_ranks alone, for a call that asks for neither counts nor key ids: d_cnt[slot]
 * becomes the number of the slot's key */
hipError_t sre_launch_tally_numbers(const uint64_t *d_off, const uint64_t *d_start, uint64_t n, uint32_t k, const uint64_t *d_blk,
    const uint32_t *d_lslot, uint64_t *d_cnt, hipStream_t stream);
/* behind either: rows 0 .. rows of d_sums (sre_hip_tally_sum_t, v aggregates a row, 8-byte aligned) are set to
 * {0, INT64_MAX, INT64_MIN, 0}; then, a lane per line, the numbers of the line's v value fields (d_vval / d_vstart: the
 * entry table of sre_launch_extract_select over the value groups, n * v entries) join the aggregates of row
 * d_cnt[d_lslot[line]] when that is below rows.  A wave sends one add, minimum, maximum and add per key and column.
 * With copies > 1 (sre_ls_copies) all of this happens in d_copies, copies x rows x v aggregates, wave w in copy
 * w % copies, and a last kernel merges the copies into d_sums */
hipError_t sre_launch_tally_sums(const void *d_buf, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n, uint32_t v,
    const uint32_t *d_lslot, const uint64_t *d_cnt, uint64_t rows, void *d_sums, void *d_copies, uint32_t copies,
    hipStream_t stream);
/* ---- the key set and the line lookup (sre_hip_lines_keyset.hip, sre_lines_keyset.h) ---- */
/* behind the split of the dictionary d_rows (d_ends: its `rows` row ends), a lane per row: the fields of row r by the
 * field rule into entries r * k + f of d_fstart / d_flen; *d_bad (all ones before) = the lowest row that does not hold
 * exactly k - 1 bytes fsep */
hipError_t sre_launch_keyset_fields(const void *d_rows, const uint64_t *d_ends, uint64_t rows, uint32_t k, uint32_t fsep,
    uint64_t *d_fstart, uint64_t *d_flen, uint64_t *d_bad, hipStream_t stream);
/* the tally's insert over the dictionary's keys, a lane per row: d_tab (nslots words, all SRE_LT_EMPTY before, nslots a
 * power of two >= 2 x rows) ends with the lowest row of every key in the key's one slot; *d_distinct (zero before) += the
 * claims, one add per workgroup */
hipError_t sre_launch_keyset_insert(const void *d_rows, const uint64_t *d_fstart, const uint64_t *d_flen, uint64_t rows,
    uint32_t k, uint64_t nslots, uint64_t hash_mask, uint64_t *d_tab, uint64_t *d_distinct, hipStream_t stream);
/* between the last select pass and sre_launch_filter_offsets, a lane per line: the key of a line with one (d_vval[line * k]
 * != 0; d_vval / d_vstart: the entry table of sre_launch_extract_select over the key groups) is looked up in the set's
 * finished table with plain loads; d_keyid[i], i < min(keyid_cap, n), = the row number of the key, -1 without one in the
 * set, -2 for a line without a key; d_fval[i] stays for a selected line (a member, with invert a keyed line that is not one)
 * and becomes 0 for every other; info->knkeyed, knmembers (zero before), one add per workgroup each */
hipError_t sre_launch_keyset_probe(const void *d_buf, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n, uint32_t k,
    const void *d_rows, const uint64_t *d_fstart, const uint64_t *d_flen, const uint64_t *d_tab, uint64_t nslots,
    uint64_t hash_mask, int invert, uint64_t *d_fval, int64_t *d_keyid, uint64_t keyid_cap, sre_lines_info_t *d_info,
    hipStream_t stream);
/* ---- the key map and the line join (sre_lines_join.h) ---- */
/* sre_launch_keyset_fields for a map of nfields fields a row, the first k its key: the key fields into entries r * k + f of
 * d_fstart / d_flen, the value columns into entries r * (nfields - k) + c of d_vstart / d_vlen; k < nfields */
hipError_t sre_launch_keymap_fields(const void *d_rows, const uint64_t *d_ends, uint64_t rows, uint32_t nfields, uint32_t k,
    uint32_t fsep, uint64_t *d_fstart, uint64_t *d_flen, uint64_t *d_vstart, uint64_t *d_vlen, uint64_t *d_bad, hipStream_t stream);
/* in the place of sre_launch_keyset_probe, a lane per line: the same walk, d_keyid and counts; d_own[i], every i < n, is the
 * key id too; d_val / d_start get the P = 1 + cols->n entries of every line as sre_lj_entries gives them (n * P words; the
 * line from d_ends, the values from the map's d_mstart / d_mlen of nvalues columns a row).  `all`: the left outer join */
hipError_t sre_launch_keyset_join(const void *d_buf, const uint64_t *d_vval, const uint64_t *d_vstart, const uint64_t *d_ends,
    uint64_t n, uint32_t k, const void *d_rows, const uint64_t *d_fstart, const uint64_t *d_flen, const uint64_t *d_mstart,
    const uint64_t *d_mlen, uint32_t nvalues, const uint64_t *d_tab, uint64_t nslots, uint64_t hash_mask, const sre_lj_cols_t *cols,
    int all, uint64_t *d_val, uint64_t *d_start, int64_t *d_own, int64_t *d_keyid, uint64_t keyid_cap, sre_lines_info_t *d_info,
    hipStream_t stream);
/* the gather over the join table (behind sre_launch_extract_offsets with k = P): output bytes [0, out_bytes) of the rows to
 * d_out.  d_dict: the map's copy of the dictionary, 16-byte aligned with 16 bytes allocated behind its text (NULL: the
 * empty map) */
hipError_t sre_launch_join_gather(const void *d_buf, void *d_out, const uint64_t *d_off, const uint64_t *d_start,
    const void *d_dict, uint64_t nentries, uint64_t out_bytes, uint32_t delim, uint32_t jsep, hipStream_t stream);
/* rows [line, start, len, output offset, key id, (output offset of the value, its length) x (p - 1)] of the first
 * min(index_cap, info->fwritten) written rows; a line without a dictionary row has (-1, -1) */
hipError_t sre_launch_join_index(const uint64_t *d_off, const uint64_t *d_start, const uint64_t *d_ends, const int64_t *d_keyid,
    uint64_t n, uint32_t p, const uint64_t *d_blk, const sre_lines_info_t *d_info, uint64_t index_cap, int64_t *d_index,
    hipStream_t stream);
/* ---- the line route by key (sre_hip_lines_route_key.hip, sre_lines_route_key.h) ---- */
/* one digit pass of the stable partition, count then (behind sre_launch_filter_offsets over the nd * nwg counts, nd =
 * 2^bits, nwg = ceil(n / SRE_LINES_ITEMS)) scatter.  Pass 0 (d_keyid != NULL, d_src unused): the n lines in line order, line
 * i the item of sort key sre_lrk_sort_key(d_keyid[i], rows, all) or dropped.  A later pass (d_keyid == NULL): the n items
 * of d_src.  d_cnt[d * nwg + w] = items of digit d of workgroup w; the scatter stores every item at its rank of d_dst, which
 * holds `total` = d_first[nd * nwg] items.  rule: SRE_LRK_RANK_BITS or SRE_LRK_RANK_TURNS, with the same result */
hipError_t sre_launch_route_key_count(const int64_t *d_keyid, const uint64_t *d_src, uint64_t n, uint64_t rows, int all,
    uint32_t pass, uint32_t bits, int rule, uint64_t *d_cnt, hipStream_t stream);
hipError_t sre_launch_route_key_scatter(const int64_t *d_keyid, const uint64_t *d_src, uint64_t n, uint64_t rows, int all,
    uint32_t pass, uint32_t bits, int rule, const uint64_t *d_first, uint64_t total, uint64_t *d_dst, hipStream_t stream);
/* the compact table from the nsel sorted items: d_cstart[r] the source offset of rank r's line under SRE_LG_ENTRY_LAST |
 * FIRST, d_cval[r] = len + 1, d_head[r] = 1 where rank r is the first of its key, else 0 */
hipError_t sre_launch_route_key_table(const uint64_t *d_items, const uint64_t *d_ends, uint64_t nsel, uint64_t nlines,
    uint64_t *d_cstart, uint64_t *d_cval, uint64_t *d_head, hipStream_t stream);
/* behind sre_launch_filter_offsets over d_head (d_hoff[0 .. nsel]) and over d_cval (d_coff[0 .. nsel]): d_hrank[b] = the rank
 * of bucket b's first line, d_hrank[nbuckets] = nsel (nsel + 1 words), then rows [id, first rank, lines, output offset,
 * bytes] of the first min(buckets_cap, nbuckets) buckets */
hipError_t sre_launch_route_key_buckets(const uint64_t *d_items, const uint64_t *d_hoff, uint64_t *d_hrank, const uint64_t *d_coff,
    uint64_t nsel, uint64_t rows, uint64_t buckets_cap, int64_t *d_buckets, hipStream_t stream);
/* d_res[0 .. SRE_LRK_RES_WORDS): nsel, the bytes of all rows, the rows that fit out_cap whole, their bytes, the non-empty
 * buckets, info->knkeyed, info->knmembers.  d_coff and d_hoff are not read when nsel == 0 */
hipError_t sre_launch_route_key_finish(const uint64_t *d_coff, const uint64_t *d_hoff, uint64_t nsel, uint64_t out_cap,
    const sre_lines_info_t *d_info, uint64_t *d_res, hipStream_t stream);
/* rows [line, start, len, output offset, id or -1 / -2] of the first min(index_cap, d_res[2]) ranks; nrows: that number */
hipError_t sre_launch_route_key_index(const uint64_t *d_items, const uint64_t *d_cstart, const uint64_t *d_coff,
    const uint64_t *d_res, uint64_t rows, uint64_t nrows, uint64_t index_cap, int64_t *d_index, hipStream_t stream);
/* ---- the line sort (sre_hip_lines_sort.hip, sre_lines_sort.h) ---- */
/* behind the last select pass, a lane per line: d_value[i] and d_class[i] of every line i < n from entry i of the value table
 * of the ONE sort group (d_vval / d_vstart: the entry table of sre_launch_extract_select over that group); d_totals[0 .. 4) =
 * the keyed lines, the numbered lines, the minimum and the maximum of the values (int64_t; set to 0, 0, INT64_MAX, INT64_MIN
 * first), at most one add per count, one minimum and one maximum per workgroup of 1024 lines */
hipError_t sre_launch_sort_values(const void *d_buf, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n, int64_t *d_value,
    int8_t *d_class, uint64_t *d_totals, hipStream_t stream);
/* one digit pass of the sort, count then (behind sre_launch_filter_offsets over the 256 * nwg counts, nwg = ceil(n /
 * SRE_LINES_ITEMS)) scatter; the digit is bits pass * 8 .. pass * 8 + 7 of the 64-bit key, pass < 8.  Pass 0 (d_value != NULL,
 * d_src / d_sline unused): the n lines in line order, line i the item of key sre_lso_key(d_class[i], d_value[i], ...) from the
 * totals the host read, or dropped.  A later pass (d_value == NULL): the n items (d_src[i], d_sline[i]), total == n.
 * d_cnt[d * nwg + w] = items of digit d of workgroup w; the scatter stores the key and the line of every item at its rank of
 * d_dkey / d_dline, which hold `total` = d_first[256 * nwg] items */
hipError_t sre_launch_sort_count(const int64_t *d_value, const int8_t *d_class, const uint64_t *d_src, uint64_t n, int64_t vmin,
    int64_t vmax, uint64_t nnumbered, int desc, int all, uint32_t pass, uint64_t *d_cnt, hipStream_t stream);
hipError_t sre_launch_sort_scatter(const int64_t *d_value, const int8_t *d_class, const uint64_t *d_src, const uint32_t *d_sline,
    uint64_t n, int64_t vmin, int64_t vmax, uint64_t nnumbered, int desc, int all, uint32_t pass, const uint64_t *d_first,
    uint64_t total, uint64_t *d_dkey, uint32_t *d_dline, hipStream_t stream);
/* the compact table of the first nout ranks of the sorted items: d_cstart[r] the source offset of the line d_lines[r] under
 * SRE_LG_ENTRY_LAST | FIRST, d_cval[r] = len + 1 */
hipError_t sre_launch_sort_table(const uint32_t *d_lines, const uint64_t *d_ends, uint64_t nout, uint64_t nlines, uint64_t *d_cstart,
    uint64_t *d_cval, hipStream_t stream);
/* behind sre_launch_filter_offsets over d_cval (d_coff[0 .. nout]; not read when nout == 0): d_res[0 .. SRE_LSO_RES_WORDS) =
 * nout, the bytes of all rows, the rows that fit out_cap whole, their bytes */
hipError_t sre_launch_sort_finish(const uint64_t *d_coff, uint64_t nout, uint64_t out_cap, uint64_t *d_res, hipStream_t stream);
/* rows [line, start, len, output offset, value, class] of the first min(index_cap, d_res[2]) ranks; nrows: that number */
hipError_t sre_launch_sort_index(const uint32_t *d_lines, const uint64_t *d_cstart, const uint64_t *d_coff, const uint64_t *d_res,
    const int64_t *d_value, const int8_t *d_class, uint64_t nlines, uint64_t nrows, uint64_t index_cap, int64_t *d_index,
    hipStream_t stream);
/* ---- the line distinct (sre_hip_lines_distinct.hip, sre_lines_distinct.h) ---- */
/* behind sre_launch_tally_insert over the key table (d_lslot, and the table of nslots words it took), a lane per line:
 * d_last[slot] (nslots words, zero before) = the highest line of the slot, one atomic maximum per distinct slot of a wave */
hipError_t sre_launch_distinct_last(const uint32_t *d_lslot, uint64_t n, uint64_t nslots, uint64_t *d_last, hipStream_t stream);
/* behind it, in front of sre_launch_filter_offsets, a lane per line: d_fval[i] stays for a line sre_ld_picks selects from its
 * slot's d_tab, d_cnt and (SRE_LD_LAST only; else d_last may be NULL) d_last words, and becomes 0 for every other; a line
 * with d_lslot[i] == SRE_LT_NONE reads nothing through it.  info->dkept (zero before) += the qualifying keys, counted at
 * their first lines, one add per workgroup */
hipError_t sre_launch_distinct_pick(const uint32_t *d_lslot, uint64_t n, uint64_t nslots, const uint64_t *d_tab, const uint64_t *d_cnt,
    const uint64_t *d_last, int which, uint64_t min_count, uint64_t max_count, int invert, uint64_t *d_fval,
    sre_lines_info_t *d_info, hipStream_t stream);
/* a lane per line: d_keycount[i] = d_cnt[slot], 0 without a slot, for i < min(keycount_cap, n); d_keyline[i] = d_tab[slot], -1
 * without one, for i < min(keyline_cap, n).  Nothing is launched when both capacities are 0 */
hipError_t sre_launch_distinct_perline(const uint32_t *d_lslot, uint64_t n, uint64_t nslots, const uint64_t *d_tab,
    const uint64_t *d_cnt, uint64_t *d_keycount, uint64_t keycount_cap, int64_t *d_keyline, uint64_t keyline_cap,
    hipStream_t stream);
/* ---- the line sort by text (sre_hip_lines_sort_text.hip, sre_lines_sort_text.h) ---- */
/* the values pass of the sort over the texts of the ONE sort group (d_vval / d_vstart as above; d_buf of len bytes): a line with
 * a match has class SRE_LSO_NUMBER and as its value its compared length (sre_lst_cut under max_bytes), any other
 * SRE_LSO_NOMATCH; d_totals[0 .. 4) = the keyed lines, twice, the shortest and the longest compared length */
hipError_t sre_launch_sort_text_values(const void *d_buf, uint64_t len, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n,
    uint64_t max_bytes, int64_t *d_value, int8_t *d_class, uint64_t *d_totals, hipStream_t stream);
/* a lane per item: d_keys[i] = the key of chunk `chunk` of item i (sre_lst_line_key).  d_lines == NULL: the nitems == n lines
 * in line order, SRE_LSO_DROPPED for a line that is not selected; otherwise item i is line d_lines[i].  No byte at or past
 * len is read */
hipError_t sre_launch_sort_text_keys(const void *d_buf, uint64_t len, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n,
    uint64_t max_bytes, const uint32_t *d_lines, uint64_t nitems, uint64_t chunk, int desc, int all, uint64_t *d_keys,
    hipStream_t stream);
/* the digit pass that makes the items, count then (behind sre_launch_filter_offsets, as for sre_launch_sort_count) scatter, over
 * the keys d_lkeys of the n lines in line order: key and line number of every line whose key is not SRE_LSO_DROPPED go to its
 * rank of d_dkey / d_dline, which hold `total` items; the digit is bits pass * 8 .. pass * 8 + 7, pass < 8 */
hipError_t sre_launch_sort_text_count(const uint64_t *d_lkeys, uint64_t n, uint32_t pass, uint64_t *d_cnt, hipStream_t stream);
hipError_t sre_launch_sort_text_scatter(const uint64_t *d_lkeys, uint64_t n, uint32_t pass, const uint64_t *d_first, uint64_t total,
    uint64_t *d_dkey, uint32_t *d_dline, hipStream_t stream);
/* rows [line, start, len, output offset, field start, field length] (sre_lst_index_row) of the first min(index_cap, d_res[2])
 * ranks; nrows: that number */
hipError_t sre_launch_sort_text_index(const void *d_buf, uint64_t len, const uint64_t *d_vval, const uint64_t *d_vstart, uint64_t n,
    const uint32_t *d_lines, const uint64_t *d_cstart, const uint64_t *d_coff, const uint64_t *d_res, uint64_t nrows,
    uint64_t index_cap, int64_t *d_index, hipStream_t stream);
/* ---- the ordered tally (sre_hip_lines_tally_top.hip, sre_lines_tally_top.h) ---- */
/* behind the tally's ranks (d_cnt[slot] is the key's number), a lane per line: d_first[key] = the line the keep pass left
 * selected for the key, the one line i with d_tab[d_lslot[i]] == i; nkeys words */
hipError_t sre_launch_tally_top_first(const uint64_t *d_tab, const uint32_t *d_lslot, const uint64_t *d_cnt, uint64_t n,
    uint64_t nkeys, uint64_t *d_first, hipStream_t stream);
/* a lane per key: d_value[k] and d_class[k] (SRE_LSO_NUMBER ordered, SRE_LSO_TEXT not) of sre_ltt_order from d_counts[k] and
 * the aggregate d_sums[k * v + by_col] (sre_ls_agg_t; not read for SRE_LTT_COUNT, may be NULL then); d_totals[0 .. 4) = the
 * keys, the ordered keys, the minimum and the maximum of their values (set to 0, 0, INT64_MAX, INT64_MIN first), at most one
 * add per count, one minimum and one maximum per workgroup of 1024 keys */
hipError_t sre_launch_tally_top_values(const uint64_t *d_counts, const void *d_sums, uint64_t nkeys, uint32_t v, int by,
    uint32_t by_col, int64_t *d_value, int8_t *d_class, uint64_t *d_totals, hipStream_t stream);
/* behind the last digit pass (d_keys[r]: the key at rank r), a lane per entry of the first nrows ranks: entries r * k + f of the
 * ordered table d_cstart / d_cval (nrows * k words; d_cval one more for its scan) from the entries d_first[key] * k + f of the
 * scanned entry table d_off / d_start (n * k entries), which the ordered table may not overlap */
hipError_t sre_launch_tally_top_table(const uint32_t *d_keys, const uint64_t *d_first, const uint64_t *d_off, const uint64_t *d_start,
    uint64_t nrows, uint64_t nkeys, uint64_t n, uint32_t k, uint64_t *d_cstart, uint64_t *d_cval, hipStream_t stream);
/* a lane per rank r < nkeys, key = d_keys[r]: d_inv[key] = r; d_ocounts[r] = d_counts[key] for r < counts_rows; the v
 * aggregates of the key to d_osums[r * v ..] for r < sums_rows; the index row of sre_ltt_index_row (sre_ltt_index_words(k)
 * words) for r < index_rows, from the scanned ordered table d_cstart / d_coff.  The three row counts are at most nrows, the
 * rows of the ordered table */
hipError_t sre_launch_tally_top_permute(const uint32_t *d_keys, uint64_t nkeys, uint64_t nrows, const uint64_t *d_counts,
    const void *d_sums, uint32_t v, const uint64_t *d_first, const uint64_t *d_ends, uint64_t n, const uint64_t *d_cstart,
    const uint64_t *d_coff, uint32_t k, const int64_t *d_value, const int8_t *d_class, uint64_t *d_ocounts, uint64_t counts_rows,
    void *d_osums, uint64_t sums_rows, int64_t *d_index, uint64_t index_rows, uint32_t *d_inv, hipStream_t stream);
/* behind it, a lane per line i < m: d_rank[i] = d_inv[d_cnt[d_lslot[i]]], -1 for a line without a slot */
hipError_t sre_launch_tally_top_ranks(const uint32_t *d_lslot, const uint64_t *d_cnt, const uint32_t *d_inv, uint64_t m,
    uint64_t nkeys, int64_t *d_rank, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
