/*
 * sre_hip_batch.cpp — the additive device-resident batched API (sregex_hip.h).
 *
 * A scanner binds one compiled program, one mode and one engine:
 *   ENGINE_VM    exact bytecode VM kernel, one lane per stream (sre_hip_vm.hip)
 *   ENGINE_SCAN  table-driven segment-parallel scanner        (sre_hip_scan.hip)
 *   ENGINE_NFA   bit-parallel NFA scanner + exact VM window   (sre_hip_nfa.hip)
 * Stream pointers/lengths are staged to the device per call; results come back
 * as fixed-stride records.  Everything enqueues on the caller's hipStream_t so
 * a driver can bracket the scan with its own events.
 */
#include <sregex_hip.h>
#include "sre_hip_runtime.h"
#include "sre_hip_scan.h"
#include "sre_scan_host.h"
#include "sre_dfa.h"
#include "sre_nfa.h"
#include "sre_hip_nfa.h"
#include "sre_nfa_wide.h"
#include "sre_hip_nfa_wide.h"
#include "sre_pwave.h"
#include "sre_hip_lines.h"
#include "sre_lines_gather.h"
#include "sre_lines_route.h"
#include "sre_lines_route_key.h"
#include "sre_lines_sort.h"
#include "sre_lines_sort_text.h"
#include "sre_lines_tally.h"
#include "sre_lines_tally_top.h"
#include "sre_lines_distinct.h"
#include "sre_lines_sums.h"
#include "sre_lines_keyset.h"
#include "sre_lines_join.h"
#include "sre_hip_streams.h"
#include "sre_streams_nfa.h"
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <chrono>
#include <initializer_list>
#include <vector>

/* speculative fix-up rounds before a FIRST / Thompson scan computes exact entry states */
#define SRE_SPECULATIVE_FIXUPS 2

struct sre_hip_scanner_s {
    sre_program_t     *prog;
    sre_hip_program_s *dp;
    int                mode, engine;
    char               kernel_name[64];
    uint32_t           ovec_slots;      /* 2 * (max_ncaps + 1) */
    /* per-call staging, grown on demand */
    size_t             cap_streams;
    const void       **d_ptrs;
    uint64_t          *d_lens;
    int64_t           *d_records;
    void              *d_ctx;           /* ENGINE_VM: per-stream VM state */
    size_t             ctx_stride, ctx_cap;
    uint64_t          *h_lens;          /* pinned staging */
    const void       **h_ptrs;
    size_t             last_n;
    hipStream_t        last_stream;
    /* ENGINE_SCAN */
    sre_dfa_t                *dfa;
    sre_scan_device_tables_t *tab;
    uint32_t                  seg_override;     /* 0 = automatic */
    uint64_t                  seg_cap_env;
    sre_scan_geom_t           geom;
    uint64_t                 *d_seg_first, *h_seg_first;
    sre_seg_summary_t        *d_sum;
    sre_seg_digest_t         *d_digest;                 /* digest_cap entries, see sre_scan_geom_t.digest */
    uint64_t                  digest_cap;
    size_t                    sum_cap;
    sre_stream_status_t      *d_status, *h_status;
    void                     *d_acc;
    int64_t                  *d_lo, *h_lo;
    uint16_t                 *d_scratch;
    size_t                    scratch_cap;
    sre_seg_lineage_t        *d_maps, *d_blocks;
    size_t                    maps_cap;
    uint8_t                  *d_fn;             /* segment transition functions + compositions + entry states */
    size_t                    fn_cap;
    int                       exact_passes;     /* of the last scan (diagnostics) */
    int                       lineage_passes;   /* of the last scan (diagnostics) */
    uint32_t                  next_init_variant;    /* compat path: a re-armed context's search */
    int                       blocks_per_cu;
    hipStream_t               tail_stream;      /* sre_hip_scanner_set_tail_stream */
    bool                      tail_stream_set;
    int                       fixup_rounds;     /* of the last scan (diagnostics) */
    hipEvent_t                ev0, ev1;         /* around the dominant scan kernel */
    int                       ev_valid;
    /* results of a call travel to pinned host memory as part of the enqueued
     * work; results() waits for this event only, so a caller can queue the
     * next buffer (on another scanner) before collecting */
    sre_int_t                *h_records;
    hipEvent_t                ev_done;
    /* d_ptrs / d_lens / d_seg_first live in ONE device block (h_* in one pinned
     * block) and d_records / d_status in another, laid out per call, so that a
     * call costs one small copy in and one out */
    uint64_t                 *d_in, *h_in;
    unsigned char            *d_out, *h_out;
    /* ENGINE_NFA */
    sre_nfa_t                *nfa;
    sre_nfa_tables_t          ntab;             /* device pointers inside */
    sre_nfa_sa_tables_t       satab;            /* the shift-and form (sre_nfa.h), when the program has one */
    bool                      use_sa;
    /* the wide form (sre_nfa_wide.h), when the 64-bit form declines for width alone */
    sre_nfa_wide_t           *wnfa;
    sre_nfa_wide_tables_t     wtab;             /* device pointers inside */
    uint64_t                 *d_wsets;          /* [nsegs][2][W] entry and exit sets of the wide kernel */
    bool                      wide_kernel;      /* the wide form runs on sre_k_nfa_wide (else, as a 64-bit shift-and
                                                   form, on sre_k_nfa_sa: nfa_wide_as_sa) */
    /* find-all counting on the NFA tier (nfa_count_rounds) */
    struct NfaCount          *cnt;
    uint8_t                  *d_sflags, *h_sflags;      /* per stream of a round: SRE_SFLAG_* */
    sre_nfa_count_req_t      *d_creq, *h_creq;
    size_t                    cnt_cap;
    int                       count_rounds;             /* of the last call (diagnostics) */
    sre_pwave_hdr_t          *h_pwave;                  /* the wave form of the exact window's step (sre_pwave.h), or NULL */
    void                     *d_pwave;
    size_t                    layout_n;                 /* streams the staging blocks are laid out for */
    sre_nfa_summary_t        *d_nsum;
    size_t                    nsum_cap;
    uint64_t                 *d_belief;
    uint8_t                  *d_bvalid;
    uint64_t                 *d_nmat;           /* the segments' singleton exit sets (exact entry sets), on demand */
    size_t                    nmat_cap;
    void                     *d_nacc;
    sre_nfa_status_t         *d_nstatus, *h_nstatus;
    const uint64_t           *d_eset;           /* stream sets: [nstreams][W] per-stream entry sets of the call in flight, else NULL */
    /* line mode (sre_hip_scan_lines), grown on demand */
    uint64_t                 *d_ends;           /* line table: one end offset per line */
    size_t                    ends_cap;
    uint64_t                 *d_lblk;           /* tile counts / per-workgroup sums of the geometry and compaction */
    size_t                    lblk_cap;
    int64_t                  *d_rows;           /* reported rows */
    size_t                    rows_cap;         /* (caps in bytes) */
    sre_lines_info_t         *d_linfo, *h_linfo;
    bool                      last_lines;       /* the last call was a line-mode call */
    int                       line_batches;     /* of the last line-mode call */
    double                    lines_kernel_ms;  /* ... the sum of its scan kernels, -1 unknown */
    bool                      lines_device;     /* ... every batch ran on the device, no per-line host work */
    size_t                    short_lines;      /* ... lines the short-line kernel took (NFA tier) */
    hipEvent_t                ev_l0, ev_l1;     /* around a batch's short-line kernel */
    /* the line filter (sre_hip_filter_lines), grown on demand */
    uint64_t                 *d_fval;           /* per-line values, then the offset table: lines + 1 words */
    size_t                    fval_cap;
    uint64_t                 *d_fblk;           /* per-workgroup sums of the scan: 2 words per SRE_LINES_ITEMS lines */
    size_t                    fblk_cap;
    /* its context lines (sre_hip_filter_lines_context) add */
    uint64_t                 *d_cbits;          /* the context bitmap: one bit per line */
    size_t                    cbits_cap;
    uint64_t                 *d_cblk;           /* block words and counts of the context pass: 4 words per SRE_LINES_ITEMS lines */
    size_t                    cblk_cap;
    uint64_t                 *d_gbits;          /* the fold's two bitmaps (marked lines, heads): two bits per line */
    size_t                    gbits_cap;
    uint64_t                 *d_gblk;           /* block words and counts of the fold pass: 5 words per SRE_LINES_ITEMS lines */
    size_t                    gblk_cap;
    uint64_t                 *d_gaux;           /* the fold's word per line: a head's next head, else the record's first line */
    size_t                    gaux_cap;
    /* the line extract (sre_hip_extract_lines) shares both, sized by its entries (lines x fields), and adds */
    uint64_t                 *d_fstart;         /* per-entry source offsets under their flags: lines x fields words */
    size_t                    fstart_cap;
    /* the line substitute (sre_hip_substitute_lines) shares the three, sized by its entries (lines x (pieces + 2)), and adds */
    uint8_t                  *d_lit;            /* the literal block: SRE_SUBST_MAX_LITERAL bytes, zero behind the literals */
    uint8_t                  *h_lit;            /* the literals the block holds, so that a repeated template uploads nothing */
    size_t                    lit_len;
    bool                      lit_valid;
    /* the line route (sre_hip_route_lines): its keys are d_fval's words (one per line), the compact table's starts
     * d_fstart's (one per selected line), the scans' sums d_fblk's; it adds */
    uint64_t                 *d_rcnt;           /* per (bucket, workgroup) counts, then first ranks: nbuckets x ceil(lines / 1024) + 1 words */
    size_t                    rcnt_cap;
    uint64_t                 *d_rval;           /* the compact table's values, then its offset table: selected lines + 1 words */
    size_t                    rval_cap;
    uint64_t                 *d_rmeta;          /* ... and bucket << 56 | line of each entry, for the index */
    size_t                    rmeta_cap;
    int32_t                  *d_rmap;           /* the call's map, nregexes + 1 words */
    int32_t                  *h_rmap;           /* the map the device holds, so that a repeated map uploads nothing */
    bool                      rmap_valid;
    uint64_t                 *d_rres, *h_rres;  /* the words the host reads: SRE_LR_RES_WORDS + 2 x SRE_LR_MAX_BUCKETS */
    /* the tallies (sre_hip_tally_lines, _sums_lines, _top_lines; tally_front): the entry table is the extract's (d_fval, d_fstart,
     * d_fblk); they add */
    uint64_t                 *d_ttab;           /* the table of keys: nslots words of line numbers, then nslots counts or key numbers;
                                                   the line distinct's LAST adds a third run, the last line of every slot */
    size_t                    ttab_cap;
    uint32_t                 *d_tslot;          /* the slot of every line */
    size_t                    tslot_cap;
    /* with value groups they add a second entry table over those: lines x columns words each */
    uint64_t                 *d_vval;
    size_t                    vval_cap;
    uint64_t                 *d_vstart;
    size_t                    vstart_cap;
    sre_ls_agg_t             *d_vcopy;          /* the copies of the aggregates the waves send to: at most SRE_LS_COPY_BYTES */
    size_t                    vcopy_cap;
    /* the line join (sre_hip_join_lines): the entry table is the extract's (d_fval, d_fstart, d_fblk), sized by lines x
     * (1 + columns), the key table the lookup's (d_vval, d_vstart); it adds */
    int64_t                  *d_jkey;           /* the key id of every line, for the index */
    size_t                    jkey_cap;
    /* the line route by key (sre_hip_route_lines_by_key): the key table is the lookup's (d_vval, d_vstart), the key ids d_jkey's
     * words, the counts of a pass d_rcnt's, the compact table the route's (d_fstart, d_rval), the head ranks d_rmeta's words,
     * the scans' sums d_fblk's, the result words d_rres's; it adds */
    uint64_t                 *d_kitem[2];       /* the items of the partition, pass by pass from one to the other: selected lines
                                                   + 1 words each (the spare one ends as the scan of the head flags) */
    size_t                    kitem_cap[2];
    /* the line sort (sre_hip_sort_lines): the value table is the lookup's key table (d_vval, d_vstart), the compact table the
     * route's (d_fstart, d_rval), the result words d_rres's.  Its items are also the ordered tally's, over keys in the place of
     * lines (sort_passes): the values d_jkey's words, the keys d_kitem's, the counts of a pass d_rcnt's, the scans' sums
     * d_fblk's.  The sort by text (sre_hip_sort_lines_text) has the same arrays: d_jkey's words hold the compared lengths, then
     * the keys of the lines in the first chunk; it adds */
    int8_t                   *d_sclass;         /* the class of every item */
    size_t                    sclass_cap;
    uint32_t                 *d_sline[2];       /* the lines of the items, moved with their keys: selected items words each */
    size_t                    sline_cap[2];
    /* the ordered tally (sre_hip_tally_top_lines): the tallies' tables and the sort's items as they are (d_rcnt and d_fblk sized
     * for the passes in front of the entry table's scan), the ordered table's values d_rval's words; it adds */
    uint64_t                 *d_pcount;         /* the count of every key, in first-appearance order */
    size_t                    pcount_cap;
    sre_ls_agg_t             *d_psums;          /* ... and its aggregates: keys x columns */
    size_t                    psums_cap;
    uint64_t                 *d_pfirst;         /* ... and its first line */
    size_t                    pfirst_cap;
    uint32_t                 *d_pinv;           /* ... and its rank in the order */
    size_t                    pinv_cap;
    uint64_t                 *d_pstart;         /* the ordered table's starts: rows in front of the limit x fields words */
    size_t                    pstart_cap;
};

/* one stream of a find-all count on the NFA tier */
struct NfaCountStream {
    const uint8_t *base;
    uint64_t       n;
    uint64_t       cur;         /* where the current search began (the previous match's end) */
    uint64_t       q;           /* a clean position of that search: where the next scanned buffer starts */
    uint64_t       horizon;     /* bytes scanned per round */
    uint32_t       var_cur, var_q, mode_q;
    int64_t        count;
    bool           done, error;
    std::vector<sre_int_t> last;    /* record of the last match */
};
struct NfaCount {
    std::vector<NfaCountStream> st;
    std::vector<size_t>         active;
};

static void
scanner_release(void *data)
{
    sre_hip_scanner_t *sc = static_cast<sre_hip_scanner_t *>(data);
    delete sc->cnt;
    free(sc->h_pwave);
    if (sc->d_pwave) (void) hipFree(sc->d_pwave);
    if (sc->d_sflags) (void) hipFree(sc->d_sflags);
    if (sc->h_sflags) (void) hipHostFree(sc->h_sflags);
    if (sc->d_creq) (void) hipFree(sc->d_creq);
    if (sc->h_creq) (void) hipHostFree(sc->h_creq);
    if (sc->d_in) (void) hipFree(sc->d_in);
    if (sc->h_in) (void) hipHostFree(sc->h_in);
    if (sc->d_out) (void) hipFree(sc->d_out);
    if (sc->h_out) (void) hipHostFree(sc->h_out);
    if (sc->d_ctx) (void) hipFree(sc->d_ctx);
    if (sc->d_sum) (void) hipFree(sc->d_sum);
    if (sc->d_digest) (void) hipFree(sc->d_digest);
    if (sc->d_acc) (void) hipFree(sc->d_acc);
    if (sc->d_lo) (void) hipFree(sc->d_lo);
    if (sc->h_lo) (void) hipHostFree(sc->h_lo);
    if (sc->d_scratch) (void) hipFree(sc->d_scratch);
    if (sc->d_fn) (void) hipFree(sc->d_fn);
    if (sc->d_maps) (void) hipFree(sc->d_maps);
    if (sc->d_blocks) (void) hipFree(sc->d_blocks);
    if (sc->ev0) (void) hipEventDestroy(sc->ev0);
    if (sc->ev1) (void) hipEventDestroy(sc->ev1);
    if (sc->ev_done) (void) hipEventDestroy(sc->ev_done);
    if (sc->ev_l0) (void) hipEventDestroy(sc->ev_l0);
    if (sc->ev_l1) (void) hipEventDestroy(sc->ev_l1);
    if (sc->d_nsum) (void) hipFree(sc->d_nsum);
    if (sc->d_belief) (void) hipFree(sc->d_belief);
    if (sc->d_bvalid) (void) hipFree(sc->d_bvalid);
    if (sc->d_nmat) (void) hipFree(sc->d_nmat);
    if (sc->d_nacc) (void) hipFree(sc->d_nacc);
    if (sc->d_ends) (void) hipFree(sc->d_ends);
    if (sc->d_lblk) (void) hipFree(sc->d_lblk);
    if (sc->d_rows) (void) hipFree(sc->d_rows);
    if (sc->d_fval) (void) hipFree(sc->d_fval);
    if (sc->d_fblk) (void) hipFree(sc->d_fblk);
    if (sc->d_cbits) (void) hipFree(sc->d_cbits);
    if (sc->d_cblk) (void) hipFree(sc->d_cblk);
    if (sc->d_gbits) (void) hipFree(sc->d_gbits);
    if (sc->d_gblk) (void) hipFree(sc->d_gblk);
    if (sc->d_gaux) (void) hipFree(sc->d_gaux);
    if (sc->d_fstart) (void) hipFree(sc->d_fstart);
    if (sc->d_lit) (void) hipFree(sc->d_lit);
    free(sc->h_lit);
    if (sc->d_rcnt) (void) hipFree(sc->d_rcnt);
    if (sc->d_rval) (void) hipFree(sc->d_rval);
    if (sc->d_rmeta) (void) hipFree(sc->d_rmeta);
    if (sc->d_rmap) (void) hipFree(sc->d_rmap);
    free(sc->h_rmap);
    if (sc->d_rres) (void) hipFree(sc->d_rres);
    if (sc->h_rres) (void) hipHostFree(sc->h_rres);
    if (sc->d_ttab) (void) hipFree(sc->d_ttab);
    if (sc->d_tslot) (void) hipFree(sc->d_tslot);
    if (sc->d_vval) (void) hipFree(sc->d_vval);
    if (sc->d_vstart) (void) hipFree(sc->d_vstart);
    if (sc->d_vcopy) (void) hipFree(sc->d_vcopy);
    if (sc->d_jkey) (void) hipFree(sc->d_jkey);
    if (sc->d_kitem[0]) (void) hipFree(sc->d_kitem[0]);
    if (sc->d_kitem[1]) (void) hipFree(sc->d_kitem[1]);
    if (sc->d_sclass) (void) hipFree(sc->d_sclass);
    if (sc->d_sline[0]) (void) hipFree(sc->d_sline[0]);
    if (sc->d_sline[1]) (void) hipFree(sc->d_sline[1]);
    if (sc->d_pcount) (void) hipFree(sc->d_pcount);
    if (sc->d_psums) (void) hipFree(sc->d_psums);
    if (sc->d_pfirst) (void) hipFree(sc->d_pfirst);
    if (sc->d_pinv) (void) hipFree(sc->d_pinv);
    if (sc->d_pstart) (void) hipFree(sc->d_pstart);
    if (sc->d_linfo) (void) hipFree(sc->d_linfo);
    if (sc->h_linfo) (void) hipHostFree(sc->h_linfo);
    if (sc->ntab.accept) (void) hipFree(const_cast<uint64_t *>(sc->ntab.accept));
    if (sc->ntab.follow) (void) hipFree(const_cast<uint64_t *>(sc->ntab.follow));
    if (sc->ntab.expand) (void) hipFree(const_cast<uint64_t *>(sc->ntab.expand));
    if (sc->ntab.kind) (void) hipFree(const_cast<uint8_t *>(sc->ntab.kind));
    if (sc->satab.accept) (void) hipFree(const_cast<uint64_t *>(sc->satab.accept));
    if (sc->satab.lut) (void) hipFree(const_cast<uint64_t *>(sc->satab.lut));
    if (sc->satab.expand) (void) hipFree(const_cast<uint64_t *>(sc->satab.expand));
    if (sc->d_wsets) (void) hipFree(sc->d_wsets);
    if (sc->wtab.accept) (void) hipFree(const_cast<uint64_t *>(sc->wtab.accept));
    if (sc->wtab.lut) (void) hipFree(const_cast<uint64_t *>(sc->wtab.lut));
    if (sc->wtab.expand) (void) hipFree(const_cast<uint64_t *>(sc->wtab.expand));
    if (sc->wtab.kind) (void) hipFree(const_cast<uint8_t *>(sc->wtab.kind));
    sre_nfa_wide_free(sc->wnfa);
    sre_nfa_free(sc->nfa);
    sre_scan_tables_release(sc->tab);
    sre_dfa_free(sc->dfa);
    free(sc);
}

/* device copies of the bit-parallel tables, padded to the slice count the
 * kernel variant is compiled for */
static int
nfa_upload(sre_hip_scanner_t *sc)
{
    const sre_nfa_t *n = sc->nfa;
    const uint32_t   ns = n->nslices;           /* already rounded to a compiled variant */
    std::vector<uint64_t> fol((size_t) ns * 256, 0), exp(16 * 256, 0);
    memcpy(fol.data(), n->follow.data(), n->follow.size() * sizeof(uint64_t));
    if (n->nassert) memcpy(exp.data(), n->expand.data(), exp.size() * sizeof(uint64_t));
    uint64_t *d_acc = NULL, *d_fol = NULL, *d_exp = NULL;
    uint8_t  *d_kind = NULL;
    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_acc), 256 * sizeof(uint64_t)));
    sc->ntab.accept = d_acc;
    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_fol), fol.size() * sizeof(uint64_t)));
    sc->ntab.follow = d_fol;
    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_exp), exp.size() * sizeof(uint64_t)));
    sc->ntab.expand = d_exp;
    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_kind), 256));
    sc->ntab.kind = d_kind;
    SRE_HIP_TRY(hipMemcpy(d_acc, n->accept, 256 * sizeof(uint64_t), hipMemcpyHostToDevice));
    SRE_HIP_TRY(hipMemcpy(d_fol, fol.data(), fol.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    SRE_HIP_TRY(hipMemcpy(d_exp, exp.data(), exp.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    SRE_HIP_TRY(hipMemcpy(d_kind, n->kind, 256, hipMemcpyHostToDevice));
    sc->ntab.nbits = n->nbits;
    sc->ntab.nslices = ns;
    sc->ntab.nassert = n->nassert;
    for (int v = 0; v < 3; v++) sc->ntab.init[v] = n->init[v];
    sc->ntab.any_bits = n->any_bits;
    sc->ntab.match_bits = n->match_bits;
    if (n->sa) {
        /* the shift-and form: its own accept table and the exception lookups */
        const sre_nfa_sa_t *a = n->sa;
        sre_nfa_sa_tables_t &t = sc->satab;
        uint64_t *d_sacc = NULL, *d_lut = NULL;
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_sacc), 256 * sizeof(uint64_t)));
        t.accept = d_sacc;
        SRE_HIP_TRY(hipMemcpy(d_sacc, a->accept, 256 * sizeof(uint64_t), hipMemcpyHostToDevice));
        if (a->nlut) {
            SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_lut), a->lut.size() * sizeof(uint64_t)));
            t.lut = d_lut;
            SRE_HIP_TRY(hipMemcpy(d_lut, a->lut.data(), a->lut.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        }
        if (a->nassert) {
            /* the expansion table, compacted to the assertion bits (bits 0 .. of the mask) */
            const size_t          per = (size_t) 1 << a->nassert;
            std::vector<uint64_t> ex(16 * per);
            for (size_t ctx = 0; ctx < 16; ctx++) {
                for (size_t v = 0; v < per; v++) ex[ctx * per + v] = a->expand[ctx * 256 + v];
            }
            uint64_t *d_ex = NULL;
            SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_ex), ex.size() * sizeof(uint64_t)));
            t.expand = d_ex;
            SRE_HIP_TRY(hipMemcpy(d_ex, ex.data(), ex.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
            t.kind = sc->ntab.kind;
            t.nassert = a->nassert;
        }
        t.w64 = a->w64;
        t.carry = a->carry;
        t.masked = a->masked;
        t.evacc = a->evacc;
        t.nlut = a->nlut;
        /* v_perm_b32 selector: result byte k = byte hot[k] of the 64-bit mask {hi, lo}; selector
         * values 0..3 pick a byte of the second source (lo), 4..7 of the first (hi) */
        t.perm = 0;
        for (uint32_t k = 0; k < 4; k++) t.perm |= (k < a->nlut ? a->hot[k] : 0u) << (8 * k);
        for (int v = 0; v < 3; v++) t.init[v] = a->init[v];
        t.seed = a->seed;
        t.any_bits = a->any_bits;
        t.match_bits = a->match_bits;
        t.msrc = a->msrc;
        t.valid = a->valid;
        t.self = a->self;
        t.shift_src = a->shift_src;
        sc->use_sa = true;
    }
    return 0;
hip_failed:
    return -1;
}

/* device copies of the wide form's tables */
static int
nfa_wide_upload(sre_hip_scanner_t *sc)
{
    const sre_nfa_wide_t  *w = sc->wnfa;
    sre_nfa_wide_tables_t &t = sc->wtab;
    const uint32_t         W = w->W;
    std::vector<uint64_t>  acc((size_t) 256 * W);
    for (unsigned c = 0; c < 256; c++) {
        for (uint32_t i = 0; i < W; i++) acc[(size_t) c * W + i] = w->accept[c][i];
    }
    uint64_t *d_acc = NULL, *d_lut = NULL, *d_exp = NULL;
    uint8_t  *d_kind = NULL;
    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_acc), acc.size() * sizeof(uint64_t)));
    t.accept = d_acc;
    SRE_HIP_TRY(hipMemcpy(d_acc, acc.data(), acc.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_kind), 256));
    t.kind = d_kind;
    SRE_HIP_TRY(hipMemcpy(d_kind, w->kind, 256, hipMemcpyHostToDevice));
    if (w->nlut) {
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_lut), w->lut.size() * sizeof(uint64_t)));
        t.lut = d_lut;
        SRE_HIP_TRY(hipMemcpy(d_lut, w->lut.data(), w->lut.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    if (w->nassert) {
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_exp), w->expand.size() * sizeof(uint64_t)));
        t.expand = d_exp;
        SRE_HIP_TRY(hipMemcpy(d_exp, w->expand.data(), w->expand.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    t.W = W;
    t.nlut = w->nlut;
    t.nassert = w->nassert;
    for (uint32_t k = 0; k < 16; k++) t.hot[k] = w->hot[k];
    memcpy(t.init, w->init, sizeof(t.init));
    memcpy(t.seed, w->seed, sizeof(t.seed));
    memcpy(t.any_bits, w->any_bits, sizeof(t.any_bits));
    memcpy(t.match_bits, w->match_bits, sizeof(t.match_bits));
    memcpy(t.msrc, w->msrc, sizeof(t.msrc));
    memcpy(t.valid, w->valid, sizeof(t.valid));
    memcpy(t.self, w->self, sizeof(t.self));
    memcpy(t.shift_src, w->shift_src, sizeof(t.shift_src));
    return 0;
hip_failed:
    return -1;
}

/* A wide form of ONE word without look-ahead assertions and with at most three lookups is a 64-bit shift-and
 * form (sre_nfa.h): masked, carried across the two halves, MATCH as event sources — it runs on the compiled
 * sre_k_nfa_sa<W64, W64, true, true, NLUT, false> instead of the wide kernel (the 64-bit builder declined the
 * program only because it counts threads before merging) */
static bool
nfa_wide_fits_sa(const sre_nfa_wide_t *w)
{
    return w->W == 1 && w->nassert == 0 && w->nlut <= SRE_NFA_SA_MAX_LUT;
}

static int
nfa_wide_as_sa(sre_hip_scanner_t *sc)
{
    const sre_nfa_wide_t *w = sc->wnfa;
    sre_nfa_sa_tables_t  &t = sc->satab;
    uint64_t              acc[256];
    for (unsigned c = 0; c < 256; c++) acc[c] = w->accept[c][0];
    uint64_t *d_sacc = NULL, *d_lut = NULL;
    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_sacc), sizeof(acc)));
    t.accept = d_sacc;
    SRE_HIP_TRY(hipMemcpy(d_sacc, acc, sizeof(acc), hipMemcpyHostToDevice));
    if (w->nlut) {
        /* [nlut][256][1]: the layout of the 64-bit form's lookups */
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_lut), w->lut.size() * sizeof(uint64_t)));
        t.lut = d_lut;
        SRE_HIP_TRY(hipMemcpy(d_lut, w->lut.data(), w->lut.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    t.w64 = w->nbits > 32;
    t.carry = t.w64;
    t.masked = 1;
    t.evacc = 1;
    t.nlut = w->nlut;
    t.perm = 0;
    for (uint32_t k = 0; k < w->nlut; k++) t.perm |= w->hot[k] << (8 * k);     /* hot bytes < 4 unless w64 */
    for (int v = 0; v < 3; v++) t.init[v] = w->init[v][0];
    t.seed = w->seed[0];
    t.any_bits = w->any_bits[0];
    t.match_bits = 0;
    t.msrc = w->msrc[0];
    t.valid = w->valid[0];
    t.self = w->self[0];
    t.shift_src = w->shift_src[0];
    t.nassert = 0;
    sc->use_sa = true;
    return 0;
hip_failed:
    return -1;
}

/* 64-bit words per set of the NFA tier's kernel */
static uint32_t
nfa_words(const sre_hip_scanner_t *sc)
{
    return sc->wide_kernel ? sc->wtab.W : 1u;
}

/* one pass of the set kernel the scanner's program runs on */
static hipError_t
nfa_launch_scan(sre_hip_scanner_t *sc, const int64_t *d_lo, const uint64_t *d_belief, const uint8_t *d_bvalid,
                hipStream_t stream)
{
    if (sc->wide_kernel) return sre_launch_nfa_wide_scan(sc->wtab, sc->geom, sc->d_nsum, sc->d_wsets, d_lo, d_belief, d_bvalid, sc->d_eset, stream);
    if (sc->use_sa) return sre_launch_nfa_sa_scan(sc->satab, sc->geom, sc->d_nsum, d_lo, d_belief, d_bvalid, sc->d_eset, stream);
    return sre_launch_nfa_scan(sc->mode == SRE_HIP_THOMPSON ? SRE_HIP_THOMPSON : SRE_HIP_PIKE_FIRST, sc->ntab, sc->geom,
                               sc->d_nsum, d_lo, d_belief, d_bvalid, sc->d_eset, stream);
}

extern "C" SRE_API int
sre_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" SRE_API int
sre_hip_set_device(int ordinal)
{
    hipError_t e = hipSetDevice(ordinal);
    return e == hipSuccess ? 0 : sre_hip_fail("hipSetDevice", e);
}

static sre_hip_scanner_t *scanner_create(sre_pool_t *pool, sre_program_t *prog, int mode, int engine, int chunk_twins);

extern "C" SRE_API sre_hip_scanner_t *
sre_hip_scanner_create(sre_pool_t *pool, sre_program_t *prog, int mode, int engine)
{
    return scanner_create(pool, prog, mode, engine, 0);
}

/* The scanner of a stream that is fed in CHUNKS (sre_vm_api.cpp): table-driven only, its
 * automaton built with the states a chunk boundary makes of look-ahead lists
 * (sre_dfa.h `rekind`).  NULL when the program is not admitted. */
extern "C" sre_hip_scanner_t *
sre_hip_scanner_create_chunked(sre_pool_t *pool, sre_program_t *prog, int mode)
{
    if (sre_hip_ready() != 0) return NULL;
    return scanner_create(pool, prog, mode, SRE_HIP_ENGINE_AUTO, 1);
}

/* the entry state of the next chunk: `state` is what the previous chunk's tail reported,
 * flags = the context's 0: neither, 1: seen_newline, 2: seen_word; 3: sre_vm_thompson_exec */
extern "C" uint32_t
sre_hip_scanner_chunk_entry(sre_hip_scanner_t *sc, uint32_t state, int flags)
{
    if (sc->dfa == NULL || sc->dfa->rekind.empty() || state >= sc->dfa->nstates || flags < 0 || flags > 3) return state;
    return sc->dfa->rekind[4 * (size_t) state + (size_t) flags];
}

static sre_hip_scanner_t *
scanner_create(sre_pool_t *pool, sre_program_t *prog, int mode, int engine, int chunk_twins)
{
    if (mode < SRE_HIP_THOMPSON || mode > SRE_HIP_PIKE_COUNT) return NULL;
    sre_hip_program_s *dp = sre_hip_program_get(prog);
    if (dp == NULL) return NULL;

    sre_hip_scanner_t *sc = static_cast<sre_hip_scanner_t *>(calloc(1, sizeof(*sc)));
    if (sc == NULL) return NULL;
    sc->prog = prog;
    sc->dp = dp;
    sc->mode = mode;
    uint32_t maxcaps = 0;
    for (uint32_t i = 0; i < prog->nregexes; i++) {
        if (prog->multi_ncaps[i] > maxcaps) maxcaps = prog->multi_ncaps[i];
    }
    sc->ovec_slots = 2 * (maxcaps + 1);
    sc->engine = SRE_HIP_ENGINE_VM;

    if (engine == SRE_HIP_ENGINE_AUTO || engine == SRE_HIP_ENGINE_SCAN) {
        /* compile step: step automaton + device tables (independent of any input) */
        const char *why = NULL;
        sc->dfa = sre_dfa_build2(prog, 4 * SRE_SCAN_MAX_STATES, chunk_twins, &why);
        if (sc->dfa) sc->tab = sre_scan_tables_build(prog, sc->dfa, mode, &why);
        if (sc->tab) {
            sc->engine = SRE_HIP_ENGINE_SCAN;
        } else if (engine == SRE_HIP_ENGINE_SCAN) {
            fprintf(stderr, "[sregex-hip] table-driven scanner not available: %s\n",
                    why ? why : "unknown");
            scanner_release(sc);
            return NULL;
        }
    }
    if (chunk_twins && sc->engine != SRE_HIP_ENGINE_SCAN) {
        scanner_release(sc);
        return NULL;
    }
    if (sc->engine == SRE_HIP_ENGINE_VM && (engine == SRE_HIP_ENGINE_AUTO || engine == SRE_HIP_ENGINE_NFA)) {
        /* the ordered-list automaton is too large (or was not asked for): the
         * bit-parallel form, if the program has one */
        const char *why = NULL;
        sc->nfa = sre_nfa_build(prog, &why);
        if (sc->nfa == NULL && why != NULL && strncmp(why, "more than 64", 12) == 0) {
            /* declined for width alone: the wide form counts its bits after merging (sre_nfa_wide.h) */
            const char *e = getenv("SRE_HIP_NFA_WIDE");     /* build options (tests) */
            sc->wnfa = sre_nfa_wide_build(prog, e ? (unsigned) strtoul(e, NULL, 0) : 0u, &why);
            if (sc->wnfa && mode == SRE_HIP_PIKE_COUNT
                && (sc->wnfa->nassert || memcmp(sc->wnfa->init[1], sc->wnfa->init[2], sizeof(sc->wnfa->init[1])) != 0)) {
                /* the 64-bit tier's find-all restrictions (below) */
                why = sc->wnfa->nassert ? "find-all counting of a look-ahead program the step automaton declines"
                                        : "find-all counting of a program whose initial closure depends on ^ (re-armed searches skip newlines)";
                sre_nfa_wide_free(sc->wnfa);
                sc->wnfa = NULL;
            }
        }
        if (sc->nfa && mode == SRE_HIP_PIKE_COUNT && (sc->nfa->nassert || sc->nfa->init[1] != sc->nfa->init[2])) {
            /* Find-all on this tier restarts searches in the middle of the stream.  A re-armed search
             * that does not start behind a newline holds the bare ".*?" list as its initial-state
             * snapshot, so the reference's leading-byte skip (sre_vm_pike.c:256-309) fires at every
             * idle position and jumps over newlines whose consumption would have listed the threads
             * behind ^: `^b+` over "b x\n\nb" finds one match, not two.  Thread SETS step every byte and
             * cannot know which positions the reference never visits, so programs whose seeded closure
             * depends on ^ keep the exact VM for find-all (found by the tier's own differential test);
             * so do look-ahead programs, whose re-armed context carries seen_word (:472-473). */
            why = sc->nfa->nassert ? "find-all counting of a look-ahead program the step automaton declines"
                                   : "find-all counting of a program whose initial closure depends on ^ (re-armed searches skip newlines)";
            sre_nfa_free(sc->nfa);
            sc->nfa = NULL;
        }
        if (sc->wnfa) sc->wide_kernel = !nfa_wide_fits_sa(sc->wnfa);
        if ((sc->nfa && nfa_upload(sc) == 0)
            || (sc->wnfa && (sc->wide_kernel ? nfa_wide_upload(sc) : nfa_wide_as_sa(sc)) == 0)) {
            sc->engine = SRE_HIP_ENGINE_NFA;
            if (mode == SRE_HIP_PIKE_COUNT) sc->cnt = new NfaCount();
            if (mode != SRE_HIP_THOMPSON && getenv("SRE_HIP_NO_PWAVE") == NULL) {
                /* the exact window's step by a wavefront, when the program has the form */
                sc->h_pwave = sre_pwave_build(prog);
                if (sc->h_pwave && !sre_pwave_fits(sc->h_pwave)) {
                    free(sc->h_pwave);
                    sc->h_pwave = NULL;
                }
                if (sc->h_pwave
                    && (hipMalloc(&sc->d_pwave, sc->h_pwave->bytes) != hipSuccess
                        || hipMemcpy(sc->d_pwave, sc->h_pwave, sc->h_pwave->bytes, hipMemcpyHostToDevice) != hipSuccess))
                {
                    if (sc->d_pwave) (void) hipFree(sc->d_pwave);
                    sc->d_pwave = NULL;
                    free(sc->h_pwave);
                    sc->h_pwave = NULL;
                }
            }
        } else if (engine == SRE_HIP_ENGINE_NFA) {
            fprintf(stderr, "[sregex-hip] bit-parallel NFA scanner not available: %s\n",
                    why ? why : "device allocation failed");
            scanner_release(sc);
            return NULL;
        }
    }
    sc->ctx_stride = mode == SRE_HIP_THOMPSON ? dp->thompson_layout.total : dp->pike_layout.total;
    if (sc->engine == SRE_HIP_ENGINE_VM && mode != SRE_HIP_THOMPSON && getenv("SRE_HIP_NO_PWAVE") == NULL) {
        /* the exact VM's Pike scans by a wavefront per stream, when the program has the form (sre_pwave.h) */
        sc->h_pwave = sre_pwave_build(prog);
        if (sc->h_pwave && !sre_pwave_fits(sc->h_pwave)) {
            free(sc->h_pwave);
            sc->h_pwave = NULL;
        }
        if (sc->h_pwave
            && (hipMalloc(&sc->d_pwave, sc->h_pwave->bytes) != hipSuccess
                || hipMemcpy(sc->d_pwave, sc->h_pwave, sc->h_pwave->bytes, hipMemcpyHostToDevice) != hipSuccess))
        {
            if (sc->d_pwave) (void) hipFree(sc->d_pwave);
            sc->d_pwave = NULL;
            free(sc->h_pwave);
            sc->h_pwave = NULL;
        }
    }

    if (sre_pool_add_cleanup(pool, scanner_release, sc) != SRE_OK) {
        scanner_release(sc);
        return NULL;
    }
    return sc;
}

extern "C" SRE_API int
sre_hip_scanner_engine(sre_hip_scanner_t *sc)
{
    return sc->engine;
}

extern "C" SRE_API size_t
sre_hip_scanner_result_slots(sre_hip_scanner_t *sc)
{
    return 2 + (size_t) sc->ovec_slots;
}

extern "C" SRE_API int
sre_hip_scanner_set_segment_bytes(sre_hip_scanner_t *sc, size_t bytes)
{
    if (bytes != 0 && (bytes % 64 != 0 || bytes > (1u << 30))) return -1;
    sc->seg_override = (uint32_t) bytes;
    return 0;
}

extern "C" SRE_API int
sre_hip_scanner_last_fixups(sre_hip_scanner_t *sc)
{
    return sc->fixup_rounds;
}

extern "C" SRE_API int
sre_hip_scanner_last_exact_passes(sre_hip_scanner_t *sc)
{
    return sc->exact_passes;
}

extern "C" SRE_API int
sre_hip_scanner_nfa_bits(sre_hip_scanner_t *sc)
{
    if (sc->engine != SRE_HIP_ENGINE_NFA) return 0;
    return 64 * (int) nfa_words(sc);
}

extern "C" SRE_API int
sre_hip_scanner_class_bits(sre_hip_scanner_t *sc)
{
    return sc->engine == SRE_HIP_ENGINE_SCAN ? (int) sc->tab->h.class_bits : 0;
}

extern "C" SRE_API const char *
sre_hip_scanner_kernel_name(sre_hip_scanner_t *sc)
{
    if (sc->kernel_name[0] == 0) {
        if (sc->engine == SRE_HIP_ENGINE_SCAN) {
            snprintf(sc->kernel_name, sizeof(sc->kernel_name), "sre_k_scan<%d, %d, %s, %s>",
                     sc->mode == SRE_HIP_PIKE_COUNT ? 2 : 1, (int) sc->tab->h.class_bits,
                     sc->tab->h.wide ? "true" : "false",
                     sc->mode == SRE_HIP_PIKE_COUNT && sc->tab->h.any_fresh ? "true" : "false");
        } else if (sc->engine == SRE_HIP_ENGINE_NFA) {
            if (sc->wide_kernel) sre_nfa_wide_kernel_name(&sc->wtab, sc->kernel_name, sizeof(sc->kernel_name));
            else if (sc->use_sa) sre_nfa_sa_kernel_name(&sc->satab, sc->kernel_name, sizeof(sc->kernel_name));
            else sre_nfa_kernel_name(sc->mode == SRE_HIP_THOMPSON ? 0 : 1, sc->ntab.nslices, sc->ntab.nassert != 0,
                                     sc->kernel_name, sizeof(sc->kernel_name));
        } else {
            snprintf(sc->kernel_name, sizeof(sc->kernel_name), "%s",
                     sc->mode == SRE_HIP_THOMPSON ? (sc->dp->has_wave ? "sre_k_thompson_wave_scan" : "sre_k_thompson_scan")
                                                  : sc->d_pwave ? "sre_k_pike_scan_wave" : "sre_k_pike_scan");
        }
    }
    return sc->kernel_name;
}

extern "C" SRE_API int
sre_hip_scanner_last_lineage_passes(sre_hip_scanner_t *sc)
{
    return sc->lineage_passes;
}

extern "C" SRE_API double
sre_hip_scanner_last_kernel_ms(sre_hip_scanner_t *sc)
{
    float ms = 0.0f;
    if (sc->last_lines) return sc->lines_kernel_ms;
    if (!sc->ev_valid) return -1.0;
    if (hipEventSynchronize(sc->ev1) != hipSuccess) return -1.0;
    if (hipEventElapsedTime(&ms, sc->ev0, sc->ev1) != hipSuccess) return -1.0;
    return (double) ms;
}

extern "C" SRE_API int
sre_hip_scanner_order_after_scan(sre_hip_scanner_t *sc, void *hip_stream)
{
    if (!sc->ev_valid) return 0;
    hipError_t e = hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), sc->ev1, 0);
    return e == hipSuccess ? 0 : sre_hip_fail("hipStreamWaitEvent", e);
}

extern "C" SRE_API int
sre_hip_scanner_set_tail_stream(sre_hip_scanner_t *sc, void *hip_stream)
{
    sc->tail_stream = static_cast<hipStream_t>(hip_stream);
    sc->tail_stream_set = hip_stream != NULL;
    return 0;
}

extern "C" SRE_API size_t
sre_hip_scanner_last_segment_bytes(sre_hip_scanner_t *sc)
{
    return sc->engine != SRE_HIP_ENGINE_VM ? sc->geom.seg_bytes : 0;
}

static size_t
record_bytes(const sre_hip_scanner_t *sc, size_t n)
{
    return n * (2 + (size_t) sc->ovec_slots) * sizeof(int64_t);
}

static int
scanner_reserve(sre_hip_scanner_t *sc, size_t n)
{
    if (n > sc->cap_streams) {
        if (sc->d_in) (void) hipFree(sc->d_in);
        if (sc->h_in) (void) hipHostFree(sc->h_in);
        if (sc->d_out) (void) hipFree(sc->d_out);
        if (sc->h_out) (void) hipHostFree(sc->h_out);
        if (sc->d_acc) (void) hipFree(sc->d_acc);
        if (sc->d_lo) (void) hipFree(sc->d_lo);
        if (sc->h_lo) (void) hipHostFree(sc->h_lo);
        sc->d_in = sc->h_in = NULL;
        sc->d_out = sc->h_out = NULL;
        sc->d_acc = NULL;
        sc->d_lo = sc->h_lo = NULL;
        sc->cap_streams = 0;
        const size_t in_bytes = (3 * n + 1) * sizeof(uint64_t);
        const size_t out_bytes = record_bytes(sc, n) + n * sizeof(sre_stream_status_t);   /* >= sre_nfa_status_t */
        static_assert(sizeof(sre_nfa_status_t) <= sizeof(sre_stream_status_t), "status block");
        static_assert(sizeof(sre_nfa_status_t) == sizeof(sre_nfa_window_t), "window layout");
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_in), in_bytes));
        SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sc->h_in), in_bytes, 0));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_out), out_bytes));
        SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sc->h_out), out_bytes, 0));
        SRE_HIP_TRY(hipMalloc(&sc->d_acc, sre_scan_verify_acc_bytes((uint32_t) n)));
        SRE_HIP_TRY(sre_scan_verify_acc_init(sc->d_acc, (uint32_t) n, NULL));
        if (sc->engine == SRE_HIP_ENGINE_NFA) {
            if (sc->d_nacc) (void) hipFree(sc->d_nacc);
            sc->d_nacc = NULL;
            SRE_HIP_TRY(hipMalloc(&sc->d_nacc, sre_nfa_verify_acc_bytes((uint32_t) n)));
            SRE_HIP_TRY(sre_nfa_verify_acc_init(sc->d_nacc, (uint32_t) n, NULL));
        }
        SRE_HIP_TRY(hipStreamSynchronize(NULL));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_lo), n * sizeof(int64_t)));
        SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sc->h_lo), n * sizeof(int64_t), 0));
        sc->cap_streams = n;
    }
    /* this call's layout: [ptrs n][lens n][seg_first n + 1] and [records n][status n] */
    sc->layout_n = n;
    sc->h_ptrs = reinterpret_cast<const void **>(sc->h_in);
    sc->h_lens = sc->h_in + n;
    sc->h_seg_first = sc->h_in + 2 * n;
    sc->d_ptrs = reinterpret_cast<const void **>(sc->d_in);
    sc->d_lens = sc->d_in + n;
    sc->d_seg_first = sc->d_in + 2 * n;
    sc->d_records = reinterpret_cast<sre_int_t *>(sc->d_out);
    sc->h_records = reinterpret_cast<sre_int_t *>(sc->h_out);
    sc->d_status = reinterpret_cast<sre_stream_status_t *>(sc->d_out + record_bytes(sc, n));
    sc->h_status = reinterpret_cast<sre_stream_status_t *>(sc->h_out + record_bytes(sc, n));
    sc->d_nstatus = reinterpret_cast<sre_nfa_status_t *>(sc->d_status);
    sc->h_nstatus = reinterpret_cast<sre_nfa_status_t *>(sc->h_status);
    /* (the NFA tier's exact window takes contexts only when the program has no wave form: nfa_windows) */
    if ((sc->engine == SRE_HIP_ENGINE_VM || (sc->engine == SRE_HIP_ENGINE_NFA && sc->mode != SRE_HIP_THOMPSON && sc->d_pwave == NULL))
        && n * sc->ctx_stride > sc->ctx_cap)
    {
        if (sc->d_ctx) (void) hipFree(sc->d_ctx);
        sc->d_ctx = NULL;
        sc->ctx_cap = 0;
        SRE_HIP_TRY(hipMalloc(&sc->d_ctx, n * sc->ctx_stride));
        sc->ctx_cap = n * sc->ctx_stride;
    }
    return 0;
hip_failed:
    return -1;
}

/* the fixed segment size (sre_hip_scanner_set_segment_bytes, else the experiment knob
 * SRE_HIP_SEG_BYTES), 0 = automatic; also reads SRE_HIP_SEG_CAP */
static uint64_t
scan_seg_knobs(sre_hip_scanner_t *sc)
{
    uint64_t seg = sc->seg_override;
    const char *e = getenv("SRE_HIP_SEG_BYTES");        /* experiment knobs */
    if (seg == 0 && e && atoi(e) > 0 && atoi(e) % 256 == 0) seg = (uint64_t) atoi(e);
    e = getenv("SRE_HIP_SEG_CAP");
    sc->seg_cap_env = e && atoi(e) > 0 ? (uint64_t) atoi(e) : 0;
    return seg;
}

/* ... on the NFA tier: the set kernels take any multiple of the 64-byte round (tests cut streams into
 * segments that are shorter than the warm-up) */
static uint64_t
nfa_seg_knobs(sre_hip_scanner_t *sc)
{
    uint64_t seg = scan_seg_knobs(sc);
    const char *e = getenv("SRE_HIP_SEG_BYTES");
    if (seg == 0 && e && atoi(e) > 0 && atoi(e) % 64 == 0) seg = (uint64_t) atoi(e);
    return seg;
}

/* the longest automatic segment (behind scan_seg_knobs: SRE_HIP_SEG_CAP) */
static uint64_t
scan_seg_cap(const sre_hip_scanner_t *sc)
{
    return sc->seg_cap_env ? sc->seg_cap_env : 40960;
}

/* the events around the dominant scan kernel */
static int
scan_events(sre_hip_scanner_t *sc)
{
    if (sc->ev0 == NULL) {
        SRE_HIP_TRY(hipEventCreate(&sc->ev0));
        SRE_HIP_TRY(hipEventCreate(&sc->ev1));
    }
    return 0;
hip_failed:
    return -1;
}

/* a call begins: the diagnostics describe it alone */
static void
call_begin(sre_hip_scanner_t *sc)
{
    sc->last_lines = false;
    sc->fixup_rounds = 0;
    sc->exact_passes = 0;
    sc->lineage_passes = 0;
    sc->ev_valid = 0;
}

/* A call's geometry begins cleared, the side channel sc->d_eset with it: what a call adds on top (the
 * digest, sentry, sflags, the per-stream entry sets) it sets afterwards, and nothing of the call before
 * is left to undo */
static void
geom_clear(sre_hip_scanner_t *sc)
{
    sc->geom = sre_scan_geom_t();
    sc->d_eset = NULL;
}

/* the geometry of a batch whose stream arrays a kernel wrote into d_ptrs / d_lens / d_seg_first
 * (never SRE_GEOM_ONE: the arrays live on the device) */
static void
geom_device(sre_hip_scanner_t *sc, uint64_t n, uint64_t seg, uint64_t nsegs)
{
    geom_clear(sc);
    sc->geom.streams = reinterpret_cast<const uint8_t *const *>(sc->d_ptrs);
    sc->geom.lens = sc->d_lens;
    sc->geom.seg_first = sc->d_seg_first;
    sc->geom.nstreams = (uint32_t) n;
    sc->geom.seg_bytes = (uint32_t) seg;
    sc->geom.nsegs = nsegs;
}

/* lanes the chip holds at once with this scanner's kernel */
static uint64_t
scan_resident(sre_hip_scanner_t *sc)
{
    if (sc->blocks_per_cu == 0) {
        sc->blocks_per_cu = sc->engine == SRE_HIP_ENGINE_NFA
                                ? (sc->wide_kernel ? sre_nfa_wide_blocks_per_cu(&sc->wtab)
                                   : sc->use_sa ? sre_nfa_sa_blocks_per_cu(&sc->satab)
                                              : sre_nfa_blocks_per_cu(sc->mode == SRE_HIP_THOMPSON ? 0 : 1, sc->ntab.nslices,
                                                                      sc->ntab.nassert != 0))
                                                             : sre_scan_blocks_per_cu(&sc->tab->h);
    }
    return (uint64_t) sre_hip_cu_count() * (uint64_t) sc->blocks_per_cu * SRE_SCAN_BLOCK;
}

static int scan_buffers(sre_hip_scanner_t *sc, size_t nstreams, uint64_t seg, uint64_t nsegs);

/* the NFA tier's per-call buffers: summaries, beliefs, the wide kernel's sets */
static int
nfa_buffers(sre_hip_scanner_t *sc, uint64_t nsegs)
{
    if (nsegs > sc->nsum_cap) {
        if (sc->d_nsum) (void) hipFree(sc->d_nsum);
        if (sc->d_belief) (void) hipFree(sc->d_belief);
        if (sc->d_bvalid) (void) hipFree(sc->d_bvalid);
        if (sc->d_wsets) (void) hipFree(sc->d_wsets);
        sc->d_nsum = NULL;
        sc->d_belief = NULL;
        sc->d_bvalid = NULL;
        sc->d_wsets = NULL;
        sc->nsum_cap = 0;
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_nsum), nsegs * sizeof(sre_nfa_summary_t)));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_belief), nsegs * nfa_words(sc) * sizeof(uint64_t)));
        if (sc->wide_kernel) SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_wsets), nsegs * 2 * nfa_words(sc) * sizeof(uint64_t)));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_bvalid), nsegs));
        sc->nsum_cap = nsegs;
    }
    return 0;
hip_failed:
    return -1;
}

/* segment geometry: one lane per segment, 256 lanes per workgroup.  The number
 * of workgroups is steered towards a whole multiple of what the chip holds at
 * once (LDS-limited: 160 KiB per CU), so the last round of workgroups is not
 * mostly empty; segments are a multiple of the 64-byte tile and at least 1 KiB
 * so that the speculative warm-up stays a few percent.  The batch is the one the host
 * described in h_ptrs / h_lens; init_variant, flags (SRE_GEOM_CONTINUES / _NO_EOF) and
 * entry_state are the call's. */
static int
scan_geometry(sre_hip_scanner_t *sc, size_t nstreams, uint32_t init_variant, uint32_t flags, uint32_t entry_state)
{
    uint64_t total = 0;
    for (size_t i = 0; i < nstreams; i++) total += sc->h_lens[i];
    uint64_t seg = scan_seg_knobs(sc);
    if (seg == 0) {
        /* as few rounds of resident workgroups as keep a segment <= ~40 KiB: longer
         * segments mean fewer summaries to verify and a smaller share of warm-up,
         * shorter ones keep every CU busy on small batches */
        const uint64_t resident = scan_resident(sc);
        /* (measured, one box, 4 GiB: the COUNT kernel at two workgroups per CU takes 1.33 ms
         * with 16 640-byte segments = two rounds of resident workgroups, 1.25 ms with 33 280 =
         * one round, and 1.67 ms with 21 760 = one and a half: a whole number of rounds
         * matters, and one long round beats two short ones; profiles/r02_experiments.txt) */
        /* (sre_scan_auto_segment:) ... and a few workgroup slots are left spare: a grid that
         * needs EVERY slot of its last round waits a whole extra round for the stragglers when
         * anything else (the tail kernels of the previous call) holds a slot at launch — 509
         * workgroups on 512 slots ran 30 % slower than 505.  A small batch does not fill the
         * chip whatever the segment size, and a lane's walk is a serial chain (~1.5 us per
         * 64-byte round): short segments, although half of what such a lane reads is then
         * warm-up (a 1 MiB chunk: 35 us at 1 KiB, 13 us at 256 B).  Rows that are a multiple
         * of 4 KiB apart land on the same HBM channels. */
        seg = sre_scan_auto_segment(total, resident, scan_seg_cap(sc));
    }
    uint64_t nsegs = 0;
    for (size_t i = 0; i < nstreams; i++) {
        sc->h_seg_first[i] = nsegs;
        uint64_t k = (sc->h_lens[i] + seg - 1) / seg;
        nsegs += k ? k : 1;             /* an empty stream still takes its EOF step */
    }
    sc->h_seg_first[nstreams] = nsegs;
    geom_clear(sc);
    sc->geom.streams = reinterpret_cast<const uint8_t *const *>(sc->d_ptrs);
    sc->geom.lens = sc->d_lens;
    sc->geom.seg_first = sc->d_seg_first;
    sc->geom.nstreams = (uint32_t) nstreams;
    sc->geom.seg_bytes = (uint32_t) seg;
    sc->geom.nsegs = nsegs;
    sc->geom.init_variant = init_variant;
    sc->geom.entry_state = entry_state;
    /* one stream: described in the kernel arguments, nothing to upload (table-driven
     * scanner; the NFA tier's window kernel reads the arrays) */
    sc->geom.one_ptr = static_cast<const uint8_t *>(sc->h_ptrs[0]);
    sc->geom.one_len = sc->h_lens[0];
    sc->geom.flags = flags | ((nstreams == 1 && sc->engine == SRE_HIP_ENGINE_SCAN) ? SRE_GEOM_ONE : 0u);

    if (sc->engine == SRE_HIP_ENGINE_NFA) return nfa_buffers(sc, nsegs);
    return scan_buffers(sc, nstreams, seg, nsegs);
}

/* the table-driven scanner's per-call buffers: summaries, their digests (not COUNT: sets
 * geom.digest), the capture walker's scratch */
static int
scan_buffers(sre_hip_scanner_t *sc, size_t nstreams, uint64_t seg, uint64_t nsegs)
{
    if (nsegs > sc->sum_cap) {
        if (sc->d_sum) (void) hipFree(sc->d_sum);
        sc->d_sum = NULL;
        sc->sum_cap = 0;
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_sum), nsegs * sizeof(sre_seg_summary_t)));
        sc->sum_cap = nsegs;
    }
    /* FIRST / Thompson: a digest per segment (sre_scan_record.h).  The scan writes it for every segment and the
     * record only where the digest does not say it all; the chain check reads digests alone.  Without the buffer
     * (COUNT, or no memory for it) every record is stored and read as it is. */
    sc->geom.digest = NULL;
    if (sc->mode != SRE_HIP_PIKE_COUNT) {
        if (nsegs > sc->digest_cap) {
            const uint64_t want = nsegs > SRE_VERIFY_ONE_SEGS ? nsegs : SRE_VERIFY_ONE_SEGS;
            if (sc->d_digest) (void) hipFree(sc->d_digest);
            sc->d_digest = NULL;
            sc->digest_cap = 0;
            if (hipMalloc(reinterpret_cast<void **>(&sc->d_digest), want * sizeof(sre_seg_digest_t)) == hipSuccess) {
                sc->digest_cap = want;
            } else {
                sc->d_digest = NULL;
                (void) hipGetLastError();
            }
        }
        sc->geom.digest = sc->d_digest;
    }
    {
        size_t need = nstreams * ((size_t) seg + 16);
        if (need > sc->scratch_cap) {
            if (sc->d_scratch) (void) hipFree(sc->d_scratch);
            sc->d_scratch = NULL;
            sc->scratch_cap = 0;
            SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_scratch), need * sizeof(uint16_t)));
            sc->scratch_cap = need;
        }
    }
    return 0;
hip_failed:
    return -1;
}

/* Pike: the exact VM over the window of every stream that is verified and holds an event (d_lo: only
 * the streams it lists; d_creq: the count requests of a find-all round, else NULL) */
static int
nfa_windows(sre_hip_scanner_t *sc, const int64_t *d_lo, const sre_nfa_count_req_t *d_creq, hipStream_t stream)
{
    const uint32_t n = sc->geom.nstreams;
    if (sc->d_pwave) {
        SRE_HIP_TRY(sre_launch_pike_window_wave(sc->d_pwave, sc->h_pwave, sc->d_ptrs, sc->d_lens, n, sc->d_records,
                                                sc->ovec_slots, reinterpret_cast<sre_nfa_window_t *>(sc->d_nstatus), d_lo,
                                                d_creq, stream));
    } else {
        /* (the window kernel zero-fills the context it uses) */
        SRE_HIP_TRY(sre_launch_pike_window(sc->dp->d_blob, sc->dp->blob_bytes, sc->d_ptrs, sc->d_lens, n, sc->d_ctx, sc->ctx_stride,
                                           sc->d_records, sc->ovec_slots,
                                           reinterpret_cast<sre_nfa_window_t *>(sc->d_nstatus), d_lo,
                                           d_creq, stream));
    }
    return 0;
hip_failed:
    return -1;
}

/* chain check of the set pass and, for Pike, the exact VM over the window of every
 * stream that is verified and holds an event (d_lo: the streams of this fix-up round) */
static int
nfa_finish(sre_hip_scanner_t *sc, const int64_t *d_lo, const sre_nfa_count_req_t *d_creq, hipStream_t stream)
{
    /* (the kernels know two modes: find-all counting is a loop of first-match searches) */
    const int kmode = sc->mode == SRE_HIP_THOMPSON ? SRE_HIP_THOMPSON : SRE_HIP_PIKE_FIRST;
    if (sc->wide_kernel) {
        SRE_HIP_TRY(sre_launch_nfa_wide_verify(kmode, sc->wtab.W, sc->geom, sc->d_nsum, sc->d_wsets, sc->d_nacc, sc->d_nstatus,
                                               sc->d_belief, sc->d_bvalid, sc->d_records, sc->ovec_slots, d_lo, stream));
    } else {
        SRE_HIP_TRY(sre_launch_nfa_verify(kmode, sc->geom, sc->d_nsum, sc->d_nacc, sc->d_nstatus,
                                          sc->d_belief, sc->d_bvalid, sc->d_records, sc->ovec_slots, d_lo, stream));
    }
    if (sc->mode != SRE_HIP_THOMPSON) return nfa_windows(sc, d_lo, d_creq, stream);
    return 0;
hip_failed:
    return -1;
}

/* find-all rounds: the first horizon and the smallest one (SRE_HIP_COUNT_HORIZON: tests force tiny ones) */
static uint64_t
count_horizon(uint64_t dflt)
{
    const char *e = getenv("SRE_HIP_COUNT_HORIZON");
    return e && atoll(e) > 0 ? (uint64_t) atoll(e) : dflt;
}

/* NFA tier: one pass over the batch in h_ptrs / h_lens (geometry, set kernel, chain check, exact
 * windows), queued; the caller queues the copy of the records and status words behind it.  A find-all
 * round hands in its per-stream flags and count requests (d_sflags / d_creq, else NULL) */
static int
nfa_enqueue_pass(sre_hip_scanner_t *sc, size_t nstreams, uint32_t init_variant, const uint8_t *d_sflags,
                 const sre_nfa_count_req_t *d_creq, hipStream_t stream)
{
    if (scan_geometry(sc, nstreams, init_variant, 0, 0) != 0) return -1;
    sc->geom.sflags = d_sflags;
    /* (a round of a find-all count is a sub-batch: the blocks keep the call's layout) */
    SRE_HIP_TRY(hipMemcpyAsync(sc->d_in, sc->h_in, (3 * sc->layout_n + 1) * sizeof(uint64_t),
                               hipMemcpyHostToDevice, stream));
    if (scan_events(sc) != 0) return -1;
    {
        /* set pass, chain check, and (Pike) the exact VM over each stream's window */
        const bool timed = !sc->ev_valid;       /* find-all: the first round's scan is the one reported */
        if (timed) SRE_HIP_TRY(hipEventRecord(sc->ev0, stream));
        SRE_HIP_TRY(nfa_launch_scan(sc, NULL, NULL, NULL, stream));
        if (timed) SRE_HIP_TRY(hipEventRecord(sc->ev1, stream));
        sc->ev_valid = 1;
    }
    if (sc->tail_stream_set && sc->tail_stream != stream) {
        SRE_HIP_TRY(hipStreamWaitEvent(sc->tail_stream, sc->ev1, 0));
        stream = sc->tail_stream;
    }
    return nfa_finish(sc, NULL, d_creq, stream);
hip_failed:
    return -1;
}

/* NFA tier: one fix-up round over the streams listed in d_lo (already on the device): past the
 * speculative rounds every remaining lane's exact entry set first, then the set pass and the chain check */
static int
nfa_fixup_round(sre_hip_scanner_t *sc, const sre_nfa_count_req_t *d_creq, hipStream_t stream)
{
    if (++sc->fixup_rounds > 1000000) {
        fprintf(stderr, "[sregex-hip] NFA scanner fix-up did not converge\n");
        return -1;
    }
    if (sc->fixup_rounds > SRE_SPECULATIVE_FIXUPS && sc->geom.nsegs <= ((size_t) 1 << 23)       /* (512 bytes a segment) */
        && getenv("SRE_HIP_NO_NFA_EXACT") == NULL) {
        /* speculation does not settle this batch (a program that never forgets): every remaining lane's
         * exact entry set from the segments' singleton exit sets — the pass below is then exact */
        if (sc->wide_kernel) {
            /* the wide matrix: 64W x W words a segment (8 KiB at 256 bits).  It takes at most half of the
             * device memory that is free; when it cannot be had, speculation goes on (slower, never wrong) */
            const size_t need = sre_nfa_wide_matrix_bytes(sc->wtab.W, sc->geom.nsegs);
            if (need > sc->nmat_cap * 64 * sizeof(uint64_t)) {
                if (sc->d_nmat) (void) hipFree(sc->d_nmat);
                sc->d_nmat = NULL;
                sc->nmat_cap = 0;
                size_t free_b = 0, total_b = 0;
                if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need <= free_b / 2
                    && hipMalloc(reinterpret_cast<void **>(&sc->d_nmat), need) == hipSuccess) {
                    sc->nmat_cap = need / (64 * sizeof(uint64_t));
                } else {
                    (void) hipGetLastError();
                    sc->d_nmat = NULL;
                }
            }
            if (sc->d_nmat) {
                SRE_HIP_TRY(sre_launch_nfa_wide_exact_entries(sc->wtab, sc->geom, sc->d_nsum, sc->d_wsets, sc->d_lo, sc->d_nmat,
                                                              sc->d_belief, sc->d_bvalid, stream));
                sc->exact_passes++;
            }
        } else {
            if (sc->geom.nsegs > sc->nmat_cap) {
                if (sc->d_nmat) (void) hipFree(sc->d_nmat);
                sc->d_nmat = NULL;
                sc->nmat_cap = 0;
                SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_nmat), sc->geom.nsegs * 64 * sizeof(uint64_t)));
                sc->nmat_cap = sc->geom.nsegs;
            }
            SRE_HIP_TRY(sre_launch_nfa_exact_entries(sc->use_sa ? 1 : 0, sc->ntab, sc->satab, sc->geom, sc->d_nsum, sc->d_lo,
                                                     sc->d_nmat, sc->d_belief, sc->d_bvalid, stream));
            sc->exact_passes++;
        }
    }
    SRE_HIP_TRY(nfa_launch_scan(sc, sc->d_lo, sc->d_belief, sc->d_bvalid, stream));
    return nfa_finish(sc, sc->d_lo, d_creq, stream);
hip_failed:
    return -1;
}

/* NFA tier: segments behind a wrong entry set are re-run — the first one from the exact carried
 * set, the ones behind it from what their predecessor's lane ended in last round (sets only grow
 * towards the truth, so corrections travel many segments per round) — until every stream's
 * verified prefix reaches its event or its end.  h_nstatus holds the status of the pass before. */
static int
nfa_settle(sre_hip_scanner_t *sc, size_t n, const sre_nfa_count_req_t *d_creq, hipStream_t stream, bool *psettled)
{
    for (bool first = true;; first = false) {
        if (!first) {
            SRE_HIP_TRY(hipMemcpyAsync(sc->h_nstatus, sc->d_nstatus, n * sizeof(sre_nfa_status_t),
                                       hipMemcpyDeviceToHost, stream));
            SRE_HIP_TRY(hipStreamSynchronize(stream));
        }
        size_t pending = 0;
        for (size_t i = 0; i < n; i++) {
            if (sc->h_nstatus[i].done) {
                sc->h_lo[i] = -1;
            } else {
                sc->h_lo[i] = sc->h_nstatus[i].first_bad;
                pending++;
            }
        }
        if (pending == 0) break;
        *psettled = false;
        SRE_HIP_TRY(hipMemcpyAsync(sc->d_lo, sc->h_lo, n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        if (nfa_fixup_round(sc, d_creq, stream) != 0) return -1;
    }
    return 0;
hip_failed:
    return -1;
}

/* NFA tier, batches that settle on the device (line mode, stream sets): fix-up rounds over the n streams
 * until every one is verified; the work list d_lo and its length are made on the device, the host reads
 * one word per round */
static int
nfa_settle_device(sre_hip_scanner_t *sc, size_t n, hipStream_t stream)
{
    for (;;) {
        SRE_HIP_TRY(sre_launch_streams_nfa_lo(sc->d_nstatus, (uint32_t) n, sc->d_lo, &sc->d_linfo->pending, stream));
        SRE_HIP_TRY(hipMemcpyAsync(&sc->h_linfo->pending, &sc->d_linfo->pending, sizeof(uint64_t), hipMemcpyDeviceToHost,
                                   stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        if (sc->h_linfo->pending == 0) break;
        if (nfa_fixup_round(sc, NULL, stream) != 0) return -1;
    }
    return 0;
hip_failed:
    return -1;
}

/*
 * Find-all counting on the NFA tier: the reference's caller iterates
 * exec(input + ovector[1], ...) on one re-armed context (sre_vm_pike.c:179-196, :586-636), every
 * search a first-match search that starts at the previous match's end.  Each ROUND here runs the
 * next piece of every unfinished stream's current search as one batch: the set kernel scans a
 * buffer that starts at a CLEAN position of the search (its start, or the last clean position the
 * previous round found: the list there is the fresh initial closure, so nothing of the stream in
 * front of it matters) and is at most `horizon` bytes long; a MATCH event in it sends the exact VM
 * over the stream from the search's start (it picks the search up at the clean position in front of
 * the event, as for a first match) and the next search starts at the match's end; no event moves
 * the buffer to its last clean position, or lets the horizon grow when it has none.  The horizon
 * follows the distance between matches, so sparse matches cost about one pass over the stream and
 * a round trip per match; dense matches run at the round-trip rate.
 */
static int
nfa_count_rounds(sre_hip_scanner_t *sc, sre_int_t *results)
{
    NfaCount    &c = *sc->cnt;
    const size_t n = c.st.size(), slots = 2 + (size_t) sc->ovec_slots;
    hipStream_t  stream = sc->last_stream;
    const bool   tail_set = sc->tail_stream_set;
    if (n > sc->cnt_cap) {
        if (sc->d_sflags) (void) hipFree(sc->d_sflags);
        if (sc->h_sflags) (void) hipHostFree(sc->h_sflags);
        if (sc->d_creq) (void) hipFree(sc->d_creq);
        if (sc->h_creq) (void) hipHostFree(sc->h_creq);
        sc->d_sflags = sc->h_sflags = NULL;
        sc->d_creq = sc->h_creq = NULL;
        sc->cnt_cap = 0;
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_sflags), n));
        SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sc->h_sflags), n, 0));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_creq), n * sizeof(sre_nfa_count_req_t)));
        SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sc->h_creq), n * sizeof(sre_nfa_count_req_t), 0));
        sc->cnt_cap = n;
    }
    sc->tail_stream_set = false;            /* every round is read back: one stream; restored on every way out */
    for (;;) {
        c.active.clear();
        for (size_t i = 0; i < n; i++) {
            NfaCountStream &t = c.st[i];
            /* a search on an empty remainder: size 0 with eof answers SRE_DECLINED (:179-196) */
            if (!t.done && t.cur >= t.n && t.count > 0) t.done = true;
            if (!t.done) c.active.push_back(i);
        }
        if (c.active.empty()) break;
        const size_t na = c.active.size();
        if (++sc->count_rounds > 100000000) goto hip_failed;
        for (size_t j = 0; j < na; j++) {
            NfaCountStream &t = c.st[c.active[j]];
            const uint64_t  left = t.n - t.q, len = left < t.horizon ? left : t.horizon;
            sc->h_ptrs[j] = t.base + t.q;
            sc->h_lens[j] = len;
            sc->h_sflags[j] = (uint8_t) (t.var_q | (t.var_cur << 2) | (t.mode_q << 4) | (len < left ? SRE_SFLAG_NO_EOF : 0u));
            sre_nfa_count_req_t &r = sc->h_creq[j];
            r.vptr = t.base + t.cur;
            r.vlen = t.n - t.cur;
            r.processed = (int64_t) t.cur;
            r.start_add = (int64_t) (t.q - t.cur);
            r.preset_flags = t.var_cur == 1 ? SRE_PRESET_SEEN_NEWLINE : 0u;
            r.pad = 0;
        }
        SRE_HIP_TRY(hipMemcpyAsync(sc->d_sflags, sc->h_sflags, na, hipMemcpyHostToDevice, stream));
        SRE_HIP_TRY(hipMemcpyAsync(sc->d_creq, sc->h_creq, na * sizeof(sre_nfa_count_req_t), hipMemcpyHostToDevice, stream));
        if (nfa_enqueue_pass(sc, na, 0, sc->d_sflags, sc->d_creq, stream) != 0) goto hip_failed;
        SRE_HIP_TRY(hipMemcpyAsync(sc->h_out, sc->d_out, record_bytes(sc, sc->layout_n) + sc->layout_n * sizeof(sre_stream_status_t),
                                   hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        {
            bool settled = true;
            if (nfa_settle(sc, na, sc->d_creq, stream, &settled) != 0) goto hip_failed;
            if (!settled) {
                SRE_HIP_TRY(hipMemcpyAsync(sc->h_out, sc->d_out, record_bytes(sc, sc->layout_n) + sc->layout_n * sizeof(sre_stream_status_t),
                                           hipMemcpyDeviceToHost, stream));
                SRE_HIP_TRY(hipStreamSynchronize(stream));
            }
        }
        for (size_t j = 0; j < na; j++) {
            NfaCountStream         &t = c.st[c.active[j]];
            const sre_nfa_status_t &w = sc->h_nstatus[j];
            const sre_int_t        *rec = sc->h_records + j * slots;
            const bool              truncated = (sc->h_sflags[j] & SRE_SFLAG_NO_EOF) != 0;
            if (getenv("SRE_HIP_DEBUG_COUNT")) {
                fprintf(stderr, "[sregex-hip] count round %d stream %zu: cur %llu q %llu var %u/%u mode %u len %llu%s -> ev %lld clean %lld "
                                "cmode %x rec %lld (%lld, %lld)\n", sc->count_rounds, c.active[j], (unsigned long long) t.cur,
                        (unsigned long long) t.q, t.var_cur, t.var_q, t.mode_q, (unsigned long long) sc->h_lens[j],
                        truncated ? " (truncated)" : "", (long long) w.ev_pos, (long long) w.clean_pos, w.clean_mode,
                        (long long) rec[0], (long long) rec[2], (long long) rec[3]);
            }
            if (w.ev_pos >= 0) {
                if (rec[0] < 0) {
                    /* (an event is a thread reaching MATCH: the exact VM finds that match or an earlier one) */
                    fprintf(stderr, "[sregex-hip] find-all on the NFA tier: the exact window found no match behind an event\n");
                    t.error = t.done = true;
                    continue;
                }
                t.count++;
                t.last.assign(rec, rec + slots);
                const uint64_t end = (uint64_t) rec[3];
                /* the next horizon: a little more than the distance from the previous match to this one */
                const uint64_t gap = end > t.cur ? end - t.cur : 1;
                t.horizon = gap + gap / 4 < count_horizon(1u << 20) ? count_horizon(1u << 20) : gap + gap / 4;
                t.cur = t.q = end;
                t.var_cur = t.var_q = (w.clean_mode & SRE_NFA_MATCH_AFTER_NL) ? 1u : 2u;
                t.mode_q = 0;
                if (w.clean_mode & SRE_NFA_WINDOW_POISONED) t.error = t.done = true;     /* :616-622: the next exec fails */
            } else if (!truncated) {
                t.done = true;                  /* SRE_DECLINED ends the iteration */
            } else if (w.clean_pos > 0) {
                t.q += (uint64_t) w.clean_pos;
                t.var_q = (w.clean_mode & SRE_NFA_CLEAN_AFTER_NL) ? 1u : 2u;
                t.mode_q = (uint32_t) (w.clean_mode & 1);
                t.horizon *= 2;
            } else {
                t.horizon *= 4;                 /* threads alive all along: the same buffer, longer */
            }
        }
    }
    sc->tail_stream_set = tail_set;
    for (size_t i = 0; i < n; i++) {
        const NfaCountStream &t = c.st[i];
        sre_int_t            *out = results + i * slots;
        if (t.count == 0) {
            out[0] = t.error ? SRE_ERROR : SRE_DECLINED;
            out[1] = 0;
            for (size_t k = 2; k < slots; k++) out[k] = -1;
        } else {
            for (size_t k = 0; k < slots; k++) out[k] = t.last[k];
            if (t.error) out[0] = SRE_ERROR;
            out[1] = (sre_int_t) t.count;
        }
    }
    return 0;
hip_failed:
    sc->tail_stream_set = tail_set;
    return -1;
}

extern "C" SRE_API int
sre_hip_scanner_last_count_rounds(sre_hip_scanner_t *sc)
{
    return sc->count_rounds;
}

extern "C" SRE_API int
sre_hip_scan_enqueue(sre_hip_scanner_t *sc, const void *const *d_streams, const size_t *lens,
    size_t nstreams, void *hip_stream)
{
    hipStream_t    stream = static_cast<hipStream_t>(hip_stream);
    const uint32_t init_variant = sc->next_init_variant;
    call_begin(sc);
    sc->next_init_variant = 0;
    if (nstreams == 0) {
        sc->last_n = 0;
        return 0;
    }
    if (scanner_reserve(sc, nstreams) != 0) return -1;
    for (size_t i = 0; i < nstreams; i++) {
        sc->h_ptrs[i] = d_streams[i];
        sc->h_lens[i] = lens[i];
    }
    if (sc->engine == SRE_HIP_ENGINE_VM) {
        SRE_HIP_TRY(hipMemcpyAsync(sc->d_in, sc->h_in, 2 * nstreams * sizeof(uint64_t),
                                   hipMemcpyHostToDevice, stream));
        if (sc->d_pwave && nstreams <= 16384) {
            /* one wavefront per stream: up to ~8000 of them run at once, and a stream's step does not
             * get slower with the length of its thread list (beyond that many streams one LANE per
             * stream keeps more of them in flight) */
            SRE_HIP_TRY(sre_launch_pike_scan_wave(sc->d_pwave, sc->h_pwave, sc->mode, sc->d_ptrs, sc->d_lens,
                                                  (uint32_t) nstreams, sc->d_records, sc->ovec_slots, stream));
        } else {
            /* zero-filled state == fresh context */
            SRE_HIP_TRY(hipMemsetAsync(sc->d_ctx, 0, nstreams * sc->ctx_stride, stream));
            SRE_HIP_TRY(sre_launch_vm_scan(sc->dp->d_blob, sc->mode, sc->d_ptrs, sc->d_lens,
                                           (uint32_t) nstreams, sc->d_ctx, sc->ctx_stride,
                                           sc->d_records, sc->ovec_slots, sc->dp->has_wave, stream));
        }
    } else if (sc->engine == SRE_HIP_ENGINE_NFA && sc->cnt != NULL) {
        /* find-all counting: a loop of first-match searches, run by results() (nfa_count_rounds) */
        NfaCount &c = *sc->cnt;
        c.st.assign(nstreams, NfaCountStream());
        for (size_t i = 0; i < nstreams; i++) {
            NfaCountStream &t = c.st[i];
            t.base = static_cast<const uint8_t *>(d_streams[i]);
            t.n = lens[i];
            t.cur = t.q = 0;
            t.horizon = count_horizon(8u << 20);
            t.var_cur = t.var_q = init_variant;
            t.mode_q = 0;
            t.count = 0;
            t.done = t.error = false;
        }
        sc->count_rounds = 0;
        sc->last_n = nstreams;
        sc->last_stream = stream;
        return 0;
    } else if (sc->engine == SRE_HIP_ENGINE_NFA) {
        if (nfa_enqueue_pass(sc, nstreams, init_variant, NULL, NULL, stream) != 0) return -1;
        if (sc->tail_stream_set && sc->tail_stream != stream) stream = sc->tail_stream;
    } else {
        if (scan_geometry(sc, nstreams, init_variant, 0, 0) != 0) return -1;
        const bool one = (sc->geom.flags & SRE_GEOM_ONE) != 0;
        if (!one) {
            static const bool dma = getenv("SRE_HIP_DMA_UPLOAD") != NULL;      /* experiment knob: the old way */
            if (dma) {
                SRE_HIP_TRY(hipMemcpyAsync(sc->d_in, sc->h_in, (3 * nstreams + 1) * sizeof(uint64_t),
                                           hipMemcpyHostToDevice, stream));
            } else {
                SRE_HIP_TRY(sre_launch_upload_words(sc->h_in, sc->d_in, (uint32_t) (3 * nstreams + 1), stream));
            }
        }
        /* speculative pass, chain check, captures — all queued; results() only
         * has to look at the status words */
        if (scan_events(sc) != 0) return -1;
        SRE_HIP_TRY(hipEventRecord(sc->ev0, stream));
        SRE_HIP_TRY(sre_launch_scan(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, NULL, NULL, stream));
        SRE_HIP_TRY(hipEventRecord(sc->ev1, stream));
        sc->ev_valid = 1;
        /* everything behind the scan kernel on the tail stream, if one is set: the caller's
         * next scan follows this one on `stream` with no gap while these small kernels run */
        if (sc->tail_stream_set && sc->tail_stream != stream) {
            SRE_HIP_TRY(hipStreamWaitEvent(sc->tail_stream, sc->ev1, 0));
            stream = sc->tail_stream;
        }
        {
            /* one small buffer: chain check and captures in one workgroup */
            const int fused = one && sc->geom.nsegs <= SRE_VERIFY_ONE_SEGS && sc->mode != SRE_HIP_PIKE_COUNT;
            if (!fused) SRE_HIP_TRY(sre_launch_verify(sc->tab->h, sc->geom, sc->d_sum, sc->d_acc, sc->d_status, stream));
            SRE_HIP_TRY(sre_launch_captures(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, sc->d_status,
                                            sc->d_scratch, sc->d_records, sc->ovec_slots,
                                            NULL, NULL, 0, fused, stream));
        }
    }
    /* records (and the scanner's status words behind them) in one copy */
    SRE_HIP_TRY(hipMemcpyAsync(sc->h_out, sc->d_out,
                               record_bytes(sc, nstreams)
                                   + (sc->engine != SRE_HIP_ENGINE_VM ? nstreams * sizeof(sre_stream_status_t) : 0),
                               hipMemcpyDeviceToHost, stream));
    if (sc->ev_done == NULL) SRE_HIP_TRY(hipEventCreateWithFlags(&sc->ev_done, hipEventDisableTiming));
    SRE_HIP_TRY(hipEventRecord(sc->ev_done, stream));
    sc->last_n = nstreams;
    sc->last_stream = stream;
    return 0;
hip_failed:
    return -1;
}

/* a host read of the device words of a line-mode call, queued: the run of sre_lines_info_t that holds every word named,
 * whatever the order of the struct, so a word added or moved changes how much is copied and never which words arrive */
typedef uint64_t sre_lines_info_t::*LinfoWord;
#define LINFO(word) (&sre_lines_info_t::word)

static hipError_t
linfo_read(sre_hip_scanner_t *sc, hipStream_t stream, std::initializer_list<LinfoWord> words)
{
    const char *base = reinterpret_cast<const char *>(sc->h_linfo);
    size_t      lo = sizeof(sre_lines_info_t), hi = 0;
    for (LinfoWord w : words) {
        const size_t at = (size_t) (reinterpret_cast<const char *>(&(sc->h_linfo->*w)) - base);
        lo = at < lo ? at : lo;
        hi = at + sizeof(uint64_t) > hi ? at + sizeof(uint64_t) : hi;
    }
    return hipMemcpyAsync(reinterpret_cast<char *>(sc->h_linfo) + lo, reinterpret_cast<const char *>(sc->d_linfo) + lo, hi - lo,
                          hipMemcpyDeviceToHost, stream);
}

/* line mode: the batch's status words reduced on the device to h_linfo->pending (streams not
 * done) and h_linfo->maps (streams with need_maps); the host reads 16 bytes */
static int
lines_status_counters(sre_hip_scanner_t *sc, size_t n, hipStream_t stream)
{
    SRE_HIP_TRY(sre_launch_lines_settle(sc->d_status, (uint32_t) n, sc->d_linfo, stream));
    SRE_HIP_TRY(linfo_read(sc, stream, {LINFO(pending), LINFO(maps)}));
    SRE_HIP_TRY(hipStreamSynchronize(stream));
    return 0;
hip_failed:
    return -1;
}

/* Segments behind a broken state chain are re-run from the exact carried state until
 * every stream's verified prefix reaches its end (h_status holds the latest status on
 * return).  with_captures: the capture kernel runs behind every round.  counters (line
 * mode): the status stays on the device, h_linfo->pending / maps hold its counts (on entry:
 * of the pass before; on return: of the last round) */
static int
scan_settle(sre_hip_scanner_t *sc, size_t n, hipStream_t stream, bool with_captures, bool *psettled,
            bool counters = false)
{
    bool settled = true;
    int  batch = sc->mode == SRE_HIP_PIKE_COUNT ? 2 : SRE_SPECULATIVE_FIXUPS + 1;
    /* h_status holds the status of the pass before.  Rounds are queued in batches and the
     * status is read once per batch: a round finds its streams and their first wrong segment
     * in the status words on the device, and is a no-op for a stream that has settled.
     * FIRST / Thompson: two speculative rounds, then the exact entry states (all three
     * queued at once); COUNT: 2, 4, 8, ... speculative rounds. */
    for (;;) {
        size_t pending = 0;
        if (counters) pending = (size_t) sc->h_linfo->pending;
        else for (size_t i = 0; i < n; i++) pending += sc->h_status[i].done ? 0 : 1;
        if (pending == 0) break;
        settled = false;
        for (int r = 0; r < batch; r++) {
            if (++sc->fixup_rounds > 1000000) {
                fprintf(stderr, "[sregex-hip] scanner fix-up did not converge\n");
                return -1;
            }
            const uint8_t *d_entry = NULL;
            static const bool count_exact = getenv("SRE_HIP_NO_COUNT_EXACT") == NULL;      /* (experiment knob) */
            if ((sc->mode != SRE_HIP_PIKE_COUNT || count_exact) && sc->fixup_rounds > SRE_SPECULATIVE_FIXUPS) {
                /* speculation does not settle this stream (an automaton that never
                 * forgets): compose the segments' transition functions instead — after
                 * this pass every lane enters with the exact state */
                if (sc->geom.nsegs > sc->fn_cap) {
                    if (sc->d_fn) (void) hipFree(sc->d_fn);
                    sc->d_fn = NULL;
                    sc->fn_cap = 0;
                    const size_t nchunks = sc->geom.nsegs / 256 + 1;
                    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_fn),
                                          sc->geom.nsegs * 64 + nchunks * 64 + nchunks + sc->geom.nsegs + 64));
                    sc->fn_cap = sc->geom.nsegs;
                }
                const size_t nchunks = sc->geom.nsegs / 256 + 1;
                uint8_t *d_comp = sc->d_fn + sc->geom.nsegs * 64, *d_chunk = d_comp + nchunks * 64;
                uint8_t *d_ent = d_chunk + nchunks;
                SRE_HIP_TRY(sre_launch_exact_entries(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, sc->d_status,
                                                     sc->d_fn, d_comp, d_chunk, d_ent, stream));
                d_entry = d_ent;
                sc->exact_passes++;
            }
            SRE_HIP_TRY(sre_launch_scan(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, sc->d_status, d_entry, stream));
            SRE_HIP_TRY(sre_launch_verify(sc->tab->h, sc->geom, sc->d_sum, sc->d_acc, sc->d_status, stream));
            if (with_captures) {
                SRE_HIP_TRY(sre_launch_captures(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum,
                                                sc->d_status, sc->d_scratch, sc->d_records,
                                                sc->ovec_slots, NULL, NULL, 0, 0, stream));
            }
        }
        if (counters) {
            if (lines_status_counters(sc, n, stream) != 0) return -1;
        } else {
            SRE_HIP_TRY(hipMemcpyAsync(sc->h_status, sc->d_status, n * sizeof(sre_stream_status_t),
                                       hipMemcpyDeviceToHost, stream));
            SRE_HIP_TRY(hipStreamSynchronize(stream));
        }
        batch = sc->mode == SRE_HIP_PIKE_COUNT ? (batch < 16 ? 2 * batch : 16) : 1;
    }
    if (psettled) *psettled = settled;
    return 0;
hip_failed:
    return -1;
}

/* a match whose lineage outran the plain backward walk: build the per-segment ancestor maps
 * of the flagged streams in parallel and walk again, jumping */
static int
scan_lineage_pass(sre_hip_scanner_t *sc, hipStream_t stream)
{
    if (sc->geom.nsegs > sc->maps_cap) {
        if (sc->d_maps) (void) hipFree(sc->d_maps);
        if (sc->d_blocks) (void) hipFree(sc->d_blocks);
        sc->d_maps = sc->d_blocks = NULL;
        sc->maps_cap = 0;
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_maps),
                              sc->geom.nsegs * sizeof(sre_seg_lineage_t)));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_blocks),
                              (sc->geom.nsegs / SRE_LINEAGE_BLOCK + 1) * sizeof(sre_seg_lineage_t)));
        sc->maps_cap = sc->geom.nsegs;
    }
    sc->lineage_passes++;
    SRE_HIP_TRY(sre_launch_lineage(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum,
                                   sc->d_status, sc->d_maps, sc->d_blocks, stream));
    SRE_HIP_TRY(sre_launch_captures(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum,
                                    sc->d_status, sc->d_scratch, sc->d_records,
                                    sc->ovec_slots, sc->d_maps, sc->d_blocks,
                                    1, 0, stream));
    return 0;
hip_failed:
    return -1;
}

extern "C" SRE_API int
sre_hip_scan_results(sre_hip_scanner_t *sc, sre_int_t *results)
{
    if (sc->last_lines) return -1;      /* the last call was a line-mode call: nothing to collect */
    if (sc->last_n == 0) return 0;
    const size_t n = sc->last_n;
    hipStream_t  stream = sc->last_stream;

    const size_t bytes = n * (2 + (size_t) sc->ovec_slots) * sizeof(int64_t);
    bool         settled = true;        /* the copies queued by enqueue() are the answer */

    if (sc->engine == SRE_HIP_ENGINE_NFA && sc->cnt != NULL) return nfa_count_rounds(sc, results);
    /* everything enqueue() queued for this call, result copies included */
    SRE_HIP_TRY(hipEventSynchronize(sc->ev_done));
    if (sc->engine == SRE_HIP_ENGINE_NFA && nfa_settle(sc, n, NULL, stream, &settled) != 0) return -1;
    if (sc->engine == SRE_HIP_ENGINE_SCAN) {
        if (scan_settle(sc, n, stream, true, &settled) != 0) return -1;
        /* a match whose lineage outran the plain backward walk: build the
         * per-segment ancestor maps in parallel and walk again, jumping */
        if (sc->mode != SRE_HIP_THOMPSON) {
            size_t want = 0;
            for (size_t i = 0; i < n; i++) want += sc->h_status[i].need_maps != 0;
            if (want) {
                settled = false;
                if (scan_lineage_pass(sc, stream) != 0) return -1;
            }
        }
    }
    if (sc->engine == SRE_HIP_ENGINE_SCAN && getenv("SRE_HIP_DEBUG_STATUS")) {
        /* diagnostics: what the chain check decided per stream */
        for (size_t i = 0; i < n && i < 8; i++) {
            const sre_stream_status_t &t = sc->h_status[i];
            fprintf(stderr, "[sregex-hip] stream %zu: rc %lld count %lld ev_pos %lld ev_sp %lld ev_state %u ev_sym %u "
                            "ev_apos %lld ev_astate %u ev_seg %lld limit %lld need_maps %d seg %u\n",
                    i, (long long) t.rc, (long long) t.count, (long long) t.ev_pos, (long long) t.ev_sp,
                    t.ev_state, t.ev_sym, (long long) t.ev_apos, t.ev_astate, (long long) t.ev_seg,
                    (long long) t.limit, t.need_maps, sc->geom.seg_bytes);
        }
        /* ... and what the lanes of the first segments recorded */
        const size_t ns = sc->geom.nsegs < 16 ? (size_t) sc->geom.nsegs : 16;
        std::vector<sre_seg_summary_t> hs(ns);
        std::vector<sre_seg_digest_t>  hd(ns);
        const bool                     dig = sc->geom.digest != NULL;
        if (hipMemcpy(hs.data(), sc->d_sum, ns * sizeof(sre_seg_summary_t), hipMemcpyDeviceToHost) == hipSuccess
            && (!dig || hipMemcpy(hd.data(), sc->geom.digest, ns * sizeof(sre_seg_digest_t), hipMemcpyDeviceToHost) == hipSuccess))
        {
            /* (a plain segment's record is its digest: sre_scan_record.h) */
            for (size_t k = 0; k < ns; k++) hs[k] = sre_scan_record_load(dig ? hd.data() : NULL, hs.data(), k, sc->geom.seg_bytes);
            for (size_t k = 0; k < ns; k++) {
                fprintf(stderr, "[sregex-hip]   seg %zu: s_in %x s_out %x flags %x count %lld cur_sp %lld term %lld "
                                "pe_pos %lld lm_pos %lld lm_sp %lld\n",
                        k, hs[k].s_in, hs[k].s_out, hs[k].flags, (long long) hs[k].count,
                        (long long) hs[k].cur_sp, (long long) hs[k].term_pos, (long long) hs[k].pe_pos,
                        (long long) hs[k].lm_pos, (long long) hs[k].lm_sp);
            }
        }
    }
    if (!settled) {
        SRE_HIP_TRY(hipMemcpyAsync(sc->h_records, sc->d_records, bytes, hipMemcpyDeviceToHost, stream));
        if (sc->engine == SRE_HIP_ENGINE_NFA) {
            SRE_HIP_TRY(hipMemcpyAsync(sc->h_nstatus, sc->d_nstatus, n * sizeof(sre_nfa_status_t),
                                       hipMemcpyDeviceToHost, stream));
        }
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    memcpy(results, sc->h_records, bytes);
    return 0;
hip_failed:
    return -1;
}

extern "C" SRE_API int
sre_hip_scan_batch(sre_hip_scanner_t *sc, const void *const *d_streams, const size_t *lens,
    size_t nstreams, sre_int_t *results, void *hip_stream)
{
    if (sre_hip_scan_enqueue(sc, d_streams, lens, nstreams, hip_stream) != 0) return -1;
    return sre_hip_scan_results(sc, results);
}

/* ---- line mode (sre_hip_scan_lines) ---- */

/* grow-only device buffer */
template <typename T>
static int
lines_grow(T **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return 0;
    if (*p) (void) hipFree(*p);
    *p = NULL;
    *cap = 0;
    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), bytes));
    *cap = bytes;
    return 0;
hip_failed:
    return -1;
}

/* lines per batch: SRE_HIP_LINES_BATCH (experiment knob, read on every call; at most 2^24) or SRE_LINES_BATCH */
static uint64_t
lines_batch_limit(void)
{
    const char     *e = getenv("SRE_HIP_LINES_BATCH");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (v < (1ll << 24) ? (uint64_t) v : (uint64_t) 1 << 24) : SRE_LINES_BATCH;
}

/* the split: the line table of the buffer in sc->d_ends, *pn lines.  The host reads one word. */
static int
lines_split(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, hipStream_t stream, uint64_t *pn)
{
    *pn = 0;
    if (len == 0) return 0;
    const uint64_t head = reinterpret_cast<uintptr_t>(d_buf) & 15u;
    const uint64_t ntiles = (head + len + SRE_LINES_TILE_BYTES - 1) / SRE_LINES_TILE_BYTES;
    /* (the same words later hold the geometry's and the compaction's per-workgroup sums) */
    const uint64_t nblk = (lines_batch_limit() + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS + 1;
    if (lines_grow(&sc->d_lblk, &sc->lblk_cap, (ntiles > nblk ? ntiles : nblk) * sizeof(uint64_t)) != 0) return -1;
    SRE_HIP_TRY(sre_launch_lines_count(d_buf, len, (uint32_t) delim, sc->d_lblk, sc->d_linfo, stream));
    SRE_HIP_TRY(hipMemcpyAsync(&sc->h_linfo->nlines, &sc->d_linfo->nlines, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    SRE_HIP_TRY(hipStreamSynchronize(stream));
    if (lines_grow(&sc->d_ends, &sc->ends_cap, sc->h_linfo->nlines * sizeof(uint64_t)) != 0) return -1;
    SRE_HIP_TRY(sre_launch_lines_write(d_buf, len, (uint32_t) delim, sc->d_lblk, sc->d_ends, stream));
    *pn = sc->h_linfo->nlines;
    return 0;
hip_failed:
    return -1;
}

/* a sink of a line-mode call: with one, a batch ends with the sink's select pass into the scanner's table (d_fval, one
 * word per entry, and d_fstart) in place of the compaction, and no row goes to the host (out / cap are NULL / 0 then) */
struct LinesSink {
    int        delim;
    void      *d_out;       /* the caller's output: out_cap bytes that do not overlap the buffer */
    size_t     out_cap;
    sre_int_t *d_index;     /* ... and room for index_cap index rows */
    size_t     index_cap;
    int        mode;        /* the row rule (sre_sel_row): 0 the lines with a match, 1 the lines without one, 2 every line */
    /* the extract and the tally: the entries line * k + field, fsep between the fields of a row; mode is 0 or 2 */
    const sre_extract_groups_t *groups;
    int                         fsep;
    /* the substitute: the entries line * (np + 2) + piece; mode is 0 or 2 */
    const sre_subst_pieces_t   *pieces;
    /* the route: a key per line by the scanner's map of nreg + 1 buckets (h_rmap / d_rmap); mode is unused */
    bool                        route;
    uint32_t                    nreg;
    /* the tally's sums: the extract's select pass runs a second time over the entries line * v + column of the value
     * groups into d_vval and d_vstart; the key table is untouched by it */
    const sre_extract_groups_t *vgroups;
    /* the filter with context: index rows of five words; d_cbits marks the context-only lines (NULL: no line is one) */
    bool                        context;
    const uint64_t             *d_cbits;
    /* the join: the batches end with the filter's select pass (mode 0) and the key groups' (vgroups) as the lookup's do; the
     * table has `join` = 1 + columns entries per line, which the join pass behind the call fills, jsep between the fields
     * of a row (fsep); its values come from d_dict, the map's copy of its dictionary */
    uint32_t                    join;
    const void                 *d_dict;
};

/* the arguments every sink call shares: false unless they are in range, the pointers stand for their sizes and the output
 * does not overlap the buffer; else the sink that describes them (of the caller's checked flags, the row rule) */
static bool
sink_open(LinesSink *sink, const sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, int flags, void *d_out,
          size_t out_cap, sre_int_t *d_index, size_t index_cap)
{
    if (sc == NULL || delim < 0 || delim > 255 || (out_cap != 0 && d_out == NULL) || (index_cap != 0 && d_index == NULL)
        || (len != 0 && d_buf == NULL))
    {
        return false;
    }
    if (len != 0 && out_cap != 0) {
        /* the output may not overlap the buffer */
        const uintptr_t b = reinterpret_cast<uintptr_t>(d_buf), o = reinterpret_cast<uintptr_t>(d_out);
        if (o < b + len && b < o + out_cap) return false;
    }
    *sink = LinesSink();
    sink->delim = sink->fsep = delim;
    sink->mode = (flags & SRE_HIP_LINES_ALL) ? 2 : (flags & SRE_HIP_LINES_INVERT) ? 1 : 0;
    sink->d_out = d_out;
    sink->out_cap = out_cap;
    sink->d_index = d_index;
    sink->index_cap = index_cap;
    return true;
}

/* the sinks that read the first match's record refuse every other mode, by name */
static bool
sink_first_match(const sre_hip_scanner_t *sc, const char *call, const char *reads)
{
    if (sc->mode == SRE_HIP_PIKE_FIRST) return true;
    fprintf(stderr, "[sregex-hip] %s: the scanner's mode must be SRE_HIP_PIKE_FIRST (the first match's %s)\n", call, reads);
    return false;
}

/* a list of capture groups packed for the select pass; false: one of them is not a group of the program */
static bool
sink_groups(const sre_hip_scanner_t *sc, const int *groups, size_t ngroups, sre_extract_groups_t *gr)
{
    memset(gr, 0, sizeof(*gr));
    gr->k = (uint32_t) ngroups;
    for (size_t f = 0; f < ngroups; f++) {
        /* ovec_slots = 2 * (max_ncaps + 1) */
        if (groups[f] < 0 || groups[f] > 0xFFFF || 2 * (size_t) groups[f] + 1 >= (size_t) sc->ovec_slots) return false;
        gr->g[f] = (uint16_t) groups[f];
    }
    return true;
}

/* entries per line of the sink's table */
static uint32_t
sink_entries(const LinesSink *sink)
{
    return sink->pieces ? sink->pieces->np + 2 : sink->groups ? sink->groups->k : sink->join ? sink->join : 1;
}

/* the select pass of a device batch (lines i0 .. d_linfo->i1, at most nmax) from its records */
static int
sink_select(sre_hip_scanner_t *sc, const LinesSink *sink, uint32_t slots, uint64_t nmax, uint64_t i0, hipStream_t stream)
{
    const int64_t          *recs = sc->d_records;
    const uint64_t         *ends = sc->d_ends;
    const sre_lines_info_t *li = sc->d_linfo;
    uint64_t               *val = sc->d_fval, *start = sc->d_fstart;
    const int               all = sink->mode == 2;
    if (sink->route) SRE_HIP_TRY(sre_launch_route_select(recs, slots, nmax, i0, sink->nreg, sc->d_rmap, ends, li, val, stream));
    else if (sink->pieces) SRE_HIP_TRY(sre_launch_subst_select(recs, slots, nmax, i0, all, sink->pieces, ends, li, val, start, stream));
    else if (sink->groups) SRE_HIP_TRY(sre_launch_extract_select(recs, slots, nmax, i0, all, sink->groups, ends, li, val, start, stream));
    else SRE_HIP_TRY(sre_launch_filter_select(recs, slots, nmax, i0, sink->mode, ends, li, val, stream));
    if (sink->vgroups) {
        SRE_HIP_TRY(sre_launch_extract_select(recs, slots, nmax, i0, all, sink->vgroups, ends, li, sc->d_vval, sc->d_vstart, stream));
    }
    return 0;
hip_failed:
    return -1;
}

/* what a line-mode call sums over its batches (lines_call publishes it) */
struct LinesTotals {
    int    fixups, exact, lineage;
    double kms;         /* the scan kernels, -1 unknown */
    size_t nshort;      /* lines the short-line kernel took */
};

/* the device routes of a line-mode call begin: room for the rows the call may report, none reported yet,
 * the events around the scan kernel */
static int
lines_device_begin(sre_hip_scanner_t *sc, uint64_t rcap, size_t width, hipStream_t stream)
{
    if (rcap && lines_grow(&sc->d_rows, &sc->rows_cap, rcap * width * sizeof(int64_t)) != 0) return -1;
    SRE_HIP_TRY(hipMemsetAsync(&sc->d_linfo->reported, 0, sizeof(uint64_t), stream));
    return scan_events(sc);
hip_failed:
    return -1;
}

/* ... a batch (lines i0 .. d_linfo->i1, at most nmax) ends: its records go through the sink's select pass, or
 * its reported rows are compacted behind the call's; the batch's diagnostics join the call's */
static int
lines_device_batch_end(sre_hip_scanner_t *sc, LinesTotals *tot, const LinesSink *sink, uint64_t nmax, uint64_t i0, int all,
                       uint64_t rcap, hipStream_t stream)
{
    const uint32_t slots = 2 + sc->ovec_slots;
    if (sink) {
        if (sink_select(sc, sink, slots, nmax, i0, stream) != 0) return -1;
    } else {
        SRE_HIP_TRY(sre_launch_lines_compact(sc->d_records, slots, nmax, i0, all, sc->d_ends, sc->d_lblk, sc->d_linfo, sc->d_rows,
                                             rcap, stream));
    }
    tot->fixups += sc->fixup_rounds;
    tot->exact += sc->exact_passes;
    tot->lineage += sc->lineage_passes;
    sc->line_batches++;
    return 0;
hip_failed:
    return -1;
}

/* ... and the call ends: how many rows it reported, and the first min(cap, reported) of them (a sink takes no row) */
static int
lines_device_end(sre_hip_scanner_t *sc, const LinesSink *sink, uint64_t n, sre_int_t *out, uint64_t rcap, size_t width,
                 uint64_t *pnrep, hipStream_t stream)
{
    if (sink) return 0;
    SRE_HIP_TRY(hipMemcpyAsync(&sc->h_linfo->reported, &sc->d_linfo->reported, sizeof(uint64_t), hipMemcpyDeviceToHost,
                               stream));
    SRE_HIP_TRY(hipStreamSynchronize(stream));
    *pnrep = n ? sc->h_linfo->reported : 0;
    {
        const uint64_t take = *pnrep < rcap ? *pnrep : rcap;
        if (take) {
            SRE_HIP_TRY(hipMemcpyAsync(out, sc->d_rows, take * width * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
            SRE_HIP_TRY(hipStreamSynchronize(stream));
        }
    }
    return 0;
hip_failed:
    return -1;
}

/* table-driven scanner: every batch on the device; the host reads a few words per batch */
static int
lines_scan_device(sre_hip_scanner_t *sc, const void *d_buf, uint64_t n, int all, sre_int_t *out, size_t cap,
                  uint64_t *pnrep, hipStream_t stream, LinesTotals *tot, const LinesSink *sink)
{
    const size_t   width = 3 + 2 + (size_t) sc->ovec_slots;
    const uint64_t bmax = lines_batch_limit();
    const uint64_t rcap = cap < n ? cap : n;
    const uint64_t seg_fixed = scan_seg_knobs(sc);
    const uint64_t resident = scan_resident(sc);
    if (lines_device_begin(sc, rcap, width, stream) != 0) return -1;
    for (uint64_t i0 = 0; i0 < n;) {
        const uint64_t nmax = bmax < n - i0 ? bmax : n - i0;
        if (scanner_reserve(sc, nmax) != 0) return -1;
        /* how many lines the batch takes, its segment size and the stream arrays, on the device */
        SRE_HIP_TRY(sre_launch_lines_geometry(d_buf, sc->d_ends, n, i0, nmax, SRE_LINES_WALK_MAX, seg_fixed, resident,
                                              scan_seg_cap(sc), reinterpret_cast<const uint8_t **>(sc->d_ptrs), sc->d_lens,
                                              sc->d_seg_first, sc->d_lblk, sc->d_linfo, stream));
        SRE_HIP_TRY(linfo_read(sc, stream, {LINFO(i1), LINFO(seg), LINFO(nsegs)}));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        const uint64_t i1 = sc->h_linfo->i1, nb = i1 - i0, seg = sc->h_linfo->seg, nsegs = sc->h_linfo->nsegs;
        call_begin(sc);         /* (to the diagnostics a batch is a call: tot sums them) */
        geom_device(sc, nb, seg, nsegs);
        if (scan_buffers(sc, nb, seg, nsegs) != 0) return -1;       /* (not COUNT: geom.digest) */
        /* scan, chain check and captures queued as for a batch of streams */
        SRE_HIP_TRY(hipEventRecord(sc->ev0, stream));
        SRE_HIP_TRY(sre_launch_scan(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, NULL, NULL, stream));
        SRE_HIP_TRY(hipEventRecord(sc->ev1, stream));
        SRE_HIP_TRY(sre_launch_verify(sc->tab->h, sc->geom, sc->d_sum, sc->d_acc, sc->d_status, stream));
        SRE_HIP_TRY(sre_launch_captures(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, sc->d_status,
                                        sc->d_scratch, sc->d_records, sc->ovec_slots, NULL, NULL, 0, 0, stream));
        /* ... and settled from two device counters */
        if (lines_status_counters(sc, nb, stream) != 0) return -1;
        if (scan_settle(sc, nb, stream, true, NULL, true) != 0) return -1;
        if (sc->mode != SRE_HIP_THOMPSON && sc->h_linfo->maps != 0 && scan_lineage_pass(sc, stream) != 0) return -1;
        if (lines_device_batch_end(sc, tot, sink, nmax, i0, all, rcap, stream) != 0) return -1;
        {
            float ms = 0.0f;
            SRE_HIP_TRY(hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
            tot->kms += ms;
        }
        i0 = i1;
    }
    return lines_device_end(sc, sink, n, out, rcap, width, pnrep, stream);
hip_failed:
    return -1;
}

/* the longest line the short-line kernel takes: SRE_HIP_LINES_SHORT_MAX (read on every call; 0: the kernel is
 * off) or SRE_LINES_SHORT_MAX; the wide forms have no such kernel */
static uint64_t
lines_short_max(const sre_hip_scanner_t *sc)
{
    if (sc->wide_kernel) return 0;
    const char *e = getenv("SRE_HIP_LINES_SHORT_MAX");
    if (e == NULL || *e == 0) return SRE_LINES_SHORT_MAX;
    const long long v = atoll(e);
    return v <= 0 ? 0 : v < (1ll << 20) ? (uint64_t) v : (uint64_t) 1 << 20;
}

/* NFA tier, Thompson and first match: every batch on the device.  Lines of at most lines_short_max() bytes take
 * no segment and go to the short-line kernel (sre_hip_lines_nfa.hip); the others go through the set pass, the
 * chain check and the fix-up rounds as a batch of streams does, settled from one device counter.  Order of a
 * batch: set pass and nfa_finish over every stream (a line without segments comes out verified and DECLINED,
 * and has no window), THEN the short-line kernel writes the short lines' status blocks and records and the work
 * list d_lo of their windows, then the window kernel runs over that list; the fix-up rounds rebuild d_lo from
 * the status blocks, in which every short line is done. */
static int
lines_scan_nfa(sre_hip_scanner_t *sc, const void *d_buf, uint64_t n, int all, sre_int_t *out, size_t cap,
               uint64_t *pnrep, hipStream_t stream, LinesTotals *tot, const LinesSink *sink)
{
    const size_t   width = 3 + 2 + (size_t) sc->ovec_slots;
    const uint64_t rcap = cap < n ? cap : n;
    const uint64_t lmax = lines_short_max(sc), short_lim = lmax ? lmax + 1 : 0;
    const uint32_t W = nfa_words(sc);
    /* what a segment costs: its summary, belief and validity byte, and the wide kernel's entry and exit sets */
    const uint64_t seg_cost = sizeof(sre_nfa_summary_t) + W * sizeof(uint64_t) + 1 + (sc->wide_kernel ? 2 * W * sizeof(uint64_t) : 0);
    uint64_t       bmax = lines_batch_limit();
    const uint64_t seg_fixed = nfa_seg_knobs(sc);
    const uint64_t resident = scan_resident(sc);
    if (sc->mode != SRE_HIP_THOMPSON && sc->d_pwave == NULL && sc->ctx_stride) {
        /* the exact window's contexts, one per line of the batch */
        const uint64_t most = SRE_LINES_NFA_WORK_MAX / sc->ctx_stride;
        if (bmax > most) bmax = most ? most : 1;
    }
    sre_lnfa_t ltab;
    memset(&ltab, 0, sizeof(ltab));
    if (short_lim) ltab = sc->use_sa ? sre_lines_nfa_tables_sa(&sc->satab) : sre_lines_nfa_tables_plain(&sc->ntab);
    if (lines_device_begin(sc, rcap, width, stream) != 0) return -1;
    if (sc->ev_l0 == NULL) {
        SRE_HIP_TRY(hipEventCreate(&sc->ev_l0));
        SRE_HIP_TRY(hipEventCreate(&sc->ev_l1));
    }
    for (uint64_t i0 = 0; i0 < n;) {
        const uint64_t nmax = bmax < n - i0 ? bmax : n - i0;
        if (scanner_reserve(sc, nmax) != 0) return -1;
        SRE_HIP_TRY(sre_launch_lines_geometry_nfa(d_buf, sc->d_ends, n, i0, nmax, short_lim, SRE_LINES_NFA_WORK_MAX, seg_cost,
                                                  seg_fixed, resident, scan_seg_cap(sc), reinterpret_cast<const uint8_t **>(sc->d_ptrs),
                                                  sc->d_lens, sc->d_seg_first, sc->d_lblk, sc->d_linfo, stream));
        SRE_HIP_TRY(linfo_read(sc, stream, {LINFO(i1), LINFO(seg), LINFO(nsegs)}));
        SRE_HIP_TRY(hipMemcpyAsync(&sc->h_linfo->nshort, &sc->d_linfo->nshort, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        const uint64_t i1 = sc->h_linfo->i1, nb = i1 - i0, seg = sc->h_linfo->seg, nsegs = sc->h_linfo->nsegs;
        const uint64_t nshort = sc->h_linfo->nshort;
        call_begin(sc);         /* (to the diagnostics a batch is a call: tot sums them) */
        geom_device(sc, nb, seg, nsegs);
        if (nsegs) {
            if (nfa_buffers(sc, nsegs) != 0) return -1;
            SRE_HIP_TRY(hipEventRecord(sc->ev0, stream));
            SRE_HIP_TRY(nfa_launch_scan(sc, NULL, NULL, NULL, stream));
            SRE_HIP_TRY(hipEventRecord(sc->ev1, stream));
            if (nfa_finish(sc, NULL, NULL, stream) != 0) return -1;
        }
        if (nshort) {
            SRE_HIP_TRY(hipEventRecord(sc->ev_l0, stream));
            SRE_HIP_TRY(sre_launch_lines_nfa(ltab, d_buf, sc->d_ends, i0, (uint32_t) nb, (uint32_t) short_lim,
                                             sc->mode == SRE_HIP_THOMPSON, sc->d_nstatus, sc->d_records, sc->ovec_slots, sc->d_lo,
                                             stream));
            SRE_HIP_TRY(hipEventRecord(sc->ev_l1, stream));
            if (sc->mode != SRE_HIP_THOMPSON && nfa_windows(sc, sc->d_lo, NULL, stream) != 0) return -1;
        }
        /* fix-up rounds over the long lines that are not verified */
        if (nsegs && nfa_settle_device(sc, nb, stream) != 0) return -1;
        if (lines_device_batch_end(sc, tot, sink, nmax, i0, all, rcap, stream) != 0) return -1;
        {
            float ms = 0.0f;
            if (nsegs) {
                SRE_HIP_TRY(hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
                tot->kms += ms;
            }
            if (nshort) {
                SRE_HIP_TRY(hipEventSynchronize(sc->ev_l1));
                SRE_HIP_TRY(hipEventElapsedTime(&ms, sc->ev_l0, sc->ev_l1));
                tot->kms += ms;
            }
        }
        tot->nshort += (size_t) nshort;
        i0 = i1;
    }
    return lines_device_end(sc, sink, n, out, rcap, width, pnrep, stream);
hip_failed:
    return -1;
}

/* find-all counting on the NFA tier and the exact VM (and the NFA tier under SRE_HIP_LINES_NFA_HOST): each
 * batch's slice of the line table comes to the host and goes through sre_hip_scan_enqueue /
 * sre_hip_scan_results; the rows are compacted on the host */
static int
lines_scan_host(sre_hip_scanner_t *sc, const void *d_buf, uint64_t n, int all, sre_int_t *out, size_t cap,
                uint64_t *pnrep, hipStream_t stream, LinesTotals *tot, const LinesSink *sink)
{
    const size_t              slots = 2 + (size_t) sc->ovec_slots, width = 3 + slots;
    const uint64_t            bmax = lines_batch_limit();
    const uint8_t            *buf = static_cast<const uint8_t *>(d_buf);
    std::vector<uint64_t>     ends;
    std::vector<const void *> ptrs;
    std::vector<size_t>       lens;
    std::vector<sre_int_t>    recs;
    std::vector<uint64_t>     vals, starts;     /* with a sink: the words of the batch's entries, uploaded */
    uint64_t                  nrep = 0;
    for (uint64_t i0 = 0; i0 < n;) {
        const uint64_t nb = bmax < n - i0 ? bmax : n - i0;
        /* ends[0]: the end of the line in front of the batch (its first line starts behind it) */
        ends.resize(nb + 1);
        if (i0) {
            SRE_HIP_TRY(hipMemcpyAsync(ends.data(), sc->d_ends + i0 - 1, (nb + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        } else {
            SRE_HIP_TRY(hipMemcpyAsync(ends.data() + 1, sc->d_ends, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        }
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        ptrs.resize(nb);
        lens.resize(nb);
        for (uint64_t j = 0; j < nb; j++) {
            const uint64_t st = (i0 + j == 0) ? 0 : ends[j] + 1;
            ptrs[j] = buf + st;
            lens[j] = ends[j + 1] - st;
        }
        recs.resize(nb * slots);
        if (sre_hip_scan_batch(sc, ptrs.data(), lens.data(), nb, recs.data(), stream) != 0) return -1;
        tot->fixups += sc->fixup_rounds;
        tot->exact += sc->exact_passes;
        tot->lineage += sc->lineage_passes;
        const double ms = sre_hip_scanner_last_kernel_ms(sc);
        tot->kms = (ms < 0 || tot->kms < 0) ? -1.0 : tot->kms + ms;
        /* with a sink, what its select pass writes, by the rules the kernels compile: the sink's table, then the sums' */
        for (int pass = 0; sink && pass < (sink->vgroups ? 2 : 1); pass++) {
            const sre_subst_pieces_t   *pc = pass ? NULL : sink->pieces;
            const sre_extract_groups_t *gr = pass ? sink->vgroups : sink->groups;
            const uint32_t              k = pc ? pc->np + 2 : gr ? gr->k : 1;
            const int                   smode = sink->mode, all_rows = smode == 2;
            vals.resize(nb * k);
            starts.resize(nb * k);
            for (uint64_t e = 0; e < nb * k; e++) {
                const uint64_t   j = e / k, st = (uint64_t) (static_cast<const uint8_t *>(ptrs[j]) - buf), len = lens[j];
                const uint32_t   f = (uint32_t) (e % k);
                const sre_int_t *rec = recs.data() + j * slots;
                if (pc) sre_sel_subst_entry(rec, SRE_DECLINED, all_rows, st, len, f, pc, &vals[e], &starts[e]);
                else if (gr) sre_sel_extract_entry(rec, SRE_DECLINED, all_rows, st, len, f, k, gr->g[f], &vals[e], &starts[e]);
                else if (sink->route) vals[e] = sre_lr_key(sre_lr_bucket(rec[0], SRE_DECLINED, sink->nreg, sc->h_rmap), len);
                else vals[e] = sre_sel_row(rec, SRE_DECLINED, smode) ? len + 1 : 0;
            }
            SRE_HIP_TRY(hipMemcpyAsync((pass ? sc->d_vval : sc->d_fval) + i0 * k, vals.data(), nb * k * sizeof(uint64_t),
                                       hipMemcpyHostToDevice, stream));
            if (pc || gr) {
                SRE_HIP_TRY(hipMemcpyAsync((pass ? sc->d_vstart : sc->d_fstart) + i0 * k, starts.data(), nb * k * sizeof(uint64_t),
                                           hipMemcpyHostToDevice, stream));
            }
            SRE_HIP_TRY(hipStreamSynchronize(stream));      /* (the next pass fills the vectors again) */
        }
        for (uint64_t j = 0; !sink && j < nb; j++) {
            const sre_int_t *rec = recs.data() + j * slots;
            if (!sre_sel_row(rec, SRE_DECLINED, all ? 2 : 0)) continue;
            if (nrep < cap) {
                sre_int_t *row = out + nrep * width;
                row[0] = (sre_int_t) (i0 + j);
                row[1] = (sre_int_t) (static_cast<const uint8_t *>(ptrs[j]) - buf);
                row[2] = (sre_int_t) lens[j];
                memcpy(row + 3, rec, slots * sizeof(sre_int_t));
            }
            nrep++;
        }
        sc->line_batches++;
        i0 += nb;
    }
    *pnrep = nrep;
    return 0;
hip_failed:
    return -1;
}

/* a line-mode call: the split and the driver of the scanner's route; with a sink its per-line array is grown to the
 * call's lines first.  The call replaces the scanner's last one; its diagnostics describe the whole call. */
static int
lines_call(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, int all, sre_int_t *out, size_t cap,
           const LinesSink *sink, uint64_t *pn, uint64_t *pnrep, hipStream_t stream)
{
    uint64_t    n = 0, nrep = 0;
    int         rc = -1;
    LinesTotals tot = {0, 0, 0, sc->engine == SRE_HIP_ENGINE_VM ? -1.0 : 0.0, 0};
    /* 0: per-line host work, 1: the table-driven scanner's device route, 2: the NFA tier's */
    int         route = sc->engine == SRE_HIP_ENGINE_SCAN ? 1 : 0;
    if (sc->engine == SRE_HIP_ENGINE_NFA && sc->cnt == NULL) {
        const char *e = getenv("SRE_HIP_LINES_NFA_HOST");       /* the per-line host route, for A/B measurements and tests */
        if (e == NULL || atoi(e) == 0) route = 2;
    }
    sc->line_batches = 0;
    if (sc->d_linfo == NULL) SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_linfo), sizeof(sre_lines_info_t)));
    if (sc->h_linfo == NULL) SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sc->h_linfo), sizeof(sre_lines_info_t), 0));
    if (lines_split(sc, d_buf, len, delim, stream, &n) == 0) {
        if (sink) {
            const uint64_t k = sink_entries(sink);
            if (lines_grow(&sc->d_fval, &sc->fval_cap, (n * k + 1) * sizeof(uint64_t)) != 0) goto hip_failed;
            if (sink->groups || sink->pieces || sink->join) {
                if (lines_grow(&sc->d_fstart, &sc->fstart_cap, n * k * sizeof(uint64_t)) != 0) goto hip_failed;
            }
            if (sink->vgroups) {
                const uint64_t v = sink->vgroups->k;
                if (lines_grow(&sc->d_vval, &sc->vval_cap, n * v * sizeof(uint64_t)) != 0) goto hip_failed;
                if (lines_grow(&sc->d_vstart, &sc->vstart_cap, n * v * sizeof(uint64_t)) != 0) goto hip_failed;
            }
            if (sink->join && lines_grow(&sc->d_jkey, &sc->jkey_cap, n * sizeof(int64_t)) != 0) goto hip_failed;
        }
        rc = route == 1   ? lines_scan_device(sc, d_buf, n, all, out, cap, &nrep, stream, &tot, sink)
             : route == 2 ? lines_scan_nfa(sc, d_buf, n, all, out, cap, &nrep, stream, &tot, sink)
                          : lines_scan_host(sc, d_buf, n, all, out, cap, &nrep, stream, &tot, sink);
    }
hip_failed:
    /* this call replaces the scanner's last one; its diagnostics describe the whole call */
    sc->last_lines = true;
    sc->last_n = 0;
    sc->ev_valid = 0;
    sc->fixup_rounds = tot.fixups;
    sc->exact_passes = tot.exact;
    sc->lineage_passes = tot.lineage;
    sc->lines_kernel_ms = rc == 0 ? tot.kms : -1.0;
    sc->lines_device = rc == 0 && route != 0;
    sc->short_lines = rc == 0 ? tot.nshort : 0;
    if (rc != 0) return -1;
    *pn = n;
    *pnrep = nrep;
    return 0;
}

extern "C" SRE_API int
sre_hip_scan_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, int flags,
    sre_int_t *out, size_t cap, size_t *nlines, size_t *nreported, void *hip_stream)
{
    if (sc == NULL || delim < 0 || delim > 255 || (flags & ~SRE_HIP_LINES_ALL) != 0 || (cap != 0 && out == NULL)
        || (len != 0 && d_buf == NULL))
    {
        return -1;
    }
    uint64_t n = 0, nrep = 0;
    if (lines_call(sc, d_buf, len, delim, (flags & SRE_HIP_LINES_ALL) != 0, out, cap, NULL, &n, &nrep,
                   static_cast<hipStream_t>(hip_stream)) != 0)
    {
        return -1;
    }
    if (nlines) *nlines = (size_t) n;
    if (nreported) *nreported = (size_t) nrep;
    return 0;
}

/* The tail of the sinks that scan an entry table (a word per line, fields or pieces), behind the line-mode call, in three
 * steps; a call may queue passes of its own between them.  First the scan to the offset table and the cut at out_cap. */
static int
sink_offsets(sre_hip_scanner_t *sc, const LinesSink *sink, uint64_t n, hipStream_t stream)
{
    const uint32_t k = sink_entries(sink);
    const uint64_t nblk = (n * k + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    if (lines_grow(&sc->d_fblk, &sc->fblk_cap, 2 * nblk * sizeof(uint64_t)) != 0) return -1;
    SRE_HIP_TRY(sink->pieces   ? sre_launch_subst_offsets(sc->d_fval, n, k, sc->d_fblk, sink->out_cap, sc->d_linfo, stream)
                : sink->groups || sink->join
                    ? sre_launch_extract_offsets(sc->d_fval, n, k, sc->d_fblk, sink->out_cap, sc->d_linfo, stream)
                               : sre_launch_filter_offsets(sc->d_fval, n, sc->d_fblk, sink->out_cap, sc->d_linfo, stream));
    return 0;
hip_failed:
    return -1;
}

/* ... then the one read of the call (the scan's four words and `more` of the call's own) into the fields every info has */
template <class Info, class... More>
static int
sink_read(sre_hip_scanner_t *sc, const LinesSink *sink, uint64_t n, Info *res, hipStream_t stream, More... more)
{
    SRE_HIP_TRY(linfo_read(sc, stream, {LINFO(fsel), LINFO(fneed), LINFO(fwritten), LINFO(fbytes), more...}));
    SRE_HIP_TRY(hipStreamSynchronize(stream));
    res->nlines = (size_t) n;
    res->nselected = (size_t) sc->h_linfo->fsel;
    res->need_bytes = (size_t) sc->h_linfo->fneed;
    res->nwritten = (size_t) sc->h_linfo->fwritten;
    res->out_bytes = (size_t) sc->h_linfo->fbytes;
    return res->out_bytes > sink->out_cap ? -1 : 0;     /* (cannot happen: the cut is made against out_cap) */
hip_failed:
    return -1;
}

/* ... then the gather of the out_bytes bytes and the index rows of the written lines, queued */
static int
sink_write(sre_hip_scanner_t *sc, const LinesSink *sink, const void *d_buf, uint64_t n, uint64_t out_bytes, uint64_t nwritten,
           hipStream_t stream)
{
    const uint32_t          k = sink_entries(sink), delim = (uint32_t) sink->delim, fsep = (uint32_t) sink->fsep;
    const uint64_t         *off = sc->d_fval, *start = sc->d_fstart, *ends = sc->d_ends, *blk = sc->d_fblk, cap = sink->index_cap;
    const sre_lines_info_t *li = sc->d_linfo;
    int64_t                *rows = sink->d_index;
    if (sink->pieces) SRE_HIP_TRY(sre_launch_subst_gather(d_buf, sink->d_out, off, start, sc->d_lit, n * k, out_bytes, delim, stream));
    else if (sink->groups) SRE_HIP_TRY(sre_launch_extract_gather(d_buf, sink->d_out, off, start, n * k, out_bytes, delim, fsep, stream));
    else if (sink->join) SRE_HIP_TRY(sre_launch_join_gather(d_buf, sink->d_out, off, start, sink->d_dict, n * k, out_bytes, delim, fsep, stream));
    else SRE_HIP_TRY(sre_launch_lines_gather(d_buf, sink->d_out, off, ends, n, out_bytes, delim, stream));
    if (nwritten == 0) return 0;
    if (sink->pieces) SRE_HIP_TRY(sre_launch_subst_index(off, start, ends, n, k, blk, li, cap, rows, stream));
    else if (sink->groups) SRE_HIP_TRY(sre_launch_extract_index(off, start, ends, n, k, blk, li, cap, rows, stream));
    else if (sink->join) SRE_HIP_TRY(sre_launch_join_index(off, start, ends, sc->d_jkey, n, k, blk, li, cap, rows, stream));
    else if (sink->context) SRE_HIP_TRY(sre_launch_context_index(off, ends, n, blk, sink->d_cbits, li, cap, rows, stream));
    else SRE_HIP_TRY(sre_launch_filter_index(off, ends, n, blk, li, cap, rows, stream));
    return 0;
hip_failed:
    return -1;
}

/* the three steps back to back and the wait for them: the whole tail of the filter, the extract and the substitute */
static int
sink_finish(sre_hip_scanner_t *sc, const LinesSink *sink, const void *d_buf, uint64_t n, sre_hip_filter_info_t *info,
            hipStream_t stream)
{
    sre_hip_filter_info_t res;
    memset(&res, 0, sizeof(res));
    if (n != 0) {
        if (sink_offsets(sc, sink, n, stream) != 0 || sink_read(sc, sink, n, &res, stream) != 0
            || sink_write(sc, sink, d_buf, n, res.out_bytes, res.nwritten, stream) != 0)
        {
            return -1;
        }
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return 0;
hip_failed:
    return -1;
}

/* The keyed calls (the lookup, the join, the route by key, the sort) open alike: the sink's row rule is the filter's mode 0
 * whatever the caller's flags are, so that every route leaves the per-line values, and the key groups are its value groups,
 * so that it leaves the key table too; the pass behind the line-mode call applies the flags.  join != 0: the join's table of
 * `join` entries per line, jsep between the fields of a row, the values from d_dict.  Then the line-mode call */
static int
keyed_call(sre_hip_scanner_t *sc, const char *call, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups,
           void *d_out, size_t out_cap, sre_int_t *d_index, size_t index_cap, uint32_t join, int jsep, const void *d_dict,
           LinesSink *sink, sre_extract_groups_t *gr, uint64_t *pn, hipStream_t stream)
{
    uint64_t nrep = 0;
    if (!sink_open(sink, sc, d_buf, len, delim, 0, d_out, out_cap, d_index, index_cap)) return -1;
    if (!sink_first_match(sc, call, "captures") || !sink_groups(sc, groups, ngroups, gr)) return -1;
    sink->vgroups = gr;
    if (join) {
        sink->join = join;
        sink->fsep = jsep;
        sink->d_dict = d_dict;
    }
    return lines_call(sc, d_buf, len, delim, 0, NULL, 0, sink, pn, &nrep, stream);
}

/* The tail of the lookup and the join behind keyed_call: the two counters zeroed, the call's own pass over the key table
 * (`pass` queues it), then the sinks' three steps with the counters in the one read, and the wait */
template <class Pass>
static int
keyed_finish(sre_hip_scanner_t *sc, const LinesSink *sink, const void *d_buf, uint64_t n, sre_hip_lookup_info_t *info, hipStream_t stream,
             Pass pass)
{
    sre_hip_lookup_info_t res;
    memset(&res, 0, sizeof(res));
    if (n != 0) {
        static_assert(offsetof(sre_lines_info_t, knmembers) == offsetof(sre_lines_info_t, knkeyed) + sizeof(uint64_t),
                      "knkeyed, knmembers are zeroed as one run");
        SRE_HIP_TRY(hipMemsetAsync(&sc->d_linfo->knkeyed, 0, 2 * sizeof(uint64_t), stream));
        SRE_HIP_TRY(pass());
        if (sink_offsets(sc, sink, n, stream) != 0) return -1;
        if (sink_read(sc, sink, n, &res, stream, LINFO(knkeyed), LINFO(knmembers)) != 0) return -1;
        res.nkeyed = (size_t) sc->h_linfo->knkeyed;
        res.nmembers = (size_t) sc->h_linfo->knmembers;
        if (sink_write(sc, sink, d_buf, n, res.out_bytes, res.nwritten, stream) != 0) return -1;
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return 0;
hip_failed:
    return -1;
}

/* The calls with a compact table (the route, the route by key, the sort) share what stands around their partition passes.
 * First the words every pass needs, for n lines and nd digits a pass: the counts, the sums of the scans (over the counts of
 * a pass, then over at most n entries of the compact table) and the result words */
static int
compact_reserve(sre_hip_scanner_t *sc, uint64_t n, uint64_t nd)
{
    const uint64_t ncnt = nd * ((n + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS);
    const uint64_t nblk = ((ncnt > n ? ncnt : n) + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
    const size_t   nres = SRE_LR_RES_WORDS + 2 * (size_t) SRE_LR_MAX_BUCKETS;
    static_assert(SRE_LRK_RES_WORDS <= SRE_LR_RES_WORDS + 2 * SRE_LR_MAX_BUCKETS && SRE_LSO_RES_WORDS <= SRE_LRK_RES_WORDS,
                  "the result words fit the route's");
    if (lines_grow(&sc->d_fblk, &sc->fblk_cap, 2 * nblk * sizeof(uint64_t)) != 0) return -1;
    if (lines_grow(&sc->d_rcnt, &sc->rcnt_cap, (ncnt + 1) * sizeof(uint64_t)) != 0) return -1;
    if (sc->d_rres == NULL) {
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_rres), nres * sizeof(uint64_t)));
        SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sc->h_rres), nres * sizeof(uint64_t), 0));
    }
    return 0;
hip_failed:
    return -1;
}

/* ... then the tail behind the call's finish pass: the one read of its nwords result words, the four every info has, and the
 * extract's gather over the compact table of nrows entries (d_rval, d_fstart: an entry table with one entry a line), queued.
 * *pindex: the index rows the call's own index pass is to write */
template <class Info>
static int
compact_finish(sre_hip_scanner_t *sc, const LinesSink *sink, const void *d_buf, uint64_t n, size_t nwords, uint64_t nrows, Info *res,
               uint64_t *pindex, hipStream_t stream)
{
    SRE_HIP_TRY(hipMemcpyAsync(sc->h_rres, sc->d_rres, nwords * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    SRE_HIP_TRY(hipStreamSynchronize(stream));
    res->nlines = (size_t) n;
    res->nselected = (size_t) sc->h_rres[SRE_LR_RES_NSEL];
    res->need_bytes = (size_t) sc->h_rres[SRE_LR_RES_NEED];
    res->nwritten = (size_t) sc->h_rres[SRE_LR_RES_WRITTEN];
    res->out_bytes = (size_t) sc->h_rres[SRE_LR_RES_BYTES];
    if (res->out_bytes > sink->out_cap || res->nselected != nrows || res->nwritten > nrows) return -1;      /* (cannot happen) */
    if (res->out_bytes != 0) {
        SRE_HIP_TRY(sre_launch_extract_gather(d_buf, sink->d_out, sc->d_rval, sc->d_fstart, nrows, res->out_bytes,
                                              (uint32_t) sink->delim, (uint32_t) sink->delim, stream));
    }
    *pindex = sink->index_cap < res->nwritten ? sink->index_cap : res->nwritten;
    return 0;
hip_failed:
    return -1;
}

/* The line filter: the line-mode call with a sink, then on the device the scan of the per-line
 * values to the offset table, the cut at out_cap, one read of four words, the gather and the index rows. */
extern "C" SRE_API int
sre_hip_filter_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, int flags, void *d_out,
    size_t out_cap, sre_int_t *d_index, size_t index_cap, sre_hip_filter_info_t *info, void *hip_stream)
{
    const int known = SRE_HIP_LINES_ALL | SRE_HIP_LINES_INVERT;
    LinesSink sink;
    if ((flags & ~known) != 0 || (flags & known) == known) return -1;
    if (!sink_open(&sink, sc, d_buf, len, delim, flags, d_out, out_cap, d_index, index_cap)) return -1;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0, nrep = 0;
    if (lines_call(sc, d_buf, len, delim, 0, NULL, 0, &sink, &n, &nrep, stream) != 0) return -1;
    return sink_finish(sc, &sink, d_buf, n, info, stream);
}

/* The line filter with context lines: sre_hip_filter_lines with one more device pass between the
 * line-mode call and the scan, the dilation of the per-line values by `before` and `after` lines, two more words in the
 * one read, and index rows of five words.  Without context no kernel of the pass runs: the values, the offset table and
 * the gather are the filter's, and the groups are counted from the offset table. */
extern "C" SRE_API int
sre_hip_filter_lines_context(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, int flags, size_t before,
    size_t after, void *d_out, size_t out_cap, sre_int_t *d_index, size_t index_cap, sre_hip_context_info_t *info,
    void *hip_stream)
{
    const int  known = SRE_HIP_LINES_ALL | SRE_HIP_LINES_INVERT;
    const bool context = before != 0 || after != 0;
    LinesSink  sink;
    if ((flags & ~known) != 0 || (flags & known) == known || ((flags & SRE_HIP_LINES_ALL) && context)
        || !sink_open(&sink, sc, d_buf, len, delim, flags, d_out, out_cap, d_index, index_cap))
    {
        return -1;
    }
    sink.context = true;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0, nrep = 0;
    if (lines_call(sc, d_buf, len, delim, 0, NULL, 0, &sink, &n, &nrep, stream) != 0) return -1;
    sre_hip_context_info_t res;
    memset(&res, 0, sizeof(res));
    if (n != 0) {
        const uint64_t nblk = (n + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
        if (lines_grow(&sc->d_cblk, &sc->cblk_cap, 4 * nblk * sizeof(uint64_t)) != 0) return -1;
        if (context) {
            if (lines_grow(&sc->d_cbits, &sc->cbits_cap, (n + 63) / 64 * sizeof(uint64_t)) != 0) return -1;
            SRE_HIP_TRY(sre_launch_context_select(sc->d_fval, sc->d_ends, n, before, after, sc->d_cbits, sc->d_cblk, sc->d_linfo,
                                                  stream));
            sink.d_cbits = sc->d_cbits;
        }
        if (sink_offsets(sc, &sink, n, stream) != 0) return -1;
        if (!context) SRE_HIP_TRY(sre_launch_context_runs(sc->d_fval, n, sc->d_cblk, sc->d_linfo, stream));
        if (sink_read(sc, &sink, n, &res, stream, LINFO(cmatched), LINFO(cgroups)) != 0) return -1;
        res.nmatched = context ? (size_t) sc->h_linfo->cmatched : res.nselected;
        res.ngroups = (size_t) sc->h_linfo->cgroups;
        if (sink_write(sc, &sink, d_buf, n, res.out_bytes, res.nwritten, stream) != 0) return -1;
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return 0;
hip_failed:
    return -1;
}

/* The line fold (rules in sre_lines_fold.h): sre_hip_filter_lines up to the per-line values, which mark the
 * continuation lines; then on the device the fold pass, which finds the heads of the records and turns the values into the
 * extract's entry table with one entry a line; the extract's scan, the cut moved back to a record boundary, one read (the
 * scan's four words and the fold's three), the extract's gather with `join` as its separator, and the two tables. */
extern "C" SRE_API int
sre_hip_fold_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, int flags, int join, size_t max_lines,
    void *d_out, size_t out_cap, sre_int_t *d_recid, size_t recid_cap, sre_int_t *d_records, size_t records_cap,
    sre_hip_fold_info_t *info, void *hip_stream)
{
    static_assert(sizeof(sre_int_t) == sizeof(int64_t), "the tables are 64-bit words");
    LinesSink sink;
    if ((flags & ~(SRE_HIP_LINES_INVERT | SRE_HIP_FOLD_NEXT)) != 0 || join < 0 || join > 255 || (d_recid == NULL) != (recid_cap == 0)
        || (d_records == NULL) != (records_cap == 0)
        || !sink_open(&sink, sc, d_buf, len, delim, flags & SRE_HIP_LINES_INVERT, d_out, out_cap, NULL, 0))
    {
        return -1;
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0, nrep = 0;
    if (lines_call(sc, d_buf, len, delim, 0, NULL, 0, &sink, &n, &nrep, stream) != 0) return -1;
    sre_hip_fold_info_t res;
    memset(&res, 0, sizeof(res));
    if (n != 0) {
        const uint64_t nblk = (n + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS;
        if (lines_grow(&sc->d_fstart, &sc->fstart_cap, n * sizeof(uint64_t)) != 0
            || lines_grow(&sc->d_fblk, &sc->fblk_cap, 2 * nblk * sizeof(uint64_t)) != 0
            || lines_grow(&sc->d_gbits, &sc->gbits_cap, 2 * ((n + 63) / 64) * sizeof(uint64_t)) != 0
            || lines_grow(&sc->d_gblk, &sc->gblk_cap, 5 * nblk * sizeof(uint64_t)) != 0
            || lines_grow(&sc->d_gaux, &sc->gaux_cap, n * sizeof(uint64_t)) != 0)
        {
            return -1;
        }
        SRE_HIP_TRY(sre_launch_fold_select(sc->d_fval, sc->d_fstart, sc->d_ends, n, (flags & SRE_HIP_FOLD_NEXT) != 0, max_lines,
                                           sc->d_gbits, sc->d_gaux, sc->d_gblk, sc->d_linfo, stream));
        SRE_HIP_TRY(sre_launch_extract_offsets(sc->d_fval, n, 1, sc->d_fblk, out_cap, sc->d_linfo, stream));
        SRE_HIP_TRY(sre_launch_fold_finish(sc->d_fval, n, sc->d_gbits, sc->d_gaux, sc->d_gblk, out_cap, sc->d_linfo, stream));
        SRE_HIP_TRY(linfo_read(sc, stream, {LINFO(fneed), LINFO(fwritten), LINFO(fbytes), LINFO(gnrec), LINFO(gmarked), LINFO(glongest)}));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        res.nlines = (size_t) n;
        res.nmarked = (size_t) sc->h_linfo->gmarked;
        res.nrecords = (size_t) sc->h_linfo->gnrec;
        res.longest = (size_t) sc->h_linfo->glongest;
        res.need_bytes = (size_t) sc->h_linfo->fneed;
        res.nwritten = (size_t) sc->h_linfo->fwritten;
        res.out_bytes = (size_t) sc->h_linfo->fbytes;
        if (res.out_bytes > out_cap) return -1;     /* (cannot happen: the cut is made against out_cap) */
        SRE_HIP_TRY(sre_launch_extract_gather(d_buf, d_out, sc->d_fval, sc->d_fstart, n, res.out_bytes, (uint32_t) delim,
                                              (uint32_t) join, stream));
        SRE_HIP_TRY(sre_launch_fold_tables(sc->d_fval, sc->d_ends, n, sc->d_gbits, sc->d_gaux, sc->d_gblk, sc->d_linfo,
                                           reinterpret_cast<int64_t *>(d_recid), recid_cap, reinterpret_cast<int64_t *>(d_records),
                                           records_cap, res.nwritten, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return 0;
hip_failed:
    return -1;
}

/* The line extract: the line-mode call with the extract's sink, then the filter's passes over the
 * entries (lines x fields): scan, cut at a line boundary, one read of four words, gather, index rows. */
extern "C" SRE_API int
sre_hip_extract_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups,
    int fsep, int flags, void *d_out, size_t out_cap, sre_int_t *d_index, size_t index_cap, sre_hip_filter_info_t *info,
    void *hip_stream)
{
    LinesSink            sink;
    sre_extract_groups_t gr;
    if (fsep < 0 || fsep > 255 || (flags & ~SRE_HIP_LINES_ALL) != 0 || groups == NULL || ngroups < 1
        || ngroups > SRE_HIP_EXTRACT_MAX_FIELDS || !sink_open(&sink, sc, d_buf, len, delim, flags, d_out, out_cap, d_index, index_cap))
    {
        return -1;
    }
    if (!sink_first_match(sc, "line extract", "captures") || !sink_groups(sc, groups, ngroups, &gr)) return -1;
    sink.groups = &gr;
    sink.fsep = fsep;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0, nrep = 0;
    if (lines_call(sc, d_buf, len, delim, 0, NULL, 0, &sink, &n, &nrep, stream) != 0) return -1;
    return sink_finish(sc, &sink, d_buf, n, info, stream);
}

/* the hash bits the tally's table index keeps: SRE_HIP_TALLY_HASH_BITS (test knob, read on every call; 0 .. 64), else all */
static uint64_t
tally_hash_mask(void)
{
    const char *e = getenv("SRE_HIP_TALLY_HASH_BITS");
    if (e == NULL || *e == 0) return ~(uint64_t) 0;
    return sre_lt_hash_mask(atoi(e));
}

/* the copies of the aggregates the sums' waves spread their atomics over: the rule's (sre_ls_copies), or at most
 * SRE_HIP_TALLY_SUM_COPIES of them (test knob, read on every call; 1: the caller's rows themselves) */
static uint32_t
tally_sum_copies(uint64_t rows, uint32_t v)
{
    const uint32_t copies = sre_ls_copies(rows, v);
    const char    *e = getenv("SRE_HIP_TALLY_SUM_COPIES");
    if (e == NULL || *e == 0) return copies;
    const int most = atoi(e);
    return most < 1 ? 1 : (uint32_t) most < copies ? (uint32_t) most : copies;
}

/* what the tallies (tally_call, sre_hip_tally_top_lines) know of a call: the sink with its key and value groups, the lines of
 * the buffer and, behind tally_front, the table of keys and the key number of every slot (the halves of d_ttab) */
struct TallyCall {
    LinesSink            sink;
    sre_extract_groups_t gr, vg;
    uint64_t             n, *tab, *cnt;
};

/* The tallies open alike: the arguments they share checked (`known`: the flags the caller has, of which the sink sees
 * SRE_HIP_LINES_ALL), the entry table over the key groups and, with value groups, the value table; then the line-mode call */
static int
tally_open(sre_hip_scanner_t *sc, const char *call, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups,
           const int *vgroups, size_t nvgroups, int fsep, int flags, int known, size_t max_keys, void *d_out, size_t out_cap,
           const uint64_t *d_counts, size_t counts_cap, sre_int_t *d_index, size_t index_cap, TallyCall *t, hipStream_t stream)
{
    uint64_t nrep = 0;
    if (fsep < 0 || fsep > 255 || (flags & ~known) != 0 || groups == NULL || ngroups < 1 || ngroups > SRE_HIP_EXTRACT_MAX_FIELDS
        || (counts_cap != 0 && d_counts == NULL) || max_keys < 1 || max_keys > SRE_LT_MAX_KEYS
        || !sink_open(&t->sink, sc, d_buf, len, delim, flags & SRE_HIP_LINES_ALL, d_out, out_cap, d_index, index_cap)
        || !sink_first_match(sc, call, "captures") || !sink_groups(sc, groups, ngroups, &t->gr)
        || !sink_groups(sc, vgroups, nvgroups, &t->vg))
    {
        return -1;
    }
    t->sink.groups = &t->gr;
    t->sink.fsep = fsep;
    if (vgroups) t->sink.vgroups = &t->vg;
    return lines_call(sc, d_buf, len, delim, 0, NULL, 0, &t->sink, &t->n, &nrep, stream);
}

/* The table of the tallies and of the line distinct for n lines and max_keys keys, grown and cleared, three memsets queued:
 * the keys' run of d_ttab to SRE_LT_EMPTY, the `zero_runs` runs behind it (the counts; the distinct's last lines) and the
 * first `words` of the info words tsel, tclaims, tover, dkept to 0.  Returns the slots of a run, 0 on failure */
static uint64_t
tally_table(sre_hip_scanner_t *sc, uint64_t n, size_t max_keys, uint32_t zero_runs, uint32_t words, hipStream_t stream)
{
    const uint64_t nslots = sre_lt_nslots(max_keys);
    if (lines_grow(&sc->d_ttab, &sc->ttab_cap, (1 + zero_runs) * nslots * sizeof(uint64_t)) != 0) return 0;
    if (lines_grow(&sc->d_tslot, &sc->tslot_cap, n * sizeof(uint32_t)) != 0) return 0;
    SRE_HIP_TRY(hipMemsetAsync(sc->d_ttab, 0xFF, nslots * sizeof(uint64_t), stream));         /* SRE_LT_EMPTY */
    SRE_HIP_TRY(hipMemsetAsync(sc->d_ttab + nslots, 0, zero_runs * nslots * sizeof(uint64_t), stream));
    static_assert(offsetof(sre_lines_info_t, tclaims) == offsetof(sre_lines_info_t, tsel) + sizeof(uint64_t)
                      && offsetof(sre_lines_info_t, tover) == offsetof(sre_lines_info_t, tsel) + 2 * sizeof(uint64_t)
                      && offsetof(sre_lines_info_t, dkept) == offsetof(sre_lines_info_t, tsel) + 3 * sizeof(uint64_t),
                  "tsel, tclaims, tover, dkept are zeroed as one run");
    SRE_HIP_TRY(hipMemsetAsync(&sc->d_linfo->tsel, 0, words * sizeof(uint64_t), stream));
    return nslots;
hip_failed:
    return 0;
}

/* Behind the line-mode call (t->n != 0): the table grown and cleared, the insert of every selected line and the keep pass
 * that leaves the first line of every key selected, the extract's scan with the cut at `cut` bytes and the one read (its
 * four words and the tally's three) into res.  0, SRE_HIP_TALLY_OVERFLOW (nothing is to be written) or -1 */
template <class Info>
static int
tally_front(sre_hip_scanner_t *sc, TallyCall *t, const void *d_buf, size_t max_keys, size_t cut, Info *res, hipStream_t stream)
{
    const uint64_t n = t->n, nslots = tally_table(sc, n, max_keys, 1, 3, stream);
    LinesSink      whole = t->sink;
    whole.out_cap = cut;
    if (nslots == 0) return -1;
    t->tab = sc->d_ttab;
    t->cnt = sc->d_ttab + nslots;
    SRE_HIP_TRY(sre_launch_tally_insert(d_buf, sc->d_fval, sc->d_fstart, n, t->gr.k, nslots, max_keys, tally_hash_mask(), t->tab, t->cnt,
                                        sc->d_tslot, sc->d_linfo, stream));
    if (sink_offsets(sc, &whole, n, stream) != 0) return -1;
    if (sink_read(sc, &whole, n, res, stream, LINFO(tsel), LINFO(tclaims), LINFO(tover)) != 0) return -1;
    /* the table selected the first line of every key: what the scan counted are the keys */
    res->nkeys = res->nselected;
    res->nselected = (size_t) sc->h_linfo->tsel;
    if (sc->h_linfo->tover != 0 || sc->h_linfo->tclaims > max_keys) {
        res->nkeys = res->need_bytes = res->nwritten = res->out_bytes = 0;      /* (only the two counts of lines stand) */
        return SRE_HIP_TALLY_OVERFLOW;
    }
    return res->nkeys == sc->h_linfo->tclaims ? 0 : -1;     /* (-1 cannot happen) */
hip_failed:
    return -1;
}

/* The line tally: the extract's call up to its select passes, then on the device the insert of every
 * selected line into the table of keys and the keep pass that leaves the first line of every key selected, then the
 * extract's scan, cut, one read (its four words and the tally's three), gather and index, and the ranks.
 * With value groups (sre_hip_tally_sums_lines; vgroups == NULL: the plain tally) every batch also
 * fills the value table, and the sums kernel is queued behind the ranks, in front of the last wait. */
static int
tally_call(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups, const int *vgroups,
    size_t nvgroups, int fsep, int flags, size_t max_keys, void *d_out, size_t out_cap, uint64_t *d_counts, size_t counts_cap,
    sre_hip_tally_sum_t *d_sums, size_t sums_cap, sre_int_t *d_keyid, size_t keyid_cap, sre_int_t *d_index, size_t index_cap,
    sre_hip_tally_info_t *info, void *hip_stream)
{
    TallyCall   t;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if ((keyid_cap != 0 && d_keyid == NULL)
        || tally_open(sc, "line tally", d_buf, len, delim, groups, ngroups, vgroups, nvgroups, fsep, flags, SRE_HIP_LINES_ALL, max_keys,
                      d_out, out_cap, d_counts, counts_cap, d_index, index_cap, &t, stream) != 0)
    {
        return -1;
    }
    sre_hip_tally_info_t res;
    memset(&res, 0, sizeof(res));
    const int rc = t.n != 0 ? tally_front(sc, &t, d_buf, max_keys, out_cap, &res, stream) : 0;
    if (rc < 0) return -1;
    if (t.n != 0 && rc == 0) {
        if (sink_write(sc, &t.sink, d_buf, t.n, res.out_bytes, res.nwritten, stream) != 0) return -1;
        SRE_HIP_TRY(sre_launch_tally_ranks(sc->d_fval, sc->d_fstart, t.n, t.gr.k, sc->d_fblk, sc->d_tslot, t.cnt, d_counts, counts_cap,
                                           reinterpret_cast<int64_t *>(d_keyid), keyid_cap, stream));
        if (vgroups && sums_cap != 0) {
            /* (without counts and key ids the ranks above launched nothing: the key numbers are still needed) */
            if (counts_cap == 0 && keyid_cap == 0) {
                SRE_HIP_TRY(sre_launch_tally_numbers(sc->d_fval, sc->d_fstart, t.n, t.gr.k, sc->d_fblk, sc->d_tslot, t.cnt, stream));
            }
            const uint64_t rows = sums_cap < res.nkeys ? sums_cap : res.nkeys;
            const uint32_t copies = tally_sum_copies(rows, t.vg.k);
            if (copies > 1 && lines_grow(&sc->d_vcopy, &sc->vcopy_cap, copies * rows * t.vg.k * sizeof(sre_ls_agg_t)) != 0) return -1;
            SRE_HIP_TRY(sre_launch_tally_sums(d_buf, sc->d_vval, sc->d_vstart, t.n, t.vg.k, sc->d_tslot, t.cnt, rows, d_sums,
                                              sc->d_vcopy, copies, stream));
        }
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return rc;
hip_failed:
    return -1;
}

extern "C" SRE_API int
sre_hip_tally_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups, int fsep,
    int flags, size_t max_keys, void *d_out, size_t out_cap, uint64_t *d_counts, size_t counts_cap, sre_int_t *d_keyid,
    size_t keyid_cap, sre_int_t *d_index, size_t index_cap, sre_hip_tally_info_t *info, void *hip_stream)
{
    return tally_call(sc, d_buf, len, delim, groups, ngroups, NULL, 0, fsep, flags, max_keys, d_out, out_cap, d_counts, counts_cap,
                      NULL, 0, d_keyid, keyid_cap, d_index, index_cap, info, hip_stream);
}

extern "C" SRE_API int
sre_hip_tally_sums_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups,
    const int *vgroups, size_t nvgroups, int fsep, int flags, size_t max_keys, void *d_out, size_t out_cap, uint64_t *d_counts,
    size_t counts_cap, sre_hip_tally_sum_t *d_sums, size_t sums_cap, sre_int_t *d_keyid, size_t keyid_cap, sre_int_t *d_index,
    size_t index_cap, sre_hip_tally_info_t *info, void *hip_stream)
{
    static_assert(sizeof(sre_hip_tally_sum_t) == sizeof(sre_ls_agg_t) && SRE_HIP_TALLY_MAX_VALUES == SRE_LS_MAX_VALUES,
                  "sre_lines_sums.h mirrors the public aggregate");
    if (vgroups == NULL || nvgroups < 1 || nvgroups > SRE_HIP_TALLY_MAX_VALUES || (sums_cap != 0 && d_sums == NULL)
        || (reinterpret_cast<uintptr_t>(d_sums) & 7u) != 0)
    {
        return -1;
    }
    return tally_call(sc, d_buf, len, delim, groups, ngroups, vgroups, nvgroups, fsep, flags, max_keys, d_out, out_cap, d_counts,
                      counts_cap, d_sums, sums_cap, d_keyid, keyid_cap, d_index, index_cap, info, hip_stream);
}

/* the number rule of the tally's sums on the host (sre_lines_sums.h) */
namespace {
struct HostText {
    const uint8_t *p;
    uint8_t byte(uint64_t at) const { return p[at]; }
};
}  // namespace

extern "C" SRE_API int
sre_hip_tally_number(const void *text, size_t len, int64_t *value)
{
    if (value == NULL || (len != 0 && text == NULL)) return 0;
    const HostText t = {static_cast<const uint8_t *>(text)};
    return sre_ls_number(t, 0, len, value) ? 1 : 0;
}

/* The template of the line substitute: the pieces in order, the literal bytes of all literal pieces back to back in
 * lit (SRE_SUBST_MAX_LITERAL bytes).  $digits and ${digits} are groups, $$ is one '$', every other byte is literal and
 * adjacent literals are one piece.  -1: a '$' in front of anything else, a group above max_group, too many pieces or
 * literal bytes */
/* ---- the key set and the line lookup (rules in sre_lines_keyset.h) ---- */

struct sre_hip_keyset_s {
    uint8_t  *d_rows;       /* the set's copy of the dictionary */
    uint64_t *d_fstart;     /* rows x k field offsets into it */
    uint64_t *d_flen;       /* ... and lengths */
    uint64_t *d_tab;        /* nslots words: SRE_LT_EMPTY or the lowest row of the slot's key */
    uint64_t *d_vstart;     /* a map's: rows x v value-column offsets into the copy */
    uint64_t *d_vlen;       /* ... and lengths */
    uint64_t  rows, distinct, nslots, hash_mask;
    uint32_t  k;            /* key fields of a row */
    uint32_t  v;            /* value columns behind them; 0: a plain set */
    int       delim;
    size_t    bytes;        /* device memory held */
};

/* the hash bits the set's table index keeps: SRE_HIP_KEYSET_HASH_BITS (test knob, read at create; 0 .. 64), else all */
static uint64_t
keyset_hash_mask(void)
{
    const char *e = getenv("SRE_HIP_KEYSET_HASH_BITS");
    if (e == NULL || *e == 0) return ~(uint64_t) 0;
    return sre_lt_hash_mask(atoi(e));
}

extern "C" SRE_API void
sre_hip_keyset_destroy(sre_hip_keyset_t *ks)
{
    if (ks == NULL) return;
    if (ks->d_rows) (void) hipFree(ks->d_rows);
    if (ks->d_fstart) (void) hipFree(ks->d_fstart);
    if (ks->d_flen) (void) hipFree(ks->d_flen);
    if (ks->d_tab) (void) hipFree(ks->d_tab);
    if (ks->d_vstart) (void) hipFree(ks->d_vstart);
    if (ks->d_vlen) (void) hipFree(ks->d_vlen);
    free(ks);
}

/* A key map: a key set whose rows carry nfields - nkeys value columns behind the nkeys key fields.
 * The plain set is the map without columns: the same passes, and its rows go through the same fields kernel as before. */
extern "C" SRE_API sre_hip_keyset_t *
sre_hip_keyset_create_map(const void *d_rows, size_t len, size_t nfields, size_t nkeys, int fsep, int delim, void *hip_stream)
{
    if (nfields < 1 || nfields > SRE_HIP_EXTRACT_MAX_FIELDS || nkeys < 1 || nkeys > nfields || fsep < 0 || fsep > 255 || delim < 0
        || delim > 255 || (nfields > 1 && fsep == delim) || (len != 0 && d_rows == NULL))
    {
        return NULL;
    }
    hipStream_t       stream = static_cast<hipStream_t>(hip_stream);
    sre_hip_keyset_t *ks = static_cast<sre_hip_keyset_t *>(calloc(1, sizeof(*ks)));
    /* what only the build needs: the split's words and tile counts, the row ends, and two words of its own */
    struct Words {
        sre_lines_info_t li;
        uint64_t         bad, distinct;
    };
    Words          *d_w = NULL;
    uint64_t       *d_tiles = NULL, *d_ends = NULL;
    uint64_t        h[2] = {0, 0};
    const uint64_t  ntiles = (len + SRE_LINES_TILE_BYTES - 1) / SRE_LINES_TILE_BYTES;
    size_t          nent = 0, nvent = 0;
    if (ks == NULL) return NULL;
    ks->k = (uint32_t) nkeys;
    ks->v = (uint32_t) (nfields - nkeys);
    ks->delim = delim;
    ks->hash_mask = keyset_hash_mask();
    ks->nslots = sre_lk_nslots(0);
    if (len != 0) {
        /* (16 bytes behind the copy: the split loads whole aligned chunks) */
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ks->d_rows), len + 16));
        SRE_HIP_TRY(hipMemcpyAsync(ks->d_rows, d_rows, len, hipMemcpyDeviceToDevice, stream));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_w), sizeof(Words)));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_tiles), ntiles * sizeof(uint64_t)));
        SRE_HIP_TRY(sre_launch_lines_count(ks->d_rows, len, (uint32_t) delim, d_tiles, &d_w->li, stream));
        SRE_HIP_TRY(hipMemcpyAsync(&h[0], &d_w->li.nlines, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        ks->rows = h[0];
        if (ks->rows > SRE_LK_MAX_ROWS) {
            fprintf(stderr, "[sregex-hip] key set: %llu rows, at most 2^30\n", (unsigned long long) ks->rows);
            goto hip_failed;
        }
        nent = (size_t) ks->rows * ks->k;
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_ends), ks->rows * sizeof(uint64_t)));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ks->d_fstart), nent * sizeof(uint64_t)));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ks->d_flen), nent * sizeof(uint64_t)));
        if (ks->v) {
            nvent = (size_t) ks->rows * ks->v;
            SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ks->d_vstart), nvent * sizeof(uint64_t)));
            SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ks->d_vlen), nvent * sizeof(uint64_t)));
        }
        SRE_HIP_TRY(sre_launch_lines_write(ks->d_rows, len, (uint32_t) delim, d_tiles, d_ends, stream));
        SRE_HIP_TRY(hipMemsetAsync(&d_w->bad, 0xFF, sizeof(uint64_t), stream));         /* SRE_LK_NO_ROW */
        SRE_HIP_TRY(hipMemsetAsync(&d_w->distinct, 0, sizeof(uint64_t), stream));
        if (ks->v) {
            SRE_HIP_TRY(sre_launch_keymap_fields(ks->d_rows, d_ends, ks->rows, (uint32_t) nfields, ks->k, (uint32_t) fsep, ks->d_fstart,
                                                 ks->d_flen, ks->d_vstart, ks->d_vlen, &d_w->bad, stream));
        } else {
            SRE_HIP_TRY(sre_launch_keyset_fields(ks->d_rows, d_ends, ks->rows, ks->k, (uint32_t) fsep, ks->d_fstart, ks->d_flen,
                                                 &d_w->bad, stream));
        }
        /* (the insert reads the fields of every row: it is queued only when every row has them) */
        SRE_HIP_TRY(hipMemcpyAsync(&h[0], &d_w->bad, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        if (h[0] != SRE_LK_NO_ROW) {
            fprintf(stderr, "[sregex-hip] key set: row %llu does not hold %u fields\n", (unsigned long long) h[0], (unsigned) nfields);
            goto hip_failed;
        }
        ks->nslots = sre_lk_nslots(ks->rows);
    }
    SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ks->d_tab), ks->nslots * sizeof(uint64_t)));
    SRE_HIP_TRY(hipMemsetAsync(ks->d_tab, 0xFF, ks->nslots * sizeof(uint64_t), stream));        /* SRE_LT_EMPTY */
    if (ks->rows != 0) {
        SRE_HIP_TRY(sre_launch_keyset_insert(ks->d_rows, ks->d_fstart, ks->d_flen, ks->rows, ks->k, ks->nslots, ks->hash_mask,
                                             ks->d_tab, &d_w->distinct, stream));
        SRE_HIP_TRY(hipMemcpyAsync(&h[1], &d_w->distinct, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    }
    SRE_HIP_TRY(hipStreamSynchronize(stream));
    ks->distinct = h[1];
    ks->bytes = (len ? len + 16 : 0) + 2 * (nent + nvent) * sizeof(uint64_t) + ks->nslots * sizeof(uint64_t);
    if (d_w) (void) hipFree(d_w);
    if (d_tiles) (void) hipFree(d_tiles);
    if (d_ends) (void) hipFree(d_ends);
    return ks;
hip_failed:
    (void) hipStreamSynchronize(stream);
    if (d_w) (void) hipFree(d_w);
    if (d_tiles) (void) hipFree(d_tiles);
    if (d_ends) (void) hipFree(d_ends);
    sre_hip_keyset_destroy(ks);
    return NULL;
}

extern "C" SRE_API sre_hip_keyset_t *
sre_hip_keyset_create(const void *d_rows, size_t len, size_t nfields, int fsep, int delim, void *hip_stream)
{
    return sre_hip_keyset_create_map(d_rows, len, nfields, nfields, fsep, delim, hip_stream);
}

extern "C" SRE_API size_t sre_hip_keyset_values(const sre_hip_keyset_t *ks) { return ks ? ks->v : 0; }
extern "C" SRE_API size_t sre_hip_keyset_rows(const sre_hip_keyset_t *ks) { return ks ? (size_t) ks->rows : 0; }
extern "C" SRE_API size_t sre_hip_keyset_distinct(const sre_hip_keyset_t *ks) { return ks ? (size_t) ks->distinct : 0; }
extern "C" SRE_API size_t sre_hip_keyset_fields(const sre_hip_keyset_t *ks) { return ks ? ks->k : 0; }
extern "C" SRE_API size_t sre_hip_keyset_slots(const sre_hip_keyset_t *ks) { return ks ? (size_t) ks->nslots : 0; }
extern "C" SRE_API size_t sre_hip_keyset_device_bytes(const sre_hip_keyset_t *ks) { return ks ? ks->bytes : 0; }

/* the set's hash on the host: the row's fields by the field rule, then the tally's hash over them */
extern "C" SRE_API uint64_t
sre_hip_keyset_hash(const void *row, size_t len, size_t nfields, int fsep)
{
    if (nfields < 1 || nfields > SRE_HIP_EXTRACT_MAX_FIELDS || fsep < 0 || fsep > 255 || (len != 0 && row == NULL)) return 0;
    uint64_t               fstart[SRE_HIP_EXTRACT_MAX_FIELDS], flen[SRE_HIP_EXTRACT_MAX_FIELDS];
    const HostText         t = {static_cast<const uint8_t *>(row)};
    const sre_lk_dict_keys keys = {t.p, fstart, flen, (uint32_t) nfields};
    if (!sre_lk_row_fields(t, 0, len, (uint32_t) nfields, (uint32_t) fsep, fstart, flen)) return 0;
    return sre_lt_hash(keys, 0);
}

/* The line lookup: the filter's call in mode 0 with the key groups as its value groups, so that every
 * route leaves the per-line values and the key table; then on the device the probe of every keyed line in the set's table,
 * which writes the key ids and clears the values of the lines the selection rule drops; then the filter's scan, cut, one
 * read (its four words and the lookup's two), gather and index. */
extern "C" SRE_API int
sre_hip_lookup_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups,
    const sre_hip_keyset_t *ks, int flags, void *d_out, size_t out_cap, sre_int_t *d_keyid, size_t keyid_cap, sre_int_t *d_index,
    size_t index_cap, sre_hip_lookup_info_t *info, void *hip_stream)
{
    LinesSink            sink;
    sre_extract_groups_t gr;
    if (ks == NULL || (flags & ~SRE_HIP_LINES_INVERT) != 0 || groups == NULL || ngroups < 1 || ngroups != ks->k
        || (keyid_cap != 0 && d_keyid == NULL))
    {
        return -1;
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0;
    if (keyed_call(sc, "line lookup", d_buf, len, delim, groups, ngroups, d_out, out_cap, d_index, index_cap, 0, 0, NULL, &sink, &gr, &n,
                   stream) != 0)
    {
        return -1;
    }
    return keyed_finish(sc, &sink, d_buf, n, info, stream, [&] {
        return sre_launch_keyset_probe(d_buf, sc->d_vval, sc->d_vstart, n, gr.k, ks->d_rows, ks->d_fstart, ks->d_flen, ks->d_tab,
                                       ks->nslots, ks->hash_mask, (flags & SRE_HIP_LINES_INVERT) != 0, sc->d_fval,
                                       reinterpret_cast<int64_t *>(d_keyid), keyid_cap, sc->d_linfo, stream);
    });
}

/* The line distinct (rules in sre_lines_distinct.h): the lookup's call (keyed_call), then on the device
 * the tally's table and insert over the KEY table, which leave every line's slot and every slot's first line and count; for
 * LAST the pass that leaves every slot's highest line; the pick pass, which clears the values of the lines the rule and the
 * flags drop; then the filter's scan, cut, one read (its four words, the tally's three and the qualifying keys), gather and
 * index; and the per-line arrays. */
extern "C" SRE_API int
sre_hip_distinct_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups, int which,
    size_t min_count, size_t max_count, int flags, size_t max_keys, void *d_out, size_t out_cap, uint64_t *d_keycount,
    size_t keycount_cap, sre_int_t *d_keyline, size_t keyline_cap, sre_int_t *d_index, size_t index_cap,
    sre_hip_distinct_info_t *info, void *hip_stream)
{
    static_assert(SRE_HIP_DISTINCT_FIRST == SRE_LD_FIRST && SRE_HIP_DISTINCT_LAST == SRE_LD_LAST
                      && SRE_HIP_DISTINCT_EVERY == SRE_LD_EVERY,
                  "sre_lines_distinct.h mirrors the public rule numbers");
    LinesSink            sink;
    sre_extract_groups_t gr;
    if (which < SRE_HIP_DISTINCT_FIRST || which > SRE_HIP_DISTINCT_EVERY || !sre_ld_range_ok(min_count, max_count)
        || (flags & ~SRE_HIP_LINES_INVERT) != 0 || max_keys < 1 || max_keys > SRE_LT_MAX_KEYS || groups == NULL || ngroups < 1
        || ngroups > SRE_HIP_EXTRACT_MAX_FIELDS || (keycount_cap != 0 && d_keycount == NULL)
        || (keyline_cap != 0 && d_keyline == NULL))
    {
        return -1;
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0;
    if (keyed_call(sc, "line distinct", d_buf, len, delim, groups, ngroups, d_out, out_cap, d_index, index_cap, 0, 0, NULL, &sink, &gr,
                   &n, stream) != 0)
    {
        return -1;
    }
    sre_hip_distinct_info_t res;
    memset(&res, 0, sizeof(res));
    if (n != 0) {
        const bool     last = which == SRE_HIP_DISTINCT_LAST;
        const uint64_t nslots = tally_table(sc, n, max_keys, last ? 2 : 1, 4, stream);
        if (nslots == 0) return -1;
        uint64_t *tab = sc->d_ttab, *cnt = tab + nslots, *lastrun = last ? cnt + nslots : NULL;
        /* (the insert's keep pass clears the key table's entries of every line but a key's first: nothing reads them again) */
        SRE_HIP_TRY(sre_launch_tally_insert(d_buf, sc->d_vval, sc->d_vstart, n, gr.k, nslots, max_keys, tally_hash_mask(), tab, cnt,
                                            sc->d_tslot, sc->d_linfo, stream));
        if (last) SRE_HIP_TRY(sre_launch_distinct_last(sc->d_tslot, n, nslots, lastrun, stream));
        SRE_HIP_TRY(sre_launch_distinct_pick(sc->d_tslot, n, nslots, tab, cnt, lastrun, which, min_count, max_count,
                                             (flags & SRE_HIP_LINES_INVERT) != 0, sc->d_fval, sc->d_linfo, stream));
        if (sink_offsets(sc, &sink, n, stream) != 0) return -1;
        if (sink_read(sc, &sink, n, &res, stream, LINFO(tsel), LINFO(tclaims), LINFO(tover), LINFO(dkept)) != 0) return -1;
        res.nkeyed = (size_t) sc->h_linfo->tsel;
        if (sc->h_linfo->tover != 0 || sc->h_linfo->tclaims > max_keys) {
            /* (only the two counts of lines stand; nothing is written) */
            res.nselected = res.need_bytes = res.nwritten = res.out_bytes = 0;
            if (info) *info = res;
            return SRE_HIP_TALLY_OVERFLOW;
        }
        res.nkeys = (size_t) sc->h_linfo->tclaims;
        res.nkeys_kept = (size_t) sc->h_linfo->dkept;
        if (sink_write(sc, &sink, d_buf, n, res.out_bytes, res.nwritten, stream) != 0) return -1;
        SRE_HIP_TRY(sre_launch_distinct_perline(sc->d_tslot, n, nslots, tab, cnt, d_keycount, keycount_cap,
                                                reinterpret_cast<int64_t *>(d_keyline), keyline_cap, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return 0;
hip_failed:
    return -1;
}

/* The line join: the lookup's call, key groups and host waits; in the probe's place the join pass, which
 * walks the same table and fills the table of 1 + nvcols entries per line; then the extract's scan and cut over that table,
 * the one read, the gather with the map's copy of the dictionary as its second extent, and the index. */
extern "C" SRE_API int
sre_hip_join_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups,
    const sre_hip_keyset_t *ks, const int *vcols, size_t nvcols, int jsep, int flags, void *d_out, size_t out_cap, sre_int_t *d_keyid,
    size_t keyid_cap, sre_int_t *d_index, size_t index_cap, sre_hip_lookup_info_t *info, void *hip_stream)
{
    LinesSink            sink;
    sre_extract_groups_t gr;
    sre_lj_cols_t        cols;
    static_assert(SRE_HIP_JOIN_MAX_VALUES == SRE_LJ_MAX_VALUES && 1 + SRE_LJ_MAX_VALUES <= SRE_EXTRACT_MAX_FIELDS,
                  "a row of the join table is a row of the extract's");
    if (ks == NULL || ks->v == 0 || (flags & ~SRE_HIP_LINES_ALL) != 0 || groups == NULL || ngroups < 1 || ngroups != ks->k
        || vcols == NULL || nvcols < 1 || nvcols > SRE_HIP_JOIN_MAX_VALUES || jsep < 0 || jsep > 255 || jsep == delim
        || delim != ks->delim || (keyid_cap != 0 && d_keyid == NULL))
    {
        return -1;
    }
    memset(&cols, 0, sizeof(cols));
    cols.n = (uint32_t) nvcols;
    for (size_t x = 0; x < nvcols; x++) {
        if (vcols[x] < 0 || (size_t) vcols[x] >= ks->v) return -1;
        cols.col[x] = (uint8_t) vcols[x];
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0;
    if (keyed_call(sc, "line join", d_buf, len, delim, groups, ngroups, d_out, out_cap, d_index, index_cap, 1 + cols.n, jsep, ks->d_rows,
                   &sink, &gr, &n, stream) != 0)
    {
        return -1;
    }
    return keyed_finish(sc, &sink, d_buf, n, info, stream, [&] {
        return sre_launch_keyset_join(d_buf, sc->d_vval, sc->d_vstart, sc->d_ends, n, gr.k, ks->d_rows, ks->d_fstart, ks->d_flen,
                                      ks->d_vstart, ks->d_vlen, ks->v, ks->d_tab, ks->nslots, ks->hash_mask, &cols,
                                      (flags & SRE_HIP_LINES_ALL) != 0, sc->d_fval, sc->d_fstart, sc->d_jkey,
                                      reinterpret_cast<int64_t *>(d_keyid), keyid_cap, sc->d_linfo, stream);
    });
}

static int
subst_parse(const uint8_t *t, size_t n, int max_group, sre_subst_pieces_t *pc, uint8_t *lit, size_t *lit_len)
{
    size_t nlit = 0;
    bool   in_literal = false;
    memset(pc, 0, sizeof(*pc));
    for (size_t i = 0; i < n;) {
        int group = -1;
        if (t[i] == '$' && !(i + 1 < n && t[i + 1] == '$')) {
            size_t     j = i + 1;
            const bool brace = j < n && t[j] == '{';
            if (brace) j++;
            const size_t d0 = j;
            long         v = 0;
            while (j < n && t[j] >= '0' && t[j] <= '9') {
                v = v * 10 + (t[j] - '0');
                if (v > 0xFFFF) return -1;
                j++;
            }
            if (j == d0) return -1;
            if (brace) {
                if (j >= n || t[j] != '}') return -1;
                j++;
            }
            if (v > max_group) return -1;
            group = (int) v;
            i = j;
        }
        if (group >= 0) {
            if (pc->np >= SRE_SUBST_MAX_PIECES) return -1;
            pc->g[pc->np++] = (int16_t) group;
            in_literal = false;
            continue;
        }
        const uint8_t c = t[i];
        i += c == '$' ? 2 : 1;
        if (nlit >= SRE_SUBST_MAX_LITERAL) return -1;
        if (!in_literal) {
            if (pc->np >= SRE_SUBST_MAX_PIECES) return -1;
            pc->g[pc->np] = -1;
            pc->off[pc->np] = (uint16_t) nlit;
            pc->len[pc->np] = 0;
            pc->np++;
            in_literal = true;
        }
        if (lit) lit[nlit] = c;
        nlit++;
        pc->len[pc->np - 1]++;
    }
    *lit_len = nlit;
    return 0;
}

extern "C" SRE_API int
sre_hip_subst_template_check(const void *tmpl, size_t tmpl_len, int max_group, int *piece_groups, size_t *npieces)
{
    sre_subst_pieces_t pc;
    size_t             nlit = 0;
    if (tmpl_len != 0 && tmpl == NULL) return -1;
    if (subst_parse(static_cast<const uint8_t *>(tmpl), tmpl_len, max_group, &pc, NULL, &nlit) != 0) return -1;
    for (uint32_t q = 0; piece_groups && q < pc.np; q++) piece_groups[q] = pc.g[q];
    if (npieces) *npieces = pc.np;
    return 0;
}

/* The line substitute: the template parsed and its literals put into the scanner's literal block,
 * the line-mode call with the substitute's sink, then the extract's passes over the entries (lines x (pieces + 2)) with
 * the lines counted by their last entries: scan, cut at a line boundary, one read of four words, gather, index rows. */
extern "C" SRE_API int
sre_hip_substitute_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const void *tmpl, size_t tmpl_len,
    int flags, void *d_out, size_t out_cap, sre_int_t *d_index, size_t index_cap, sre_hip_filter_info_t *info, void *hip_stream)
{
    LinesSink sink;
    if ((flags & ~SRE_HIP_LINES_ALL) != 0 || (tmpl_len != 0 && tmpl == NULL)
        || !sink_open(&sink, sc, d_buf, len, delim, flags, d_out, out_cap, d_index, index_cap))
    {
        return -1;
    }
    if (!sink_first_match(sc, "line substitute", "captures")) return -1;
    sre_subst_pieces_t pc;
    uint8_t            lit[SRE_SUBST_MAX_LITERAL];
    size_t             nlit = 0;
    /* ovec_slots = 2 * (max_ncaps + 1) */
    if (subst_parse(static_cast<const uint8_t *>(tmpl), tmpl_len, (int) sc->ovec_slots / 2 - 1, &pc, lit, &nlit) != 0) return -1;
    /* a literal delimiter would make two rows of one line */
    if (nlit != 0 && memchr(lit, delim, nlit) != NULL) return -1;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    /* the literal block: allocated once, uploaded when the literals differ from the ones it holds */
    if (sc->d_lit == NULL) {
        sc->lit_valid = false;
        if (sc->h_lit == NULL) sc->h_lit = static_cast<uint8_t *>(calloc(1, SRE_SUBST_MAX_LITERAL));
        if (sc->h_lit == NULL) return -1;
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_lit), SRE_SUBST_MAX_LITERAL));
    }
    if (!sc->lit_valid || sc->lit_len != nlit || memcmp(sc->h_lit, lit, nlit) != 0) {
        const size_t padded = (nlit + 15) / 16 * 16;
        sc->lit_valid = false;
        memset(sc->h_lit, 0, SRE_SUBST_MAX_LITERAL);
        memcpy(sc->h_lit, lit, nlit);
        sc->lit_len = nlit;
        if (padded) SRE_HIP_TRY(hipMemcpyAsync(sc->d_lit, sc->h_lit, padded, hipMemcpyHostToDevice, stream));
        sc->lit_valid = true;
    }
    {
        uint64_t n = 0, nrep = 0;
        sink.pieces = &pc;
        if (lines_call(sc, d_buf, len, delim, 0, NULL, 0, &sink, &n, &nrep, stream) != 0) {
            sc->lit_valid = false;      /* (the upload may not have run) */
            return -1;
        }
        return sink_finish(sc, &sink, d_buf, n, info, stream);
    }
hip_failed:
    return -1;
}

/* The line route: the line-mode call with the route's sink (a key per line), then on the device the
 * per-(bucket, workgroup) counts and their scan, one read of the selected lines, the scatter into the compact table, the
 * filter's scan over it, the cut and the bucket totals, one read of 4 + 2 nbuckets words, the extract's gather over the
 * compact table and the index rows.  (Its table is compact and its result words are its own: it shares the sinks'
 * argument checks and none of their tail.) */
extern "C" SRE_API int
sre_hip_route_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *bucket_of, size_t nbuckets,
    void *d_out, size_t out_cap, sre_int_t *d_index, size_t index_cap, sre_hip_filter_info_t *info,
    sre_hip_route_bucket_t *buckets, void *hip_stream)
{
    LinesSink sink;
    if (nbuckets < 1 || nbuckets > SRE_LR_MAX_BUCKETS || !sink_open(&sink, sc, d_buf, len, delim, 0, d_out, out_cap, d_index, index_cap)) {
        return -1;
    }
    if (!sink_first_match(sc, "line route", "regex id")) return -1;
    const uint32_t R = sc->prog->nregexes;
    if (bucket_of == NULL && nbuckets != R) return -1;
    std::vector<int32_t> map(R + 1);
    for (uint32_t r = 0; r <= R; r++) {
        const int b = bucket_of ? bucket_of[r] : (r < R ? (int) r : -1);
        if (b < -1 || b >= (int) nbuckets) return -1;
        map[r] = b;
    }
    hipStream_t           stream = static_cast<hipStream_t>(hip_stream);
    const uint32_t        nb = (uint32_t) nbuckets;
    sre_hip_filter_info_t res;
    memset(&res, 0, sizeof(res));
    if (buckets) memset(buckets, 0, nbuckets * sizeof(*buckets));
    /* the map on the device, uploaded when it differs from the one it holds */
    if (sc->d_rmap == NULL) {
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_rmap), (R + 1) * sizeof(int32_t)));
        sc->h_rmap = static_cast<int32_t *>(malloc((R + 1) * sizeof(int32_t)));
        if (sc->h_rmap == NULL) return -1;
        sc->rmap_valid = false;
    }
    if (!sc->rmap_valid || memcmp(sc->h_rmap, map.data(), (R + 1) * sizeof(int32_t)) != 0) {
        sc->rmap_valid = false;
        memcpy(sc->h_rmap, map.data(), (R + 1) * sizeof(int32_t));
        SRE_HIP_TRY(hipMemcpyAsync(sc->d_rmap, sc->h_rmap, (R + 1) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        sc->rmap_valid = true;
    }
    {
        uint64_t n = 0, nrep = 0;
        sink.route = true;
        sink.nreg = R;
        if (lines_call(sc, d_buf, len, delim, 0, NULL, 0, &sink, &n, &nrep, stream) != 0) return -1;
        if (n != 0) {
            const uint64_t nwg = (n + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS, ncnt = nb * nwg;
            uint64_t       nrows = 0;
            if (compact_reserve(sc, n, nb) != 0) return -1;
            SRE_HIP_TRY(sre_launch_route_count(sc->d_fval, n, nb, sc->d_rcnt, stream));
            SRE_HIP_TRY(sre_launch_filter_offsets(sc->d_rcnt, ncnt, sc->d_fblk, ~(uint64_t) 0, sc->d_linfo, stream));
            /* the selected lines size the compact table */
            SRE_HIP_TRY(hipMemcpyAsync(sc->h_rres, sc->d_rcnt + ncnt, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
            SRE_HIP_TRY(hipStreamSynchronize(stream));
            const uint64_t nsel = sc->h_rres[0];
            if (nsel > n) return -1;        /* (cannot happen: every line is counted once) */
            if (nsel != 0) {
                if (lines_grow(&sc->d_fstart, &sc->fstart_cap, nsel * sizeof(uint64_t)) != 0) return -1;
                if (lines_grow(&sc->d_rval, &sc->rval_cap, (nsel + 1) * sizeof(uint64_t)) != 0) return -1;
                if (lines_grow(&sc->d_rmeta, &sc->rmeta_cap, nsel * sizeof(uint64_t)) != 0) return -1;
                SRE_HIP_TRY(sre_launch_route_scatter(sc->d_fval, sc->d_ends, n, nb, sc->d_rcnt, nsel, sc->d_fstart, sc->d_rval,
                                                     sc->d_rmeta, stream));
                SRE_HIP_TRY(sre_launch_filter_offsets(sc->d_rval, nsel, sc->d_fblk, out_cap, sc->d_linfo, stream));
            }
            SRE_HIP_TRY(sre_launch_route_finish(sc->d_rcnt, n, nb, sc->d_rval, nsel, out_cap, sc->d_rres, stream));
            if (compact_finish(sc, &sink, d_buf, n, SRE_LR_RES_WORDS + 2 * (size_t) nb, nsel, &res, &nrows, stream) != 0) return -1;
            if (buckets) {
                size_t at = 0;
                for (uint32_t b = 0; b < nb; b++) {
                    buckets[b].nlines = (size_t) sc->h_rres[SRE_LR_RES_WORDS + 2 * b];
                    buckets[b].bytes = (size_t) sc->h_rres[SRE_LR_RES_WORDS + 2 * b + 1];
                    buckets[b].offset = at;
                    at += buckets[b].bytes;
                }
            }
            if (nrows != 0) {
                SRE_HIP_TRY(sre_launch_route_index(sc->d_rval, sc->d_fstart, sc->d_rmeta, sc->d_rres, nrows, index_cap, d_index,
                                                   stream));
            }
            SRE_HIP_TRY(hipStreamSynchronize(stream));
        }
    }
    if (info) *info = res;
    return 0;
hip_failed:
    return -1;
}

/* the digit width of the route by key: SRE_HIP_ROUTE_KEY_DIGIT_BITS (test knob, read on every call; 1 .. 8), else 8 */
static uint32_t
route_key_digit_bits(void)
{
    const char *e = getenv("SRE_HIP_ROUTE_KEY_DIGIT_BITS");
    return sre_lrk_digit_bits(e && *e ? atol(e) : 0);
}

/* ... and its rank rule inside a slot: SRE_HIP_ROUTE_KEY_RANK=turns (measurement knob, read on every call) takes the route's
 * wave rule, anything else the ballots per digit bit; the results are the same */
static int
route_key_rank_rule(void)
{
    const char *e = getenv("SRE_HIP_ROUTE_KEY_RANK");
    return e && strcmp(e, "turns") == 0 ? SRE_LRK_RANK_TURNS : SRE_LRK_RANK_BITS;
}

/* The line route by key: the lookup's call and probe, the key ids into the scanner's own array; then the
 * stable partition of the lines by their sort key, one count / scan / scatter per digit, with one read of the selected lines
 * behind the first scan; then the compact table from the sorted items, the scans over its values and over the head flags,
 * the bucket rows, the cut, one read of the result words, the extract's gather over the compact table and the index rows. */
extern "C" SRE_API int
sre_hip_route_lines_by_key(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups,
    const sre_hip_keyset_t *ks, int flags, void *d_out, size_t out_cap, sre_int_t *d_keyid, size_t keyid_cap, sre_int_t *d_index,
    size_t index_cap, sre_int_t *d_buckets, size_t buckets_cap, sre_hip_route_key_info_t *info, void *hip_stream)
{
    LinesSink            sink;
    sre_extract_groups_t gr;
    if (ks == NULL || (flags & ~SRE_HIP_LINES_ALL) != 0 || groups == NULL || ngroups < 1 || ngroups != ks->k
        || (keyid_cap != 0 && d_keyid == NULL) || (buckets_cap != 0 && d_buckets == NULL))
    {
        return -1;
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0;
    if (keyed_call(sc, "line route by key", d_buf, len, delim, groups, ngroups, d_out, out_cap, d_index, index_cap, 0, 0, NULL, &sink,
                   &gr, &n, stream) != 0)
    {
        return -1;
    }
    sre_hip_route_key_info_t res;
    memset(&res, 0, sizeof(res));
    if (n > SRE_LRK_MAX_LINES) {
        fprintf(stderr, "[sregex-hip] line route by key: %llu lines, at most 2^32 - 1\n", (unsigned long long) n);
        return -1;
    }
    if (n != 0) {
        const int      all = (flags & SRE_HIP_LINES_ALL) != 0, rule = route_key_rank_rule();
        const uint64_t rows = ks->rows;
        const uint32_t bits = route_key_digit_bits(), passes = sre_lrk_passes(sre_lrk_max_key(rows, all), bits);
        const uint64_t nd = (uint64_t) 1 << bits, nwg = (n + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS, ncnt = nd * nwg;
        uint64_t       nrows = 0;
        if (compact_reserve(sc, n, nd) != 0) return -1;
        if (lines_grow(&sc->d_jkey, &sc->jkey_cap, n * sizeof(int64_t)) != 0) return -1;
        /* the lookup's probe, the ids of all lines into the scanner's array; the caller's are a copy */
        SRE_HIP_TRY(hipMemsetAsync(&sc->d_linfo->knkeyed, 0, 2 * sizeof(uint64_t), stream));
        SRE_HIP_TRY(sre_launch_keyset_probe(d_buf, sc->d_vval, sc->d_vstart, n, gr.k, ks->d_rows, ks->d_fstart, ks->d_flen, ks->d_tab,
                                            ks->nslots, ks->hash_mask, 0, sc->d_fval, sc->d_jkey, n, sc->d_linfo, stream));
        if (keyid_cap != 0) {
            SRE_HIP_TRY(hipMemcpyAsync(d_keyid, sc->d_jkey, (keyid_cap < n ? keyid_cap : n) * sizeof(int64_t), hipMemcpyDeviceToDevice,
                                       stream));
        }
        /* pass 0 over the lines; its total sizes the item arrays and the compact table */
        SRE_HIP_TRY(sre_launch_route_key_count(sc->d_jkey, NULL, n, rows, all, 0, bits, rule, sc->d_rcnt, stream));
        SRE_HIP_TRY(sre_launch_filter_offsets(sc->d_rcnt, ncnt, sc->d_fblk, ~(uint64_t) 0, sc->d_linfo, stream));
        SRE_HIP_TRY(hipMemcpyAsync(sc->h_rres, sc->d_rcnt + ncnt, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        const uint64_t nsel = sc->h_rres[0];
        if (nsel > n) return -1;        /* (cannot happen: every line is counted once) */
        const uint64_t *hoff = NULL, *items = NULL;
        if (nsel != 0) {
            uint32_t cur = 0;
            if (lines_grow(&sc->d_kitem[0], &sc->kitem_cap[0], (nsel + 1) * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_kitem[1], &sc->kitem_cap[1], (nsel + 1) * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_fstart, &sc->fstart_cap, nsel * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_rval, &sc->rval_cap, (nsel + 1) * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_rmeta, &sc->rmeta_cap, (nsel + 1) * sizeof(uint64_t)) != 0) return -1;
            SRE_HIP_TRY(sre_launch_route_key_scatter(sc->d_jkey, NULL, n, rows, all, 0, bits, rule, sc->d_rcnt, nsel, sc->d_kitem[0],
                                                     stream));
            /* the later passes over the nsel items, from one array to the other */
            for (uint32_t p = 1; p < passes; p++, cur ^= 1u) {
                const uint64_t pcnt = nd * ((nsel + SRE_LINES_ITEMS - 1) / SRE_LINES_ITEMS);
                SRE_HIP_TRY(sre_launch_route_key_count(NULL, sc->d_kitem[cur], nsel, rows, all, p, bits, rule, sc->d_rcnt, stream));
                SRE_HIP_TRY(sre_launch_filter_offsets(sc->d_rcnt, pcnt, sc->d_fblk, ~(uint64_t) 0, sc->d_linfo, stream));
                SRE_HIP_TRY(sre_launch_route_key_scatter(NULL, sc->d_kitem[cur], nsel, rows, all, p, bits, rule, sc->d_rcnt, nsel,
                                                         sc->d_kitem[cur ^ 1u], stream));
            }
            /* the compact table and the head flags from the sorted items; the scan of the flags, then of the values (the
             * second leaves the words of d_linfo as the cut at out_cap gives them) */
            uint64_t *head = sc->d_kitem[cur ^ 1u];
            items = sc->d_kitem[cur];
            SRE_HIP_TRY(sre_launch_route_key_table(items, sc->d_ends, nsel, n, sc->d_fstart, sc->d_rval, head, stream));
            SRE_HIP_TRY(sre_launch_filter_offsets(head, nsel, sc->d_fblk, ~(uint64_t) 0, sc->d_linfo, stream));
            SRE_HIP_TRY(sre_launch_filter_offsets(sc->d_rval, nsel, sc->d_fblk, out_cap, sc->d_linfo, stream));
            SRE_HIP_TRY(sre_launch_route_key_buckets(items, head, sc->d_rmeta, sc->d_rval, nsel, rows, buckets_cap,
                                                     reinterpret_cast<int64_t *>(d_buckets), stream));
            hoff = head;
        }
        SRE_HIP_TRY(sre_launch_route_key_finish(sc->d_rval, hoff, nsel, out_cap, sc->d_linfo, sc->d_rres, stream));
        if (compact_finish(sc, &sink, d_buf, n, SRE_LRK_RES_WORDS, nsel, &res, &nrows, stream) != 0) return -1;
        res.nkeyed = (size_t) sc->h_rres[SRE_LRK_RES_NKEYED];
        res.nmembers = (size_t) sc->h_rres[SRE_LRK_RES_NMEMBERS];
        res.nbuckets = (size_t) sc->h_rres[SRE_LRK_RES_NBUCKETS];
        if (nrows != 0) {
            SRE_HIP_TRY(sre_launch_route_key_index(items, sc->d_fstart, sc->d_rval, sc->d_rres, rows, nrows,
                                                   index_cap, reinterpret_cast<int64_t *>(d_index), stream));
        }
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return 0;
hip_failed:
    return -1;
}

/* The digit passes of the sort, of the ordered tally and of one chunk of the sort by text, queued behind the read of the totals
 * of the values pass (vmin, vmax, nnum; compact_reserve has the counts of a pass): the passes over the digits digits[0 ..
 * ndigits), at least one, in that order.  from < 0: the items do not exist yet; the item arrays of the nsel items selected (at
 * least one) are sized, the first digit's pass makes the items in pair 0 and drops the unselected, over the n values and classes
 * (d_jkey, d_sclass; the digit is 0) or, d_lkeys != NULL, over the keys of the n lines.  from >= 0: the n == nsel items are in
 * that pair.  The later passes move them from one pair of arrays to the other.  Returns the pair that holds the sorted items,
 * -1 on failure */
static int
sort_passes(sre_hip_scanner_t *sc, uint64_t n, uint64_t nsel, int64_t vmin, int64_t vmax, uint64_t nnum, int desc, int all,
            const uint32_t *digits, uint32_t ndigits, const uint64_t *d_lkeys, int from, hipStream_t stream)
{
    const uint64_t nd = (uint64_t) 1 << SRE_LSO_DIGIT_BITS, per = SRE_LINES_ITEMS;
    uint32_t       cur = from < 0 ? 0u : (uint32_t) from, p = 0;
    if (ndigits == 0 || (from >= 0 && n != nsel)) return -1;
    if (from < 0) {
        for (int h = 0; h < 2; h++) {
            if (lines_grow(&sc->d_kitem[h], &sc->kitem_cap[h], (nsel + 1) * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_sline[h], &sc->sline_cap[h], nsel * sizeof(uint32_t)) != 0) return -1;
        }
        if (d_lkeys) SRE_HIP_TRY(sre_launch_sort_text_count(d_lkeys, n, digits[0], sc->d_rcnt, stream));
        else {
            SRE_HIP_TRY(sre_launch_sort_count(sc->d_jkey, sc->d_sclass, NULL, n, vmin, vmax, nnum, desc, all, digits[0], sc->d_rcnt,
                                              stream));
        }
        SRE_HIP_TRY(sre_launch_filter_offsets(sc->d_rcnt, nd * ((n + per - 1) / per), sc->d_fblk, ~(uint64_t) 0, sc->d_linfo, stream));
        if (d_lkeys) {
            SRE_HIP_TRY(sre_launch_sort_text_scatter(d_lkeys, n, digits[0], sc->d_rcnt, nsel, sc->d_kitem[0], sc->d_sline[0], stream));
        } else {
            SRE_HIP_TRY(sre_launch_sort_scatter(sc->d_jkey, sc->d_sclass, NULL, NULL, n, vmin, vmax, nnum, desc, all, digits[0], sc->d_rcnt,
                                                nsel, sc->d_kitem[0], sc->d_sline[0], stream));
        }
        p = 1;
    }
    for (; p < ndigits; p++, cur ^= 1u) {
        SRE_HIP_TRY(sre_launch_sort_count(NULL, NULL, sc->d_kitem[cur], nsel, vmin, vmax, nnum, desc, all, digits[p], sc->d_rcnt,
                                          stream));
        SRE_HIP_TRY(sre_launch_filter_offsets(sc->d_rcnt, nd * ((nsel + per - 1) / per), sc->d_fblk, ~(uint64_t) 0, sc->d_linfo, stream));
        SRE_HIP_TRY(sre_launch_sort_scatter(NULL, NULL, sc->d_kitem[cur], sc->d_sline[cur], nsel, vmin, vmax, nnum, desc, all,
                                            digits[p], sc->d_rcnt, nsel, sc->d_kitem[cur ^ 1u], sc->d_sline[cur ^ 1u], stream));
    }
    return (int) cur;
hip_failed:
    return -1;
}

/* the digit list of a sort whose key is one word: 0 .. passes - 1 */
static const uint32_t sort_digits[SRE_LSO_MAX_PASSES] = {0, 1, 2, 3, 4, 5, 6, 7};

/* The line sort: the lookup's call with the one sort group as its value group; then the values pass,
 * which leaves the value and the class of every line and the four totals; one read of those, which sizes the item arrays and
 * fixes the keys and the number of passes; then one count / scan / scatter per digit of the key, the compact table of the
 * rows in front of the limit, its scan and cut, one read of the result words, the extract's gather over the compact table
 * and the index rows. */
extern "C" SRE_API int
sre_hip_sort_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, int group, int flags, size_t limit, void *d_out,
    size_t out_cap, sre_int_t *d_index, size_t index_cap, sre_hip_sort_info_t *info, void *hip_stream)
{
    LinesSink            sink;
    sre_extract_groups_t gr;
    if ((flags & ~(SRE_HIP_LINES_ALL | SRE_HIP_SORT_DESC)) != 0) return -1;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0;
    if (keyed_call(sc, "line sort", d_buf, len, delim, &group, 1, d_out, out_cap, d_index, index_cap, 0, 0, NULL, &sink, &gr, &n,
                   stream) != 0)
    {
        return -1;
    }
    sre_hip_sort_info_t res;
    memset(&res, 0, sizeof(res));
    res.vmin = INT64_MAX;
    res.vmax = INT64_MIN;
    if (n > SRE_LRK_MAX_LINES) {
        fprintf(stderr, "[sregex-hip] line sort: %llu lines, at most 2^32 - 1\n", (unsigned long long) n);
        return -1;
    }
    if (n != 0) {
        const int      all = (flags & SRE_HIP_LINES_ALL) != 0, desc = (flags & SRE_HIP_SORT_DESC) != 0;
        uint64_t       nrows = 0;
        static_assert(offsetof(sre_lines_info_t, snumbered) == offsetof(sre_lines_info_t, skeyed) + sizeof(uint64_t)
                          && offsetof(sre_lines_info_t, svmin) == offsetof(sre_lines_info_t, skeyed) + 2 * sizeof(uint64_t)
                          && offsetof(sre_lines_info_t, svmax) == offsetof(sre_lines_info_t, skeyed) + 3 * sizeof(uint64_t),
                      "skeyed, snumbered, svmin, svmax are the four totals of the values pass, in that order");
        if (compact_reserve(sc, n, (uint64_t) 1 << SRE_LSO_DIGIT_BITS) != 0) return -1;
        if (lines_grow(&sc->d_jkey, &sc->jkey_cap, n * sizeof(int64_t)) != 0) return -1;
        if (lines_grow(&sc->d_sclass, &sc->sclass_cap, n * sizeof(int8_t)) != 0) return -1;
        /* the value and the class of every line, and the totals: the one read that sizes everything behind it */
        SRE_HIP_TRY(sre_launch_sort_values(d_buf, sc->d_vval, sc->d_vstart, n, sc->d_jkey, sc->d_sclass, &sc->d_linfo->skeyed, stream));
        SRE_HIP_TRY(linfo_read(sc, stream, {LINFO(skeyed), LINFO(snumbered), LINFO(svmin), LINFO(svmax)}));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        const uint64_t nkeyed = sc->h_linfo->skeyed, nnum = sc->h_linfo->snumbered;
        const int64_t  vmin = (int64_t) sc->h_linfo->svmin, vmax = (int64_t) sc->h_linfo->svmax;
        if (nnum > nkeyed || nkeyed > n || (nnum != 0 && vmin > vmax)) return -1;        /* (cannot happen) */
        const uint64_t nsel = sre_lso_selected(n, nnum, all), nout = sre_lso_limited(nsel, limit);
        const uint32_t passes = sre_lso_passes(n, nnum, sre_lso_range(nnum, vmin, vmax), all);
        const uint32_t *lines = NULL;
        if (nsel != 0) {
            if (lines_grow(&sc->d_fstart, &sc->fstart_cap, nout * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_rval, &sc->rval_cap, (nout + 1) * sizeof(uint64_t)) != 0) return -1;
            const int cur = sort_passes(sc, n, nsel, vmin, vmax, nnum, desc, all, sort_digits, passes, NULL, -1, stream);
            if (cur < 0) return -1;
            /* the compact table of the rows in front of the limit; its scan leaves the words of d_linfo as the cut at out_cap
             * gives them */
            lines = sc->d_sline[cur];
            SRE_HIP_TRY(sre_launch_sort_table(lines, sc->d_ends, nout, n, sc->d_fstart, sc->d_rval, stream));
            SRE_HIP_TRY(sre_launch_filter_offsets(sc->d_rval, nout, sc->d_fblk, out_cap, sc->d_linfo, stream));
        }
        SRE_HIP_TRY(sre_launch_sort_finish(sc->d_rval, nout, out_cap, sc->d_rres, stream));
        if (compact_finish(sc, &sink, d_buf, n, SRE_LSO_RES_WORDS, nout, &res, &nrows, stream) != 0) return -1;
        res.nkeyed = (size_t) nkeyed;
        res.nnumbered = (size_t) nnum;
        res.passes = passes;
        res.vmin = vmin;
        res.vmax = vmax;
        if (nrows != 0) {
            SRE_HIP_TRY(sre_launch_sort_index(lines, sc->d_fstart, sc->d_rval, sc->d_rres, sc->d_jkey, sc->d_sclass, n, nrows, index_cap,
                                              reinterpret_cast<int64_t *>(d_index), stream));
        }
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return 0;
hip_failed:
    return -1;
}

/* the plan of the sort by text on the host (sre_lines_sort_text.h): pairs[2 i], pairs[2 i + 1] = chunk and digit of pass i for
 * i < min(cap, length); returns the length */
extern "C" SRE_API size_t
sre_hip_sort_text_plan(size_t minlen, size_t maxlen, int rest, uint64_t *pairs, size_t cap)
{
    const uint64_t              len = sre_lst_plan(minlen, maxlen, rest != 0, NULL, 0);
    const uint64_t              take = pairs == NULL ? 0 : len < cap ? len : cap;
    std::vector<sre_lst_pass_t> plan((size_t) take);
    (void) sre_lst_plan(minlen, maxlen, rest != 0, plan.data(), take);
    for (uint64_t i = 0; i < take; i++) {
        pairs[2 * i] = plan[(size_t) i].chunk;
        pairs[2 * i + 1] = plan[(size_t) i].digit;
    }
    return (size_t) len;
}

/* The passes of the sort by text, queued behind the read of the totals: chunk by chunk in the plan's order the keys of the
 * chunk (for the first chunk those of the n lines into d_jkey's words, whose lengths have been read; later those of the items
 * into the pair that holds them), then the chunk's digits through sort_passes.  An empty plan still has to make the items:
 * one pass over digit 0 of chunk 0, in which all keys are equal then.  Returns the pair that holds the sorted items */
static int
sort_text_passes(sre_hip_scanner_t *sc, const void *d_buf, uint64_t len, uint64_t n, uint64_t nsel, uint64_t max_bytes, int desc, int all,
                 const std::vector<sre_lst_pass_t> &plan, hipStream_t stream)
{
    static const sre_lst_pass_t only = {0, 0};
    const sre_lst_pass_t       *pl = plan.empty() ? &only : plan.data();
    const size_t                npl = plan.empty() ? 1 : plan.size();
    uint64_t                   *lkeys = reinterpret_cast<uint64_t *>(sc->d_jkey);
    int                         cur = -1;
    for (size_t at = 0; at < npl;) {
        uint32_t digits[SRE_LSO_MAX_PASSES], nd = 0;
        const uint64_t chunk = pl[at].chunk;
        while (at < npl && pl[at].chunk == chunk && nd < SRE_LSO_MAX_PASSES) digits[nd++] = pl[at++].digit;
        if (cur < 0) {
            SRE_HIP_TRY(sre_launch_sort_text_keys(d_buf, len, sc->d_vval, sc->d_vstart, n, max_bytes, NULL, n, chunk, desc, all, lkeys,
                                                  stream));
            cur = sort_passes(sc, n, nsel, 0, 0, 0, desc, all, digits, nd, lkeys, -1, stream);
        } else {
            SRE_HIP_TRY(sre_launch_sort_text_keys(d_buf, len, sc->d_vval, sc->d_vstart, n, max_bytes, sc->d_sline[cur], nsel, chunk, desc,
                                                  all, sc->d_kitem[cur], stream));
            cur = sort_passes(sc, nsel, nsel, 0, 0, 0, desc, all, digits, nd, NULL, cur, stream);
        }
        if (cur < 0) return -1;
    }
    return cur;
hip_failed:
    return -1;
}

/* The line sort by text: the numeric sort's call with another value and another key.  The values pass
 * leaves the compared length of every keyed line and the totals (keyed, keyed, minlen, maxlen); the one read of those sizes
 * the item arrays and fixes the plan; then per chunk the keys and the digit passes, and the numeric sort's table, scan and
 * cut, finish, read and gather; the index rows are the call's own. */
extern "C" SRE_API int
sre_hip_sort_lines_text(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, int group, size_t max_bytes, int flags,
    size_t limit, void *d_out, size_t out_cap, sre_int_t *d_index, size_t index_cap, sre_hip_sort_text_info_t *info, void *hip_stream)
{
    LinesSink            sink;
    sre_extract_groups_t gr;
    if ((flags & ~(SRE_HIP_LINES_ALL | SRE_HIP_SORT_DESC)) != 0) return -1;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t    n = 0;
    if (keyed_call(sc, "line sort by text", d_buf, len, delim, &group, 1, d_out, out_cap, d_index, index_cap, 0, 0, NULL, &sink, &gr, &n,
                   stream) != 0)
    {
        return -1;
    }
    sre_hip_sort_text_info_t res;
    memset(&res, 0, sizeof(res));
    res.minlen = SIZE_MAX;
    if (n > SRE_LRK_MAX_LINES) {
        fprintf(stderr, "[sregex-hip] line sort by text: %llu lines, at most 2^32 - 1\n", (unsigned long long) n);
        return -1;
    }
    if (n != 0) {
        const int all = (flags & SRE_HIP_LINES_ALL) != 0, desc = (flags & SRE_HIP_SORT_DESC) != 0;
        uint64_t  nrows = 0;
        if (compact_reserve(sc, n, (uint64_t) 1 << SRE_LSO_DIGIT_BITS) != 0) return -1;
        if (lines_grow(&sc->d_jkey, &sc->jkey_cap, n * sizeof(int64_t)) != 0) return -1;
        if (lines_grow(&sc->d_sclass, &sc->sclass_cap, n * sizeof(int8_t)) != 0) return -1;
        /* the compared length of every keyed line, and the totals: the one read that sizes everything behind it */
        SRE_HIP_TRY(sre_launch_sort_text_values(d_buf, len, sc->d_vval, sc->d_vstart, n, max_bytes, sc->d_jkey, sc->d_sclass,
                                                &sc->d_linfo->skeyed, stream));
        SRE_HIP_TRY(linfo_read(sc, stream, {LINFO(skeyed), LINFO(snumbered), LINFO(svmin), LINFO(svmax)}));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        const uint64_t nkeyed = sc->h_linfo->skeyed;
        const int64_t  vmin = (int64_t) sc->h_linfo->svmin, vmax = (int64_t) sc->h_linfo->svmax;
        if (sc->h_linfo->snumbered != nkeyed || nkeyed > n || (nkeyed != 0 && (vmin < 0 || vmin > vmax || (uint64_t) vmax > len))) {
            return -1;      /* (cannot happen) */
        }
        const uint64_t minlen = nkeyed ? (uint64_t) vmin : SIZE_MAX, maxlen = nkeyed ? (uint64_t) vmax : 0;
        const uint64_t nsel = sre_lst_selected(n, nkeyed, all), nout = sre_lso_limited(nsel, limit);
        const int      rest = all && nkeyed < n;
        std::vector<sre_lst_pass_t> plan((size_t) sre_lst_plan(minlen, maxlen, rest, NULL, 0));
        (void) sre_lst_plan(minlen, maxlen, rest, plan.data(), plan.size());
        const uint32_t *lines = NULL;
        if (nsel != 0) {
            if (lines_grow(&sc->d_fstart, &sc->fstart_cap, nout * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_rval, &sc->rval_cap, (nout + 1) * sizeof(uint64_t)) != 0) return -1;
            const int cur = sort_text_passes(sc, d_buf, len, n, nsel, max_bytes, desc, all, plan, stream);
            if (cur < 0) return -1;
            lines = sc->d_sline[cur];
            SRE_HIP_TRY(sre_launch_sort_table(lines, sc->d_ends, nout, n, sc->d_fstart, sc->d_rval, stream));
            SRE_HIP_TRY(sre_launch_filter_offsets(sc->d_rval, nout, sc->d_fblk, out_cap, sc->d_linfo, stream));
        }
        SRE_HIP_TRY(sre_launch_sort_finish(sc->d_rval, nout, out_cap, sc->d_rres, stream));
        if (compact_finish(sc, &sink, d_buf, n, SRE_LSO_RES_WORDS, nout, &res, &nrows, stream) != 0) return -1;
        res.nkeyed = (size_t) nkeyed;
        res.passes = plan.size();
        res.minlen = (size_t) minlen;
        res.maxlen = (size_t) maxlen;
        if (nrows != 0) {
            SRE_HIP_TRY(sre_launch_sort_text_index(d_buf, len, sc->d_vval, sc->d_vstart, n, lines, sc->d_fstart, sc->d_rval, sc->d_rres,
                                                   nrows, index_cap, reinterpret_cast<int64_t *>(d_index), stream));
        }
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return 0;
hip_failed:
    return -1;
}

/* The ordered tally: the tally's call up to its one read, with the cut left open (the rows come out in
 * another order); the ranks and the sums into the scanner's own arrays; the first line and the order value of every key and
 * the four totals, one read; the sort's digit passes over the keys; the ordered table of the rows in front of the limit, the
 * extract's scan and cut over it, one read of its four words; the extract's gather, then counts, aggregates, index rows and
 * ranks in output order. */
extern "C" SRE_API int
sre_hip_tally_top_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, const int *groups, size_t ngroups,
    const int *vgroups, size_t nvgroups, int fsep, int flags, size_t max_keys, int by, size_t by_col, size_t limit, void *d_out,
    size_t out_cap, uint64_t *d_counts, size_t counts_cap, sre_hip_tally_sum_t *d_sums, size_t sums_cap, sre_int_t *d_rank,
    size_t rank_cap, sre_int_t *d_index, size_t index_cap, sre_hip_tally_top_info_t *info, void *hip_stream)
{
    static_assert(SRE_HIP_TOP_COUNT == SRE_LTT_COUNT && SRE_HIP_TOP_SUM == SRE_LTT_SUM && SRE_HIP_TOP_MIN == SRE_LTT_MIN
                      && SRE_HIP_TOP_MAX == SRE_LTT_MAX && SRE_HIP_TOP_N == SRE_LTT_N,
                  "sre_lines_tally_top.h mirrors the public enum");
    TallyCall   t;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if ((sums_cap != 0 && d_sums == NULL) || (rank_cap != 0 && d_rank == NULL) || (reinterpret_cast<uintptr_t>(d_sums) & 7u) != 0
        || nvgroups > SRE_HIP_TALLY_MAX_VALUES || (vgroups == NULL) != (nvgroups == 0) || (nvgroups == 0 && sums_cap != 0)
        || !sre_ltt_by_ok(by, by_col, nvgroups)
        || tally_open(sc, "ordered tally", d_buf, len, delim, groups, ngroups, vgroups, nvgroups, fsep, flags,
                      SRE_HIP_LINES_ALL | SRE_HIP_SORT_DESC, max_keys, d_out, out_cap, d_counts, counts_cap, d_index, index_cap, &t,
                      stream) != 0)
    {
        return -1;
    }
    sre_hip_tally_top_info_t res;
    memset(&res, 0, sizeof(res));
    res.vmin = INT64_MAX;
    res.vmax = INT64_MIN;
    const uint32_t k = t.gr.k, v = (uint32_t) nvgroups;
    const uint64_t n = t.n;
    /* the counts and the scans' sums of the digit passes over the keys (at most n, at most max_keys) are reserved in front of
     * the scan of the entry table: its block sums in d_fblk, which the ranks read, stay where they are */
    if (n != 0 && compact_reserve(sc, n < max_keys ? n : max_keys, (uint64_t) 1 << SRE_LSO_DIGIT_BITS) != 0) return -1;
    /* the scan of the entry table without a cut: its rows are the source of the ordered table */
    const int rc = n != 0 ? tally_front(sc, &t, d_buf, max_keys, ~(size_t) 0, &res, stream) : 0;
    if (rc < 0) return -1;
    if (n != 0 && rc == 0) {
        const uint64_t nkeys = res.nkeys;
        if (nkeys > n) return -1;       /* (cannot happen) */
        const uint64_t nrows = sre_ltt_rows(nkeys, limit);
        res.nrows = (size_t) nrows;
        res.need_bytes = res.nwritten = res.out_bytes = 0;      /* (the front's are those of the scan without a cut) */
        if (nkeys != 0) {
            const bool with_sums = v != 0 && (by != SRE_LTT_COUNT || sums_cap != 0);
            if (lines_grow(&sc->d_pcount, &sc->pcount_cap, nkeys * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_pfirst, &sc->pfirst_cap, nkeys * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_pinv, &sc->pinv_cap, nkeys * sizeof(uint32_t)) != 0) return -1;
            if (lines_grow(&sc->d_jkey, &sc->jkey_cap, nkeys * sizeof(int64_t)) != 0) return -1;
            if (lines_grow(&sc->d_sclass, &sc->sclass_cap, nkeys * sizeof(int8_t)) != 0) return -1;
            if (lines_grow(&sc->d_pstart, &sc->pstart_cap, nrows * k * sizeof(uint64_t)) != 0) return -1;
            if (lines_grow(&sc->d_rval, &sc->rval_cap, (nrows * k + 1) * sizeof(uint64_t)) != 0) return -1;
            if (with_sums && lines_grow(&sc->d_psums, &sc->psums_cap, nkeys * v * sizeof(sre_ls_agg_t)) != 0) return -1;
            /* the tally's ranks and sums, into the scanner's arrays: d_pcount[key], d_psums[key], cnt[slot] = key */
            SRE_HIP_TRY(sre_launch_tally_ranks(sc->d_fval, sc->d_fstart, n, k, sc->d_fblk, sc->d_tslot, t.cnt, sc->d_pcount, nkeys, NULL,
                                               0, stream));
            if (with_sums) {
                const uint32_t copies = tally_sum_copies(nkeys, v);
                if (copies > 1 && lines_grow(&sc->d_vcopy, &sc->vcopy_cap, copies * nkeys * v * sizeof(sre_ls_agg_t)) != 0) return -1;
                SRE_HIP_TRY(sre_launch_tally_sums(d_buf, sc->d_vval, sc->d_vstart, n, v, sc->d_tslot, t.cnt, nkeys, sc->d_psums,
                                                  sc->d_vcopy, copies, stream));
            }
            const sre_ls_agg_t *psums = with_sums ? sc->d_psums : NULL;
            SRE_HIP_TRY(sre_launch_tally_top_first(t.tab, sc->d_tslot, t.cnt, n, nkeys, sc->d_pfirst, stream));
            /* the order value and the class of every key, and the totals: the one read that fixes the sort keys */
            SRE_HIP_TRY(sre_launch_tally_top_values(sc->d_pcount, psums, nkeys, v, by, (uint32_t) by_col, sc->d_jkey, sc->d_sclass,
                                                    &sc->d_linfo->skeyed, stream));
            SRE_HIP_TRY(linfo_read(sc, stream, {LINFO(skeyed), LINFO(snumbered), LINFO(svmin), LINFO(svmax)}));
            SRE_HIP_TRY(hipStreamSynchronize(stream));
            const uint64_t nordered = sc->h_linfo->snumbered;
            const int64_t  vmin = (int64_t) sc->h_linfo->svmin, vmax = (int64_t) sc->h_linfo->svmax;
            if (sc->h_linfo->skeyed != nkeys || nordered > nkeys || (nordered != 0 && vmin > vmax)) return -1;   /* (cannot happen) */
            if (!sre_ltt_range_ok(nordered, vmin, vmax)) {
                fprintf(stderr, "[sregex-hip] ordered tally: the order values span %lld .. %lld, more than 2^64 - 3\n",
                        (long long) vmin, (long long) vmax);
                return -1;
            }
            const uint32_t passes = sre_ltt_passes(nkeys, nordered, vmin, vmax);
            /* the sort's passes over the keys: every key is selected */
            const int cur = sort_passes(sc, nkeys, nkeys, vmin, vmax, nordered, (flags & SRE_HIP_SORT_DESC) != 0, 1, sort_digits, passes,
                                        NULL, -1, stream);
            if (cur < 0) return -1;
            const uint32_t *keys = sc->d_sline[cur];
            /* the ordered table of the rows in front of the limit (its source is the entry table: d_fval, d_fstart), the
             * extract's scan and cut over it, and the one read of the result words */
            SRE_HIP_TRY(sre_launch_tally_top_table(keys, sc->d_pfirst, sc->d_fval, sc->d_fstart, nrows, nkeys, n, k, sc->d_pstart,
                                                   sc->d_rval, stream));
            SRE_HIP_TRY(sre_launch_extract_offsets(sc->d_rval, nrows, k, sc->d_fblk, out_cap, sc->d_linfo, stream));
            SRE_HIP_TRY(linfo_read(sc, stream, {LINFO(fsel), LINFO(fneed), LINFO(fwritten), LINFO(fbytes)}));
            SRE_HIP_TRY(hipStreamSynchronize(stream));
            const uint64_t nwritten = sc->h_linfo->fwritten, out_bytes = sc->h_linfo->fbytes;
            if (sc->h_linfo->fsel != nrows || nwritten > nrows || out_bytes > out_cap) return -1;        /* (cannot happen) */
            res.nordered = (size_t) nordered;
            res.need_bytes = (size_t) sc->h_linfo->fneed;
            res.nwritten = (size_t) nwritten;
            res.out_bytes = (size_t) out_bytes;
            res.passes = passes;
            res.vmin = vmin;
            res.vmax = vmax;
            SRE_HIP_TRY(sre_launch_extract_gather(d_buf, d_out, sc->d_rval, sc->d_pstart, nrows * k, out_bytes, (uint32_t) delim,
                                                  (uint32_t) fsep, stream));
            /* counts, aggregates and index rows in output order, the inverse permutation, then the ranks of the lines */
            const uint64_t counts_rows = counts_cap < nrows ? counts_cap : nrows, sums_rows = sums_cap < nrows ? sums_cap : nrows;
            const uint64_t index_rows = index_cap < nwritten ? index_cap : nwritten;
            SRE_HIP_TRY(sre_launch_tally_top_permute(keys, nkeys, nrows, sc->d_pcount, psums, v, sc->d_pfirst, sc->d_ends, n, sc->d_pstart,
                                                     sc->d_rval, k, sc->d_jkey, sc->d_sclass, d_counts, counts_rows, d_sums, sums_rows,
                                                     reinterpret_cast<int64_t *>(d_index), index_rows, sc->d_pinv, stream));
        }
        SRE_HIP_TRY(sre_launch_tally_top_ranks(sc->d_tslot, t.cnt, sc->d_pinv, rank_cap < n ? rank_cap : n, nkeys,
                                               reinterpret_cast<int64_t *>(d_rank), stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (info) *info = res;
    return rc;
hip_failed:
    return -1;
}

extern "C" SRE_API int
sre_hip_scanner_last_line_batches(sre_hip_scanner_t *sc)
{
    return sc->line_batches;
}

extern "C" SRE_API int
sre_hip_scanner_last_lines_device(sre_hip_scanner_t *sc)
{
    return sc->lines_device ? 1 : 0;
}

extern "C" SRE_API size_t
sre_hip_scanner_last_short_lines(sre_hip_scanner_t *sc)
{
    return sc->short_lines;
}

/* One device-resident buffer through the scanner, for sre_vm_*_exec on large
 * whole-buffer calls.  `init_variant` is the SRE_DFA_INIT_* of a search on a
 * re-armed context; *poisoned reports the "threads still listed at eof" state
 * (sre_vm_pike.c:616-622). */
extern "C" int
sre_hip_scan_one(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int init_variant,
    sre_int_t *rec, int *poisoned, hipStream_t stream)
{
    const void *ptrs[1] = {d_buf};
    size_t      lens[1] = {len};
    sc->next_init_variant = (uint32_t) init_variant;
    if (sre_hip_scan_enqueue(sc, ptrs, lens, 1, stream) != 0) return -1;
    if (sre_hip_scan_results(sc, rec) != 0) return -1;
    if (poisoned) {
        *poisoned = sc->engine == SRE_HIP_ENGINE_SCAN ? sc->h_status[0].error
                  : sc->engine == SRE_HIP_ENGINE_NFA ? (sc->h_nstatus[0].clean_mode & SRE_NFA_WINDOW_POISONED) != 0 : 0;
    }
    return 0;
}

/*
 * One CHUNK of one stream through the table-driven scanner, for the chunked use of
 * sre_vm_pike_exec (sre_vm_api.cpp): scan + chain check (+ fix-up rounds), then
 * sre_k_stream_tail.  `continues`: the search is under way, `entry_state` is the
 * automaton state the previous chunk ended in and *d_ctx holds its threads' capture
 * vectors; otherwise a search starts at the chunk's first byte with `init_variant`.
 * `base`: absolute stream offset of the chunk.  The result lands in *h_res (pinned,
 * device-visible as d_res).  Synchronous.
 */
extern "C" int
sre_hip_scan_stream_chunk(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int init_variant,
    int continues, uint32_t entry_state, int eof, int64_t base, sre_stream_ctx_t *d_ctx,
    sre_stream_result_t *d_res, const sre_stream_result_t *h_res, uint32_t ovec_slots, hipStream_t stream,
    void (*midway)(void *), void *midway_arg)
{
    /* (midway: what the caller still has to do for the chunk to arrive — it runs after the
     * launches, and on every way out) */
    struct Midway {
        void (*fn)(void *);
        void  *arg;
        void   run() { if (fn) fn(arg); fn = nullptr; }
        ~Midway() { run(); }
    } mid{midway, midway_arg};
    if (sc->engine != SRE_HIP_ENGINE_SCAN || sc->mode == SRE_HIP_PIKE_COUNT) return -1;
    call_begin(sc);
    if (scanner_reserve(sc, 1) != 0) return -1;
    sc->h_ptrs[0] = d_buf;
    sc->h_lens[0] = len;
    if (scan_geometry(sc, 1, (uint32_t) init_variant, (continues ? SRE_GEOM_CONTINUES : 0u) | (eof ? 0u : SRE_GEOM_NO_EOF),
                      entry_state) != 0)
    {
        return -1;
    }
    /* two launches per chunk: the scan, and the chain check + tail in one workgroup; should
     * the speculative entry states of the chunk's lanes have been wrong (rare), the tail
     * says so and the rounds are run first */
    SRE_HIP_TRY(sre_launch_scan(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, NULL, NULL, stream));
    {
        /* (a large chunk has too many segments for one workgroup: the chain check's own kernels) */
        const int fused = sc->geom.nsegs <= SRE_VERIFY_ONE_SEGS;
        if (!fused) SRE_HIP_TRY(sre_launch_verify(sc->tab->h, sc->geom, sc->d_sum, sc->d_acc, sc->d_status, stream));
        SRE_HIP_TRY(sre_launch_stream_tail(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, sc->d_status,
                                           sc->d_scratch, d_ctx, d_res, base, eof, ovec_slots, fused, stream));
    }
    mid.run();
    /* the result lands in host-visible memory, rc last: watching that word costs less than
     * the runtime's wait (an interrupt and a wake-up) — for as long as a chunk of this size
     * can reasonably take, then the ordinary wait */
    {
        const volatile int64_t *prc = &h_res->rc;
        const auto              t0 = std::chrono::steady_clock::now();
        const auto              limit = std::chrono::microseconds(200 + (int64_t) (len >> 12));
        while (*prc == SRE_STREAM_PENDING) {
            if (std::chrono::steady_clock::now() - t0 > limit) {
                SRE_HIP_TRY(hipStreamSynchronize(stream));
                break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (h_res->rc == SRE_STREAM_UNSETTLED) {
        SRE_HIP_TRY(hipMemcpyAsync(sc->h_status, sc->d_status, sizeof(sre_stream_status_t),
                                   hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        if (scan_settle(sc, 1, stream, false, NULL) != 0) return -1;
        SRE_HIP_TRY(sre_launch_stream_tail(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, sc->d_status,
                                           sc->d_scratch, d_ctx, d_res, base, eof, ovec_slots, 0, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
    }
    sc->last_n = 0;
    return 0;
hip_failed:
    return -1;
}

/* can chunks of a stream go through this scanner?  (the carried state has room for 64
 * threads of 64 capture slots) */
extern "C" int
sre_hip_scanner_streams(sre_hip_scanner_t *sc)
{
    if (sc->engine != SRE_HIP_ENGINE_SCAN) return 0;
    if (sc->mode == SRE_HIP_THOMPSON) return 1;         /* the state alone */
    return sc->mode == SRE_HIP_PIKE_FIRST && sc->tab->h.max_threads <= SRE_STREAM_MAX_THREADS
           && sc->tab->h.nslots <= SRE_STREAM_MAX_SLOTS;
}

/* ---- stream sets (sre_hip_streams_*) ---- */

struct sre_hip_streams_s {
    sre_hip_scanner_t    *sc;           /* the set's own scanner: tables, per-call buffers, fix-up rounds */
    size_t                n;
    sre_streams_layout_t  L;
    int64_t              *d_rows;       /* n context rows */
    size_t                rows_bytes;
    uint8_t              *d_rekind;     /* [nstates][4], NULL: a chunk boundary leaves every state as it is */
    sre_streams_feed_t   *d_feed, *h_feed;      /* what a call hands in: three words a stream (h_: pinned) */
    uint32_t             *d_sentry;
    unsigned char        *d_out, *h_out;        /* [sre_streams_info_t][n records] */
    sre_stream_result_t  *d_tailres;    /* one per workgroup of the tail kernel */
    uint64_t             *d_idx;        /* sre_hip_streams_reset */
    size_t                idx_cap;
    int                   fixups, launches;
    /* the bit-parallel NFA tier (sre_hip_streams_create_engine): rows of 1 + W words, sre_streams_nfa.h */
    int                   engine;       /* SRE_HIP_ENGINE_SCAN or SRE_HIP_ENGINE_NFA */
    uint32_t              W;            /* 64-bit words of a thread set */
    sre_streams_nfa_init_t init0;       /* the set of a fresh stream */
    uint64_t             *d_eset;       /* [n][W] the sets the streams of a call enter with */
    uint8_t              *d_sflags;     /* [n] SRE_SFLAG_* */
    int                   exact_passes;
};

static sre_hip_streams_t *streams_create_on(sre_pool_t *pool, sre_hip_scanner_t *sc, int mode, size_t nstreams);

static void
streams_release(void *data)
{
    sre_hip_streams_t *ss = static_cast<sre_hip_streams_t *>(data);
    if (ss->d_rows) (void) hipFree(ss->d_rows);
    if (ss->d_rekind) (void) hipFree(ss->d_rekind);
    if (ss->d_feed) (void) hipFree(ss->d_feed);
    if (ss->h_feed) (void) hipHostFree(ss->h_feed);
    if (ss->d_sentry) (void) hipFree(ss->d_sentry);
    if (ss->d_out) (void) hipFree(ss->d_out);
    if (ss->h_out) (void) hipHostFree(ss->h_out);
    if (ss->d_tailres) (void) hipFree(ss->d_tailres);
    if (ss->d_idx) (void) hipFree(ss->d_idx);
    if (ss->d_eset) (void) hipFree(ss->d_eset);
    if (ss->d_sflags) (void) hipFree(ss->d_sflags);
    free(ss);
}

extern "C" SRE_API sre_hip_streams_t *
sre_hip_streams_create(sre_pool_t *pool, sre_program_t *prog, int mode, size_t nstreams)
{
    if (pool == NULL || prog == NULL || nstreams == 0 || nstreams > (size_t) 1 << 30) return NULL;
    if (mode != SRE_HIP_THOMPSON && mode != SRE_HIP_PIKE_FIRST) {
        fprintf(stderr, "[sregex-hip] stream set: mode must be SRE_HIP_THOMPSON or SRE_HIP_PIKE_FIRST\n");
        return NULL;
    }
    if (sre_hip_ready() != 0) return NULL;
    if (mode == SRE_HIP_THOMPSON && prog->lookahead_asserts) {
        /* (sre_vm_api.cpp thompson_stream_route: \A, ^ and \b are local to a call's buffer in that VM) */
        fprintf(stderr, "[sregex-hip] stream set: a Thompson program with look-ahead assertions has no chunked scanner\n");
        return NULL;
    }
    /* as the compat path's chunk route: look-ahead programs on the automaton with chunk-boundary twins */
    sre_hip_scanner_t *sc = scanner_create(pool, prog, mode, SRE_HIP_ENGINE_SCAN, prog->lookahead_asserts ? 1 : 0);
    if (sc == NULL) return NULL;
    return streams_create_on(pool, sc, mode, nstreams);
}

/* the set around its scanner (table-driven or NFA tier): rows, feed words, records */
static sre_hip_streams_t *
streams_create_on(sre_pool_t *pool, sre_hip_scanner_t *sc, int mode, size_t nstreams)
{
    if (sc->engine == SRE_HIP_ENGINE_SCAN && !sre_hip_scanner_streams(sc)) {
        fprintf(stderr, "[sregex-hip] stream set: more than %u listed threads or capture slots\n", SRE_STREAM_MAX_THREADS);
        return NULL;
    }
    sre_hip_streams_t *ss = static_cast<sre_hip_streams_t *>(calloc(1, sizeof(*ss)));
    if (ss == NULL) return NULL;
    ss->sc = sc;
    ss->n = nstreams;
    ss->engine = sc->engine;
    if (sc->engine == SRE_HIP_ENGINE_NFA) {
        /* the context is the thread set: one flag word and W set words (sre_streams_nfa.h) */
        ss->W = nfa_words(sc);
        for (uint32_t w = 0; w < ss->W; w++) {
            ss->init0.w[w] = sc->wide_kernel ? sc->wtab.init[0][w] : sc->use_sa ? sc->satab.init[0] : sc->ntab.init[0];
        }
        ss->L.row_words = 1 + ss->W;
    } else {
        ss->L.nslots = mode == SRE_HIP_THOMPSON ? 0 : sc->tab->h.nslots;
        ss->L.max_threads = mode == SRE_HIP_THOMPSON ? 0 : sc->tab->h.max_threads;
        ss->L.row_words = SRE_SROW_HDR + ss->L.nslots * (1 + 2 * ss->L.max_threads);
    }
    ss->L.ovec_slots = sc->ovec_slots;
    ss->L.rec_slots = SRE_SREC_HDR + sc->ovec_slots;
    ss->rows_bytes = nstreams * ss->L.row_words * sizeof(int64_t);
    {
        const size_t out_bytes = sizeof(sre_streams_info_t) + nstreams * ss->L.rec_slots * sizeof(int64_t);
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss->d_rows), ss->rows_bytes));
        SRE_HIP_TRY(hipMemset(ss->d_rows, 0, ss->rows_bytes));
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss->d_feed), nstreams * sizeof(sre_streams_feed_t)));
        SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ss->h_feed), nstreams * sizeof(sre_streams_feed_t), 0));
        if (ss->engine == SRE_HIP_ENGINE_NFA) {
            SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss->d_eset), nstreams * ss->W * sizeof(uint64_t)));
            SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss->d_sflags), nstreams));
        } else {
            SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss->d_sentry), nstreams * sizeof(uint32_t)));
        }
        SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss->d_out), out_bytes));
        SRE_HIP_TRY(hipMemset(ss->d_out, 0, out_bytes));
        SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ss->h_out), out_bytes, 0));
        if (ss->engine == SRE_HIP_ENGINE_SCAN) SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss->d_tailres), SRE_STREAMS_TAIL_GRID * sizeof(sre_stream_result_t)));
        if (sc->d_linfo == NULL) SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc->d_linfo), sizeof(sre_lines_info_t)));
        if (sc->h_linfo == NULL) SRE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sc->h_linfo), sizeof(sre_lines_info_t), 0));
        if (ss->engine == SRE_HIP_ENGINE_SCAN && !sc->dfa->rekind.empty()) {
            std::vector<uint8_t> rk(sc->dfa->rekind.size());
            for (size_t i = 0; i < rk.size(); i++) rk[i] = (uint8_t) sc->dfa->rekind[i];
            SRE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss->d_rekind), rk.size()));
            SRE_HIP_TRY(hipMemcpy(ss->d_rekind, rk.data(), rk.size(), hipMemcpyHostToDevice));
        }
    }
    if (sre_pool_add_cleanup(pool, streams_release, ss) != SRE_OK) goto hip_failed;
    return ss;
hip_failed:
    streams_release(ss);
    return NULL;
}

extern "C" SRE_API sre_hip_streams_t *
sre_hip_streams_create_engine(sre_pool_t *pool, sre_program_t *prog, int mode, int engine, size_t nstreams)
{
    if (engine == SRE_HIP_ENGINE_SCAN) return sre_hip_streams_create(pool, prog, mode, nstreams);
    if (pool == NULL || prog == NULL || nstreams == 0 || nstreams > (size_t) 1 << 30) return NULL;
    if (engine != SRE_HIP_ENGINE_AUTO && engine != SRE_HIP_ENGINE_NFA) {
        fprintf(stderr, "[sregex-hip] stream set: engine must be SRE_HIP_ENGINE_AUTO, _SCAN or _NFA\n");
        return NULL;
    }
    /* The NFA tier feeds Thompson streams of programs without look-ahead assertions: there the context
     * is the thread set.  A first match needs the clean position in front of the event for its exact
     * window, and that position may lie in a chunk that is gone. */
    const bool nfa_ok = mode == SRE_HIP_THOMPSON && !prog->lookahead_asserts;
    if (!nfa_ok) {
        if (engine == SRE_HIP_ENGINE_AUTO) return sre_hip_streams_create(pool, prog, mode, nstreams);
        fprintf(stderr, "[sregex-hip] stream set: the NFA tier feeds chunks in mode SRE_HIP_THOMPSON to programs without look-ahead assertions only\n");
        return NULL;
    }
    if (sre_hip_ready() != 0) return NULL;
    /* (AUTO: the table-driven scanner when it admits the program, else the NFA tier; no look-ahead, so no chunk twins) */
    sre_hip_scanner_t *sc = scanner_create(pool, prog, mode, engine, 0);
    if (sc == NULL) return NULL;
    if (sc->engine != SRE_HIP_ENGINE_SCAN && sc->engine != SRE_HIP_ENGINE_NFA) {
        fprintf(stderr, "[sregex-hip] stream set: neither the table-driven scanner nor the NFA tier admits the program\n");
        return NULL;
    }
    return streams_create_on(pool, sc, mode, nstreams);
}

extern "C" SRE_API int
sre_hip_streams_engine(sre_hip_streams_t *ss)
{
    return ss->engine;
}

extern "C" SRE_API int
sre_hip_streams_nfa_bits(sre_hip_streams_t *ss)
{
    return ss->engine == SRE_HIP_ENGINE_NFA ? sre_hip_scanner_nfa_bits(ss->sc) : 0;
}

extern "C" SRE_API int
sre_hip_streams_last_exact_passes(sre_hip_streams_t *ss)
{
    return ss->exact_passes;
}

extern "C" SRE_API size_t
sre_hip_streams_count(sre_hip_streams_t *ss)
{
    return ss->n;
}

extern "C" SRE_API size_t
sre_hip_streams_result_slots(sre_hip_streams_t *ss)
{
    return ss->L.rec_slots;
}

extern "C" SRE_API size_t
sre_hip_streams_device_bytes(sre_hip_streams_t *ss)
{
    return ss->rows_bytes;
}

extern "C" SRE_API int
sre_hip_streams_last_fixups(sre_hip_streams_t *ss)
{
    return ss->fixups;
}

extern "C" SRE_API int
sre_hip_streams_last_launches(sre_hip_streams_t *ss)
{
    return ss->launches;
}

extern "C" SRE_API int
sre_hip_streams_reset(sre_hip_streams_t *ss, const size_t *idx, size_t n)
{
    if (ss == NULL || (n != 0 && idx == NULL)) return -1;
    if (n == 0) return 0;
    for (size_t i = 0; i < n; i++) {
        if (idx[i] >= ss->n) return -1;
    }
    if (lines_grow(&ss->d_idx, &ss->idx_cap, n * sizeof(uint64_t)) != 0) return -1;
    {
        std::vector<uint64_t> h(idx, idx + n);
        SRE_HIP_TRY(hipMemcpy(ss->d_idx, h.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    SRE_HIP_TRY(sre_launch_streams_reset(ss->d_rows, ss->L.row_words, ss->d_idx, n, NULL));
    SRE_HIP_TRY(hipStreamSynchronize(NULL));
    return 0;
hip_failed:
    return -1;
}

/* workgroups of the table-driven set's tail kernel: one per active stream, at most SRE_STREAMS_TAIL_GRID */
static uint32_t
streams_tail_grid(uint64_t nactive)
{
    return (uint32_t) (nactive < SRE_STREAMS_TAIL_GRID ? nactive : SRE_STREAMS_TAIL_GRID);
}

/* The call on the NFA tier: prologue (geometry, entry sets, the records of streams that need no byte),
 * set pass + chain check, tail; fix-up rounds — the exact-entry fallback among them — run from device
 * counters: per round the host reads one word, never the streams' status blocks. */
static int
streams_feed_nfa(sre_hip_streams_t *ss, sre_int_t *results, hipStream_t stream)
{
    sre_hip_scanner_t  *sc = ss->sc;
    const size_t        n = ss->n;
    sre_streams_info_t *d_info = reinterpret_cast<sre_streams_info_t *>(ss->d_out);
    const volatile sre_streams_info_t *h_info = reinterpret_cast<sre_streams_info_t *>(ss->h_out);
    int64_t            *d_recs = reinterpret_cast<int64_t *>(ss->d_out + sizeof(sre_streams_info_t));
    const size_t        out_bytes = sizeof(sre_streams_info_t) + n * ss->L.rec_slots * sizeof(int64_t);
    {
        const uint64_t seg_fixed = nfa_seg_knobs(sc);
        const uint64_t resident = scan_resident(sc);
        SRE_HIP_TRY(sre_launch_upload_words(reinterpret_cast<const uint64_t *>(ss->h_feed),
                                            reinterpret_cast<uint64_t *>(ss->d_feed), (uint32_t) (3 * n), stream));
        SRE_HIP_TRY(sre_launch_streams_nfa_prologue(ss->d_feed, (uint32_t) n, ss->d_rows, ss->W, ss->init0, ss->L.rec_slots, seg_fixed,
                                                    resident, scan_seg_cap(sc),
                                                    reinterpret_cast<const uint8_t **>(sc->d_ptrs), sc->d_lens, sc->d_seg_first,
                                                    ss->d_sflags, ss->d_eset, d_recs, d_info, stream));
        /* the host sizes the call's buffers and grids from two of its words */
        SRE_HIP_TRY(hipMemcpyAsync(ss->h_out, ss->d_out, sizeof(sre_streams_info_t), hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        ss->launches += 3;
    }
    if (h_info->nsegs != 0) {
        if (nfa_buffers(sc, h_info->nsegs) != 0) return -1;
        geom_device(sc, n, h_info->seg, h_info->nsegs);
        /* per stream: whether more chunks follow, and the set it enters with */
        sc->geom.sflags = ss->d_sflags;
        sc->d_eset = ss->d_eset;
        SRE_HIP_TRY(nfa_launch_scan(sc, NULL, NULL, NULL, stream));
        if (nfa_finish(sc, NULL, NULL, stream) != 0) return -1;
        SRE_HIP_TRY(sre_launch_streams_nfa_tail(ss->d_feed, (uint32_t) n, ss->d_rows, ss->W, sc->d_seg_first, sc->d_nstatus, sc->d_nsum,
                                                sc->wide_kernel ? sc->d_wsets : NULL, ss->L.rec_slots, d_recs, d_info, 0, stream));
        ss->launches += 1 + 3 + 1;
    }
    SRE_HIP_TRY(hipMemcpyAsync(ss->h_out, ss->d_out, out_bytes, hipMemcpyDeviceToHost, stream));
    SRE_HIP_TRY(hipStreamSynchronize(stream));
    ss->launches += 1;
    if (h_info->unsettled != 0) {
        /* speculative entry sets of some stream's lanes were wrong: fix-up rounds over the streams that
         * are not verified */
        if (nfa_settle_device(sc, n, stream) != 0) return -1;
        SRE_HIP_TRY(hipMemsetAsync(&d_info->unsettled, 0, sizeof(uint64_t), stream));
        SRE_HIP_TRY(sre_launch_streams_nfa_tail(ss->d_feed, (uint32_t) n, ss->d_rows, ss->W, sc->d_seg_first, sc->d_nstatus, sc->d_nsum,
                                                sc->wide_kernel ? sc->d_wsets : NULL, ss->L.rec_slots, d_recs, d_info, 1, stream));
        SRE_HIP_TRY(hipMemcpyAsync(ss->h_out, ss->d_out, out_bytes, hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        ss->fixups = sc->fixup_rounds;
        ss->exact_passes = sc->exact_passes;
        ss->launches += 3;
        if (h_info->unsettled != 0) {
            fprintf(stderr, "[sregex-hip] stream set: %llu streams did not settle\n", (unsigned long long) h_info->unsettled);
            return -1;
        }
    }
    memcpy(results, ss->h_out + sizeof(sre_streams_info_t), n * ss->L.rec_slots * sizeof(int64_t));
    return 0;
hip_failed:
    return -1;
}

/* One exec() per fed stream.  The host fills three words a stream; everything else of the call —
 * which streams take part, the geometry, the entry states, the tails, the records — happens on
 * the device in a number of launches and copies that does not depend on the size of the set. */
extern "C" SRE_API int
sre_hip_streams_feed(sre_hip_streams_t *ss, const void *const *d_chunks, const size_t *lens,
    const unsigned char *eof, sre_int_t *results, void *hip_stream)
{
    if (ss == NULL || d_chunks == NULL || lens == NULL || eof == NULL || results == NULL) return -1;
    hipStream_t         stream = static_cast<hipStream_t>(hip_stream);
    sre_hip_scanner_t  *sc = ss->sc;
    const size_t        n = ss->n;
    sre_streams_info_t *d_info = reinterpret_cast<sre_streams_info_t *>(ss->d_out);
    const volatile sre_streams_info_t *h_info = reinterpret_cast<sre_streams_info_t *>(ss->h_out);
    int64_t            *d_recs = reinterpret_cast<int64_t *>(ss->d_out + sizeof(sre_streams_info_t));
    const size_t        out_bytes = sizeof(sre_streams_info_t) + n * ss->L.rec_slots * sizeof(int64_t);
    ss->fixups = 0;
    ss->launches = 0;
    ss->exact_passes = 0;
    call_begin(sc);
    sc->last_n = 0;
    for (size_t i = 0; i < n; i++) {
        ss->h_feed[i].ptr = (uint64_t) reinterpret_cast<uintptr_t>(d_chunks[i]);
        ss->h_feed[i].len = d_chunks[i] ? lens[i] : 0;
        ss->h_feed[i].flags = d_chunks[i] ? (SRE_SFEED_FED | (eof[i] ? SRE_SFEED_EOF : 0u)) : 0u;
    }
    if (scanner_reserve(sc, n) != 0) return -1;
    if (ss->engine == SRE_HIP_ENGINE_NFA) return streams_feed_nfa(ss, results, stream);
    {
        const uint64_t seg_fixed = scan_seg_knobs(sc);
        const uint64_t resident = scan_resident(sc);
        SRE_HIP_TRY(sre_launch_upload_words(reinterpret_cast<const uint64_t *>(ss->h_feed),
                                            reinterpret_cast<uint64_t *>(ss->d_feed), (uint32_t) (3 * n), stream));
        SRE_HIP_TRY(sre_launch_streams_prologue(ss->d_feed, (uint32_t) n, ss->d_rows, ss->L, ss->d_rekind, sc->tab->h.init[0],
                                                seg_fixed, resident, scan_seg_cap(sc),
                                                reinterpret_cast<const uint8_t **>(sc->d_ptrs), sc->d_lens, sc->d_seg_first,
                                                ss->d_sentry, d_recs, d_info, stream));
        /* the host sizes the call's buffers and grids from two of its words */
        SRE_HIP_TRY(hipMemcpyAsync(ss->h_out, ss->d_out, sizeof(sre_streams_info_t), hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        ss->launches += 3;
    }
    if (h_info->nsegs != 0) {
        const uint64_t seg = h_info->seg, nsegs = h_info->nsegs;
        const uint32_t grid = streams_tail_grid(h_info->nactive);
        /* (the walker's scratch: one block per workgroup of the tail kernel, not per stream) */
        if (scan_buffers(sc, grid, seg, nsegs) != 0) return -1;
        /* (behind scan_buffers: the set's chain check takes no digest) */
        geom_device(sc, n, seg, nsegs);
        sc->geom.sentry = ss->d_sentry;
        SRE_HIP_TRY(sre_launch_scan(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, NULL, NULL, stream));
        SRE_HIP_TRY(sre_launch_verify(sc->tab->h, sc->geom, sc->d_sum, sc->d_acc, sc->d_status, stream));
        SRE_HIP_TRY(sre_launch_streams_tail(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, sc->d_status, sc->d_scratch,
                                            ss->d_rows, ss->L, ss->d_tailres, d_recs, d_info, grid, 0, stream));
        ss->launches += 1 + (sc->mode == SRE_HIP_PIKE_FIRST && sc->tab->h.nshadow ? 4 : 3) + 1;
    }
    SRE_HIP_TRY(hipMemcpyAsync(ss->h_out, ss->d_out, out_bytes, hipMemcpyDeviceToHost, stream));
    SRE_HIP_TRY(hipStreamSynchronize(stream));
    ss->launches += 1;
    if (h_info->unsettled != 0) {
        /* speculative entry states of some stream's lanes were wrong: the fix-up rounds over the
         * streams that are not done, driven from device counters, then their tails */
        const uint32_t grid = streams_tail_grid(h_info->nactive);
        sc->h_linfo->pending = h_info->unsettled;
        sc->h_linfo->maps = 0;
        if (scan_settle(sc, n, stream, false, NULL, true) != 0) return -1;
        SRE_HIP_TRY(hipMemsetAsync(&d_info->unsettled, 0, sizeof(uint64_t), stream));
        SRE_HIP_TRY(sre_launch_streams_tail(sc->tab->d_tab, sc->tab->h, sc->geom, sc->d_sum, sc->d_status, sc->d_scratch,
                                            ss->d_rows, ss->L, ss->d_tailres, d_recs, d_info, grid, 1, stream));
        SRE_HIP_TRY(hipMemcpyAsync(ss->h_out, ss->d_out, out_bytes, hipMemcpyDeviceToHost, stream));
        SRE_HIP_TRY(hipStreamSynchronize(stream));
        ss->fixups = sc->fixup_rounds;
        ss->exact_passes = sc->exact_passes;
        ss->launches += 3;
        if (h_info->unsettled != 0) {
            fprintf(stderr, "[sregex-hip] stream set: %llu streams did not settle\n", (unsigned long long) h_info->unsettled);
            return -1;
        }
    }
    memcpy(results, ss->h_out + sizeof(sre_streams_info_t), n * ss->L.rec_slots * sizeof(int64_t));
    return 0;
hip_failed:
    return -1;
}

/* ------------------------------------------------------------------ helpers */

extern "C" SRE_API void *
sre_hip_alloc(size_t bytes)
{
    void *p = NULL;
    if (sre_hip_ready() != 0) return NULL;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) {
        sre_hip_fail("hipMalloc", e);
        return NULL;
    }
    return p;
}

extern "C" SRE_API void
sre_hip_free(void *d_ptr)
{
    if (d_ptr) (void) hipFree(d_ptr);
}

extern "C" SRE_API int
sre_hip_upload(void *d_dst, const void *h_src, size_t bytes)
{
    hipError_t e = hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : sre_hip_fail("hipMemcpy H2D", e);
}

extern "C" SRE_API int
sre_hip_download(void *h_dst, const void *d_src, size_t bytes)
{
    hipError_t e = hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : sre_hip_fail("hipMemcpy D2H", e);
}

extern "C" SRE_API int
sre_hip_synchronize(void *hip_stream)
{
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(hip_stream));
    return e == hipSuccess ? 0 : sre_hip_fail("hipStreamSynchronize", e);
}

extern "C" SRE_API int
sre_hip_gen_data(void *d_dst, size_t n, const void *h_tail, size_t tail_len, void *hip_stream)
{
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    void       *d_tail = NULL;
    int         rc = -1;
    if (sre_hip_ready() != 0 || tail_len > n) return -1;
    SRE_HIP_TRY(hipMalloc(&d_tail, tail_len ? tail_len : 1));
    if (tail_len) {
        SRE_HIP_TRY(hipMemcpyAsync(d_tail, h_tail, tail_len, hipMemcpyHostToDevice, stream));
    }
    SRE_HIP_TRY(sre_launch_gen_data(d_dst, n, tail_len, d_tail, stream));
    SRE_HIP_TRY(hipStreamSynchronize(stream));
    rc = 0;
hip_failed:
    if (d_tail) (void) hipFree(d_tail);
    return rc;
}

static uint32_t *
ceiling_sink(void)
{
    static uint32_t *d_sink = NULL;
    if (d_sink == NULL
        && hipMalloc(reinterpret_cast<void **>(&d_sink), SRE_CEILING_GRID * sizeof(uint32_t)) != hipSuccess)
    {
        d_sink = NULL;
    }
    return d_sink;
}

extern "C" SRE_API int
sre_hip_read_pattern(const void *d_src, size_t n, unsigned seg_bytes, unsigned tile,
                     unsigned lds_bytes, void *hip_stream)
{
    if (sre_hip_ready() != 0) return -1;
    uint32_t *d_sink = ceiling_sink();
    if (d_sink == NULL) return -1;
    SRE_HIP_TRY(sre_launch_read_pattern(d_src, n, seg_bytes, tile, lds_bytes, d_sink,
                                        static_cast<hipStream_t>(hip_stream)));
    return 0;
hip_failed:
    return -1;
}

extern "C" SRE_API int
sre_hip_read_ceiling(const void *d_src, size_t n, void *hip_stream)
{
    if (sre_hip_ready() != 0) return -1;
    uint32_t *d_sink = ceiling_sink();
    if (d_sink == NULL) return -1;
    SRE_HIP_TRY(sre_launch_read_ceiling(d_src, n, d_sink, static_cast<hipStream_t>(hip_stream)));
    return 0;
hip_failed:
    return -1;
}
