/*
 * sregex_hip.h — ADDITIVE device-resident, batched entry points (C ABI).
 *
 * The reference's executors take host pointers
 * (sre_vm_pike_exec / sre_vm_thompson_exec, reference src/sregex/sregex.h:133-134,
 * 147-148), so through them a GPU matcher is PCIe-bound.  These entry points
 * are what a maintainer binds when the streams already live in HBM: many
 * independent streams (one context each, reference README.markdown:376) are
 * scanned in one call with the same compiled sre_program_t.  They replace, per
 * stream, the call sequence
 *     ctx = sre_vm_pike_create_ctx(pool, prog, ovector, ovecsize);   sre_vm_pike.c:94-145
 *     rc  = sre_vm_pike_exec(ctx, stream, len, 1, NULL);             sre_vm_pike.c:148-689
 * (resp. the Thompson pair, sre_vm_thompson.c:25-60 / :63-270), and for
 * SRE_HIP_PIKE_COUNT the find-all iteration a caller writes around it
 * (re-feeding from ovector[1]; sre_vm_pike.c:179-196, 624-628).
 *
 * Plain pointers and sizes only; no torch / C++ types.  See INTEGRATION.md for
 * the C, ctypes and cgo-style bindings.
 */
#ifndef SREGEX_AMD_SREGEX_HIP_H
#define SREGEX_AMD_SREGEX_HIP_H

#include <sregex/sregex.h>

#ifdef __cplusplus
extern "C" {
#endif

/* what to compute per stream */
enum {
    SRE_HIP_THOMPSON   = 0,  /* match / no match                 (sre_vm_thompson_exec) */
    SRE_HIP_PIKE_FIRST = 1,  /* first match: regex id + captures (sre_vm_pike_exec)     */
    SRE_HIP_PIKE_COUNT = 2   /* iterate sre_vm_pike_exec from each match end: count     */
};

/* which device engine runs it */
enum {
    SRE_HIP_ENGINE_AUTO = 0, /* table-driven scanner when the program admits one  */
    SRE_HIP_ENGINE_VM   = 1, /* exact bytecode VM kernel, one lane per stream     */
    SRE_HIP_ENGINE_SCAN = 2, /* table-driven segment-parallel scanner, or fail    */
    SRE_HIP_ENGINE_NFA  = 3  /* bit-parallel NFA scanner (<= 256 list-able threads as 1, 2
                                or 4 64-bit words per lane), or fail: the tier for programs
                                whose ordered-list automaton is too large */
};

typedef struct sre_hip_scanner_s  sre_hip_scanner_t;

/* number of HIP devices visible to this process (0 if none) */
SRE_API int sre_hip_device_count(void);

/* select the device used by subsequently created programs/scanners */
SRE_API int sre_hip_set_device(int ordinal);

/*
 * Create a scanner for `prog`.  Owned by `pool` (freed by sre_destroy_pool).
 * Returns NULL (with a diagnostic on stderr) when no HIP device is usable or
 * when `engine` == SRE_HIP_ENGINE_SCAN and the program admits no table.
 */
SRE_API sre_hip_scanner_t *sre_hip_scanner_create(sre_pool_t *pool,
    sre_program_t *prog, int mode, int engine);

/* engine actually chosen: SRE_HIP_ENGINE_VM, SRE_HIP_ENGINE_SCAN or SRE_HIP_ENGINE_NFA */
SRE_API int sre_hip_scanner_engine(sre_hip_scanner_t *sc);

/*
 * Tuning / testing knob of the table-driven scanner: bytes per segment (one
 * lane walks one segment).  0 restores the automatic choice (about 256K lanes
 * per call, at least 4 KiB per segment); otherwise a multiple of 64.
 */
SRE_API int sre_hip_scanner_set_segment_bytes(sre_hip_scanner_t *sc, size_t bytes);

/* diagnostics: fix-up rounds the last scan needed (0 = every assumed segment
 * entry state was right) */
SRE_API int sre_hip_scanner_last_fixups(sre_hip_scanner_t *sc);

/* diagnostics: 1 when the last scan's speculative fix-up rounds did not settle and the
 * exact entry state of every remaining segment was computed by composing the
 * segments' transition functions (FIRST / Thompson; an automaton that never forgets) */
SRE_API int sre_hip_scanner_last_exact_passes(sre_hip_scanner_t *sc);

/* diagnostics: how many sre_vm_pike_exec / sre_vm_thompson_exec calls of this process went
 * where — out[0] one whole buffer through a throughput scanner, out[1] a chunk of a chunked
 * stream through the table-driven scanner, out[2] the exact VM kernel */
SRE_API void sre_hip_compat_route_counts(unsigned long long out[3]);

/* The compat entry points (sregex.h) keep released device streams — a HIP stream, a VM context, staging
 * buffers of at most 8 MiB each — in a process-wide free list of at most 32 for the next context.  This
 * call frees them all and returns how many there were.
 * THREADS: as in the reference, distinct programs and pools may be used from different threads (the
 * library's process-wide state is locked); the contexts of ONE program must not run concurrently (they
 * share the program's device scanners — the reference's programs carry the VM's generation tags,
 * src/sregex/sre_vm_bytecode.h:51, and are not re-entrant either).  A scanner of the batched API below
 * belongs to one thread at a time. */
SRE_API int sre_hip_compat_trim(void);

/* diagnostics: find-all counting on the NFA tier (a program the step automaton declines) is a loop of
 * first-match searches, run in rounds over all streams of the call: how many rounds the last call took */
SRE_API int sre_hip_scanner_last_count_rounds(sre_hip_scanner_t *sc);

/* diagnostics: 1 when the last scan had to build per-segment ancestor maps to
 * reconstruct the captures of a match spanning many segments */
SRE_API int sre_hip_scanner_last_lineage_passes(sre_hip_scanner_t *sc);

/* class bits per input byte of the scanner's fast table (1, 2, 4 or 8: one table
 * lookup advances 8 / bits bytes); 0 for the VM engine.  Names the kernel
 * variant (sre_k_scan<mode, bits>) in profiles. */
SRE_API int sre_hip_scanner_class_bits(sre_hip_scanner_t *sc);

/* bits of the thread set a lane of the NFA tier holds: 64, 128 or 256 (counted after equivalent
 * threads are merged); 0 unless the scanner runs on the NFA tier */
SRE_API int sre_hip_scanner_nfa_bits(sre_hip_scanner_t *sc);

/* name of the dominant kernel of a scan with this scanner, as rocprofv3 prints it
 * (e.g. "sre_k_scan<1, 2>"); owned by the scanner */
SRE_API const char *sre_hip_scanner_kernel_name(sre_hip_scanner_t *sc);

/* measurement: duration (ms) of the segment-scan kernel of the last enqueued
 * scan, from hipEvents recorded on the caller's stream around that launch;
 * -1 when the exact VM engine ran.  Waits for the kernel. */
SRE_API double sre_hip_scanner_last_kernel_ms(sre_hip_scanner_t *sc);

/* Two scanners taking turns on ONE stream: with a tail stream set, everything a call queues
 * behind its scan kernel (chain check, capture walk, the copy of the records) goes to that
 * stream, ordered after the scan by an event; the next call's scan kernel then follows
 * on the scan stream without a gap.  NULL: everything on the stream of the call. */
SRE_API int sre_hip_scanner_set_tail_stream(sre_hip_scanner_t *sc, void *hip_stream);

/*
 * Make `hip_stream` wait until the dominant (segment-scan) kernel of sc's last enqueued
 * scan has finished — not for the small kernels and copies behind it.  A driver that
 * alternates two scanners on two streams calls this on the OTHER scanner before each
 * enqueue: the big kernels then run one after the other (neither is slowed down by
 * sharing the GPU), while the chain check, the capture walk and the copy of the
 * records of one step overlap with the scan of the next.  No-op before the first scan.
 */
SRE_API int sre_hip_scanner_order_after_scan(sre_hip_scanner_t *sc, void *hip_stream);

/* segment size the last scan used (0 for the VM engine) */
SRE_API size_t sre_hip_scanner_last_segment_bytes(sre_hip_scanner_t *sc);

/*
 * Per-stream result record, in sre_int_t units:
 *     [0] rc     regex id (>= 0; SRE_OK for Thompson) of the (last) match, or
 *                SRE_DECLINED when there is none; SRE_ERROR when the iteration
 *                of COUNT mode ended with SRE_ERROR (sre_vm_pike.c:165-168 after
 *                :616-622) — [1] and the ovector are still those of the matches
 *                found before
 *     [1] count  matches found (COUNT mode; 0/1 otherwise)
 *     [2..]      ovector of the (last) match, 2 * (max_ncaps + 1) slots,
 *                absolute byte offsets, -1 = unset   (sre_vm_pike.c:945-989)
 * sre_hip_scanner_result_slots() = 2 + 2 * (max_ncaps + 1).
 */
SRE_API size_t sre_hip_scanner_result_slots(sre_hip_scanner_t *sc);

/*
 * Enqueue the scan of `nstreams` device-resident streams on `hip_stream`
 * (a hipStream_t, NULL = default stream).  `d_streams[i]` is a DEVICE pointer
 * to `lens[i]` bytes; both arrays are HOST arrays.  Asynchronous: returns
 * after the kernels are queued.  0 on success, -1 on failure.
 *
 * The copy of the result records to pinned host memory is part of the queued
 * work and sre_hip_scan_results() waits for an event behind it, not for the
 * whole stream: a caller that alternates two scanners (enqueue on one, then
 * collect from the other) keeps the GPU busy without a gap between scans.
 * One call per scanner may be in flight; the streams must stay unchanged until
 * sre_hip_scan_results() has returned.
 */
SRE_API int sre_hip_scan_enqueue(sre_hip_scanner_t *sc,
    const void *const *d_streams, const size_t *lens, size_t nstreams,
    void *hip_stream);

/*
 * Wait for the last enqueued scan and copy its records to `results`
 * (host, nstreams * result_slots entries).  0 on success.
 */
SRE_API int sre_hip_scan_results(sre_hip_scanner_t *sc, sre_int_t *results);

/* convenience: enqueue + results */
SRE_API int sre_hip_scan_batch(sre_hip_scanner_t *sc,
    const void *const *d_streams, const size_t *lens, size_t nstreams,
    sre_int_t *results, void *hip_stream);

/* ---- line mode: one device buffer of delimited records, each record its own stream ---- */

enum { SRE_HIP_LINES_ALL = 1 };   /* report every line, not only the lines with a match */

/*
 * Line mode.  d_buf is a DEVICE pointer to len bytes of records separated by the byte
 * `delim` (0..255), at any alignment.  Each line is matched as an independent stream with
 * a fresh context, exactly as sre_hip_scan_batch matches it.  Synchronous: returns when the
 * rows are in `out`.  Everything runs on hip_stream.
 *
 * How the buffer is split (the rules of grep and wc -l):
 *   - a line is a maximal run of bytes between delimiters; the delimiter belongs to no line;
 *   - a buffer that ends with the delimiter has no empty line after it; one that does not
 *     end with it has a final line without a delimiter;
 *   - len == 0 gives 0 lines, "\n" one empty line, "a\n\nb" the lines "a", "" and "b";
 *   - an empty line is a stream of length 0 and takes its EOF step, as an empty stream of
 *     the batched API does;
 *   - '\r' is an ordinary byte.
 *
 * *nlines    = number of lines in the buffer.
 * *nreported = number of reported lines: every line with SRE_HIP_LINES_ALL, otherwise the
 *              lines whose rc is not SRE_DECLINED (COUNT mode's SRE_ERROR lines are reported).
 * The first min(cap, *nreported) reported lines are written to `out` in line order,
 * 3 + sre_hip_scanner_result_slots(sc) sre_int_t each:
 *   [0] line number (0-based)   [1] offset of the line's first byte in the buffer
 *   [2] line length
 *   [3..] exactly the record sre_hip_scan_batch returns for (d_buf + [1], [2]) as one
 *         stream: rc, count, ovector (offsets relative to the line's first byte).
 * out may be NULL when cap == 0 (counts only).  nlines / nreported may be NULL.
 * Returns 0 on success, -1 on bad arguments or failure.
 *
 * The table-driven scanner does the whole call on the device (split, per-line geometry,
 * fix-up rounds, compaction of the rows), and so do Thompson and first-match scanners of the
 * bit-parallel NFA tier: there short lines (at most SRE_HIP_LINES_SHORT_MAX bytes, environment,
 * read on every call, default 512; 0 turns it off; 64-bit forms only) go one to a lane through
 * a kernel of their own and the longer ones through the tier's set pass.  Find-all counting on
 * the tier and the exact VM take each batch of lines through sre_hip_scan_enqueue /
 * sre_hip_scan_results on the host, and SRE_HIP_LINES_NFA_HOST=1 (environment, read on every
 * call) keeps every scanner of the tier on that route.  Line mode ignores
 * sre_hip_scanner_set_tail_stream.  A call of either kind replaces the scanner's last
 * call: after a line-mode call sre_hip_scan_results returns -1, and the diagnostics
 * (last_fixups, last_exact_passes, last_lineage_passes: sums over the call's batches;
 * last_kernel_ms: the summed scan kernels of all batches, or -1) describe the whole call.
 * SRE_HIP_LINES_BATCH (environment, read on every call) caps the lines per internal batch.
 */
SRE_API int sre_hip_scan_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    int flags, sre_int_t *out, size_t cap, size_t *nlines, size_t *nreported, void *hip_stream);

/* diagnostics: internal batches of lines the last sre_hip_scan_lines call ran (0 before the
 * first call) */
SRE_API int sre_hip_scanner_last_line_batches(sre_hip_scanner_t *sc);
/* 1 when every batch of the last sre_hip_scan_lines call ran on the device with no per-line
 * host work (the table-driven scanner; Thompson and first-match scanners of the NFA tier),
 * else 0; 0 before the first call */
SRE_API int sre_hip_scanner_last_lines_device(sre_hip_scanner_t *sc);
/* lines of the last sre_hip_scan_lines call that the NFA tier's short-line kernel took */
SRE_API size_t sre_hip_scanner_last_short_lines(sre_hip_scanner_t *sc);

/* ---- line filter: the selected lines themselves, compacted into a device buffer ---- */

enum { SRE_HIP_LINES_INVERT = 2 };   /* select the lines WITHOUT a match (grep -v) */

typedef struct {
    size_t nlines;      /* lines in the buffer (as sre_hip_scan_lines) */
    size_t nselected;   /* lines selected */
    size_t need_bytes;  /* bytes all selected lines take in the output: sum of (len + 1) */
    size_t nwritten;    /* selected lines actually written (whole lines only) */
    size_t out_bytes;   /* bytes written to d_out */
} sre_hip_filter_info_t;

/*
 * Line filter: grep and grep -v from one device buffer to another.  The split of d_buf, the
 * matching of every line and the engine a scanner routes to are exactly those of
 * sre_hip_scan_lines on the same arguments; what comes back is the text of the selected
 * lines in device memory, not rows on the host.
 *
 * Which lines are selected:
 *   - flags == 0: the lines sre_hip_scan_lines reports without SRE_HIP_LINES_ALL, that is the
 *     lines whose rc is not SRE_DECLINED (COUNT mode's SRE_ERROR lines are selected);
 *   - SRE_HIP_LINES_INVERT: the lines whose rc is SRE_DECLINED instead;
 *   - SRE_HIP_LINES_ALL: every line;
 *   - ALL | INVERT, and any other flag bit, return -1.
 *
 * Output.  d_out is a DEVICE pointer at any alignment to out_cap bytes that do not overlap
 * [d_buf, d_buf + len) (an overlap returns -1).  It receives the selected lines in line order,
 * each as its bytes followed by ONE `delim` byte; a final line that had no delimiter in the
 * source gets one too.  The output is therefore a well-formed line buffer itself: without
 * INVERT, filtering it again with the same scanner and flags selects all its lines and
 * reproduces it byte for byte.  info->need_bytes is the sum of len + 1 over the selected lines
 * whatever out_cap is.
 *
 * Truncation.  Only whole lines are written: info->nwritten is the largest k for which the
 * first k selected lines take at most out_cap bytes, info->out_bytes that total.  No byte of
 * d_out at or beyond out_bytes is touched and nothing is written in front of d_out.  d_out may
 * be NULL when out_cap == 0 (a sizing call).
 *
 * Index.  d_index is an optional DEVICE array: for each of the first min(index_cap, nwritten)
 * written lines it receives 4 sre_int_t,
 *   [0] line number   [1] offset of the line in d_buf   [2] line length
 *   [3] offset of the line in d_out.
 * d_index may be NULL when index_cap == 0.  info may be NULL.
 *
 * The call is synchronous and all its work runs on hip_stream.  On the routes where
 * sre_hip_scanner_last_lines_device() is 1 (the table-driven scanner; Thompson and first-match
 * scanners of the NFA tier) the host reads a fixed number of words per batch and per call: no
 * rows, records or per-line values travel to the host.  The other routes (find-all counting on
 * the tier, the exact VM, SRE_HIP_LINES_NFA_HOST=1) keep their per-line host work and upload
 * one word per line.  The call replaces the scanner's last call exactly as sre_hip_scan_lines
 * does, and the diagnostics (last_fixups, last_line_batches, last_lines_device,
 * last_short_lines, last_kernel_ms: the scan kernels, not the gather) describe it the same
 * way.  len == 0 gives all zeros in info and success.  All offsets and totals are 64-bit.
 * Beyond what line mode takes, a scanner keeps 8 bytes per line of the largest call (plus 16
 * bytes per 1024 lines) of device memory, grow-only, freed with the scanner.
 * Returns 0 on success, -1 on bad arguments or failure.
 */
SRE_API int sre_hip_filter_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    int flags, void *d_out, size_t out_cap, sre_int_t *d_index, size_t index_cap,
    sre_hip_filter_info_t *info, void *hip_stream);

/* ---- line filter with context lines: grep -A / -B / -C ---- */

typedef struct {
    size_t nlines;      /* lines in the buffer */
    size_t nmatched;    /* lines the match rule selects (what sre_hip_filter_lines would select) */
    size_t nselected;   /* nmatched + context-only lines */
    size_t ngroups;     /* maximal runs of adjacent selected lines (what grep separates with "--") */
    size_t need_bytes;  /* sum of (len + 1) over the selected lines */
    size_t nwritten;    /* selected lines written (whole lines only) */
    size_t out_bytes;   /* bytes written to d_out */
} sre_hip_context_info_t;

/*
 * Line filter with context: the matching lines and the lines around them (grep -A after,
 * -B before, -C both), selected on the device.  The split of d_buf, the matching of every line
 * and the engine a scanner routes to are exactly those of sre_hip_filter_lines on the same
 * (sc, d_buf, len, delim); every scanner mode and every engine route is accepted.
 *
 * The match rule.  Line j is MATCHED when sre_hip_filter_lines with the same flags would select
 * it:
 *   - flags == 0: its rc is not SRE_DECLINED;
 *   - SRE_HIP_LINES_INVERT: its rc is SRE_DECLINED (grep -v -C);
 *   - SRE_HIP_LINES_ALL: every line, and then only with before == after == 0: ALL with context
 *     returns -1;
 *   - ALL | INVERT, and any other flag bit, return -1.
 *
 * Selection.  Line i is SELECTED when it is matched, or when some matched line j has
 * j < i <= j + after (-A) or i < j <= i + before (-B).  Every selected line is written once, in
 * line order, however many contexts overlap, as GNU grep does.  before and after may be any
 * size_t: a value at or above the number of lines means "to the end of the buffer", and nothing
 * overflows.  The work per line does not depend on them.
 *
 * before == after == 0 gives byte for byte the output, the index words [0] .. [3] and the counts
 * of sre_hip_filter_lines (nselected == nmatched), and no kernel of the context pass runs.
 *
 * Output, truncation.  As sre_hip_filter_lines: d_out is a DEVICE pointer at any alignment to
 * out_cap bytes that do not overlap [d_buf, d_buf + len) (an overlap returns -1); each selected
 * line is its bytes followed by ONE delim byte, an empty context line still takes that byte, and
 * a final line without a delimiter gets one; only whole lines are written, no byte at or beyond
 * out_bytes is touched and nothing in front of d_out; d_out may be NULL when out_cap == 0 (a
 * sizing call).  Not offered: a group separator in the output (grep's "--").  The output stays a
 * well-formed line buffer of source lines; a caller that wants the separator puts it in front
 * of the rows whose index word [4] has bit 1, other than the first.
 *
 * Index.  d_index is an optional DEVICE array: for each of the first min(index_cap, nwritten)
 * written lines it receives FIVE sre_int_t, with or without context,
 *   [0] line number   [1] offset of the line in d_buf   [2] line length
 *   [3] offset of the line in d_out
 *   [4] flags: bit 0 set for a context-only line (selected, not matched itself); bit 1 set for
 *       the first line of a group (line 0, or a line whose predecessor is not selected).
 * d_index may be NULL when index_cap == 0.  info may be NULL.
 *
 * Counts.  info->nmatched, nselected, ngroups and need_bytes are totals over the whole buffer,
 * whatever out_cap is.
 *
 * The call is synchronous and all its work runs on hip_stream.  On the routes where
 * sre_hip_scanner_last_lines_device() is 1 nothing per line travels to the host: the host reads
 * two words more than sre_hip_filter_lines does, in the same copy.  The other routes keep their
 * per-line host work and upload one word per line, as for the filter; the context pass runs
 * behind them on the device.  Batch cuts need no care: the pass runs once, over the values of
 * the whole call.  The call replaces the scanner's last call and the diagnostics describe it
 * exactly as for sre_hip_filter_lines.  len == 0 gives all zeros in info and success.
 * Beyond what sre_hip_filter_lines takes, a scanner keeps one bit per line of the largest call
 * with context plus 32 bytes per 1024 lines of the largest call of device memory, grow-only,
 * freed with the scanner.  Returns 0 on success, -1 on bad arguments or failure.
 */
SRE_API int sre_hip_filter_lines_context(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    int flags, size_t before, size_t after, void *d_out, size_t out_cap,
    sre_int_t *d_index, size_t index_cap, sre_hip_context_info_t *info, void *hip_stream);

/* ---- line fold: continuation lines joined into multi-line records ---- */

enum { SRE_HIP_FOLD_NEXT = 8 };   /* a marked line continues into the FOLLOWING line (default: it belongs to the line in front of it) */

typedef struct {
    size_t nlines, nmarked, nrecords, longest, need_bytes, nwritten, out_bytes;
} sre_hip_fold_info_t;

/*
 * Line fold: the lines of d_buf joined into multi-line records, from one device buffer to
 * another (logstash's multiline codec, Filebeat's multiline.pattern / negate / match, Fluent
 * Bit's multiline parser, awk '/^[0-9]{4}-/{if (r) print r; r=$0; next} {r = r "\x01" $0}').
 * A stack trace, a wrapped message or a pretty-printed object becomes ONE line of the output,
 * its source lines separated by the byte `join`, so that every other line call sees it as one
 * record.  The split of d_buf, the matching of every line and the engine a scanner routes to
 * are exactly those of sre_hip_filter_lines on the same (sc, d_buf, len, delim): only match /
 * no match of a line is used, and every scanner mode and every engine route is accepted.
 *
 * The rule, over the n lines of the split.  Line i is MARKED when it has a match (its rc is not
 * SRE_DECLINED), with SRE_HIP_LINES_INVERT when it has none.
 *   - default (logstash what => previous): a marked line is a continuation of the record in
 *     front of it.  Line i is a natural head when i == 0 or line i is not marked.
 *   - SRE_HIP_FOLD_NEXT (what => next): a marked line is joined to the line behind it.  Line i is
 *     a natural head when i == 0 or line i - 1 is not marked.
 * With h(i) the nearest natural head at or in front of line i (line 0 always is one), line i is
 * a HEAD when it is a natural head, or when max_lines != 0 and (i - h(i)) % max_lines == 0:
 * max_lines caps the lines of a record and splits a runaway record into pieces of at most
 * max_lines lines; 0 means no cap.  A RECORD is a head and the lines up to the next head.
 *
 * The four combinations of logstash's pattern / negate / what:
 *   - lines that do not start with a timestamp belong to the previous line:
 *     pattern ^\d{4}-\d\d-\d\d, flags SRE_HIP_LINES_INVERT;
 *   - indented lines and "Caused by:" belong to the previous line:
 *     pattern ^(\s|Caused by:), flags 0;
 *   - a line ending in a backslash continues into the next:
 *     pattern \\$, flags SRE_HIP_FOLD_NEXT;
 *   - everything up to a terminator line is one record:
 *     the terminator's pattern, flags SRE_HIP_FOLD_NEXT | SRE_HIP_LINES_INVERT.
 * Any flag bit outside SRE_HIP_LINES_INVERT | SRE_HIP_FOLD_NEXT returns -1.
 *
 * Output.  d_out is a DEVICE pointer at any alignment to out_cap bytes that do not overlap
 * [d_buf, d_buf + len) (an overlap returns -1).  EVERY line of the buffer is written, in line
 * order: line i's bytes, then `delim` when line i is the last line of its record (i == n - 1 or
 * line i + 1 is a head), otherwise the byte `join` (0 .. 255, else -1).  The output is a
 * well-formed line buffer with one record per line; when `join` occurs in no line and is not
 * the delimiter, folding it again with the same scanner reproduces it.  join == delim is allowed:
 * the output is then the input with a final delimiter, and the call is useful for its tables.
 * info->need_bytes is the sum of the line lengths plus n, whatever out_cap is.
 *
 * Truncation.  Only whole RECORDS are written: info->nwritten is the largest number of leading
 * records whose bytes fit out_cap, info->out_bytes their size.  No byte of d_out at or beyond
 * out_bytes is touched and nothing in front of d_out.  d_out == NULL with out_cap == 0 is the
 * sizing call; d_out == NULL with out_cap != 0 returns -1.
 *
 * Tables, both optional DEVICE arrays.  A table pointer must be NULL exactly when its capacity
 * is 0, else -1.
 *   - d_recid[i], for the first min(recid_cap, n) lines: the record number of line i (the heads at
 *     or in front of i, minus 1), whatever out_cap is.
 *   - d_records: for each of the first min(records_cap, nwritten) records FIVE sre_int_t,
 *       [0] first line   [1] lines   [2] offset of the first line in d_buf
 *       [3] bytes of the record in d_out without its final delimiter   [4] offset in d_out.
 *
 * Counts.  info->nlines, nmarked (marked lines), nrecords (heads), longest (the lines of the
 * longest record) and need_bytes are totals over the whole buffer.  info may be NULL.
 *
 * Not offered: SRE_HIP_LINES_ALL; a join string of more or fewer than one byte (so the
 * backslash of a continuation line is not stripped); a cap on a record's bytes; unfolding, that
 * is translating `join` back to the delimiter; records across calls or stream sets (the last
 * record of a buffer may continue in the next); selecting records in the same call: filter the
 * output instead.
 *
 * The call is synchronous and all its work runs on hip_stream; the host waits as often as in
 * sre_hip_filter_lines and reads three words more in the same copy.  Nothing per line or per
 * record travels to the host on the device routes; the other routes keep their per-line host
 * work as for the filter, and the fold pass runs behind them on the device.  Batch cuts need no
 * care: the pass runs once, over the values of the whole call.  The call replaces the scanner's
 * last call and the diagnostics describe it exactly as for sre_hip_filter_lines.  len == 0 gives
 * all zeros in info and success.  Beyond what sre_hip_filter_lines takes, a scanner keeps 16
 * bytes and two bits per line plus 40 bytes per 1024 lines of the largest fold call of device
 * memory, grow-only, freed with the scanner.  Returns 0 on success, -1 on bad arguments or
 * failure, with info untouched.
 */
SRE_API int sre_hip_fold_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim, int flags, int join,
    size_t max_lines, void *d_out, size_t out_cap, sre_int_t *d_recid, size_t recid_cap,
    sre_int_t *d_records, size_t records_cap, sre_hip_fold_info_t *info, void *hip_stream);

/* ---- line extract: capture groups of each matching line as delimited rows in a device buffer ---- */

enum { SRE_HIP_EXTRACT_MAX_FIELDS = 32 };

/*
 * Line extract: the text of chosen capture groups of every matching line, as rows of fields in
 * device memory (cuDF extract, regexp_extract, sed -n 's/../\1/p').  The split of d_buf, the
 * matching of every line and the engine a scanner routes to are exactly those of
 * sre_hip_scan_lines on the same (sc, d_buf, len, delim).  sc must have been created with
 * SRE_HIP_PIKE_FIRST: a line's record then holds the captures of its FIRST match, and those are
 * the only ones offered.  Thompson and COUNT scanners return -1 with a diagnostic on stderr.
 *
 * Groups.  groups[0 .. ngroups) are capture group numbers, 0 the whole match, in any order, with
 * repeats allowed; 1 <= ngroups <= SRE_HIP_EXTRACT_MAX_FIELDS and every group lies in
 * [0, max_ncaps] (max_ncaps = (result_slots - 2) / 2 - 1), anything else returns -1.  With
 * several regexes the group is that of the regex that matched, as the record's ovector has it.
 *
 * Which lines are selected:
 *   - flags == 0: the lines whose rc is not SRE_DECLINED;
 *   - SRE_HIP_LINES_ALL: every line, a line without a match with every field unset, so row i of
 *     the output is line i of the input;
 *   - SRE_HIP_LINES_INVERT, and any other bit, return -1.
 *
 * Output.  Each selected line gives one row, in line order: field 0, fsep, field 1, fsep, ..,
 * field K - 1, delim (K = ngroups, fsep a byte 0..255, for instance '\t').  Field f is the bytes
 * [ov[2g], ov[2g + 1]) of the line for g = groups[f], and empty when the group is unset
 * (ov[2g] < 0 or ov[2g + 1] < ov[2g]) or the line has no match.  Nothing is escaped: a field may
 * contain fsep; it cannot contain delim.  Fields may overlap or nest.  d_out is a DEVICE pointer
 * at any alignment to out_cap bytes that do not overlap [d_buf, d_buf + len) (an overlap returns
 * -1).  info->need_bytes is the sum over the selected lines of (field lengths + K) whatever
 * out_cap is; info->nselected counts lines.
 *
 * Truncation.  Only whole rows are written: info->nwritten is the largest k for which the first
 * k rows take at most out_cap bytes, info->out_bytes that total.  No byte of d_out at or beyond
 * out_bytes is touched and nothing is written in front of d_out.  d_out may be NULL when
 * out_cap == 0 (a sizing call).
 *
 * Index.  d_index is an optional DEVICE array: for each of the first min(index_cap, nwritten)
 * rows it receives 4 + 2 * ngroups sre_int_t,
 *   [0] line number   [1] offset of the line in d_buf   [2] line length
 *   [3] offset of the row in d_out
 *   then per field [offset of the field in d_buf, length], or [-1, -1] for an unset field (how
 *   a caller tells unset from empty).
 * d_index may be NULL when index_cap == 0.  info may be NULL.
 *
 * The call is synchronous and all its work runs on hip_stream.  It replaces the scanner's last
 * call and the diagnostics describe it exactly as for sre_hip_filter_lines.  On the device
 * routes (the table-driven scanner; first match on the NFA tier, 64-bit and wide forms) the host
 * reads a fixed number of words per batch and per call; on the host route (the exact VM,
 * SRE_HIP_LINES_NFA_HOST=1) the host fills the per-field values from the records it holds and
 * uploads them batch by batch.  len == 0 gives all zeros in info and success.  Beyond what line
 * mode takes, a scanner keeps 16 bytes per line and field of the largest call (plus 16 bytes
 * per 1024 of them) of device memory, grow-only, shared with sre_hip_filter_lines, freed with
 * the scanner.  Returns 0 on success, -1 on bad arguments or failure.
 */
SRE_API int sre_hip_extract_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const int *groups, size_t ngroups, int fsep, int flags, void *d_out, size_t out_cap,
    sre_int_t *d_index, size_t index_cap, sre_hip_filter_info_t *info, void *hip_stream);

/* ---- line substitute: the first match of each line rewritten by a template, into a device buffer ---- */

enum { SRE_HIP_SUBST_MAX_PIECES = 30, SRE_HIP_SUBST_MAX_LITERAL = 4096 };

/*
 * The template of sre_hip_substitute_lines, parsed on the host (no device needed).  tmpl is
 * tmpl_len bytes, NUL allowed, in the syntax of ngx.re.sub:
 *   - `$` and the longest run of decimal digits behind it: that capture group (0: the match);
 *   - `${digits}`: that group, so that `${1}0` is group 1 and then the literal `0`;
 *   - `$$`: one `$`;
 *   - every other byte is literal.  Adjacent literal bytes are ONE piece.
 * Returns -1 for a `$` in front of anything else or at the end, `${` without digits or without
 * `}`, a group above max_group, more than SRE_HIP_SUBST_MAX_PIECES pieces, or more than
 * SRE_HIP_SUBST_MAX_LITERAL literal bytes in all.  The empty template is valid and has no piece
 * (it deletes the match).  On success *npieces (may be NULL) is the number of pieces and
 * piece_groups (NULL, or SRE_HIP_SUBST_MAX_PIECES ints) receives for each piece its group
 * number, or -1 for a literal piece.  For a scanner, max_group is its max_ncaps,
 * (result_slots - 2) / 2 - 1.
 */
SRE_API int sre_hip_subst_template_check(const void *tmpl, size_t tmpl_len, int max_group,
    int *piece_groups, size_t *npieces);

/*
 * Line substitute: sed 's/RE/TEMPLATE/' from one device buffer to another (ngx.re.sub, cuDF
 * replace_with_backrefs).  The split of d_buf, the matching of every line, the routing and the
 * demand for an SRE_HIP_PIKE_FIRST scanner are exactly those of sre_hip_extract_lines on the
 * same (sc, d_buf, len, delim); Thompson and COUNT scanners return -1 with a diagnostic.  Only
 * the FIRST match of a line is rewritten (sed without `g`).
 *
 * Template.  tmpl is HOST memory, parsed as sre_hip_subst_template_check parses it with
 * max_group = the scanner's max_ncaps; what fails there returns -1 here, and so does a literal
 * byte equal to delim (a row would no longer be one line).
 *
 * Which lines are selected:
 *   - flags == 0: the lines with a match (sed -n 's/../../p');
 *   - SRE_HIP_LINES_ALL: every line, a line without a match copied unchanged (sed 's/../../'),
 *     so row i of the output is line i of the input;
 *   - SRE_HIP_LINES_INVERT, and any other bit, return -1.
 *
 * Output.  Each selected line gives one row, in line order.  With [m0, m1) = [ov[0], ov[1]) the
 * first match of the line, the row is line[0, m0), each piece of the template in order,
 * line[m1, len), one delim.  A literal piece is its bytes; a group piece is the bytes
 * [ov[2g], ov[2g + 1]) of the line, and empty when the group is unset (anything but
 * 0 <= ov[2g] <= ov[2g + 1] <= len).  With several regexes the groups are those of the regex that
 * matched.  A selected line whose group 0 fails that rule is copied unchanged.  d_out is a DEVICE
 * pointer at any alignment to out_cap bytes that do not overlap [d_buf, d_buf + len) (an overlap
 * returns -1).  info->need_bytes is the sum over the selected lines of
 * len - (m1 - m0) + replacement length + 1 whatever out_cap is; info->nselected counts lines.
 *
 * Truncation.  Only whole rows are written: info->nwritten is the largest k for which the first
 * k rows take at most out_cap bytes, info->out_bytes that total.  No byte of d_out at or beyond
 * out_bytes is touched and nothing is written in front of d_out.  d_out may be NULL when
 * out_cap == 0 (a sizing call).
 *
 * Index.  d_index is an optional DEVICE array: for each of the first min(index_cap, nwritten)
 * rows it receives 8 sre_int_t,
 *   [0] line number   [1] offset of the line in d_buf   [2] line length
 *   [3] offset of the row in d_out
 *   [4] offset of the match in d_buf   [5] its length
 *   [6] offset of the replacement in d_out   [7] its length
 * with [4] .. [7] all -1 for a line that was copied unchanged (no match, with SRE_HIP_LINES_ALL).
 * d_index may be NULL when index_cap == 0.  info may be NULL.
 *
 * The call is synchronous and all its work runs on hip_stream.  It replaces the scanner's last
 * call and the diagnostics describe it exactly as for sre_hip_extract_lines; the routes, and what
 * the host reads and uploads on each, are the extract's too.  len == 0 gives all zeros in info
 * and success.  Beyond what line mode takes, a scanner keeps 16 bytes per line and entry
 * (pieces + 2 entries a line) of the largest call (plus 16 bytes per 1024 of them) of device
 * memory, grow-only, shared with sre_hip_filter_lines and sre_hip_extract_lines, and 4 KiB for
 * the literal bytes of the last template, which a repeated call does not upload again; all freed
 * with the scanner.  A batch holds at most 2^24 lines x 32 entries.  Returns 0 on success, -1 on
 * bad arguments or failure.
 */
SRE_API int sre_hip_substitute_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const void *tmpl, size_t tmpl_len, int flags, void *d_out, size_t out_cap,
    sre_int_t *d_index, size_t index_cap, sre_hip_filter_info_t *info, void *hip_stream);

/* ---- line route: each line grouped by the regex that matched, bucket by bucket in a device buffer ---- */

enum { SRE_HIP_ROUTE_MAX_BUCKETS = 256 };

typedef struct {
    size_t nlines;      /* lines of the bucket, over the whole buffer */
    size_t offset;      /* where the bucket starts in d_out when everything fits: the bytes of the buckets in front */
    size_t bytes;       /* bytes the bucket takes: sum of (len + 1) over its lines */
} sre_hip_route_bucket_t;

/*
 * Line route: every line classified by the regex of a multi-regex program that matched it and
 * written to the bucket of that regex (awk '/a/{print > "a"} /b/{print > "b"}', the `route`
 * transform of a log pipeline).  The split of d_buf, the matching of every line, the routing to
 * an engine, the batching and the diagnostics are exactly those of sre_hip_extract_lines on the
 * same (sc, d_buf, len, delim).  sc must have been created with SRE_HIP_PIKE_FIRST: a line's rc
 * is then the id of the regex of its FIRST match, Pike's leftmost-then-priority choice when
 * several regexes match the line.  Thompson and COUNT scanners return -1 with a diagnostic on
 * stderr.
 *
 * The map.  With R the regexes of the program, bucket_of is a HOST array of R + 1 ints: entry r
 * (0 <= r < R) is the bucket of a line whose first match belongs to regex r, entry R the bucket
 * of a line without a match.  -1 drops the line; any other value must lie in [0, nbuckets).
 * bucket_of == NULL is the identity with unmatched lines dropped, and nbuckets must then be R.
 * 1 <= nbuckets <= SRE_HIP_ROUTE_MAX_BUCKETS; anything else returns -1.  The call takes no
 * flags, the map says it all: grep is {0, .., 0, -1}, grep -v is {-1, .., -1, 0}, "route plus
 * rest" is {0, 1, .., R - 1, R}.  A line whose rc is an error is dropped.
 *
 * Output.  ONE device buffer, bucket-major: all lines of bucket 0 in line order, then bucket 1,
 * and so on, each line as its bytes followed by ONE delim byte (a final source line without a
 * delimiter gets one too), so the output and every bucket's slice of it are well-formed line
 * buffers.  d_out is a DEVICE pointer at any alignment to out_cap bytes that do not overlap
 * [d_buf, d_buf + len) (an overlap returns -1).  buckets is an optional HOST array of nbuckets
 * entries: buckets[b].nlines and .bytes are the totals of bucket b whatever out_cap is, .offset
 * is where bucket b starts when everything fits.  info->nselected is the routed lines,
 * info->need_bytes the sum of the buckets' bytes.
 *
 * Truncation.  Whole lines only, in output order: info->nwritten is the largest k for which the
 * first k rows of the bucket-major order take at most out_cap bytes, info->out_bytes that
 * total.  No byte of d_out at or beyond out_bytes is touched and nothing is written in front of
 * d_out.  d_out may be NULL when out_cap == 0 (a sizing call).
 *
 * Index.  d_index is an optional DEVICE array: for each of the first min(index_cap, nwritten)
 * rows in output order it receives 5 sre_int_t,
 *   [0] line number   [1] offset of the line in d_buf   [2] line length
 *   [3] offset of the line in d_out   [4] bucket.
 * d_index may be NULL when index_cap == 0.  info may be NULL.
 *
 * The call is synchronous and all its work runs on hip_stream.  It replaces the scanner's last
 * call and the diagnostics describe it exactly as for sre_hip_filter_lines.  On the device
 * routes (the table-driven scanner; first match on the NFA tier, 64-bit and wide forms) the
 * host reads a fixed number of words per batch, one word and then 4 + 2 * nbuckets words per
 * call, and uploads the map only when it differs from the last call's: nothing per line
 * travels to the host.  On the host route (the exact VM, SRE_HIP_LINES_NFA_HOST=1) the host
 * fills one word per line from the records it holds and uploads them batch by batch.
 * len == 0 gives all zeros in info and buckets, and success.  Not offered: a separate output
 * pointer per bucket, context lines, routing by anything but the first match's regex.
 * Beyond what line mode takes, a scanner keeps of the largest call 8 bytes per line (shared
 * with sre_hip_filter_lines), 24 bytes per routed line (8 of them shared with
 * sre_hip_extract_lines), 8 bytes per bucket and 1024 lines, and 4 bytes per regex; all
 * grow-only device memory, freed with the scanner.  Returns 0 on success, -1 on bad arguments
 * or failure.
 */
SRE_API int sre_hip_route_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const int *bucket_of, size_t nbuckets, void *d_out, size_t out_cap,
    sre_int_t *d_index, size_t index_cap, sre_hip_filter_info_t *info,
    sre_hip_route_bucket_t *buckets, void *hip_stream);

/* ---- line tally: the distinct capture-group texts of the lines and how many lines carry each ---- */

typedef struct {
    size_t nlines;      /* lines of the buffer */
    size_t nselected;   /* lines that have a key (sum of all counts) */
    size_t nkeys;       /* distinct keys */
    size_t need_bytes;  /* bytes of all key rows */
    size_t nwritten;    /* key rows written (whole rows only) */
    size_t out_bytes;
} sre_hip_tally_info_t;

enum { SRE_HIP_TALLY_OVERFLOW = 1 };

/*
 * Line tally: `extract | sort | uniq -c` without the sort: one row per DISTINCT tuple of field
 * texts, and how many lines carry it ("lines per status code / client address / host").  The
 * split of d_buf, the matching of every line, the routing to an engine, the batching, the
 * diagnostics, the demand for an SRE_HIP_PIKE_FIRST scanner (Thompson and COUNT scanners return
 * -1 with a diagnostic), the rules for groups / ngroups / fsep, the flags (0 or
 * SRE_HIP_LINES_ALL; any other bit returns -1) and the overlap check of d_out are exactly those
 * of sre_hip_extract_lines on the same (sc, d_buf, len, delim).
 *
 * Key.  The key of a selected line is the tuple of its K = ngroups field texts as the extract
 * defines them; an unset group is an empty field.  Two lines have the same key when every field
 * has the same length and the same bytes: ("ab", "c") and ("a", "bc") are different keys
 * although their rows are the same text when a field contains fsep.  With SRE_HIP_LINES_ALL the
 * lines without a match share the key whose fields are all empty.
 *
 * Output.  One row per distinct key in the extract's row format (field 0, fsep, .., field K - 1,
 * delim), ordered by the FIRST line that carries each key: key k is the k-th key to appear, and
 * row k is exactly the row sre_hip_extract_lines writes for that first line.  The result does
 * not depend on the order in which the device processes the lines.  Truncation is the
 * extract's: whole rows only, info->nwritten of them in info->out_bytes bytes, nothing at or
 * beyond out_bytes is touched, d_out may be NULL with out_cap == 0 (a sizing call).
 * info->need_bytes is the bytes of all info->nkeys rows whatever out_cap is.
 *
 * d_counts is an optional DEVICE array: d_counts[k], k < min(counts_cap, nkeys), is the number
 * of lines with key k.  d_keyid is an optional DEVICE array: d_keyid[i], i < min(keyid_cap,
 * nlines), is the key number of line i, or -1 for a line without a key.  Neither depends on
 * out_cap: a sizing call delivers both in full.  d_index is an optional DEVICE array of the
 * extract's index rows (4 + 2 * ngroups sre_int_t) for the first min(index_cap, nwritten) key
 * rows, each describing the key's first line.  Each may be NULL when its capacity is 0; nothing
 * beyond the entries named here is touched.  info->nselected is the sum of all counts.
 *
 * max_keys and overflow.  1 <= max_keys <= 2^30, anything else returns -1.  When the buffer holds
 * more than max_keys distinct keys the call returns SRE_HIP_TALLY_OVERFLOW: nothing is written to
 * d_out, d_counts, d_keyid or d_index, and info holds nlines and nselected and zeros elsewhere.
 * nkeys == max_keys succeeds.
 *
 * The call is synchronous and all its work runs on hip_stream; the host waits exactly as often
 * as in sre_hip_extract_lines (the overflow flag and nselected travel with the words that call
 * reads).  On the host route (the exact VM, SRE_HIP_LINES_NFA_HOST=1) the per-field values are
 * uploaded as there, and everything behind them runs on the device.  len == 0 gives all zeros in
 * info and success.  Beyond what sre_hip_extract_lines takes (and shares), a scanner keeps 16
 * bytes per table slot, slots = the power of two >= 2 * max_keys and at least 1024, and 4 bytes
 * per line of the largest call; grow-only device memory, freed with the scanner.  Not offered:
 * keys ordered by count or text, top-k, every match of a line, caseless keys.
 * Returns 0 on success, SRE_HIP_TALLY_OVERFLOW, or -1 on bad arguments or failure.
 */
SRE_API int sre_hip_tally_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const int *groups, size_t ngroups, int fsep, int flags, size_t max_keys,
    void *d_out, size_t out_cap,
    uint64_t *d_counts, size_t counts_cap,
    sre_int_t *d_keyid, size_t keyid_cap,
    sre_int_t *d_index, size_t index_cap,
    sre_hip_tally_info_t *info, void *hip_stream);

/* ---- line tally with sums: sum, min, max of a numeric capture group per key ---- */

enum { SRE_HIP_TALLY_MAX_VALUES = 8 };

typedef struct {
    int64_t  sum;   /* of the lines' numbers, modulo 2^64 (two's complement wrap) */
    int64_t  min;   /* INT64_MAX when n == 0 */
    int64_t  max;   /* INT64_MIN when n == 0 */
    uint64_t n;     /* lines of the key whose field is a number */
} sre_hip_tally_sum_t;

/*
 * Line tally with sums: `SELECT key, COUNT(*), SUM(v), MIN(v), MAX(v) .. GROUP BY key`, or
 * awk '{ s[$1] += $10 }' ("bytes sent per client", "total and worst request time per endpoint").
 * d_out, d_counts, d_keyid, d_index, info, max_keys, overflow, the argument checks and the host's
 * waits on the stream are exactly those of sre_hip_tally_lines on the same (sc, d_buf, len, delim,
 * groups, ngroups, fsep, flags, max_keys); that call's contract is not restated here.
 *
 * Value columns.  vgroups names 1 <= nvgroups <= SRE_HIP_TALLY_MAX_VALUES capture groups under the
 * range rule of groups[]; a value group may also be a key group and may appear twice.
 * nvgroups == 0 or beyond the maximum, vgroups == NULL, sums_cap != 0 with d_sums == NULL, or a
 * d_sums that is not 8-byte aligned returns -1.
 *
 * Number rule.  The text of value group v in a line's first match is a number when it is an
 * optional single '-' followed by 1 to 18 bytes that are all '0' .. '9', and nothing else.  Its
 * value is the decimal value, negated after '-': "-0" is 0, "007" is 7.  Anything else is not a
 * number and touches nothing: an unset or empty group, "+1", "-", "1 ", "12a", 19 or more digits,
 * and every value column of a line without a match under SRE_HIP_LINES_ALL.  18 digits keep every
 * value inside int64; only the sum can wrap, and it wraps modulo 2^64.
 *
 * d_sums is an optional DEVICE array: d_sums[k * nvgroups + v], k < min(sums_cap, nkeys), is the
 * aggregate of value column v over all lines of key k; sums_cap counts keys.  A column in which no
 * line of the key is a number is {0, INT64_MAX, INT64_MIN, 0}.  d_sums does not depend on out_cap:
 * a sizing call delivers it in full.  Nothing at or beyond row min(sums_cap, nkeys) is touched, and
 * on SRE_HIP_TALLY_OVERFLOW nothing of d_sums is written.  Sum, min, max and n do not depend on
 * the order in which the device meets the lines: the result is bit-exact.
 *
 * Beyond what sre_hip_tally_lines takes (and shares), a scanner keeps 16 bytes per line and value
 * column of the largest call, and at most 8 MiB of working copies of the aggregates; grow-only
 * device memory, freed with the scanner.
 * sre_hip_tally_lines itself never allocates or fills it.  Not offered: fractions, exponents,
 * hexadecimal, '+', floating-point sums, averages (divide sum by n), sums over every match of a
 * line.  Returns 0 on success, SRE_HIP_TALLY_OVERFLOW, or -1 on bad arguments or failure.
 */
SRE_API int sre_hip_tally_sums_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const int *groups, size_t ngroups, const int *vgroups, size_t nvgroups, int fsep, int flags,
    size_t max_keys, void *d_out, size_t out_cap,
    uint64_t *d_counts, size_t counts_cap,
    sre_hip_tally_sum_t *d_sums, size_t sums_cap,
    sre_int_t *d_keyid, size_t keyid_cap,
    sre_int_t *d_index, size_t index_cap,
    sre_hip_tally_info_t *info, void *hip_stream);

/* host only, needs no device: the number rule above on len bytes of text.  1: a number, *value is
 * it; 0: not a number, *value is untouched */
SRE_API int sre_hip_tally_number(const void *text, size_t len, int64_t *value);

/* ---- key sets and the line lookup: select the lines whose captured key is in a device key set ---- */

typedef struct sre_hip_keyset_s sre_hip_keyset_t;

/*
 * A key set: the distinct keys of a DICTIONARY, kept on the device for any number of lookups
 * (`grep -F -f keys` on a field, `WHERE ip IN (...)`, awk's `NR==FNR{s[$1];next} $3 in s`).
 *
 * Row format.  d_rows is a device pointer at any alignment to len bytes in the row format that
 * sre_hip_extract_lines and sre_hip_tally_lines write: field 0, fsep, .., field K - 1, delim, with
 * K = nfields.  The rows are split by the split rule of line mode: a final row without delim is a
 * row, and len == 0 is the empty set, which is valid.  A row must hold exactly nfields - 1 bytes
 * equal to fsep; with nfields == 1 nothing is split and fsep is ignored.  When a row breaks that
 * rule, create returns NULL with one diagnostic line on stderr that names the LOWEST such row.
 *
 * create returns NULL without touching the device when nfields < 1 or nfields >
 * SRE_HIP_EXTRACT_MAX_FIELDS, when fsep or delim is outside 0 .. 255, or when fsep == delim with
 * nfields > 1; and NULL behind the count of the rows when there are more than 2^30 of them.
 *
 * Ownership.  The set keeps its own copy of the rows: d_rows may be freed or overwritten as soon as
 * create has returned.  create is synchronous on hip_stream.  The set is immutable afterwards;
 * any number of scanners and streams of the same device may use it at once.  Its device memory
 * (sre_hip_keyset_device_bytes: the copy, 16 bytes per field of every row, 8 bytes per slot) is
 * freed by sre_hip_keyset_destroy; a NULL set is ignored there.
 *
 * Keys and ids.  The key of a row is the tuple of its field texts, compared as the tally compares
 * keys: every length first, then the bytes, so ("ab", "c") and ("a", "bc") differ.  The ID of a
 * key is the lowest row number that carries it; sre_hip_keyset_distinct is the number of keys,
 * sre_hip_keyset_rows the number of rows.  The table has sre_hip_keyset_slots words, the power of
 * two >= 2 * rows and at least 1024.
 *
 * sre_hip_keyset_hash is the set's hash of one row (its text WITHOUT the delimiter) on the host;
 * it needs no device.  A row's home slot, where its search begins and from where it moves up one
 * word at a time around the table's end, is hash & (slots - 1): a caller may shard keys by it.
 * It returns 0 for arguments out of range and for a row that breaks the field rule.
 * SRE_HIP_KEYSET_HASH_BITS=n (test knob, read at create) keeps the low n bits of the hash in
 * front of the index; a lookup takes the mask from the set.
 *
 * Key maps.  sre_hip_keyset_create_map builds a set whose rows carry VALUE COLUMNS behind the key:
 * a row holds nfields fields under the same field rule (exactly nfields - 1 bytes equal to fsep, the
 * diagnostic names the lowest bad row), the first nkeys fields are the key, the other nfields -
 * nkeys fields are value columns 0 .., which sre_hip_join_lines appends to the lines that carry the
 * key.  It returns NULL without touching the device unless 1 <= nkeys <= nfields <=
 * SRE_HIP_EXTRACT_MAX_FIELDS, and for everything create refuses.  sre_hip_keyset_create(..,
 * nfields, ..) is create_map with nkeys == nfields.  sre_hip_keyset_fields is the number of KEY
 * fields and sre_hip_keyset_values the number of value columns (0 for a plain set), so a map is a
 * valid argument of sre_hip_lookup_lines; sre_hip_keyset_hash is given the key fields only.  The
 * id of a key is still the lowest row that carries it, and the VALUES of a key are the values of
 * that row: the first row wins and later rows of the same key are ignored.  (awk's m[$1]=$2 keeps
 * the LAST row; sort the dictionary the other way round for that.)  A map remembers its delim and
 * keeps 16 more bytes per value column of every row, which device_bytes counts.
 *
 * Not offered: mutable sets (build a new one), last-row-wins, caseless keys, rows whose fields
 * contain fsep.
 */
SRE_API sre_hip_keyset_t *sre_hip_keyset_create(const void *d_rows, size_t len, size_t nfields,
    int fsep, int delim, void *hip_stream);
SRE_API sre_hip_keyset_t *sre_hip_keyset_create_map(const void *d_rows, size_t len, size_t nfields,
    size_t nkeys, int fsep, int delim, void *hip_stream);
SRE_API size_t sre_hip_keyset_values(const sre_hip_keyset_t *ks);   /* nfields - nkeys; 0 for a plain set */
SRE_API void sre_hip_keyset_destroy(sre_hip_keyset_t *ks);
SRE_API size_t sre_hip_keyset_rows(const sre_hip_keyset_t *ks);
SRE_API size_t sre_hip_keyset_distinct(const sre_hip_keyset_t *ks);
SRE_API size_t sre_hip_keyset_fields(const sre_hip_keyset_t *ks);
SRE_API size_t sre_hip_keyset_slots(const sre_hip_keyset_t *ks);
SRE_API size_t sre_hip_keyset_device_bytes(const sre_hip_keyset_t *ks);
SRE_API uint64_t sre_hip_keyset_hash(const void *row, size_t len, size_t nfields, int fsep);

typedef struct {
    size_t nlines;      /* lines of the buffer */
    size_t nkeyed;      /* lines with a match, i.e. with a key */
    size_t nmembers;    /* of those, lines whose key is in the set */
    size_t nselected;   /* lines the flags select */
    size_t need_bytes;  /* bytes all of them take */
    size_t nwritten;    /* selected lines written (whole lines only) */
    size_t out_bytes;
} sre_hip_lookup_info_t;

/*
 * Line lookup: the lines of d_buf whose captured key is in the set (the semi-join), or with
 * SRE_HIP_LINES_INVERT the lines with a key that is not (the anti-join).  The split of d_buf, the
 * matching of every line, the routing to an engine, the batching, the diagnostics, the demand for
 * an SRE_HIP_PIKE_FIRST scanner (Thompson and COUNT scanners return -1 with a diagnostic) and the
 * range rule of groups are exactly those of sre_hip_extract_lines on the same (sc, d_buf, len,
 * delim); the overlap check of d_out is the filter's.  ks == NULL and ngroups !=
 * sre_hip_keyset_fields(ks) return -1.
 *
 * Selection.  A line is KEYED when it has a match; its key is the tuple of the texts of the capture
 * groups `groups` of its first match, an unset group an empty field.  A keyed line is a MEMBER
 * when that tuple equals the key of some row of the set.  flags == 0 selects the members,
 * SRE_HIP_LINES_INVERT the keyed lines that are not members.  A line without a match has no key
 * and is never selected.  Any other flag bit, SRE_HIP_LINES_ALL included, returns -1.
 *
 * Output, truncation, the sizing call and d_index are those of sre_hip_filter_lines byte for byte:
 * the selected lines in line order, each followed by one delim, whole lines only, nothing at or
 * beyond out_bytes touched, d_out == NULL with out_cap == 0 sizes the output, index rows of the
 * filter's four words.
 *
 * d_keyid is an optional DEVICE array: d_keyid[i], i < min(keyid_cap, nlines), is the id of the
 * line's key in the set (a row number of the dictionary) for a member, -1 for a keyed line that is
 * not a member, -2 for a line without a key.  It does not depend on flags or out_cap; the
 * dictionary row of written line r is d_keyid[index[r][0]].  info->nkeyed and info->nmembers are
 * totals over the buffer whatever out_cap is.  len == 0 gives zeros and success; an empty set
 * makes no line a member.
 *
 * The call is synchronous and all its work runs on hip_stream; the host waits exactly as often as
 * in sre_hip_filter_lines.  The set is only read.  Beyond what sre_hip_filter_lines takes, a
 * scanner keeps the 16 bytes per line and key group that sre_hip_tally_sums_lines keeps per value
 * column (the same grow-only memory, freed with the scanner).  Not offered: every match of a line,
 * caseless keys, Thompson and COUNT scanners, stream sets.  The dictionary's value columns joined
 * into the output are sre_hip_join_lines; the lines grouped by their dictionary row are
 * sre_hip_route_lines_by_key.
 * Returns 0 on success, -1 on bad arguments or failure.
 */
SRE_API int sre_hip_lookup_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const int *groups, size_t ngroups, const sre_hip_keyset_t *ks, int flags,
    void *d_out, size_t out_cap,
    sre_int_t *d_keyid, size_t keyid_cap,
    sre_int_t *d_index, size_t index_cap,
    sre_hip_lookup_info_t *info, void *hip_stream);

/* ---- the line distinct: select lines by first, last or count of their key ---- */

enum { SRE_HIP_DISTINCT_FIRST = 0, SRE_HIP_DISTINCT_LAST = 1, SRE_HIP_DISTINCT_EVERY = 2 };

typedef struct {
    size_t nlines;      /* lines of the buffer */
    size_t nkeyed;      /* lines with a match, i.e. with a key */
    size_t nkeys;       /* distinct keys */
    size_t nkeys_kept;  /* distinct keys whose count is within [min_count, max_count] */
    size_t nselected;   /* lines the rule and the flags select */
    size_t need_bytes;  /* sum of (len + 1) over them */
    size_t nwritten;    /* selected lines written (whole lines only) */
    size_t out_bytes;
} sre_hip_distinct_info_t;

/*
 * Line distinct: the lines of d_buf deduplicated by a captured key: the first or the last line of
 * every key, or every line of the keys that occur a given number of times.  It writes whole lines
 * where sre_hip_tally_lines writes one row of key fields per key:
 *   awk '!seen[k]++', and sort -u behind a sort      SRE_HIP_DISTINCT_FIRST, min 1, max 0
 *   the latest record per key                        SRE_HIP_DISTINCT_LAST,  min 1, max 0
 *   uniq -u (keys that occur once)                   SRE_HIP_DISTINCT_FIRST, min 1, max 1
 *   uniq -d (one line per repeated key)              SRE_HIP_DISTINCT_FIRST, min 2, max 0
 *   uniq -D, GROUP BY key HAVING COUNT(*) >= n       SRE_HIP_DISTINCT_EVERY, min n, max 0
 *
 * What is the lookup's.  The split of d_buf, the matching of every line, the routing to an engine,
 * the batching and the diagnostics are exactly those of sre_hip_lookup_lines on the same (sc,
 * d_buf, len, delim); so are the demand for an SRE_HIP_PIKE_FIRST scanner (Thompson and COUNT
 * scanners return -1 with a diagnostic), the range rule of groups (1 to
 * SRE_HIP_EXTRACT_MAX_FIELDS of them) and the overlap check of d_out.
 *
 * Key.  A line is KEYED when it has a match; its key is the tuple of the texts of the capture
 * groups `groups` of its first match, compared as sre_hip_tally_lines compares keys: field by
 * field, lengths first, so ("ab", "c") and ("a", "bc") differ.  An unset group is an empty field.
 * A line without a match has no key and is never selected.
 *
 * Count range.  The count c of a key is the number of keyed lines that carry it, over the WHOLE
 * buffer: equal keys need not be adjacent, unlike uniq's.  A key QUALIFIES when min_count <= c
 * and (max_count == 0 or c <= max_count).  min_count == 0, and a nonzero max_count below
 * min_count, return -1.
 *
 * Rule.  A keyed line is PICKED when its key qualifies and, with SRE_HIP_DISTINCT_FIRST, it is the
 * lowest line of its key; with SRE_HIP_DISTINCT_LAST the highest; with SRE_HIP_DISTINCT_EVERY
 * always.  Any other `which` returns -1.
 *
 * Flags.  flags == 0 selects the picked lines; SRE_HIP_LINES_INVERT selects the keyed lines that
 * are NOT picked (with FIRST, 1, 0: the duplicates the plain call removes).  Any other flag bit,
 * SRE_HIP_LINES_ALL included, returns -1.
 *
 * Output, truncation, the sizing call and d_index are those of sre_hip_filter_lines byte for byte:
 * the selected lines in line order, each followed by one delim, whole lines only, nothing at or
 * beyond out_bytes touched, d_out == NULL with out_cap == 0 sizes the output, index rows of the
 * filter's four words.  The output is a line buffer again.
 *
 * Per-line arrays.  d_keycount and d_keyline are optional DEVICE arrays.  d_keycount[i], i <
 * min(keycount_cap, nlines), is the count of line i's key, 0 for a line without a key.
 * d_keyline[i], i < min(keyline_cap, nlines), is the lowest line that carries line i's key, -1
 * for a line without one: a deterministic name of the key, and the line whose row
 * sre_hip_tally_lines writes for it.  Neither depends on which, the range, flags or out_cap.  A
 * NULL pointer with a nonzero capacity returns -1.
 *
 * Totals.  info->nkeyed, nkeys, nkeys_kept, nselected and need_bytes are totals over the buffer
 * whatever out_cap is.  With FIRST or LAST and no INVERT, nselected == nkeys_kept.
 *
 * max_keys and overflow are the tally's: 1 <= max_keys <= 2^30, else -1; a buffer with more than
 * max_keys distinct keys returns SRE_HIP_TALLY_OVERFLOW, nothing is written to d_out, d_keycount,
 * d_keyline or d_index, and info holds nlines and nkeyed and zeros elsewhere; nkeys == max_keys
 * succeeds.  SRE_HIP_TALLY_HASH_BITS is the tally's knob here too.
 *
 * len == 0 gives all zeros and success.  The call is synchronous and all its work runs on
 * hip_stream; the result does not depend on the order in which the device meets the lines.  The
 * host waits exactly as often as in sre_hip_lookup_lines: the overflow flag and the totals travel
 * in the one read of the filter's four words.  On the device routes nothing per line or per key
 * travels to the host.
 *
 * Memory.  Beyond what sre_hip_lookup_lines takes, a scanner keeps the table of
 * sre_hip_tally_lines (16 bytes per slot, slots = the power of two at or above max(1024, 2 x
 * max_keys), and 4 bytes per line for the slots of the lines; the same memory), and for
 * SRE_HIP_DISTINCT_LAST 8 bytes per slot more.  All grow-only device memory, freed with the
 * scanner.
 *
 * Not offered: SRE_HIP_LINES_ALL; adjacency-only uniq semantics (keys are counted over the whole
 * buffer); caseless keys; key numbers in first-appearance order (sre_hip_tally_lines gives
 * those); a fifth index word; every match of a line; Thompson and COUNT scanners; stream sets.
 * Returns 0 on success, SRE_HIP_TALLY_OVERFLOW, or -1 on bad arguments or failure; a call that
 * returns -1 for its arguments leaves info untouched.
 */
SRE_API int sre_hip_distinct_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const int *groups, size_t ngroups, int which, size_t min_count, size_t max_count, int flags,
    size_t max_keys, void *d_out, size_t out_cap,
    uint64_t *d_keycount, size_t keycount_cap,
    sre_int_t *d_keyline, size_t keyline_cap,
    sre_int_t *d_index, size_t index_cap,
    sre_hip_distinct_info_t *info, void *hip_stream);

/* ---- the line join: append a key map's value columns to each matching line ---- */

enum { SRE_HIP_JOIN_MAX_VALUES = 31 };

/*
 * Line join: every line of d_buf whose captured key is in the key map ks, with the chosen value
 * columns of the key's dictionary row behind it (the equi-join: awk's
 * `NR==FNR{m[$1]=$2;next} ($3 in m){print $0, m[$3]}`, SQL's JOIN); with SRE_HIP_LINES_ALL every
 * line, the ones without a dictionary row with empty values (LEFT JOIN).
 *
 * On the same (sc, d_buf, len, delim, groups, ngroups, ks) the split, the matching, the routing to
 * an engine, the batching, the diagnostics, the demand for an SRE_HIP_PIKE_FIRST scanner, the range
 * rule of groups, ngroups == sre_hip_keyset_fields(ks), the overlap check, d_keyid (-1 not a
 * member, -2 no key; independent of flags and out_cap), info->nkeyed, info->nmembers and the number
 * of host waits are exactly those of sre_hip_lookup_lines.
 *
 * Returns -1 as well: for ks == NULL or a set without value columns; for nvcols < 1, nvcols >
 * SRE_HIP_JOIN_MAX_VALUES, vcols == NULL or a column outside [0, sre_hip_keyset_values(ks)); for
 * jsep outside 0 .. 255 or equal to delim; for a delim that is not the one the map was created
 * with (a value could hold the call's delimiter, and a row would no longer be one line); for any
 * flag bit other than SRE_HIP_LINES_ALL.  vcols may be in any order and may repeat.
 *
 * Selection.  flags == 0 selects the members (the inner join).  SRE_HIP_LINES_ALL selects every
 * line (the left outer join): a line that is not a member or has no key gets every value field
 * empty, so row i of the output is line i of the input.  SRE_HIP_LINES_INVERT is not offered: the
 * anti-join has no values and is sre_hip_lookup_lines.
 *
 * Output.  One row per selected line, in line order:
 *     line bytes, jsep, value vcols[0], jsep, .., value vcols[V - 1], delim
 * Nothing is escaped.  need_bytes is the sum over the selected lines of len + 1 + the sum of (value
 * length + 1).  Truncation and the sizing call are the extract's: whole rows only, nothing at or
 * beyond out_bytes is touched, nothing in front of d_out.
 *
 * Index.  A row has 5 + 2 * nvcols words: [0] line, [1] start, [2] len, [3] the row's offset in
 * d_out, [4] the dictionary row, or -1 / -2 as in d_keyid, then per value column [the offset of the
 * value in d_out, its length], or [-1, -1] for a row without a dictionary row.
 *
 * len == 0 gives zeros and success.  With flags == 0 an empty map selects nothing, with
 * SRE_HIP_LINES_ALL every line with empty value fields.
 *
 * Memory.  Beyond what sre_hip_lookup_lines takes, a scanner keeps 16 bytes per line and entry of
 * the join's table, 1 + nvcols entries a line (the extract's grow-only table), and 8 bytes per
 * line for the index's key ids.  The map is only read.  Not offered: a default text for missing
 * values, last-row-wins, joining extracted fields instead of the whole line, INVERT, caseless keys.
 * Returns 0 on success, -1 on bad arguments or failure.
 */
SRE_API int sre_hip_join_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const int *groups, size_t ngroups, const sre_hip_keyset_t *ks,
    const int *vcols, size_t nvcols, int jsep, int flags,
    void *d_out, size_t out_cap,
    sre_int_t *d_keyid, size_t keyid_cap,
    sre_int_t *d_index, size_t index_cap,
    sre_hip_lookup_info_t *info, void *hip_stream);

/* ---- the line route by key: group lines by the dictionary row of their key ---- */

typedef struct {
    size_t nlines, nkeyed, nmembers;   /* as sre_hip_lookup_info_t */
    size_t nselected;                  /* lines the flags select */
    size_t nbuckets;                   /* NON-EMPTY buckets among them */
    size_t need_bytes, nwritten, out_bytes;
} sre_hip_route_key_info_t;

/*
 * Line route by key: the lines of d_buf grouped by the dictionary row of their captured key, in
 * ONE output buffer (awk's `{ print > $3 }`, GROUP BY with the rows kept, the `sort -s -k` in
 * front of any per-key processing).
 *
 * On the same (sc, d_buf, len, delim, groups, ngroups, ks) the split, the matching, the routing to
 * an engine, the batching, the diagnostics, the demand for an SRE_HIP_PIKE_FIRST scanner (Thompson
 * and COUNT scanners return -1 with a diagnostic), the range rule of groups, ngroups ==
 * sre_hip_keyset_fields(ks), the overlap check, d_keyid (-1 for a keyed line that is not a member,
 * -2 for a line without a key; independent of flags and out_cap), info->nkeyed and info->nmembers
 * are exactly those of sre_hip_lookup_lines.  A key map is a valid set; its value columns are
 * ignored.
 *
 * Selection and order.  flags == 0 selects the members; SRE_HIP_LINES_ALL selects every line, so
 * the output is a permutation of the input's lines.  Any other bit returns -1, SRE_HIP_LINES_INVERT
 * included: there is nothing to group by then, that is sre_hip_lookup_lines.  The output is
 * bucket-major.  The buckets are the dictionary ids in ascending order (an id is the lowest row
 * that carries the key, so the rows of sre_hip_tally_lines used as the dictionary give
 * first-appearance order); with ALL the bucket of the keyed lines that are not members (id -1)
 * follows the last dictionary bucket and the bucket of the lines without a key (id -2) comes
 * last.  Inside a bucket the lines are in line order.  Each line is its bytes plus ONE delim, as
 * sre_hip_route_lines writes them: the output and every bucket's slice of it are line buffers.
 *
 * Truncation, the sizing call and the guards are those of sre_hip_route_lines: whole lines only,
 * in output order; nothing at or beyond out_bytes is touched and nothing in front of d_out; d_out
 * == NULL with out_cap == 0 sizes the output.
 *
 * Index.  d_index is an optional DEVICE array: for each of the first min(index_cap, nwritten) rows
 * in output order it receives 5 sre_int_t,
 *   [0] line number   [1] offset of the line in d_buf   [2] line length
 *   [3] offset of the line in d_out   [4] the dictionary id, or -1 / -2 as in d_keyid.
 *
 * Bucket table.  d_buckets is an optional DEVICE array (per-bucket totals cannot travel to the
 * host when the set has a million rows): for each of the first min(buckets_cap, nbuckets)
 * NON-EMPTY buckets in output order it receives 5 sre_int_t,
 *   [0] id (-1 / -2 for the two rest buckets)   [1] rank of its first line among the selected lines
 *   [2] its lines   [3] its offset in the full output   [4] its bytes.
 * The table and info->nbuckets are totals over the buffer whatever out_cap is.  A key of the set
 * that no line carries has no row.  A NULL pointer with a cap other than 0 returns -1, for d_out,
 * d_keyid, d_index and d_buckets alike.
 *
 * len == 0 gives zeros and success.  An empty set selects nothing with flags == 0 and gives the one
 * or two rest buckets with SRE_HIP_LINES_ALL.
 *
 * Limits.  A sort item packs the id and the line number into one 64-bit word, 32 bits for the line:
 * a buffer may hold at most 2^32 - 1 lines, a larger one returns -1 with one diagnostic line.
 *
 * The call is synchronous and all its work runs on hip_stream.  Up to the probe the host waits as
 * often as in sre_hip_lookup_lines; behind it as often as in sre_hip_route_lines: one word that
 * sizes the compact table, one read of 7 result words, then the end.  That does not depend on the
 * lines, the set or the number of passes; nothing per line or per bucket travels to the host.  The
 * partition is a radix sort of one 8-bit digit of the id per pass: 1 pass up to 256 ids, 2 up to
 * 65536, 3 up to 2^24, 4 beyond.  SRE_HIP_ROUTE_KEY_DIGIT_BITS=n, 1 <= n <= 8, is a test knob read
 * on every call that forces narrower digits and so more passes; anything else means 8.
 * SRE_HIP_ROUTE_KEY_RANK=turns is a measurement knob, read on every call as well: the rank of a
 * line inside a wave by one ballot per distinct digit, the rule of sre_hip_route_lines, in place
 * of one ballot per digit bit.  The results are identical.
 *
 * Memory.  Beyond what sre_hip_lookup_lines takes, a scanner keeps of the largest call 8 bytes per
 * line (the key ids, shared with sre_hip_join_lines), 2 KiB per 1024 lines (the counts of a pass,
 * shared with sre_hip_route_lines), and per selected line 16 bytes for the two item arrays, 16
 * for the compact table and 8 for the head ranks (the last 24 shared with sre_hip_route_lines);
 * all grow-only device memory, freed with the scanner.  The set is only read.
 *
 * Not offered: a separate output pointer per bucket; grouping by the buffer's own keys in one call
 * (tally, build a set from the tally's rows, then route by it: that matches the lines twice);
 * ordering the buckets by anything but the dictionary id; INVERT, caseless keys, every match of a
 * line; Thompson and COUNT scanners, stream sets.
 * Returns 0 on success, -1 on bad arguments or failure.
 */
SRE_API int sre_hip_route_lines_by_key(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const int *groups, size_t ngroups, const sre_hip_keyset_t *ks, int flags,
    void *d_out, size_t out_cap,
    sre_int_t *d_keyid, size_t keyid_cap,
    sre_int_t *d_index, size_t index_cap,
    sre_int_t *d_buckets, size_t buckets_cap,
    sre_hip_route_key_info_t *info, void *hip_stream);

/* ---- the line sort: order lines by a numeric capture group, with top-k ---- */

enum { SRE_HIP_SORT_DESC = 4 };   /* largest value first */

typedef struct {
    size_t  nlines;
    size_t  nkeyed;      /* lines with a match */
    size_t  nnumbered;   /* of those, lines whose sort field is a number */
    size_t  nselected;   /* rows of the full output: min(limit, candidates), limit == 0: all */
    size_t  need_bytes, nwritten, out_bytes;
    size_t  passes;      /* digit passes the call made (0 when nothing was selected) */
    int64_t vmin, vmax;  /* over the numbered lines; INT64_MAX / INT64_MIN when there is none */
} sre_hip_sort_info_t;

/*
 * Line sort: the lines of d_buf ordered by the number in one capture group of their first match,
 * optionally only the first `limit` of them (`sort -s -n -k`, `sort -s -rn | head`, ORDER BY v
 * [DESC] LIMIT k: "the 100 slowest requests", "responses by size, largest first").
 *
 * On the same (sc, d_buf, len, delim) and groups = {group} the split, the matching, the routing to
 * an engine, the batching, the diagnostics, the demand for an SRE_HIP_PIKE_FIRST scanner (Thompson
 * and COUNT scanners return -1 with a diagnostic), the range rule of `group` and the overlap check
 * of d_out are exactly those of sre_hip_lookup_lines.
 *
 * The value.  A line is NUMBERED when it has a match and the text of `group` in its first match
 * is a number under the number rule of sre_hip_tally_sums_lines (sre_hip_tally_number tells the
 * same on the host): "-0" is 0 and "007" is 7; an unset or empty group, "+1", "1 " and 19 digits
 * are not numbers.  Its value is that number.  info->nkeyed counts the lines with a match,
 * info->nnumbered the numbered ones, info->vmin and info->vmax are the extremes of the values.
 *
 * Selection and order.  flags == 0 selects the numbered lines, ordered by value ascending;
 * SRE_HIP_SORT_DESC orders them descending.  Lines of equal value stay in line order in BOTH
 * directions (sort -s -n, sort -s -n -r).  SRE_HIP_LINES_ALL selects every line: the lines that
 * are not numbered (keyed lines whose field is no number, and lines without a match) come behind
 * ALL numbered lines, in line order, whatever the direction, so the output is a permutation of
 * the input's lines.  limit != 0 keeps the first `limit` rows of that order (| head -n limit):
 * info->nselected and info->need_bytes describe the limited output; nnumbered, nkeyed, vmin and
 * vmax are totals over the buffer whatever limit and out_cap are.  SRE_HIP_LINES_INVERT and every
 * other bit return -1.
 *
 * Each row is the line's bytes plus ONE delim, so the output is a line buffer again.  Because the
 * sort is stable, a second call on the output sorts by a second column: sort by column B, then
 * sort the result by column A, and the lines are ordered by (A, B, line).  That is why one column
 * a call is enough.
 *
 * Truncation, the sizing call and the guards are those of sre_hip_route_lines: whole lines only,
 * in output order; nothing at or beyond out_bytes is touched and nothing in front of d_out; d_out
 * == NULL with out_cap == 0 sizes the output.  A NULL pointer with a cap other than 0 returns -1,
 * for d_out and d_index alike.  len == 0 gives zeros and success, with vmin / vmax the identities
 * INT64_MAX / INT64_MIN.
 *
 * Index.  d_index is an optional DEVICE array: for each of the first min(index_cap, nwritten) rows
 * in output order it receives 6 sre_int_t,
 *   [0] line number   [1] offset of the line in d_buf   [2] line length
 *   [3] offset of the line in d_out   [4] the value (0 when the line is not numbered)
 *   [5] the class: 1 numbered, -1 keyed but no number, -2 no match.
 *
 * Limits.  A sort item carries the line number in 32 bits: a buffer may hold at most 2^32 - 1
 * lines, a larger one returns -1 with one diagnostic line.
 *
 * The call is synchronous and all its work runs on hip_stream.  Up to the value table the host
 * waits as often as in sre_hip_lookup_lines; behind it as often as in sre_hip_route_lines_by_key:
 * one read of four words (nkeyed, nnumbered, vmin, vmax) that sizes the item arrays and fixes the
 * keys, one read of 4 result words, then the end.  Nothing per line travels to the host.  The
 * sort key is the value's distance from vmin (from vmax when descending), an unsigned 64-bit word;
 * the sort is a stable radix sort of one 8-bit digit of it per pass, and the pass count follows
 * the DATA: info->passes is 1 for values within 255 of each other, 2 for HTTP status codes, 3 for
 * a range below 2^24, 8 for the full 18-digit range.  It is always the full sort, then the cut at limit: every pass
 * runs over all selected lines however small limit is.
 *
 * Memory.  Beyond what sre_hip_lookup_lines takes, a scanner keeps of the largest call 9 bytes per
 * line (the values, shared with sre_hip_join_lines' key ids, and one byte of class), 2 KiB per
 * 1024 lines (the counts of a pass, shared with sre_hip_route_lines), per selected line 24 bytes
 * for the two pairs of item arrays (16 of them shared with sre_hip_route_lines_by_key) and per
 * row in front of the limit 16 bytes for the compact table (shared with sre_hip_route_lines); all
 * grow-only device memory, freed with the scanner.
 *
 * Not offered: text or locale order, floating point, sort -u; several columns in one call
 * (compose, see above); sorting extracted fields instead of whole lines (extract from the sorted
 * output); a per-line value array supplied by the caller (it would give "tally rows by count");
 * INVERT, every match of a line; Thompson and COUNT scanners, stream sets.
 * Byte order of the group's text is a call of its own, sre_hip_sort_lines_text.
 * Returns 0 on success, -1 on bad arguments or failure.
 */
SRE_API int sre_hip_sort_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    int group, int flags, size_t limit,
    void *d_out, size_t out_cap,
    sre_int_t *d_index, size_t index_cap,
    sre_hip_sort_info_t *info, void *hip_stream);

/* ---- the ordered tally: key rows ordered by count or by an aggregate, with a limit ---- */

enum { SRE_HIP_TOP_COUNT = 0, SRE_HIP_TOP_SUM = 1, SRE_HIP_TOP_MIN = 2, SRE_HIP_TOP_MAX = 3, SRE_HIP_TOP_N = 4 };

typedef struct {
    size_t  nlines;      /* lines of the buffer */
    size_t  nselected;   /* lines that have a key (the sum of all counts) */
    size_t  nkeys;       /* distinct keys, whatever limit is */
    size_t  nordered;    /* keys whose order column holds a value */
    size_t  nrows;       /* rows of the limited output: min(limit, nkeys), nkeys when limit == 0 */
    size_t  need_bytes, nwritten, out_bytes;   /* of those nrows rows; truncation as in the tally */
    size_t  passes;      /* digit passes of the sort */
    int64_t vmin, vmax;  /* extremes of the order values; INT64_MAX / INT64_MIN when nordered == 0 */
} sre_hip_tally_top_info_t;

/*
 * Ordered tally: sre_hip_tally_sums_lines whose rows, counts, aggregates and index come out in a
 * chosen order, optionally only the first `limit` keys (`sort | uniq -c | sort -rn | head`, GROUP
 * BY key ORDER BY COUNT(*) DESC LIMIT k: "the ten busiest clients", "endpoints by total bytes").
 * It offers what the "Not offered" lists of sre_hip_tally_lines ("keys ordered by count ..,
 * top-k") and of sre_hip_sort_lines ("a per-line value array ..") decline, for counts and
 * aggregates; the order stays on the device, and so does the output.
 *
 * What is the tally's.  On the same (sc, d_buf, len, delim, groups, ngroups, vgroups, nvgroups,
 * fsep, max_keys) and the SRE_HIP_LINES_ALL bit of flags the split, the matching, the routing to
 * an engine (host routes included), the batching, the diagnostics, the demand for an
 * SRE_HIP_PIKE_FIRST scanner, the key, the rules of groups / vgroups / fsep, the number rule,
 * max_keys and SRE_HIP_TALLY_OVERFLOW are exactly those of sre_hip_tally_sums_lines.  On overflow
 * nothing of the caller's arrays is written and info holds nlines and nselected only.
 *
 * Flags.  flags is any of SRE_HIP_LINES_ALL | SRE_HIP_SORT_DESC; any other bit returns -1.
 * nvgroups == 0 with vgroups == NULL is allowed only with by == SRE_HIP_TOP_COUNT and sums_cap
 * == 0; d_sums must be 8-byte aligned.
 *
 * The order value of key k: SRE_HIP_TOP_COUNT its count; SRE_HIP_TOP_N the n of value column
 * by_col; SRE_HIP_TOP_SUM / _MIN / _MAX that field of column by_col, the sum as d_sums holds it,
 * after wrapping.  `by` outside the enum, by_col >= nvgroups for a column order and by_col != 0
 * for SRE_HIP_TOP_COUNT return -1.  A key is ORDERED unless by is SUM, MIN or MAX and the
 * column's n is 0.  info->nordered counts the ordered keys, vmin / vmax are their extremes; they
 * are the identities INT64_MAX / INT64_MIN without an ordered key, for len == 0 (zeros elsewhere,
 * and success) and on overflow.
 *
 * The order.  First the ordered keys by order value, ascending, or descending with
 * SRE_HIP_SORT_DESC; keys of equal value in first-appearance order in BOTH directions; then the
 * keys that are not ordered, in first-appearance order, whatever the direction.  The sort, its
 * stability and info->passes are those of sre_hip_sort_lines over the keys.  limit != 0 keeps the
 * first `limit` rows: info->nrows = min(limit, nkeys).  It is always the full sort, then the cut.
 *
 * Outputs, all in output order.  Row r of d_out is the tally's row of the key at rank r, in the
 * extract's row format.  Truncation and the sizing call are the tally's: whole rows, and d_out ==
 * NULL with out_cap == 0 sizes the output; need_bytes, nwritten and out_bytes describe the nrows
 * rows.  d_counts[r] holds the count for r below min(counts_cap, nrows), d_sums[r * nvgroups + v]
 * the aggregates for r below min(sums_cap, nrows), both whatever out_cap is.  d_index holds for
 * the first min(index_cap, nwritten) rows the extract's index row of the key's first line, 4 + 2
 * ngroups sre_int_t with [3] the row's offset in THIS output, and two more words: the key's
 * number in first-appearance order, and its order value (0 when not ordered); 6 + 2 ngroups
 * sre_int_t a row.  d_rank[i], for i below min(rank_cap, nlines), is the rank of line i's key in
 * the FULL order, whatever limit and out_cap are, -1 for a line without a key.  The output with
 * limit == 0 is a valid dictionary for sre_hip_keyset_create, and d_rank then equals the key ids
 * sre_hip_lookup_lines gives against it.  Nothing beyond the entries named is touched.  A NULL
 * pointer with a cap other than 0 returns -1, for every array.
 *
 * Range.  The sort's key rule reserves the all-ones key and gives the keys that are not ordered
 * RANGE + 1, so a call whose vmax - vmin exceeds 2^64 - 3 returns -1 with one diagnostic line and
 * nothing written to the caller's arrays.  Only sums that wrapped reach that.  An item carries
 * the key's number in 32 bits, which max_keys <= 2^30 guarantees.
 *
 * The call is synchronous and all its work runs on hip_stream.  The host waits as often as in
 * sre_hip_tally_sums_lines, plus two reads: one of the four totals (nkeys, nordered, vmin, vmax),
 * which fixes the sort keys and the passes, and one of the four result words.  Nothing per key or
 * per line travels to the host.
 *
 * Memory.  Beyond what sre_hip_tally_sums_lines takes, a scanner keeps of the largest call per
 * key 20 + 32 nvgroups bytes of its own (count, aggregates, first line, inverse rank) and 8
 * ngroups bytes per row in front of the limit (the ordered table's starts); with
 * sre_hip_sort_lines it shares per key 9 bytes (value and class), 24 bytes of items and 2 KiB per
 * 1024 keys of counts, and with sre_hip_route_lines 8 ngroups bytes per row.  Nothing is kept per
 * line.  All grow-only device memory, freed with the scanner; sre_hip_tally_lines,
 * sre_hip_tally_sums_lines and sre_hip_sort_lines neither allocate nor fill the call's own.
 *
 * Not offered: order by key text; several order columns in one call; a partial top-k selection
 * in place of the full sort; floating-point averages; every match of a line; Thompson and COUNT
 * scanners; stream sets.
 * Returns 0 on success, SRE_HIP_TALLY_OVERFLOW, or -1 on bad arguments or failure.
 */
SRE_API int sre_hip_tally_top_lines(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    const int *groups, size_t ngroups, const int *vgroups, size_t nvgroups, int fsep, int flags,
    size_t max_keys, int by, size_t by_col, size_t limit,
    void *d_out, size_t out_cap,
    uint64_t *d_counts, size_t counts_cap,
    sre_hip_tally_sum_t *d_sums, size_t sums_cap,
    sre_int_t *d_rank, size_t rank_cap,
    sre_int_t *d_index, size_t index_cap,
    sre_hip_tally_top_info_t *info, void *hip_stream);

/* ---- the line sort by text: order lines by the bytes of a capture group ---- */

typedef struct {
    size_t nlines;
    size_t nkeyed;      /* lines with a match */
    size_t nselected;   /* rows of the full output: min(limit, candidates), limit == 0: all */
    size_t need_bytes, nwritten, out_bytes;
    size_t passes;      /* the length of the plan: digit passes that can move a line */
    size_t minlen, maxlen;   /* shortest and longest COMPARED text over the keyed lines; SIZE_MAX / 0 when there is none */
} sre_hip_sort_text_info_t;

/*
 * Line sort by text: the lines of d_buf ordered by the BYTES of one capture group of their first
 * match, optionally only the first `limit` of them (`LC_ALL=C sort -s -k`, ORDER BY text [DESC]
 * LIMIT k: by client address as text, by host name or URL path, by an ISO timestamp with a
 * fraction, by a hexadecimal id, by any key longer than 18 digits).  It is what the "Not offered"
 * list of sre_hip_sort_lines declines as "text .. order", in byte order.
 *
 * What is the numeric sort's.  On the same (sc, d_buf, len, delim, group) the split, the matching,
 * the routing to an engine (host routes included), the batching, the diagnostics, the demand for
 * an SRE_HIP_PIKE_FIRST scanner, the range rule of `group`, the overlap check of d_out, limit,
 * truncation at whole lines, the sizing call, the NULL-pointer rule and the bound of 2^32 - 1
 * lines are exactly those of sre_hip_sort_lines.
 *
 * The text.  A line with a match is KEYED; its text is the bytes of `group` in the first match,
 * and an unset group is the empty text, as an unset group is an empty field in the extract's rows
 * (the index row tells the two apart).  max_bytes != 0 compares only the first max_bytes bytes of
 * the text (sort -k1.1,1.N); max_bytes == 0 compares the whole text.  info->nkeyed counts the
 * keyed lines, info->minlen and info->maxlen are the shortest and the longest COMPARED text over
 * them, SIZE_MAX and 0 without a keyed line (and for len == 0, with zeros elsewhere and success).
 *
 * The order is that of memcmp over unsigned bytes with a proper prefix first (LC_ALL=C sort).  Any
 * byte other than delim may occur, NUL included: "a" < "a\0" < "a\0\0" < "aa".
 *
 * Flags.  flags is any of SRE_HIP_LINES_ALL | SRE_HIP_SORT_DESC; any other bit returns -1 with
 * info untouched.  flags == 0 writes the keyed lines ascending, SRE_HIP_SORT_DESC descending.
 * Lines of equal compared text stay in line order in BOTH directions.  SRE_HIP_LINES_ALL selects
 * every line: the lines without a match come behind ALL keyed lines, in line order, whatever the
 * direction, so the output is a permutation of the input's lines.
 *
 * Each row is the line's bytes plus ONE delim, so the output is a line buffer again, and the sort
 * is stable: a second call, this one or sre_hip_sort_lines, on the output sorts by a second
 * column.
 *
 * Index.  d_index is an optional DEVICE array: for each of the first min(index_cap, nwritten) rows
 * in output order it receives 6 sre_int_t,
 *   [0] line number   [1] offset of the line in d_buf   [2] line length
 *   [3] offset of the line in d_out
 *   [4] offset of the field in d_buf   [5] its FULL length, whatever max_bytes is;
 * [4] and [5] are -1, -1 for an unset group and for a line without a match.
 *
 * The plan.  The compared text is cut into chunks of 7 bytes; the key of a chunk is a 64-bit word
 * of its bytes, big-endian, and the count of bytes it holds, and the sort is a stable radix sort
 * of one 8-bit digit of one chunk per pass, last chunk first.  After the one read of (nkeyed,
 * minlen, maxlen) the host lists the (chunk, digit) passes at which two selected lines can differ
 * at all; sre_hip_sort_text_plan tells the same list, and info->passes is its length: maxlen for
 * texts of one length, about 8/7 of maxlen + 1 otherwise, eight for chunk 0 when ALL has a line
 * without a match to place, 0 when every compared text is empty.  THE COST IS LINEAR IN maxlen:
 * every pass runs over all selected lines, however small limit is, and max_bytes is the caller's
 * bound on it.
 *
 * The call is synchronous and all its work runs on hip_stream.  The host waits exactly as often
 * as in sre_hip_sort_lines: one read of four words behind the value table, one read of 4 result
 * words, then the end.  Nothing per line travels to the host.
 *
 * Memory.  The call has no arrays of its own: per line 9 bytes (compared length, then the key of
 * the first chunk, and a byte of class), 2 KiB per 1024 lines of counts, per selected line 24
 * bytes of items and per row in front of the limit 16 bytes of compact table, all of them the
 * arrays sre_hip_sort_lines keeps; grow-only device memory, freed with the scanner.
 *
 * Not offered: locale or caseless order; several columns in one call (compose, see above);
 * sort -u; text order for the keys of sre_hip_tally_top_lines; a radix sort that skips passes by
 * looking at histograms; Thompson and COUNT scanners; stream sets.
 * Returns 0 on success, -1 on bad arguments or failure.
 */
SRE_API int sre_hip_sort_lines_text(sre_hip_scanner_t *sc, const void *d_buf, size_t len, int delim,
    int group, size_t max_bytes, int flags, size_t limit,
    void *d_out, size_t out_cap,
    sre_int_t *d_index, size_t index_cap,
    sre_hip_sort_text_info_t *info, void *hip_stream);

/* The plan of sre_hip_sort_lines_text on the host, from what its info reports; rest: the call had
 * SRE_HIP_LINES_ALL and at least one line without a match.  pairs[2 i] and pairs[2 i + 1] receive
 * the chunk and the digit (0: the count byte, 7 - j: byte j of the chunk) of pass i, for i below
 * min(cap, length); pairs may be NULL with cap 0.  Returns the length.  Needs no device. */
SRE_API size_t sre_hip_sort_text_plan(size_t minlen, size_t maxlen, int rest, uint64_t *pairs, size_t cap);

/* ---- stream sets: many device-resident streams of one program, fed chunk by chunk ---- */

typedef struct sre_hip_streams_s sre_hip_streams_t;

/*
 * A stream set: nstreams independent streams of one compiled program, each the equivalent of
 * one reference context (sre_vm_pike_create_ctx, sre_vm_pike.c:94-145, resp.
 * sre_vm_thompson_create_ctx) whose state — the ordered thread list as an automaton state, one
 * capture vector per listed thread, the pending match, processed_bytes, seen_newline /
 * seen_word — lives on the device between calls.  mode: SRE_HIP_PIKE_FIRST or SRE_HIP_THOMPSON.
 * Owned by `pool`.
 *
 * Returns NULL (with a diagnostic on stderr) when the program's chunks cannot run on the
 * table-driven scanner: a program the step automaton declines (the NFA tier's and the exact
 * VM's programs), one with more than 64 listed threads or 64 capture slots, or a Thompson
 * program with look-ahead assertions (that VM's \A ^ \b are local to a call's buffer).  Pike
 * programs with look-ahead assertions are admitted.
 *
 * Scope: ONE search per stream.  A stream is closed by its first final answer (a match,
 * SRE_DECLINED, SRE_ERROR) and stays closed until sre_hip_streams_reset gives its slot a fresh
 * context.  Re-arming a context inside the chunk that held the match (the find-all iteration
 * of sre_vm_pike.c:179-196, 624-628) and SRE_HIP_PIKE_COUNT over chunks are not offered.
 */
SRE_API sre_hip_streams_t *sre_hip_streams_create(sre_pool_t *pool, sre_program_t *prog,
    int mode, size_t nstreams);

/* as sre_hip_streams_create, with the engine chosen like sre_hip_scanner_create's:
 * SRE_HIP_ENGINE_SCAN = exactly sre_hip_streams_create; SRE_HIP_ENGINE_NFA = the bit-parallel NFA tier
 * (64, 128 or 256 bits) or NULL; SRE_HIP_ENGINE_AUTO = the table-driven scanner when it admits the program's
 * chunks, else the NFA tier, else NULL.  SRE_HIP_ENGINE_VM: NULL.
 *
 * The NFA tier takes SRE_HIP_THOMPSON streams of programs without look-ahead assertions (counted
 * repeats, `(a|b)*a(a|b){k}`-shaped rules): there a stream's context is its thread set, so feeding in
 * chunks equals feeding the whole buffer.  Every other combination is NULL with a diagnostic on stderr;
 * a Pike first match is not offered (its exact window starts at a position that may lie in a chunk that
 * is gone).  feed, reset, the record and the diagnostics are those of the table-driven set. */
SRE_API sre_hip_streams_t *sre_hip_streams_create_engine(sre_pool_t *pool, sre_program_t *prog,
    int mode, int engine, size_t nstreams);
SRE_API int sre_hip_streams_engine(sre_hip_streams_t *ss);     /* SRE_HIP_ENGINE_SCAN or _NFA */
SRE_API int sre_hip_streams_nfa_bits(sre_hip_streams_t *ss);   /* 64 / 128 / 256, 0 on the scanner */

SRE_API size_t sre_hip_streams_count(sre_hip_streams_t *ss);

/* sre_int_t per record: 5 + 2 * (max_ncaps + 1) */
SRE_API size_t sre_hip_streams_result_slots(sre_hip_streams_t *ss);

/* HBM the set holds for its contexts: nstreams rows of 8 * (4 + nslots * (1 + 2 * max_threads))
 * bytes, nslots and max_threads being the program's capture slots and longest thread list
 * (Thompson: 32 bytes a stream).  On the NFA tier: nstreams * 8 * (1 + W) bytes, W = nfa_bits / 64 —
 * one flag word (started, match pending, closed, the closing rc) and the thread set */
SRE_API size_t sre_hip_streams_device_bytes(sre_hip_streams_t *ss);

/*
 * One exec() per stream.  d_chunks, lens and eof are HOST arrays of nstreams entries:
 * d_chunks[i] is a DEVICE pointer to lens[i] bytes at any alignment, eof[i] != 0 marks stream
 * i's last chunk.  d_chunks[i] == NULL: stream i is not fed in this call.  lens[i] == 0 with a
 * non-NULL pointer IS a call (the reference answers SRE_AGAIN, or takes its EOF step with eof).
 * Synchronous; all work on hip_stream.  The number of kernel launches, copies and waits of a
 * call does not depend on nstreams (fix-up rounds aside).  0 on success, -1 on failure.
 *
 * results: nstreams records of sre_hip_streams_result_slots() sre_int_t each:
 *   [0] rc      what sre_vm_pike_exec(ctx_i, chunk, len, eof, &pending) (resp.
 *               sre_vm_thompson_exec) returns for this call after the same earlier calls:
 *               regex id (SRE_OK for Thompson), SRE_AGAIN, SRE_DECLINED, SRE_ERROR
 *   [1] state   0 open (more chunks welcome); 1 closed by this call (rc is final); 2 was
 *               closed before this call (the chunk was ignored and not read; [0] and [2..]
 *               repeat the closing record); 3 not fed in this call (rest of the record
 *               undefined)
 *   [2..4]      has_pending, pending[0], pending[1]: the reference's *pending_matched after
 *               SRE_AGAIN (sre_vm_pike.c:640-688); 0, -1, -1 otherwise
 *   [5..]       ovector, 2 * (max_ncaps + 1) slots, ABSOLUTE stream offsets, -1 unset.  On a
 *               match: the captures (:945-989).  On SRE_AGAIN: [5] and [6] are the temporary
 *               match range of prepare_temp_captures (:692-735), the others -1.
 */
SRE_API int sre_hip_streams_feed(sre_hip_streams_t *ss, const void *const *d_chunks,
    const size_t *lens, const unsigned char *eof, sre_int_t *results, void *hip_stream);

/* give streams idx[0..n) fresh contexts (a new flow takes over the slot).  Synchronous. */
SRE_API int sre_hip_streams_reset(sre_hip_streams_t *ss, const size_t *idx, size_t n);

/* diagnostics: fix-up rounds of the last feed (as sre_hip_scanner_last_fixups) */
SRE_API int sre_hip_streams_last_fixups(sre_hip_streams_t *ss);

/* diagnostics: kernels and copies the last feed queued (fix-up rounds: the batches of rounds) */
SRE_API int sre_hip_streams_last_launches(sre_hip_streams_t *ss);

/* diagnostics: exact-entry passes of the last feed's fix-up rounds (as sre_hip_scanner_last_exact_passes) */
SRE_API int sre_hip_streams_last_exact_passes(sre_hip_streams_t *ss);

/* ---- helpers for drivers that have no HIP runtime binding of their own ---- */

/* device buffer management (hipMalloc / hipFree / hipMemcpy) */
SRE_API void *sre_hip_alloc(size_t bytes);
SRE_API void  sre_hip_free(void *d_ptr);
SRE_API int   sre_hip_upload(void *d_dst, const void *h_src, size_t bytes);
SRE_API int   sre_hip_download(void *h_dst, const void *d_src, size_t bytes);
SRE_API int   sre_hip_synchronize(void *hip_stream);

/*
 * Fill d_dst[0..n) with the reference benchmark stream, generated on device
 * (bench/gen-data.pl:9 restated):  byte i is "abccc"[i % 5] for
 * i < n - tail_len, and the last tail_len bytes are `tail`.  With
 * n = 5 * k + tail_len this is exactly  "abccc" x k . tail.
 */
SRE_API int sre_hip_gen_data(void *d_dst, size_t n, const void *h_tail,
    size_t tail_len, void *hip_stream);

/*
 * Plain streaming read of n bytes (16 B per lane, grid-stride) — the box's
 * measured HBM read ceiling, reported next to the scanner's rate.  Writes one
 * checksum word per workgroup into an internal buffer.  Asynchronous.
 */
SRE_API int sre_hip_read_ceiling(const void *d_src, size_t n, void *hip_stream);

/*
 * The scanner's staging access pattern with no automaton work: the first
 * n / seg_bytes rows of seg_bytes (a multiple of 128) each, one row per lane,
 * tile (64, 128 or 256) bytes of every row per round, fetched one round ahead.
 * lds_bytes of dynamic LDS are requested only to pin the workgroups per CU to
 * what the scanner gets.  The rate this reaches is the ceiling the access
 * pattern itself allows; bench.py reports it next to the plain read ceiling.
 * Asynchronous.
 */
SRE_API int sre_hip_read_pattern(const void *d_src, size_t n, unsigned seg_bytes,
    unsigned tile, unsigned lds_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
