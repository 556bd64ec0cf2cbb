/*
 * sre_hip_nfa_wide.hip — the wide bit-parallel NFA scanner (gfx950): the NFA tier for programs whose
 * thread sets need more than the 64 bits of sre_hip_nfa.hip (host form: sre_nfa_wide.h).
 *
 * Geometry, staging and exactness are those of sre_k_nfa_sa: one lane walks one segment, 64 bytes per
 * round staged through LDS in half lines (sre_hip_tile.h tile2_*), each round tests for an event once
 * and a round with an event is replayed byte by byte; entry sets are speculative (a 128-byte warm-up,
 * which can only under-estimate) and verified by the chain check.  The lane's set is W 64-bit words:
 *
 *      t  = S & accept[byte];   ev |= t & msrc
 *      S' = ((t & shift_src) << 1, carried across words) | (t & self) | seed | OR_k lut[k][byte hot[k] of t]
 *
 * NL lookups per byte, all issued back to back: the form's own tables, padded up to the compiled count
 * with a table of zeros.  The byte of the mask that indexes a lookup is a kernel argument (uniform).
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "sre_hip_nfa_wide.h"
#include "sre_hip_tile.h"
#include "sre_nfa_wide.h"

namespace {

__device__ inline uint32_t
nfaw_stream_of(const sre_scan_geom_t &G, uint64_t g)
{
    uint32_t a = 0, b = G.nstreams;
    while (b - a > 1) {
        uint32_t m = (a + b) >> 1;
        if (geom_first(G, m) <= g) a = m; else b = m;
    }
    return a;
}

typedef const __attribute__((address_space(3))) uint64_t *lds_u64_t;
typedef const __attribute__((address_space(3))) uint32_t *lds_u32_t;

/* LDS layout of a workgroup (all dynamic; its size: sre_nfa_wide.h sre_nfa_wide_lds): tile | row descriptors |
 * accept [256][W] | kinds [256] | zero table [256][W] (when NL > nlut) | lut [nlut][256][W] | expand [16][1 << nassert][W] */
__host__ __device__ constexpr uint32_t
nfaw_off_acc(void) { return SRE_SCAN_BLOCK * SRE_TILE2_ROWB + SRE_SCAN_BLOCK * 16; }
static_assert(nfaw_off_acc() == SRE_NFA_WIDE_TILE_LDS, "the builder's LDS formula counts this staging");

/*
 * sre_k_nfa_wide<W, NL, LA>: W words per set, NL lookups per byte (>= the form's nlut), LA: the program
 * has look-ahead assertions (bits 0 .. nassert - 1 of word 0).  Both modes in one kernel: clean
 * positions are sampled every 16 bytes.
 */
template <int W, int NL, bool LA>
__global__ __launch_bounds__(SRE_SCAN_BLOCK) void
sre_k_nfa_wide(sre_nfa_wide_tables_t T, sre_scan_geom_t G, sre_nfa_summary_t *__restrict__ sum,
               uint64_t *__restrict__ sets, const int64_t *__restrict__ lo, const uint64_t *__restrict__ belief,
               const uint8_t *__restrict__ bvalid, const uint64_t *__restrict__ eset)
{
    constexpr int      TILE = SRE_SCAN_ROUND;
    constexpr int      WARM = SRE_SCAN_LINE;
    constexpr uint32_t ROWB = SRE_TILE2_ROWB;
    constexpr uint32_t ESZ = 8u * W;
    constexpr int      GRP = W >= 4 ? 2 : 4;       /* accept reads in flight ahead of the chain */
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *tile = lds;
    RowDesc *rows = reinterpret_cast<RowDesc *>(lds + SRE_SCAN_BLOCK * ROWB);
    const uint32_t tid = threadIdx.x;
    const bool     padded = (uint32_t) NL > T.nlut;     /* slots beyond the form's lookups read zeros */
    const uint32_t o_acc = nfaw_off_acc(), o_kind = o_acc + 256 * ESZ, o_zero = o_kind + 256 * 4,
                   o_lut = o_zero + (padded ? 256 * ESZ : 0u), o_exp = o_lut + T.nlut * 256 * ESZ;
    const uint32_t XCOL = LA ? (ESZ << T.nassert) : 0u, XROW = 4u * XCOL;
    {
        uint64_t *acc_w = reinterpret_cast<uint64_t *>(lds + o_acc);
        uint64_t *zero_w = reinterpret_cast<uint64_t *>(lds + o_zero);
        uint64_t *lut_w = reinterpret_cast<uint64_t *>(lds + o_lut);
#pragma unroll
        for (int i = 0; i < W; i++) {
            acc_w[tid * W + i] = T.accept[tid * W + i];
            if (padded) zero_w[tid * W + i] = 0;
        }
        for (uint32_t i = tid; i < T.nlut * 256u * W; i += SRE_SCAN_BLOCK) lut_w[i] = T.lut[i];
        if (LA) {
            const uint32_t kd = T.kind[tid];
            reinterpret_cast<uint32_t *>(lds + o_kind)[tid] =
                ((kd & 3u) * XCOL) | ((kd & 4u) ? 0x8000u : 0u) | (((kd & 3u) * XROW) << 16);
            uint64_t *exp_w = reinterpret_cast<uint64_t *>(lds + o_exp);
            for (uint32_t i = tid; i < (16u << T.nassert) * W; i += SRE_SCAN_BLOCK) exp_w[i] = T.expand[i];
        }
    }
    const uint32_t lds_base = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) uint8_t *) lds;
    /* per lookup slot: the 32-bit word of t and the bit offset of its byte, the table (zeros beyond nlut) */
    uint32_t lw[NL ? NL : 1], lsh[NL ? NL : 1], lbase[NL ? NL : 1];
#pragma unroll
    for (int q = 0; q < NL; q++) {
        const bool real = (uint32_t) q < T.nlut;
        const uint32_t h = real ? T.hot[q] : 0u;
        lw[q] = h >> 2;
        lsh[q] = (h & 3u) * 8u;
        lbase[q] = lds_base + (real ? o_lut + (uint32_t) q * 256u * ESZ : o_zero);
    }
    const uint32_t amask = LA ? ((1u << T.nassert) - 1u) : 0u;
    uint32_t       prev_off = 3u * XROW;        /* LA: the expansion-table row of the byte in front (3: stream start) */

    /* ---- which segment am I ---- */
    const uint64_t g = (uint64_t) blockIdx.x * SRE_SCAN_BLOCK + tid;
    bool           active = g < G.nsegs;
    uint32_t       sidx = 0;
    uint64_t       k = 0;
    if (active) {
        sidx = nfaw_stream_of(G, g);
        k = g - geom_first(G, sidx);
        if (lo != nullptr && (lo[sidx] < 0 || (int64_t) k < lo[sidx])) active = false;
    }
    const uint8_t *data = nullptr;
    int64_t        n = 0, seg_a = 0, seg_b = 0;
    uint64_t       S[W], s_in[W];
    bool           warm = false, finished = false, last_seg = false;
    int64_t        first_ev = -1, last_clean = -1;
    int32_t        clean_mode = 0;
    RowDesc        mine;
    mine.addr = 0;
    mine.lo = 0;
    mine.hi16 = -1;
    const uint32_t sfl = (active && G.sflags != nullptr) ? G.sflags[sidx] : 0u;
    const uint32_t v_init = G.sflags != nullptr ? SRE_SFLAG_INIT(sfl) : G.init_variant;
    const uint32_t v_snap = G.sflags != nullptr ? SRE_SFLAG_SNAP(sfl) : G.init_variant;
    const bool     no_eof = G.sflags != nullptr ? (sfl & SRE_SFLAG_NO_EOF) != 0 : (G.flags & SRE_GEOM_NO_EOF) != 0;
#pragma unroll
    for (int i = 0; i < W; i++) S[i] = s_in[i] = 0;
    if (active) {
        data = geom_ptr(G, sidx);
        n = (int64_t) geom_len(G, sidx);
        seg_a = (int64_t) k * G.seg_bytes;
        seg_b = seg_a + G.seg_bytes;
        last_seg = (k + 1 == geom_first(G, sidx + 1) - geom_first(G, sidx));
        if (seg_b > n) seg_b = n;
        if (k == 0) {
            /* eset: the stream's own entry set [nstreams][W] (a stream set's carried context), else the batch's */
#pragma unroll
            for (int i = 0; i < W; i++) S[i] = eset != nullptr ? eset[(size_t) sidx * W + i] : T.init[v_init][i];
            last_clean = 0;
            clean_mode = (int32_t) SRE_SFLAG_MODE(sfl);
        } else if (lo != nullptr && ((int64_t) k == lo[sidx] || bvalid[g])) {
#pragma unroll
            for (int i = 0; i < W; i++) S[i] = belief[g * W + i];
        } else {
            warm = true;
            /* (a warm-up from offset 0 starts as segment 0 does: with a carried entry set it is exact) */
            const uint32_t v = seg_a <= WARM ? v_init : 2u;
#pragma unroll
            for (int i = 0; i < W; i++) S[i] = seg_a <= WARM && eset != nullptr ? eset[(size_t) sidx * W + i] : T.init[v][i];
        }
#pragma unroll
        for (int i = 0; i < W; i++) s_in[i] = S[i];
        mine.addr = (uint64_t) reinterpret_cast<uintptr_t>(data) + (uint64_t) (seg_a - WARM);
        mine.lo = warm ? (seg_a >= WARM ? 0 : (int32_t) (WARM - seg_a)) : WARM;
        mine.hi16 = (int32_t) (WARM + (seg_b - seg_a)) - 16;
        if (LA) {
            const int64_t first_pos = warm ? (seg_a >= WARM ? seg_a - WARM : 0) : seg_a;
            if (first_pos > 0) prev_off = (T.kind[data[first_pos - 1]] & 3u) * XROW;
        }
    }
    rows[tid] = mine;

    uint64_t snap[W], valid[W];
#pragma unroll
    for (int i = 0; i < W; i++) {
        snap[i] = T.init[v_snap][i];
        valid[i] = T.valid[i];
    }
    /* how the reference arrives at a clean position: see sre_k_nfa */
    auto clean_kind = [&](bool before_is_snap, bool prev_clean, bool leading) -> int {
        if (leading || !before_is_snap) return 0;
        return prev_clean ? 1 : -1;
    };
    uint64_t evv = 0;
    auto expand = [&](uint32_t col_off) {
        const uint32_t at = lds_base + o_exp + prev_off + col_off + (((uint32_t) S[0] & amask) * ESZ);
#pragma unroll
        for (int i = 0; i < W; i++) S[i] |= *(lds_u64_t) (uintptr_t) (at + 8u * i);
#pragma unroll
        for (int i = 0; i < W; i++) evv |= S[i] & T.match_bits[i];
    };
    /* one step; returns whether only the ".*?" thread consumed the byte */
    auto step = [&](const uint64_t (&a)[W], uint32_t kk) -> bool {
        if (LA) {
            if (__builtin_amdgcn_ballot_w64(((uint32_t) S[0] & amask) != 0) != 0) expand(kk & 0x7fffu);
            prev_off = kk >> 16;
        }
        uint64_t t[W], e[W];
        uint32_t t32[2 * W];
#pragma unroll
        for (int i = 0; i < W; i++) {
            t[i] = S[i] & a[i];
            t32[2 * i] = (uint32_t) t[i];
            t32[2 * i + 1] = (uint32_t) (t[i] >> 32);
            e[i] = T.seed[i];
        }
#pragma unroll
        for (int q = 0; q < NL; q++) {
            uint32_t v = t32[0];
#pragma unroll
            for (int i = 1; i < 2 * W; i++) v = lw[q] == (uint32_t) i ? t32[i] : v;
            const uint32_t at = lbase[q] + __builtin_amdgcn_ubfe(v, lsh[q], 8) * ESZ;
#pragma unroll
            for (int i = 0; i < W; i++) e[i] |= *(lds_u64_t) (uintptr_t) (at + 8u * i);
        }
        uint64_t nonany = 0, carry = 0;
#pragma unroll
        for (int i = 0; i < W; i++) {
            const uint64_t ts = t[i] & T.shift_src[i];
            S[i] = (ts << 1) | carry | (t[i] & T.self[i]) | e[i];
            carry = ts >> 63;
            evv |= t[i] & T.msrc[i];
            nonany |= t[i] & ~T.any_bits[i];
        }
        return nonany == 0;
    };
    auto is_snap = [&](const uint64_t (&b)[W]) -> bool {
        uint64_t d = 0;
#pragma unroll
        for (int i = 0; i < W; i++) d |= (b[i] ^ snap[i]) & valid[i];
        return d == 0;
    };
    auto accept_at = [&](uint32_t byte, uint64_t (&a)[W], uint32_t &kk) {
        const uint32_t at = lds_base + o_acc + byte * ESZ;
#pragma unroll
        for (int i = 0; i < W; i++) a[i] = *(lds_u64_t) (uintptr_t) (at + 8u * i);
        kk = LA ? *(lds_u32_t) (uintptr_t) (lds_base + o_kind + byte * 4u) : 0u;
    };
    auto save_in = [&]() {
#pragma unroll
        for (int i = 0; i < W; i++) s_in[i] = S[i] & valid[i];
    };

    const uint32_t nrounds = WARM / TILE + G.seg_bytes / TILE;
    const uint32_t lag = (tid >> 5) & 1u;
    uint4          regs[4], hold[2];
    hold[0] = hold[1] = make_uint4(0, 0, 0, 0);
    __syncthreads();                        /* tables and row descriptors are complete */
    tile2_fetch(regs, rows, tid, 0);
    for (uint32_t s = 0; s <= nrounds; s++) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        tile2_store(regs, hold, tile, tid, s);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (s < nrounds) tile2_fetch(regs, rows, tid, s + 1);

        if (s < lag || s - lag >= nrounds) continue;
        const uint32_t r = s - lag;
        const bool     warm_round = (r < WARM / TILE);
        if (!active || finished || (warm_round && !warm)) continue;
        const int64_t base = seg_a - WARM + (int64_t) r * TILE;
        if (base >= seg_b || base < 0) continue;

        uint64_t       s0[W];
#pragma unroll
        for (int i = 0; i < W; i++) s0[i] = S[i];
        const uint32_t prev_off0 = prev_off;
        if (base + TILE <= seg_b) {
            /* the common round: 64 steps, then one look at the event */
            const uint8_t *src = tile + tid * ROWB;
            int32_t        clean_at = -1, clean_how = 0;
            bool           c14 = false;
            /* a 16-byte piece per iteration: the whole round unrolled holds too many registers */
#pragma unroll 1
            for (int q = 0; q < TILE / 16; q++) {
                const uint4 piece = *reinterpret_cast<const uint4 *>(src + 16 * q);
#pragma unroll
                for (int j0 = 0; j0 < 16; j0 += GRP) {
                    uint64_t av[GRP][W];
                    uint32_t ak[GRP];
#pragma unroll
                    for (int i = 0; i < GRP; i++) {
                        const int      j = j0 + i;
                        const uint32_t word = (j >> 2) == 0 ? piece.x : (j >> 2) == 1 ? piece.y : (j >> 2) == 2 ? piece.z : piece.w;
                        accept_at((word >> (8 * (j & 3))) & 0xffu, av[i], ak[i]);
                    }
#pragma unroll
                    for (int i = 0; i < GRP; i++) {
                        const int j = j0 + i;
                        uint64_t  before[W];
                        if (j == 15) {
#pragma unroll
                            for (int w = 0; w < W; w++) before[w] = S[w];
                        }
                        const bool cl = step(av[i], ak[i]);
                        if (j == 14) c14 = cl;
                        if (j == 15 && cl) {
                            const int how = clean_kind(is_snap(before), c14, LA && (ak[i] & 0x8000u) != 0);
                            if (how >= 0) {
                                clean_at = 16 * q + j + 1;
                                clean_how = how;
                            }
                        }
                    }
                }
            }
            if (evv == 0) {
                if (warm_round) {
                    if (r + 1 == WARM / TILE) save_in();
                } else if (clean_at >= 0) {
                    last_clean = base + clean_at;
                    clean_mode = clean_how;
                }
                continue;
            }
            if (warm_round) {
                /* an event in front of the segment is somebody else's */
                evv = 0;
                if (r + 1 == WARM / TILE) save_in();
                continue;
            }
#pragma unroll
            for (int i = 0; i < W; i++) S[i] = s0[i];
            prev_off = prev_off0;
            evv = 0;
        }
        /* byte by byte: a round with an event, or the ragged end of the stream */
        {
            const int64_t end = base + TILE <= seg_b ? base + TILE : seg_b;
            bool          prev_clean = (base == 0);
#pragma unroll 1
            for (int64_t p = base; p < end; p++) {
                const uint32_t b = data[p];
                uint64_t       before[W], a[W];
                uint32_t       kk;
#pragma unroll
                for (int i = 0; i < W; i++) before[i] = S[i];
                accept_at(b, a, kk);
                const bool cl = step(a, kk);
                if (evv != 0) {
                    if (!warm_round) {
                        first_ev = p;
                        finished = true;
                        break;
                    }
                    evv = 0;
                    prev_clean = false;
                } else if (!warm_round && cl) {
                    const int how = clean_kind(is_snap(before), prev_clean, LA && (kk & 0x8000u) != 0);
                    if (how >= 0) {
                        last_clean = p + 1;
                        clean_mode = how;
                    }
                    prev_clean = true;
                } else {
                    prev_clean = false;
                }
            }
            if (warm_round && r + 1 == WARM / TILE) save_in();
        }
    }

    if (!active) return;
    if (LA && last_seg && !finished && !no_eof) {
        /* the extra iteration at end of input: assertions that hold in front of the end list their
         * continuations; a MATCH among them is an event */
        expand(3u * XCOL);
        if (evv != 0) first_ev = n;
    }
    sre_nfa_summary_t out;
    out.s_in = s_in[0];
    out.s_out = S[0] & valid[0];
    out.first_ev = first_ev;
    out.last_clean = last_clean < 0 ? -1 : last_clean * 2 + clean_mode;
    sum[g] = out;
#pragma unroll
    for (int i = 0; i < W; i++) {
        sets[g * 2 * W + i] = s_in[i];
        sets[g * 2 * W + W + i] = S[i] & valid[i];
    }
}

/* ===================================================================== chain check on W-word sets */

template <int W>
__global__ __launch_bounds__(256) void
sre_k_nfa_wide_verify_a(sre_scan_geom_t G, const sre_nfa_summary_t *__restrict__ sum, const uint64_t *__restrict__ sets,
                        sre_nfa_acc_t *__restrict__ acc, uint64_t *__restrict__ belief, uint8_t *__restrict__ bvalid)
{
    const uint64_t g = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G.nsegs) return;
    const uint32_t s = nfaw_stream_of(G, g);
    const uint64_t k = g - geom_first(G, s);
    if (k > 0) {
        uint64_t d = 0;
#pragma unroll
        for (int i = 0; i < W; i++) {
            const uint64_t out = sets[(g - 1) * 2 * W + W + i];
            d |= sets[g * 2 * W + i] ^ out;
            belief[g * W + i] = out;
        }
        const bool ended = sum[g - 1].first_ev >= 0;
        if (!ended && d != 0) atomicMin(&acc[s].bad, (unsigned long long) k);
        bvalid[g] = ended ? 0 : 1;
    } else {
        bvalid[g] = 0;
    }
    if (sum[g].first_ev >= 0) atomicMin(&acc[s].end, (unsigned long long) k);
}

/* ===================================================================== exact entry sets */

/*
 * As sre_k_nfa_seg_matrix / sre_k_nfa_exact_entries (sre_hip_nfa.hip), at W words: a workgroup of 64W lanes
 * walks every unsettled segment, lane i entering with the singleton {i}, and stores the 64W exit sets
 * (64W x W words a segment); then one wave per stream runs the recurrence
 *      T_{k+1} = E_k u U_{i in T_k \ B_k} F_k({i})
 * from the verified prefix up to the first segment that reports an event and leaves T_k as every lane's belief.
 */
template <int W>
__device__ inline void
nfaw_generic_step(const sre_nfa_wide_tables_t &T, uint64_t (&S)[W], uint32_t byte, uint32_t prevk, uint32_t ck)
{
    if (T.nassert) {
        const uint64_t idx = S[0] & ((1ull << T.nassert) - 1);
        if (idx) {
            const uint64_t *x = T.expand + (((size_t) (prevk * 4 + ck) << T.nassert) + (size_t) idx) * W;
#pragma unroll
            for (int i = 0; i < W; i++) S[i] |= x[i];
        }
    }
    uint64_t t[W], r[W], carry = 0;
#pragma unroll
    for (int i = 0; i < W; i++) {
        t[i] = S[i] & T.accept[(size_t) byte * W + i];
        const uint64_t ts = t[i] & T.shift_src[i];
        r[i] = (ts << 1) | carry | (t[i] & T.self[i]) | T.seed[i];
        carry = ts >> 63;
    }
    for (uint32_t q = 0; q < T.nlut; q++) {
        const uint32_t h = T.hot[q];
        const uint32_t x = (uint32_t) (t[h >> 3] >> (8 * (h & 7))) & 0xffu;
        const uint64_t *l = T.lut + ((size_t) q * 256 + x) * W;
#pragma unroll
        for (int i = 0; i < W; i++) r[i] |= l[i];
    }
#pragma unroll
    for (int i = 0; i < W; i++) S[i] = r[i];
}

template <int W>
__global__ __launch_bounds__(64 * W) void
sre_k_nfa_wide_seg_matrix(sre_nfa_wide_tables_t T, sre_scan_geom_t G, const int64_t *__restrict__ lo, uint64_t *__restrict__ mat)
{
    const uint64_t g = blockIdx.x;
    if (g >= G.nsegs) return;
    const uint32_t bit = threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t sidx = nfaw_stream_of(G, g);
    const uint64_t k = g - geom_first(G, sidx);
    if (lo[sidx] < 0 || (int64_t) k < lo[sidx]) return;
    const uint8_t *data = geom_ptr(G, sidx);
    const int64_t  n = (int64_t) geom_len(G, sidx);
    const int64_t  seg_a = (int64_t) k * G.seg_bytes;
    int64_t        seg_b = seg_a + G.seg_bytes;
    if (seg_b > n) seg_b = n;
    uint64_t S[W];
#pragma unroll
    for (int i = 0; i < W; i++) S[i] = ((uint32_t) i == bit >> 6 ? (1ull << (bit & 63)) : 0ull) & T.valid[i];
    uint32_t prevk = 3;
    if (T.nassert && seg_a > 0) prevk = T.kind[data[seg_a - 1]] & 3u;
    for (int64_t p = seg_a; p < seg_b; p += 64) {
        const int64_t  idx = p + lane;
        const uint32_t mybyte = idx < seg_b ? data[idx] : 0u;
        const uint32_t nb = seg_b - p < 64 ? (uint32_t) (seg_b - p) : 64u;
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t byte = (uint32_t) __builtin_amdgcn_readlane((int) mybyte, (int) j);
            const uint32_t ck = T.kind[byte] & 3u;
            nfaw_generic_step<W>(T, S, byte, prevk, ck);
            prevk = ck;
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) mat[(g * 64 * W + bit) * W + i] = S[i] & T.valid[i];
}

/* what the recurrence needs of one segment: whether it ends the scan, its lane's believed entry set and exit
 * set, and the exit sets of this lane's singletons (lane + 64c); none of it depends on the chain, so the next
 * segment's arrives while this one is folded */
template <int W>
struct NfawSeg {
    uint64_t sin[W], sout[W], rows[W][W];
    bool     ev;
};

template <int W>
__device__ inline void
nfaw_load_seg(const sre_nfa_summary_t *sum, const uint64_t *sets, const uint64_t *mat, uint64_t g, uint32_t lane,
              NfawSeg<W> &d)
{
    d.ev = sum[g].first_ev >= 0;
#pragma unroll
    for (int i = 0; i < W; i++) {
        d.sin[i] = sets[g * 2 * W + i];
        d.sout[i] = sets[g * 2 * W + W + i];
    }
#pragma unroll
    for (int c = 0; c < W; c++) {
#pragma unroll
        for (int i = 0; i < W; i++) d.rows[c][i] = mat[(g * 64 * W + 64u * c + lane) * W + i];
    }
}

template <int W>
__global__ __launch_bounds__(64) void
sre_k_nfa_wide_exact_entries(sre_scan_geom_t G, const sre_nfa_summary_t *__restrict__ sum, const uint64_t *__restrict__ sets,
                             const int64_t *__restrict__ lo, const uint64_t *__restrict__ mat, uint64_t *__restrict__ belief,
                             uint8_t *__restrict__ bvalid)
{
    const uint32_t s = blockIdx.x;
    if (s >= G.nstreams || lo[s] < 0) return;
    const uint32_t lane = threadIdx.x;
    const uint64_t first = geom_first(G, s), nseg = geom_first(G, s + 1) - first;
    const uint64_t kstart = (uint64_t) lo[s];
    if (kstart == 0 || kstart >= nseg) return;
    uint64_t T[W];
#pragma unroll
    for (int i = 0; i < W; i++) T[i] = belief[(first + kstart) * W + i];     /* the verified prefix's exit set */
    uint64_t   stop = nseg;
    NfawSeg<W> cur, nxt;
    nfaw_load_seg<W>(sum, sets, mat, first + kstart, lane, cur);
    for (uint64_t kk = kstart; kk < nseg; kk++) {
        const uint64_t g = first + kk;
        if (kk + 1 < nseg) nfaw_load_seg<W>(sum, sets, mat, g + 1, lane, nxt);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < W; i++) belief[g * W + i] = T[i];
            bvalid[g] = 1;
        }
        if (cur.ev || kk + 1 == nseg) {
            stop = kk + 1;
            break;
        }
        uint64_t r[W];
#pragma unroll
        for (int i = 0; i < W; i++) r[i] = 0;
#pragma unroll
        for (int c = 0; c < W; c++) {
            const uint64_t missing = T[c] & ~cur.sin[c];
            if ((missing >> lane) & 1ull) {
#pragma unroll
                for (int i = 0; i < W; i++) r[i] |= cur.rows[c][i];
            }
        }
#pragma unroll
        for (int i = 0; i < W; i++) {
            uint64_t v = r[i];
            for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
            T[i] = cur.sout[i] | v;
        }
        cur = nxt;
    }
    /* behind the first event nothing is needed: those lanes keep their warm-up */
    for (uint64_t q = stop + lane; q < nseg; q += 64) bvalid[first + q] = 0;
}

typedef void (*nfaw_kernel_t)(sre_nfa_wide_tables_t, sre_scan_geom_t, sre_nfa_summary_t *, uint64_t *, const int64_t *,
                              const uint64_t *, const uint8_t *, const uint64_t *);

template <int W, bool LA>
nfaw_kernel_t
nfaw_kernel_nl(uint32_t nlut)
{
    switch (sre_nfa_wide_round_lut(nlut)) {
    case 0: return sre_k_nfa_wide<W, 0, LA>;
    case 1: return sre_k_nfa_wide<W, 1, LA>;
    case 2: return sre_k_nfa_wide<W, 2, LA>;
    case 4: return sre_k_nfa_wide<W, 4, LA>;
    case 8: return sre_k_nfa_wide<W, 8, LA>;
    default: return sre_k_nfa_wide<W, 16, LA>;
    }
}

nfaw_kernel_t
nfaw_kernel(const sre_nfa_wide_tables_t &t)
{
    const bool la = t.nassert != 0;
    switch (t.W) {
    case 1: return la ? nfaw_kernel_nl<1, true>(t.nlut) : nfaw_kernel_nl<1, false>(t.nlut);
    case 2: return la ? nfaw_kernel_nl<2, true>(t.nlut) : nfaw_kernel_nl<2, false>(t.nlut);
    case 4: return la ? nfaw_kernel_nl<4, true>(t.nlut) : nfaw_kernel_nl<4, false>(t.nlut);
    default: return nullptr;
    }
}

}  // namespace

extern "C" size_t
sre_nfa_wide_kernel_lds(const sre_nfa_wide_tables_t *t)
{
    return sre_nfa_wide_lds(t->W, t->nlut, t->nassert);
}

extern "C" const char *
sre_nfa_wide_kernel_name(const sre_nfa_wide_tables_t *t, char *buf, size_t n)
{
    snprintf(buf, n, "sre_k_nfa_wide<%u, %u, %s>", t->W, sre_nfa_wide_round_lut(t->nlut), t->nassert ? "true" : "false");
    return buf;
}

extern "C" int
sre_nfa_wide_blocks_per_cu(const sre_nfa_wide_tables_t *t)
{
    int         n = 0;
    const void *k = reinterpret_cast<const void *>(nfaw_kernel(*t));
    if (k == nullptr) return 1;
    const size_t lds = sre_nfa_wide_kernel_lds(t);
    if (lds > 64 * 1024) (void) hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, SRE_SCAN_BLOCK, lds);
    if (e != hipSuccess || n < 1) n = 1;
    if (n > 8) n = 8;
    return n;
}

extern "C" hipError_t
sre_launch_nfa_wide_scan(sre_nfa_wide_tables_t tab, sre_scan_geom_t geom, sre_nfa_summary_t *d_sum, uint64_t *d_sets,
                         const int64_t *d_lo, const uint64_t *d_belief, const uint8_t *d_bvalid, const uint64_t *d_entry,
                         hipStream_t stream)
{
    if (geom.nsegs == 0) return hipSuccess;
    const uint32_t grid = (uint32_t) ((geom.nsegs + SRE_SCAN_BLOCK - 1) / SRE_SCAN_BLOCK);
    nfaw_kernel_t  kern = nfaw_kernel(tab);
    const size_t   lds = sre_nfa_wide_kernel_lds(&tab);
    if (kern == nullptr || tab.nlut > SRE_NFA_WIDE_MAX_LUT || lds > SRE_NFA_WIDE_LDS_BUDGET) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(SRE_SCAN_BLOCK), lds, stream, tab, geom, d_sum, d_sets, d_lo, d_belief, d_bvalid, d_entry);
    return hipGetLastError();
}

extern "C" hipError_t
sre_launch_nfa_wide_verify(int mode, uint32_t W, sre_scan_geom_t geom, const sre_nfa_summary_t *d_sum, const uint64_t *d_sets,
                           void *d_acc, sre_nfa_status_t *d_status, uint64_t *d_belief, uint8_t *d_bvalid, int64_t *d_records,
                           uint32_t ovec_slots, const int64_t *d_lo, hipStream_t stream)
{
    if (geom.nstreams == 0) return hipSuccess;
    sre_nfa_acc_t *acc = static_cast<sre_nfa_acc_t *>(d_acc);
    const uint32_t gseg = (uint32_t) ((geom.nsegs + 255) / 256);
    if (W == 1) hipLaunchKernelGGL(sre_k_nfa_wide_verify_a<1>, dim3(gseg), dim3(256), 0, stream, geom, d_sum, d_sets, acc, d_belief, d_bvalid);
    else if (W == 2) hipLaunchKernelGGL(sre_k_nfa_wide_verify_a<2>, dim3(gseg), dim3(256), 0, stream, geom, d_sum, d_sets, acc, d_belief, d_bvalid);
    else hipLaunchKernelGGL(sre_k_nfa_wide_verify_a<4>, dim3(gseg), dim3(256), 0, stream, geom, d_sum, d_sets, acc, d_belief, d_bvalid);
    return sre_launch_nfa_verify_tail(mode, geom, d_sum, d_acc, d_status, d_records, ovec_slots, d_lo, stream);
}

extern "C" size_t
sre_nfa_wide_matrix_bytes(uint32_t W, uint64_t nsegs)
{
    return (size_t) nsegs * 64 * W * W * sizeof(uint64_t);
}

extern "C" hipError_t
sre_launch_nfa_wide_exact_entries(sre_nfa_wide_tables_t tab, sre_scan_geom_t geom, const sre_nfa_summary_t *d_sum,
                                  const uint64_t *d_sets, const int64_t *d_lo, uint64_t *d_mat, uint64_t *d_belief,
                                  uint8_t *d_bvalid, hipStream_t stream)
{
    if (geom.nsegs == 0) return hipSuccess;
    const dim3 gs((uint32_t) geom.nsegs), gt(geom.nstreams);
    switch (tab.W) {
    case 1:
        hipLaunchKernelGGL(sre_k_nfa_wide_seg_matrix<1>, gs, dim3(64), 0, stream, tab, geom, d_lo, d_mat);
        hipLaunchKernelGGL(sre_k_nfa_wide_exact_entries<1>, gt, dim3(64), 0, stream, geom, d_sum, d_sets, d_lo, d_mat, d_belief, d_bvalid);
        break;
    case 2:
        hipLaunchKernelGGL(sre_k_nfa_wide_seg_matrix<2>, gs, dim3(128), 0, stream, tab, geom, d_lo, d_mat);
        hipLaunchKernelGGL(sre_k_nfa_wide_exact_entries<2>, gt, dim3(64), 0, stream, geom, d_sum, d_sets, d_lo, d_mat, d_belief, d_bvalid);
        break;
    default:
        hipLaunchKernelGGL(sre_k_nfa_wide_seg_matrix<4>, gs, dim3(256), 0, stream, tab, geom, d_lo, d_mat);
        hipLaunchKernelGGL(sre_k_nfa_wide_exact_entries<4>, gt, dim3(64), 0, stream, geom, d_sum, d_sets, d_lo, d_mat, d_belief, d_bvalid);
        break;
    }
    return hipGetLastError();
}
