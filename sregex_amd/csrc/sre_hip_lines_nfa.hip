/*
 * sre_hip_lines_nfa.hip — the short-line kernel of line mode on the bit-parallel NFA tier
 * (gfx950).
 *
 * The set kernels (sre_hip_nfa.hip) are built for long segments: a lane runs a fixed number of
 * staging rounds, only whole 64-byte tiles take the fast round, and every stream costs a summary,
 * the chain check and a geometry entry.  A log line is 100 bytes.  Here ONE LANE takes ONE LINE of
 * at most `lmax` bytes, consecutive lanes consecutive lines (a wave reads one contiguous span of the
 * buffer), from the line table alone:
 *
 *   input   each lane brings the 16-byte aligned pieces that cover the next 64 bytes of ITS line
 *           into its own LDS row (five pieces: the line starts anywhere in the first one) and reads
 *           them back at the line's alignment, four bytes a word.  Rows are private to their lane,
 *           so there is no barrier; the pieces of the next round are in flight while this one
 *           steps.  A piece may reach past the line, never past the 16-byte aligned extent of the
 *           buffer (the rule of sre_hip_tile.h): only pieces that hold a byte of the line are
 *           loaded.  No byte is loaded from global memory on its own, the ragged tail included.
 *   step    sre_lines_nfa.h, the text the CPU model compiles; tables in LDS, 64-bit words.
 *   output  the status block and the record the chain check would write for a verified stream
 *           (sre_k_nfa_verify_c), with the exact window from offset 0; and the line's entry in the
 *           work list of the window kernel (lo: 0 = a Pike line with an event, else -1).
 */
#include <hip/hip_runtime.h>
#include "sre_hip_lines.h"
#include "sre_hip_tile.h"
#include "sre_lines_nfa.h"

#define RC_DECLINED (-5)
#define RC_ERROR    (-1)

#define SRE_LNFA_BLOCK 256u
#define SRE_LNFA_ROWB  80u      /* five 16-byte pieces: 64 bytes at any alignment */

namespace {

typedef const __attribute__((address_space(1))) sre_u32x4 *gptr_x4;

/* the aligned pieces of round r (bytes 64r .. 64r + 63 of the line): piece q starts at row offset
 * 64r + 16q from the aligned address at or below the line's first byte; it is loaded when it holds a
 * byte of the line, which occupies the offsets [m, m + n) */
__device__ inline void
lnfa_fetch(sre_u32x4 (&regs)[5], uint64_t abase, uint32_t m, uint32_t n, uint32_t r)
{
#pragma unroll
    for (uint32_t q = 0; q < 5; q++) {
        const uint32_t off = 64u * r + 16u * q;
        sre_u32x4      v = {0, 0, 0, 0};
        if (off < m + n) v = *reinterpret_cast<gptr_x4>(abase + off);
        regs[q] = v;
    }
}

template <bool SA, bool LA>
__global__ __launch_bounds__(SRE_LNFA_BLOCK) void
sre_k_lines_nfa(sre_lnfa_t G, const uint8_t *__restrict__ buf, const uint64_t *__restrict__ ends, uint64_t i0, uint32_t nb,
                uint32_t short_lim, int thompson, sre_nfa_status_t *__restrict__ status, int64_t *__restrict__ records,
                uint32_t ovec_slots, int64_t *__restrict__ lo)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t tid = threadIdx.x;
    /* [accept][tab][expand][rows][kind] */
    const uint32_t nexp = LA ? (16u << G.xshift) : 0u;
    uint64_t      *acc_w = reinterpret_cast<uint64_t *>(lds);
    uint64_t      *tab_w = acc_w + 256;
    uint64_t      *exp_w = tab_w + G.ntab * 256u;
    uint8_t       *rows = reinterpret_cast<uint8_t *>(exp_w + nexp);
    uint8_t       *kind_w = rows + SRE_LNFA_BLOCK * SRE_LNFA_ROWB;
    acc_w[tid] = G.accept[tid];
    for (uint32_t i = tid; i < G.ntab * 256u; i += SRE_LNFA_BLOCK) tab_w[i] = G.tab[i];
    if (LA) {
        for (uint32_t i = tid; i < nexp; i += SRE_LNFA_BLOCK) exp_w[i] = G.expand[i];
        kind_w[tid] = G.kind[tid];
    }
    sre_lnfa_t T = G;
    T.sa = SA;
    T.la = LA;
    T.accept = acc_w;
    T.tab = tab_w;
    T.expand = exp_w;
    T.kind = kind_w;
    __syncthreads();                        /* the tables are complete; nothing below is shared */

    const uint32_t j = blockIdx.x * SRE_LNFA_BLOCK + tid;
    if (j >= nb) return;
    const uint64_t i = i0 + j;
    const uint64_t st = i == 0 ? 0 : ends[i - 1] + 1, len = ends[i] - st;
    if (len >= short_lim) {
        lo[j] = -1;                         /* a long line: the set pass has it */
        return;
    }
    const uint32_t n = (uint32_t) len;
    const uint64_t addr = (uint64_t) reinterpret_cast<uintptr_t>(buf) + st;
    const uint32_t m = (uint32_t) (addr & 15u);
    const uint64_t abase = addr - m;
    uint8_t       *row = rows + tid * SRE_LNFA_ROWB;
    const uint32_t *roww = reinterpret_cast<const uint32_t *>(row) + (m >> 2);
    const uint32_t sub = m & 3u;

    sre_lnfa_lane_t L;
    sre_lnfa_begin(T, L);
    sre_u32x4 regs[5];
    bool      hit = false;
    if (n) lnfa_fetch(regs, abase, m, n, 0);
    for (uint32_t r = 0; 64u * r < n && !hit; r++) {
#pragma unroll
        for (uint32_t q = 0; q < 5; q++) *reinterpret_cast<sre_u32x4 *>(row + 16u * q) = regs[q];
        if (64u * (r + 1) < n) lnfa_fetch(regs, abase, m, n, r + 1);
        const uint32_t left = n - 64u * r, cnt = left < 64u ? left : 64u;
        uint32_t       w0 = roww[0];
#pragma unroll 1
        for (uint32_t g = 0; 4u * g < cnt && !hit; g++) {
            const uint32_t w1 = roww[g + 1];
            const uint32_t w = __builtin_amdgcn_alignbyte(w1, w0, sub);
            w0 = w1;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++) {
                if (hit || 4u * g + b >= cnt) break;
                hit = sre_lnfa_byte(T, L, (w >> (8u * b)) & 0xffu, (int64_t) (64u * r + 4u * g + b)) != 0;
            }
        }
    }
    if (!hit) sre_lnfa_end(T, L, (int64_t) n);

    sre_nfa_status_t s;
    s.first_bad = 0;
    s.ev_pos = L.ev;
    s.clean_pos = 0;                        /* offset 0 of a line is clean, and the window from it is short */
    s.done = 1;
    s.clean_mode = 0;
    status[j] = s;
    int64_t *rec = records + (size_t) j * (2 + ovec_slots);
    for (uint32_t q = 0; q < ovec_slots; q++) rec[2 + q] = -1;
    if (L.ev < 0) {
        rec[0] = RC_DECLINED;
        rec[1] = 0;
    } else {
        rec[0] = thompson ? 0 : RC_ERROR;   /* Pike: the window kernel fills it in */
        rec[1] = 1;
    }
    lo[j] = (L.ev >= 0 && !thompson) ? 0 : -1;
}

typedef void (*lnfa_kernel_t)(sre_lnfa_t, const uint8_t *, const uint64_t *, uint64_t, uint32_t, uint32_t, int,
                              sre_nfa_status_t *, int64_t *, uint32_t, int64_t *);

lnfa_kernel_t
lnfa_kernel(const sre_lnfa_t &t)
{
    if (t.sa) return t.la ? sre_k_lines_nfa<true, true> : sre_k_lines_nfa<true, false>;
    return t.la ? sre_k_lines_nfa<false, true> : sre_k_lines_nfa<false, false>;
}

size_t
lnfa_lds_bytes(const sre_lnfa_t &t)
{
    return ((size_t) 256 + (size_t) t.ntab * 256 + (t.la ? (size_t) 16 << t.xshift : 0)) * sizeof(uint64_t)
           + (size_t) SRE_LNFA_BLOCK * SRE_LNFA_ROWB + 256;
}

}  // namespace

extern "C" sre_lnfa_t
sre_lines_nfa_tables_plain(const sre_nfa_tables_t *p)
{
    sre_lnfa_t t;
    sre_lnfa_set_plain(t, p->nslices, p->nassert, p->init[0], p->match_bits);
    t.accept = p->accept;
    t.tab = p->follow;
    t.expand = p->expand;
    t.kind = p->kind;
    return t;
}

extern "C" sre_lnfa_t
sre_lines_nfa_tables_sa(const sre_nfa_sa_tables_t *a)
{
    sre_lnfa_t t;
    uint32_t   hot[3];
    /* v_perm_b32 selector (sre_hip_nfa.h): 0..3 a byte of the low word, 4..7 of the high one (w64 only) */
    for (uint32_t q = 0; q < 3; q++) hot[q] = (a->perm >> (8 * q)) & (a->w64 ? 7u : 3u);
    /* the device's expansion table is compacted to the assertion bits, bits 0 .. nassert - 1 */
    sre_lnfa_set_sa(t, a->w64, a->carry, a->masked, a->evacc, a->nlut, hot, a->init[0], a->seed, a->self, a->shift_src,
                    a->match_bits, a->msrc, a->nassert, 0, a->nassert);
    t.accept = a->accept;
    t.tab = a->lut;
    t.expand = a->expand;
    t.kind = a->kind;
    return t;
}

extern "C" hipError_t
sre_launch_lines_nfa(sre_lnfa_t tab, const void *d_buf, const uint64_t *d_ends, uint64_t i0, uint32_t nb, uint32_t short_lim,
                     int thompson, sre_nfa_status_t *d_status, int64_t *d_records, uint32_t ovec_slots, int64_t *d_lo,
                     hipStream_t stream)
{
    if (nb == 0) return hipSuccess;
    lnfa_kernel_t kern = lnfa_kernel(tab);
    const size_t  lds = lnfa_lds_bytes(tab);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((nb + SRE_LNFA_BLOCK - 1) / SRE_LNFA_BLOCK), dim3(SRE_LNFA_BLOCK), lds, stream, tab,
                       static_cast<const uint8_t *>(d_buf), d_ends, i0, nb, short_lim, thompson, d_status, d_records,
                       ovec_slots, d_lo);
    return hipGetLastError();
}
