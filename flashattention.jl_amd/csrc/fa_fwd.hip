// fa_fwd.hip — dense flash-attention forward for gfx950 (MI355X, CDNA4).
//
// Replaces the blockwise forward dense_fa!(O, l, m, Q, K, V)
// (reference src/dense.jl:21-102).  Same result — O = softmax(τ Q Kᵀ) V with
// l = Σ exp(s − m), m = max s per query row (src/dense.jl:78-91) — computed
// MI355X-first rather than translated:
//
//  * one workgroup = 4 waves = 128 query rows of one batch slab; each wave owns
//    32 query rows for the whole key sweep (FA-2 order: O accumulates
//    unnormalised in fp32 registers and is divided by l once at the end; the
//    reference renormalises O every tile, src/dense.jl:89 — mathematically
//    equal, documented in DESIGN.md);
//  * key/value tiles of 64 tokens are staged HBM → registers → LDS (issue the
//    next tile's global loads before computing the current one, write them
//    after the tile's barrier: async-STAGE split);
//  * both tile products run on MFMA.  Scores are computed TRANSPOSED,
//    Sᵀ = K·Qᵀ (keys on accumulator rows / registers, queries on lanes), so the
//    fp32 score tile converted to bf16 is already the B operand of Oᵀ = Vᵀ·Pᵀ:
//    no LDS round trip for P, and row max / row sum are register reductions
//    plus one v_permlane32_swap;
//  * the reference layout keeps tokens contiguous, so the QKᵀ contraction
//    (over features) is strided: K tiles are read with the gfx950 transpose
//    read ds_read_b64_tr_b16 from an XOR-swizzled image (conflict-free), while
//    Vᵀ fragments (contraction over tokens, contiguous) are plain ds_read_b128
//    from a padded image (conflict-free);
//  * the key order inside each 16-key group of a K fragment is permuted
//    (bits 2 and 3 swapped) so that each lane's 8 bf16 P values cover 8
//    CONSECUTIVE keys, which makes the Vᵀ fragment one 16-byte read;
//  * exp2 with τ·log2(e) folded into one FMA; the running max is kept in raw
//    dot-product units and converted to natural-log units (m = τ·max) on store;
//  * ragged N / Nk: keys past Nk get score −inf (the reference CUDA kernel
//    zero-fills them, src/cuda/flash.jl:45 — Appendix A.4, not inherited),
//    queries past N are computed on zeros and not stored;
//  * head dims are padded (zero features) to the compiled class 32/64/128,
//    so the reference's own test shape (dqk = 12, dv = 6, test/test.jl:6-10)
//    runs on the same kernels;
//  * blockIdx is remapped so that all workgroups of one batch slab share an
//    XCD (its 4 MiB L2 then serves the slab's K/V re-reads).
//
// fp32 inputs use the exact-f32 MFMA v_mfma_f32_32x32x2_f32 (no TF32 on
// gfx950) with the same structure; that path exists for fp32 parity, the
// performance path is bf16 / fp16.
#include <type_traits>

#include "fa_common.h"
#include "fa_internal.h"
#include "fa_dense_plan.h"
#include "fa_fwd_params.h"
#include "../../include/fa_hip.h"

// Diagnostic hooks (tools/exp/fwd_stamp.hip; empty / 0 in the product build):
// FA_FWD_STAMP(k) records s_memtime / s_memrealtime at phase k of dense_fwd_tiled;
// FA_FWD_ABL selects timing-only ablations that compute WRONG results
// (1: no v_exp, 2: no row sum, 4: no row max).
#ifndef FA_FWD_STAMP
#define FA_FWD_STAMP(k)
#endif
#ifndef FA_FWD_ABL
#define FA_FWD_ABL 0
#endif
// FA_FWD_OAUX: cache-policy bits of the LDS-staged O stores (0 plain; A/B builds only)
#ifndef FA_FWD_OAUX
#define FA_FWD_OAUX 0
#endif

namespace fa {

thread_local int g_fwd_variant = kFwdAuto;   // a DenseFwdVariant (fa_dense_plan.h): benchmark knob, fa_debug_set_fwd_variant
thread_local int g_fwd_last_path = 0;   // fa_debug_fwd_last_path: 30 when the last fast launch ran fa_fwd_p4
thread_local int g_dense_fwd_last[3] = {-1, -1, -1};   // fa_debug_dense_last_launch: kernel, mask, pad
thread_local float g_fwd_rescale_log2 = kRescaleLog2;  // fa_debug_set_rescale_threshold (accuracy tests)
thread_local int g_causal_rev = 2;   // causal fast forward: launch order of the query blocks (fa_debug_set_causal_order)

// FwdParams: fa_fwd_params.h (shared with fa_fwd_pipe.hip)

constexpr int kBM = 128;  // query rows per workgroup (4 waves x 32)
constexpr int kBN = 64;   // keys per tile
constexpr int kThreads = 256;

// One 16-byte chunk (16/sizeof(T) elements) of row `row`, columns
// [col0, col0+EPC) of a row-major [nrows][ncols] slab; zero out of range.
template <class T>
__device__ __forceinline__ u32x4 load_chunk(const T* base, int row, int col0, int nrows,
                                            int ncols, bool fast) {
    constexpr int EPC = 16 / sizeof(T);
    u32x4 z = {0u, 0u, 0u, 0u};
    if (row >= nrows) return z;
    const T* src = base + (int64_t)row * ncols;
    if (fast) {
        if (col0 >= ncols) return z;
        return *(const u32x4*)(src + col0);
    }
    union {
        T e[EPC];
        u32x4 v;
    } u;
#pragma unroll
    for (int e = 0; e < EPC; ++e) u.e[e] = (col0 + e < ncols) ? src[col0 + e] : (T)0.0f;
    return u.v;
}

// {(T)(a * s), (T)(b * s)} as one dword, a in the low half.  For f16 hipcc compiles
// (T)(x * s) to one v_fma_mixlo_f16 (the product rounded once, where a multiply and a packed
// conversion round twice), so the pair is built from that instruction and its high-half
// twin: the bits then match the per-element stores of every other forward path.
template <class T>
__device__ __forceinline__ unsigned pack_scaled(float a, float b, float s) {
    if constexpr (std::is_same<T, f16>::value) {
        unsigned r;
        asm("v_fma_mixlo_f16 %0, %1, %3, 0\n\tv_fma_mixhi_f16 %0, %2, %3, 0" : "=&v"(r) : "v"(a), "v"(b), "v"(s));
        return r;
    } else {
        typedef T T2 __attribute__((ext_vector_type(2)));
        const T2 v = {(T)(a * s), (T)(b * s)};
        return __builtin_bit_cast(unsigned, v);
    }
}

// Causal launches (fa_causal_fwd): query i sees keys j <= i + off, off = Nk - N >= 0, so key 0
// is visible to every query and tile 0 is never skipped: the running max is finite after
// tile 0, a row masked whole in a later tile has tile max -inf, leaves the running max alone
// and gets P = exp2(-inf) = 0.  Tiles of `bn` keys a workgroup whose last query row is
// q_last needs: up to the last visible key of its last real query.
__device__ __forceinline__ int causal_ntiles(int nt, int q_last, int N, int off, int bn) {
    return min(nt, (min(q_last, N - 1) + off) / bn + 1);
}

// Local launches (fa_local_fwd; LOCAL instantiations, never CAUSAL and never SPLIT): query i sees
// keys i + off - wleft <= j <= i + off + wright, off = Nk - N >= 0.  The host clamps both
// sides to [0, Nk], and a side equal to Nk binds nowhere (i + off - Nk < 0, i + off + Nk >= Nk),
// so "no bound" needs no case of its own.  The key i + off exists, so every query sees a
// key; but with a left edge the first tile a wave computes can hide whole rows (their
// windows begin in the next tile), so a row's running max can still be -inf after a tile:
// the LOCAL bodies keep alpha = 1 and exponent offset 0 for such a row (P = exp2(-inf) = 0)
// instead of the NaN of -inf - -inf.  Tiles of `bn` keys [local_tile0, local_ntiles) of a
// workgroup with query rows q_first .. q_last.
__device__ __forceinline__ int local_tile0(int q_first, int off, int wleft, int bn) {
    return max(0, q_first + off - wleft) / bn;
}
__device__ __forceinline__ int local_ntiles(int nt, int q_last, int N, int off, int wright, int bn) {
    return min(nt, (min(q_last, N - 1) + off + wright) / bn + 1);
}

// Varlen launches (fa_varlen_fwd; kMaskVarlen instantiations, which are LOCAL bodies): slab b is
// the leading nq = q_lens[b] queries and nk = k_lens[b] keys of its (N, Nk) slab, off = nk - nq
// of either sign, the window clamped per slab (varlen_extents).  N and ldk stay the strides; nq,
// nk and off replace N, Nk and Nk - N in every bound.  What fa_local_fwd rules out now happens:
// a query i < nq sees no key when i + off + right < 0 (nk < nq under a right bound) or nk = 0,
// rows i >= nq are not queries at all, and a workgroup's tile range can be empty.  The rows
// without a key keep m = -inf, l = 0 and O = 0 through the LOCAL bodies (alpha = 1, exponent
// offset 0, P = exp2(-inf) = 0), and the epilogues store exactly that state: O = 0, l = 0,
// m = -inf, by a select on (row < nq and l > 0), never a division by l = 0.
// The last tile + 1 of a workgroup with query rows .. q_last: 0 when its last query's right
// limit is negative (local_ntiles divides a negative number towards zero).
__device__ __forceinline__ int varlen_ntiles(int nt, int q_last, int nq, int off, int wright, int bn) {
    const int hi = min(q_last, nq - 1) + off + wright;
    return hi < 0 ? 0 : min(nt, hi / bn + 1);
}
// The empty-row state of the rows [q0, q0 + rows) below N of slab b: O = 0, l = 0, m = -inf.
template <class T>
__device__ __forceinline__ void store_empty_rows(const FwdParams& p, int b, int q0, int rows, int nthreads) {
    const int N = p.N, dv = p.dv, n = min(rows, N - q0);
    T* const Ob = (T*)p.O + (int64_t)b * N * dv;
    for (int i = threadIdx.x; i < n * dv; i += nthreads) Ob[(int64_t)(i / n) * N + q0 + i % n] = (T)0.0f;
    for (int i = threadIdx.x; i < n; i += nthreads) {
        p.l[(int64_t)b * N + q0 + i] = 0.0f;
        p.m[(int64_t)b * N + q0 + i] = kNegInf;
    }
}

// N's and Nk's roles as BOUNDS in the masked bodies below (strides stay N, Nk / ldk): the launch's
// own extents, Nk - N and window, or under VARLEN the slab's (`ve`, varlen_extents).  Macros, not
// variables or lambdas: each expands to the parent's own expression at its use, so the dense,
// causal and local instantiations compile to the code they had (tools/asm_same.py).
#define FA_NKE (VARLEN ? ve.nk : Nk)
#define FA_OFF (VARLEN ? ve.off : (Nk - N))
#define FA_WL (VARLEN ? ve.left : p.wleft)
#define FA_WR (VARLEN ? ve.right : p.wright)

// --------------------------------------------------------------------------
// bf16 / fp16 forward (v_mfma_f32_32x32x16_{bf16,f16})
// --------------------------------------------------------------------------
template <class T, int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(kThreads) void dense_fwd_generic(FwdParams p) {
    constexpr bool CAUSAL = MASK == kMaskCausal, LOCAL = MASK == kMaskLocal || MASK == kMaskVarlen, VARLEN = MASK == kMaskVarlen;
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    constexpr int KROW = kBN * 2;       // K image: [D][64 keys], 128-B rows, 32-B chunk XOR swizzle
    constexpr int VROW = kBN * 2 + 16;  // V image: [DV][64 keys], 144-B rows (pad → conflict-free b128)
    constexpr int KCH = D * 8 / kThreads;   // 16-B K chunks per thread per tile
    constexpr int VCH = DV * 8 / kThreads;
    static_assert(KCH >= 1 && VCH >= 1, "head dim class too small");
    __shared__ __attribute__((aligned(16))) char smem[D * KROW + DV * VROW];
    char* const klds = smem;
    char* const vlds = smem + D * KROW;

    const int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int b = lid / p.nqb;
    const int qb = lid - b * p.nqb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int N = p.N, Nk = p.Nk, d = p.d, dv = p.dv;
    const T* __restrict__ Qb = (const T*)p.Q + (int64_t)b * N * d;
    const T* __restrict__ Kb = (const T*)p.K + (int64_t)b * Nk * d;
    const T* __restrict__ Vb = (const T*)p.V + (int64_t)b * Nk * dv;
    const bool fast = p.fast != 0;
    // the slab's extents in every bound below (VARLEN: per slab, varlen_ntiles' comment; N and Nk
    // stay the strides); a workgroup with no query, or whose queries see no key, stores the
    // empty-row state and leaves before any load or barrier (block-uniform)
    VarlenExt ve{};
    if constexpr (VARLEN) {
        ve = varlen_extents(fwd_q_lens(p), fwd_k_lens(p), b, N, Nk, p.wleft, p.wright);
        if (qb * kBM >= ve.nq || local_tile0(qb * kBM, ve.off, ve.left, kBN) >=
                                     varlen_ntiles((ve.nk + kBN - 1) / kBN, qb * kBM + kBM - 1, ve.nq, ve.off, ve.right, kBN)) {
            store_empty_rows<T>(p, b, qb * kBM, kBM, kThreads);
            return;
        }
    }

    // Q^T fragments (B operand of S^T = K Q^T), kept in registers:
    // lane (r, h), k-step s holds Q[query qi][features 16s+8h .. 16s+8h+7].
    const int qi = qb * kBM + wave * 32 + r;
    F8 qf[D / 16];
#pragma unroll
    for (int s = 0; s < D / 16; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int f = 16 * s + 8 * h + e;
            qf[s][e] = (qi < N && f < d) ? Qb[(int64_t)f * N + qi] : (T)0.0f;
        }

    // Per-lane LDS offsets of the transposed K reads.  16-lane group g: kh = g&1
    // selects keys 0-15 / 16-31 of a 32-key block; lane 4q+pp supplies feature
    // row q and the 4-key chunk sigma(pp) (sigma swaps 1 and 2 → lane r ends up
    // holding key pi(r) = r with bits 2 and 3 swapped).
    const int g = lane >> 4, kh = g & 1, ii = lane & 15, qq = ii >> 2, pp = ii & 3;
    const int sig = (pp == 1) ? 2 : (pp == 2) ? 1 : pp;
    int koff[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
        koff[kb] = (8 * h + qq) * KROW + (((kb * 2 + kh) ^ (((qq >> 1) & 1) << 1)) * 32) + 8 * sig;
    const int voff = r * VROW + 16 * h;  // + cb*32*VROW + (kb*32+16s)*2

    f32x16 oacc[DV / 32];
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) oacc[cb][x] = 0.0f;
    float m_run = kNegInf, l_run = 0.0f;
    const float c = p.scale_log2;

    u32x4 kreg[KCH], vreg[VCH];
    auto gload = [&](int j) {
        const int key0 = j * kBN;
#pragma unroll
        for (int it = 0; it < KCH; ++it) {
            const int ch = tid + kThreads * it;
            kreg[it] = load_chunk<T>(Kb, ch >> 3, key0 + (ch & 7) * 8, d, Nk, fast);
        }
#pragma unroll
        for (int it = 0; it < VCH; ++it) {
            const int ch = tid + kThreads * it;
            vreg[it] = load_chunk<T>(Vb, ch >> 3, key0 + (ch & 7) * 8, dv, Nk, fast);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int it = 0; it < KCH; ++it) {
            const int ch = tid + kThreads * it, f = ch >> 3, pc = ch & 7;
            const int off = f * KROW + (((pc >> 1) ^ (((f >> 1) & 1) << 1)) * 32) + (pc & 1) * 16;
            *(u32x4*)(klds + off) = kreg[it];
        }
#pragma unroll
        for (int it = 0; it < VCH; ++it) {
            const int ch = tid + kThreads * it;
            *(u32x4*)(vlds + (ch >> 3) * VROW + (ch & 7) * 16) = vreg[it];
        }
    };

    int ntiles = (FA_NKE + kBN - 1) / kBN;
    if constexpr (CAUSAL)   // tiles up to the block's last query's last visible key (causal_ntiles)
        ntiles = causal_ntiles(ntiles, qb * kBM + kBM - 1, N, (Nk - N), kBN);
    int jbeg = 0;
    if constexpr (LOCAL) {   // the tiles between the block's first query's left edge and its last query's right edge
        jbeg = local_tile0(qb * kBM, FA_OFF, FA_WL, kBN);
        if constexpr (VARLEN) ntiles = varlen_ntiles(ntiles, qb * kBM + kBM - 1, ve.nq, ve.off, ve.right, kBN);
        else ntiles = local_ntiles(ntiles, qb * kBM + kBM - 1, N, Nk - N, p.wright, kBN);
    }
    gload(jbeg);
    lstore();
    __syncthreads();

    for (int j = jbeg; j < ntiles; ++j) {
        const bool more = j + 1 < ntiles;
        if (more) gload(j + 1);

        // ---- S^T = K Q^T : two 32-key accumulator blocks ----
        f32x16 sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int x = 0; x < 16; ++x) sacc[kb][x] = 0.0f;
#pragma unroll
            for (int s = 0; s < D / 16; ++s) {
                const char* a = klds + koff[kb] + 16 * s * KROW;
                const F4 lo = __builtin_bit_cast(F4, ds_read_tr16(a));
                const F4 hi = __builtin_bit_cast(F4, ds_read_tr16(a + 4 * KROW));
                const F8 af = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                sacc[kb] = mfma32x32x16(af, qf[s], sacc[kb]);
            }
        }

        // ---- mask keys >= Nk (last tile only) ----
        const int key0 = j * kBN;
        if (key0 + kBN > FA_NKE) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int kt = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
                    if (key0 + kt >= FA_NKE) sacc[kb][x] = kNegInf;
                }
        }
        if constexpr (CAUSAL) {   // keys past the lane's query + off (tiles that straddle the wave's diagonal)
            if (key0 + kBN - 1 > qb * kBM + wave * 32 + (Nk - N)) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int kt = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
                        if (key0 + kt > qi + (Nk - N)) sacc[kb][x] = kNegInf;
                    }
            }
        }
        if constexpr (LOCAL) {   // after the ragged mask; only on tiles that straddle an edge of the wave's band
            const int w0 = qb * kBM + wave * 32 + FA_OFF;
            if (key0 + kBN - 1 > w0 + FA_WR || key0 < w0 + 31 - FA_WL) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int kt = key0 + kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
                        if (kt > qi + FA_OFF + FA_WR || kt < qi + FA_OFF - FA_WL) sacc[kb][x] = kNegInf;
                    }
            }
        }

        // ---- online softmax (raw dot-product units; exp2 with folded scale) ----
        float mt = kNegInf;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) mt = fmaxf(mt, sacc[kb][x]);
        mt = swap_halves_max(mt);
        const float m_new = fmaxf(m_run, mt);
        float alpha = exp2_fast((m_run - m_new) * c);
        const float mc = m_new * c;
        // LOCAL: a row with no visible key so far keeps alpha = 1 and subtracts 0 (no -inf - -inf,
        // local_tile0's comment); the exponent is (s - m) c, exactly 0 for the row's max, so that
        // a query with one visible key gets l = 1 and that key's V bit for bit (dense_fwd_tiled)
        float msub = 0.0f;
        if constexpr (LOCAL) {
            msub = m_new == kNegInf ? 0.0f : m_new;
            if (m_new == kNegInf) alpha = 1.0f;
        }
        float ls = 0.0f;
        F8 pf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pv = exp2_fast(LOCAL ? (sacc[kb][x] - msub) * c : fmaf(sacc[kb][x], c, -mc));
                ls += pv;
                pf[kb][x >> 3][x & 7] = (T)pv;
            }
        l_run = l_run * alpha + ls;
        m_run = m_new;
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) oacc[cb][x] *= alpha;

        // ---- O^T += V^T P^T ----
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const F8 va = *(const F8*)(vlds + voff + cb * 32 * VROW + (kb * 32 + 16 * s) * 2);
                    oacc[cb] = mfma32x32x16(va, pf[kb][s], oacc[cb]);
                }

        __syncthreads();
        if (more) {
            lstore();
            __syncthreads();
        }
    }

    // ---- epilogue: O = O / l ; l, m in natural-log units ----
    const float lt = swap_halves_sum(l_run);
    const float inv = 1.0f / lt;
    if constexpr (VARLEN) {   // a row past nq or without a key: O = 0, l = 0, m = -inf, by select
        if (qi < N) {
            const bool live = qi < ve.nq && lt > 0.0f;
            T* Ob = (T*)p.O + (int64_t)b * N * dv;
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int cc = cb * 32 + acc_row(x, h);
                    if (cc < dv) Ob[(int64_t)cc * N + qi] = live ? (T)(oacc[cb][x] * inv) : (T)0.0f;
                }
            if (h == 0) {
                p.m[(int64_t)b * N + qi] = live ? m_run * p.scale : kNegInf;
                p.l[(int64_t)b * N + qi] = live ? lt : 0.0f;
            }
        }
        return;
    }
    if (qi < N) {
        T* Ob = (T*)p.O + (int64_t)b * N * dv;
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int cc = cb * 32 + acc_row(x, h);
                if (cc < dv) Ob[(int64_t)cc * N + qi] = (T)(oacc[cb][x] * inv);
            }
        if (h == 0) {
            p.m[(int64_t)b * N + qi] = m_run * p.scale;
            p.l[(int64_t)b * N + qi] = lt;
        }
    }
}

// --------------------------------------------------------------------------
// fp32 forward (exact f32 MFMA v_mfma_f32_32x32x2_f32)
// --------------------------------------------------------------------------
template <int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(kThreads) void dense_fwd_generic_f32(FwdParams p) {
    constexpr bool CAUSAL = MASK == kMaskCausal, LOCAL = MASK == kMaskLocal || MASK == kMaskVarlen, VARLEN = MASK == kMaskVarlen;
    constexpr int KROWF = kBN;       // K image [D][64] floats
    constexpr int VROWF = kBN + 1;   // V image [DV][65] floats (pad → conflict-free column reads)
    constexpr int KCH = D * 16 / kThreads;
    constexpr int VCH = DV * 16 / kThreads;
    static_assert(KCH >= 1 && VCH >= 1, "head dim class too small");
    __shared__ __attribute__((aligned(16))) float smem[D * KROWF + DV * VROWF];
    float* const klds = smem;
    float* const vlds = smem + D * KROWF;

    const int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int b = lid / p.nqb;
    const int qb = lid - b * p.nqb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int N = p.N, Nk = p.Nk, d = p.d, dv = p.dv;
    const float* __restrict__ Qb = (const float*)p.Q + (int64_t)b * N * d;
    const float* __restrict__ Kb = (const float*)p.K + (int64_t)b * Nk * d;
    const float* __restrict__ Vb = (const float*)p.V + (int64_t)b * Nk * dv;
    const bool fast = p.fast != 0;
    // the slab's extents in every bound below (VARLEN: per slab, varlen_ntiles' comment; N and Nk
    // stay the strides); a workgroup with no query, or whose queries see no key, stores the
    // empty-row state and leaves before any load or barrier (block-uniform)
    VarlenExt ve{};
    if constexpr (VARLEN) {
        ve = varlen_extents(fwd_q_lens(p), fwd_k_lens(p), b, N, Nk, p.wleft, p.wright);
        if (qb * kBM >= ve.nq || local_tile0(qb * kBM, ve.off, ve.left, kBN) >=
                                     varlen_ntiles((ve.nk + kBN - 1) / kBN, qb * kBM + kBM - 1, ve.nq, ve.off, ve.right, kBN)) {
            store_empty_rows<float>(p, b, qb * kBM, kBM, kThreads);
            return;
        }
    }

    const int qi = qb * kBM + wave * 32 + r;
    float qf[D / 2];  // lane (r, h), step t: Q[qi][feature 2t+h]
#pragma unroll
    for (int t = 0; t < D / 2; ++t) {
        const int f = 2 * t + h;
        qf[t] = (qi < N && f < d) ? Qb[(int64_t)f * N + qi] : 0.0f;
    }

    f32x16 oacc[DV / 32];
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) oacc[cb][x] = 0.0f;
    float m_run = kNegInf, l_run = 0.0f;
    const float c = p.scale_log2;

    u32x4 kreg[KCH], vreg[VCH];
    auto gload = [&](int j) {
        const int key0 = j * kBN;
#pragma unroll
        for (int it = 0; it < KCH; ++it) {
            const int ch = tid + kThreads * it;
            kreg[it] = load_chunk<float>(Kb, ch >> 4, key0 + (ch & 15) * 4, d, Nk, fast);
        }
#pragma unroll
        for (int it = 0; it < VCH; ++it) {
            const int ch = tid + kThreads * it;
            vreg[it] = load_chunk<float>(Vb, ch >> 4, key0 + (ch & 15) * 4, dv, Nk, fast);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int it = 0; it < KCH; ++it) {
            const int ch = tid + kThreads * it;
            *(u32x4*)(klds + (ch >> 4) * KROWF + (ch & 15) * 4) = kreg[it];
        }
#pragma unroll
        for (int it = 0; it < VCH; ++it) {
            const int ch = tid + kThreads * it;
            float* dst = vlds + (ch >> 4) * VROWF + (ch & 15) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e] = __uint_as_float(vreg[it][e]);
        }
    };

    int ntiles = (FA_NKE + kBN - 1) / kBN;
    if constexpr (CAUSAL)   // tiles up to the block's last query's last visible key (causal_ntiles)
        ntiles = causal_ntiles(ntiles, qb * kBM + kBM - 1, N, (Nk - N), kBN);
    int jbeg = 0;
    if constexpr (LOCAL) {   // the tiles between the block's first query's left edge and its last query's right edge
        jbeg = local_tile0(qb * kBM, FA_OFF, FA_WL, kBN);
        if constexpr (VARLEN) ntiles = varlen_ntiles(ntiles, qb * kBM + kBM - 1, ve.nq, ve.off, ve.right, kBN);
        else ntiles = local_ntiles(ntiles, qb * kBM + kBM - 1, N, Nk - N, p.wright, kBN);
    }
    gload(jbeg);
    lstore();
    __syncthreads();

    for (int j = jbeg; j < ntiles; ++j) {
        const bool more = j + 1 < ntiles;
        if (more) gload(j + 1);

        f32x16 sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int x = 0; x < 16; ++x) sacc[kb][x] = 0.0f;
#pragma unroll
            for (int t = 0; t < D / 2; ++t)
                sacc[kb] = mfma32x32x2(klds[(2 * t + h) * KROWF + kb * 32 + r], qf[t], sacc[kb]);
        }

        const int key0 = j * kBN;
        if (key0 + kBN > FA_NKE) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int x = 0; x < 16; ++x)
                    if (key0 + kb * 32 + acc_row(x, h) >= FA_NKE) sacc[kb][x] = kNegInf;
        }
        if constexpr (CAUSAL) {
            if (key0 + kBN - 1 > qb * kBM + wave * 32 + (Nk - N)) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int x = 0; x < 16; ++x)
                        if (key0 + kb * 32 + acc_row(x, h) > qi + (Nk - N)) sacc[kb][x] = kNegInf;
            }
        }
        if constexpr (LOCAL) {
            const int w0 = qb * kBM + wave * 32 + FA_OFF;
            if (key0 + kBN - 1 > w0 + FA_WR || key0 < w0 + 31 - FA_WL) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int kt = key0 + kb * 32 + acc_row(x, h);
                        if (kt > qi + FA_OFF + FA_WR || kt < qi + FA_OFF - FA_WL) sacc[kb][x] = kNegInf;
                    }
            }
        }

        float mt = kNegInf;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) mt = fmaxf(mt, sacc[kb][x]);
        mt = swap_halves_max(mt);
        const float m_new = fmaxf(m_run, mt);
        float alpha = exp2_fast((m_run - m_new) * c);
        const float mc = m_new * c;
        // LOCAL: a row with no visible key so far keeps alpha = 1 and subtracts 0 (no -inf - -inf,
        // local_tile0's comment); the exponent is (s - m) c, exactly 0 for the row's max, so that
        // a query with one visible key gets l = 1 and that key's V bit for bit (dense_fwd_tiled)
        float msub = 0.0f;
        if constexpr (LOCAL) {
            msub = m_new == kNegInf ? 0.0f : m_new;
            if (m_new == kNegInf) alpha = 1.0f;
        }
        float ls = 0.0f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pv = exp2_fast(LOCAL ? (sacc[kb][x] - msub) * c : fmaf(sacc[kb][x], c, -mc));
                ls += pv;
                sacc[kb][x] = pv;
            }
        l_run = l_run * alpha + ls;
        m_run = m_new;
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) oacc[cb][x] *= alpha;

#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int x = 0; x < 16; ++x)
                    oacc[cb] = mfma32x32x2(vlds[(cb * 32 + r) * VROWF + kb * 32 + acc_row(x, h)],
                                           sacc[kb][x], oacc[cb]);

        __syncthreads();
        if (more) {
            lstore();
            __syncthreads();
        }
    }

    const float lt = swap_halves_sum(l_run);
    const float inv = 1.0f / lt;
    if constexpr (VARLEN) {   // a row past nq or without a key: O = 0, l = 0, m = -inf, by select
        if (qi < N) {
            const bool live = qi < ve.nq && lt > 0.0f;
            float* Ob = (float*)p.O + (int64_t)b * N * dv;
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int cc = cb * 32 + acc_row(x, h);
                    if (cc < dv) Ob[(int64_t)cc * N + qi] = live ? (float)(oacc[cb][x] * inv) : (float)0.0f;
                }
            if (h == 0) {
                p.m[(int64_t)b * N + qi] = live ? m_run * p.scale : kNegInf;
                p.l[(int64_t)b * N + qi] = live ? lt : 0.0f;
            }
        }
        return;
    }
    if (qi < N) {
        float* Ob = (float*)p.O + (int64_t)b * N * dv;
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int cc = cb * 32 + acc_row(x, h);
                if (cc < dv) Ob[(int64_t)cc * N + qi] = oacc[cb][x] * inv;
            }
        if (h == 0) {
            p.m[(int64_t)b * N + qi] = m_run * p.scale;
            p.l[(int64_t)b * N + qi] = lt;
        }
    }
}

// --------------------------------------------------------------------------
// bf16 / fp16 fast path: K/V rows 16-B aligned, Nk % 8 == 0, slab < 4 GiB.
//
// Differences from the generic kernel:
//  * every global access is an unconditional buffer load through a per-slab
//    descriptor (num_records = slab bytes): reads of padded feature rows
//    (f >= d) fall outside the slab and return 0, so the loop body has no
//    divergent control flow and hipcc keeps the tile loads in flight across the
//    whole compute phase (no vmcnt(0) next to the issue);
//  * LDS is double-buffered: tile j+1's registers are written into the other
//    buffer right after tile j's compute, one barrier per tile;
//  * lazy rescaling: the running max used for the exponentials (m_used) is
//    only raised when a tile's max exceeds it by more than kRescaleLog2 (in
//    log2 units), so the O / l rescale is a rare, wave-uniform branch; P is then
//    bounded by 2^kRescaleLog2 (bf16 keeps its relative precision), and the
//    exact max is tracked separately for the returned m (and l is converted to
//    it at the end).
// --------------------------------------------------------------------------

// --------------------------------------------------------------------------
// bf16 / fp16 fast path, generalised geometry: NW waves x 32 query rows per
// workgroup, BN keys per tile (the v2 structure: double-buffered LDS, one
// barrier per tile, lazy rescale, branch-free buffer loads).  The partial-tile
// V zeroing runs only on the last tile.
// --------------------------------------------------------------------------
//
// CAUSAL (fa_causal_fwd; never with SPLIT): the workgroup's tiles end at its last query's
// last visible key; loads, LDS stores and the barrier stay workgroup-uniform; a wave whose
// last query is before a tile's first key skips that tile's compute, and the per-element
// select runs only on tiles that straddle the wave's diagonal (both tests wave-uniform).
//
// LOCAL (fa_local_fwd; never with SPLIT or CAUSAL; the window is in p.wleft / p.wright, see
// local_tile0): the workgroup's tiles run from its first query's left edge to its last query's
// right edge, in the default launch order (a bounded band makes the blocks near-uniform); a
// wave computes a tile only if some query of it sees the tile, and selects on the tiles that
// straddle its left or its right diagonal (all tests wave-uniform; both edges and the
// ragged mask can meet in one tile).  A row whose window begins after the wave's first tile
// keeps m_used = -inf there: the rescale is row-local as for CAUSAL, with alpha = 1 for a row
// that does not move, and the exponent's offset is 0 while m_used = -inf (P = 0).
template <class T, int D, int DV, int NW, int BN, int NQB, bool SPLIT = false, bool WIDE = false, DenseMask MASK = kMaskNone>
__device__ __forceinline__ void dense_fwd_tiled(const FwdParams& p) {
    constexpr bool CAUSAL = MASK == kMaskCausal, LOCAL = MASK == kMaskLocal || MASK == kMaskVarlen, VARLEN = MASK == kMaskVarlen;
    static_assert(!(CAUSAL && SPLIT), "causal launches never split the keys");
    static_assert(!(LOCAL && SPLIT), "local launches never split the keys");
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    constexpr int NTH = 64 * NW;
    constexpr int BM = 32 * NW * NQB;           // query rows per workgroup
    constexpr int NKB = BN / 32;                // 32-key accumulator blocks per tile
    constexpr int KROW = BN * 2;                // K image row (bytes)
    constexpr int VROW = BN * 2 + 16;           // V image row (bytes), padded
    constexpr int KBYTES = D * KROW, VBYTES = DV * VROW, STAGE = KBYTES + VBYTES;
    constexpr int CPR = BN / 8;                 // 16-B chunks per row
    constexpr int KTOT = D * CPR, VTOT = DV * CPR;   // 16-B chunks per tile
    constexpr int KCH = (KTOT + NTH - 1) / NTH;
    constexpr int VCH = (VTOT + NTH - 1) / NTH;
    static_assert(KTOT % NTH == 0 || KTOT < NTH, "tile split");
    static_assert(VTOT % NTH == 0 || VTOT < NTH, "tile split");
    // WIDE: Q arrives by LDS-DMA (16-B coalesced loads, no VGPRs) into a [feature][BM
    // tokens] image read back by transposed reads, and O leaves through the same image
    // as 16-B row stores, instead of 2-byte gathers / scatters (one per feature and
    // query).  The 32-B blocks of image row f are XOR-ed with (f & 3) | (bit 2 of f) << 2:
    // conflict-free transposed reads (4 rows), paired b32 writes (rows f, f + 2 per 32-lane
    // group) and b128 reads of the epilogue.
    constexpr int ROWB = BM * 2;
    constexpr int QOOFF = (2 * STAGE + 16 + 255) & ~255;
    constexpr int QOB = WIDE ? (D > DV ? D : DV) * ROWB : 0;
    __shared__ __attribute__((aligned(256))) char smem[QOOFF + QOB];   // +16 past the stages: dump slot
    auto qo_at = [](int f, int byteoff) {
        const int X = (f & 3) | (((f >> 2) & 1) << 2);
        return f * ROWB + (((byteoff >> 5) ^ X) << 5) + (byteoff & 31);
    };
    char* const qoimg = smem + QOOFF;

    // K image swizzle: XOR the 32-B chunk index so that the 4 feature rows a
    // transposed read touches land on distinct banks (128-B rows: rows f and
    // f+1 are 32 banks apart already; 256-B rows need a 2-bit XOR).
    auto kswz = [](int f) { return BN == 64 ? (((f >> 1) & 1) << 1) : ((f & 3) << 1); };

    FA_FWD_STAMP(0);
    int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int split = SPLIT ? lid % p.nsplit : 0;
    if (SPLIT) lid /= p.nsplit;
    if constexpr (CAUSAL) {   // launch order of the query blocks (A/B in DESIGN §2.7)
        if (p.causal & 4) {
            // block-major inside an XCD's share of the grid (consecutive ids, xcd_remap): the
            // last (heaviest) block of each of its slabs first, then the one before, ...
            const int per = p.total_wg >> 3, ns = per / p.nqb;
            const int base = lid / per * per, loc = lid - base;
            lid = base + (loc % ns) * p.nqb + (p.nqb - 1 - loc / ns);
        } else if (p.causal & 2) {   // slab-major, a slab's heaviest block first
            lid = lid / p.nqb * p.nqb + (p.nqb - 1 - lid % p.nqb);
        }
    }
    const int b = lid / p.nqb;
    const int qb = lid - b * p.nqb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int N = p.N, Nk = p.Nk, d = p.d, dv = p.dv;
    // the slab's extents in every bound below (VARLEN: the two lengths come by scalar loads, b is
    // uniform; varlen_ntiles' comment).  A workgroup whose first row is >= nq, or whose tile range
    // [jt0, jt1) is empty (none of its queries sees a key), stores the empty-row state of its
    // rows below N and leaves here: before any K/V load, LDS store or barrier, block-uniformly, so
    // the pipeline below always has a tile.
    VarlenExt ve{};
    if constexpr (VARLEN) {
        ve = varlen_extents(fwd_q_lens(p), fwd_k_lens(p), b, N, Nk, p.wleft, p.wright);
        if (qb * BM >= ve.nq || local_tile0(qb * BM, ve.off, ve.left, BN) >=
                                    varlen_ntiles((ve.nk + BN - 1) / BN, qb * BM + BM - 1, ve.nq, ve.off, ve.right, BN)) {
            store_empty_rows<T>(p, b, qb * BM, BM, NTH);
            return;
        }
    }
    const auto qrs = slab_rsrc((const T*)p.Q + (int64_t)b * N * d, (uint32_t)(N * d * (int)sizeof(T)));
    const int ldk = p.ldk;
    const auto krs = slab_rsrc((const T*)p.K + (int64_t)b * ldk * d, (uint32_t)(ldk * d * (int)sizeof(T)));
    const auto vrs = slab_rsrc((const T*)p.V + (int64_t)b * ldk * dv, (uint32_t)(ldk * dv * (int)sizeof(T)));

    // The first K/V tile's loads go out before anything else (ahead of the Q image's DMA, so
    // that they are not queued behind it); only what feeds them is computed first.
    // Threads past the chunk count (small head dims at 8 waves) load an
    // out-of-range offset (→ 0) and store into a scratch slot past the tile.
    const bool kact = KTOT >= NTH || tid < KTOT, vact = VTOT >= NTH || tid < VTOT;
    int kgo[KCH], vgo[VCH];
#pragma unroll
    for (int it = 0; it < KCH; ++it) {
        const int ch = tid + NTH * it, f = ch / CPR, pc = ch % CPR;
        kgo[it] = kact ? (f * ldk + pc * 8) * 2 : 0x7FFFFFF0;
    }
#pragma unroll
    for (int it = 0; it < VCH; ++it) {
        const int ch = tid + NTH * it, f = ch / CPR, pc = ch % CPR;
        vgo[it] = vact ? (f * ldk + pc * 8) * 2 : 0x7FFFFFF0;
    }
    const int NT = (FA_NKE + BN - 1) / BN;
    const bool ragged = (FA_NKE % BN) != 0;
    // key tiles [jt0, jt1) of this workgroup (all tiles unless split-KV)
    // (causal: up to the last tile any of the workgroup's queries sees)
    // (local: from the first query's left edge to the last query's right edge; jt0 < jt1)
    const int jt0 = SPLIT ? split * p.tps : LOCAL ? local_tile0(qb * BM, FA_OFF, FA_WL, BN) : 0;
    int jt1 = SPLIT ? min(NT, jt0 + p.tps) : NT;
    if constexpr (CAUSAL) jt1 = causal_ntiles(NT, qb * BM + BM - 1, N, (Nk - N), BN);
    if constexpr (LOCAL && !VARLEN) jt1 = local_ntiles(NT, qb * BM + BM - 1, N, Nk - N, p.wright, BN);
    if constexpr (VARLEN) jt1 = varlen_ntiles(NT, qb * BM + BM - 1, ve.nq, ve.off, ve.right, BN);

    u32x4 kreg[KCH], vreg[VCH];
    auto gload = [&](int j) {
        const int kb0 = j * BN * 2;
#pragma unroll
        for (int it = 0; it < KCH; ++it) kreg[it] = __builtin_amdgcn_raw_buffer_load_b128(krs, kgo[it] + kb0, 0, 0);
#pragma unroll
        for (int it = 0; it < VCH; ++it) vreg[it] = __builtin_amdgcn_raw_buffer_load_b128(vrs, vgo[it] + kb0, 0, 0);
    };
    gload(jt0);
    FA_FWD_STAMP(5);

    int qiv[NQB];
    F8 qf[NQB][D / 16];
    if constexpr (WIDE) {
        static_assert(D * ROWB % (1024 * NW) == 0, "Q image DMA split");
#pragma unroll
        for (int it = 0; it < D * ROWB / 1024 / NW; ++it) {
            const int k = it * NW + wave;
            const int P = k * 1024 + lane * 16, f = P / ROWB, pb = P - f * ROWB;
            const int X = (f & 3) | (((f >> 2) & 1) << 2);
            const int lb = (((pb >> 5) ^ X) << 5) + (pb & 31);     // logical byte = 2 * token
            __builtin_amdgcn_raw_ptr_buffer_load_lds(qrs, (__attribute__((address_space(3))) void*)(qoimg + k * 1024), 16,
                                                     (f * N + qb * BM) * 2 + lb, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < NQB; ++u) qiv[u] = qb * BM + (wave * NQB + u) * 32 + r;
        FA_FWD_STAMP(4);
    }
#pragma unroll
    for (int u = 0; u < NQB && !WIDE; ++u) {
        qiv[u] = qb * BM + (wave * NQB + u) * 32 + r;
#pragma unroll
        for (int s = 0; s < D / 16; ++s)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int f = 16 * s + 8 * h + e;
                const unsigned short w = __builtin_amdgcn_raw_buffer_load_b16(qrs, (f * N + qiv[u]) * 2, 0, 0);
                qf[u][s][e] = __builtin_bit_cast(T, w);
            }
    }

    const int g = lane >> 4, kh = g & 1, ii = lane & 15, qq = ii >> 2, pp = ii & 3;
    const int sig = (pp == 1) ? 2 : (pp == 2) ? 1 : pp;
    int koff[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
        koff[kb] = (8 * h + qq) * KROW + (((kb * 2 + kh) ^ kswz(qq)) * 32) + 8 * sig;
    const int voff = r * VROW + 16 * h;

    int kso[KCH], vso[VCH];
#pragma unroll
    for (int it = 0; it < KCH; ++it) {
        const int ch = tid + NTH * it, f = ch / CPR, pc = ch % CPR;
        kso[it] = kact ? f * KROW + (((pc >> 1) ^ kswz(f)) * 32) + (pc & 1) * 16 : 2 * STAGE;
    }
#pragma unroll
    for (int it = 0; it < VCH; ++it) {
        const int ch = tid + NTH * it, f = ch / CPR, pc = ch % CPR;
        vso[it] = vact ? f * VROW + pc * 16 : 2 * STAGE - KBYTES;
    }

    f32x16 oacc[NQB][DV / 32];
#pragma unroll
    for (int u = 0; u < NQB; ++u)
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) oacc[u][cb][x] = 0.0f;
    float m_used[NQB], m_true[NQB], l_run[NQB];
#pragma unroll
    for (int u = 0; u < NQB; ++u) { m_used[u] = kNegInf; m_true[u] = kNegInf; l_run[u] = 0.0f; }
    const float c = p.scale_log2;
    const float thr_raw = p.rescale_log2 / c;

    auto lstore = [&](char* buf, int j) {
        if (ragged && j == NT - 1) {   // keys >= Nk read the next feature row: zero V there
#pragma unroll
            for (int it = 0; it < VCH; ++it) {
                const int ch = tid + NTH * it;
                if (j * BN + (ch % CPR) * 8 >= FA_NKE) vreg[it] = u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int it = 0; it < KCH; ++it) *(u32x4*)((kact ? buf : smem) + kso[it]) = kreg[it];
#pragma unroll
        for (int it = 0; it < VCH; ++it) *(u32x4*)((vact ? buf : smem) + KBYTES + vso[it]) = vreg[it];
    };

    auto compute = [&](const char* klds, const char* vlds, int j) {
        f32x16 sacc[NQB][NKB];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
            for (int u = 0; u < NQB; ++u)
#pragma unroll
                for (int x = 0; x < 16; ++x) sacc[u][kb][x] = 0.0f;
#pragma unroll
            for (int s = 0; s < D / 16; ++s) {
                const char* a = klds + koff[kb] + 16 * s * KROW;
                const F4 lo = __builtin_bit_cast(F4, ds_read_tr16(a));
                const F4 hi = __builtin_bit_cast(F4, ds_read_tr16(a + 4 * KROW));
                const F8 af = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int u = 0; u < NQB; ++u) sacc[u][kb] = mfma32x32x16(af, qf[u][s], sacc[u][kb]);
            }
        }
        if (ragged && j == NT - 1) {
            const int key0 = j * BN;
#pragma unroll
            for (int u = 0; u < NQB; ++u)
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int kt = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
                        if (key0 + kt >= FA_NKE) sacc[u][kb][x] = kNegInf;
                    }
        }
        if constexpr (CAUSAL) {
            // a select, not a bias; only on tiles with a key past the wave's first query's limit
            // (it can meet the ragged mask above in one tile)
            // w0: the key limit (query row + off) of the wave's first query, relative to the tile, in
            // a scalar register; the lane's part (r - 8 h) is rebuilt from the lane id here, so
            // the mask keeps no vector register alive across the loop
            const int w0 = qb * BM + __builtin_amdgcn_readfirstlane(wave) * NQB * 32 + (Nk - N) - j * BN;
            if (BN - 1 > w0) {
                const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                const int lr = (ln & 31) - 8 * (ln >> 5) + w0;
#pragma unroll
                for (int u = 0; u < NQB; ++u)
#pragma unroll
                    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                        for (int x = 0; x < 16; ++x) {
                            // key ktc + 32 u + 8 h of the tile is hidden from the wave's query row 32 u + r
                            const int ktc = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 16 * (x >> 3) - 32 * u;
                            if (ktc > lr) sacc[u][kb][x] = kNegInf;
                        }
            }
        }
        if constexpr (LOCAL) {
            // the same select on each side of the band: wr, wl are the right and left key limits of
            // the wave's first query relative to the tile (scalars); the lane term is rebuilt from
            // the lane id inside each branch, so no mask register lives across the loop
            const int wf = qb * BM + __builtin_amdgcn_readfirstlane(wave) * NQB * 32 + FA_OFF - j * BN;
            const int wrt = wf + FA_WR, wlt = wf - FA_WL;
            if (BN - 1 > wrt) {   // a key past the first query's right limit
                const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                const int lr = (ln & 31) - 8 * (ln >> 5) + wrt;
#pragma unroll
                for (int u = 0; u < NQB; ++u)
#pragma unroll
                    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                        for (int x = 0; x < 16; ++x) {
                            const int ktc = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 16 * (x >> 3) - 32 * u;
                            if (ktc > lr) sacc[u][kb][x] = kNegInf;
                        }
            }
            if (wlt + NQB * 32 - 1 > 0) {   // a key before the last query's left limit
                const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                const int ll = (ln & 31) - 8 * (ln >> 5) + wlt;
#pragma unroll
                for (int u = 0; u < NQB; ++u)
#pragma unroll
                    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                        for (int x = 0; x < 16; ++x) {
                            const int ktc = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 16 * (x >> 3) - 32 * u;
                            if (ktc < ll) sacc[u][kb][x] = kNegInf;
                        }
            }
        }
        F8 pf[NQB][NKB][2];
#pragma unroll
        for (int u = 0; u < NQB; ++u) {
            // lane-local tile max (this lane's half of the keys): the lazy check needs no
            // cross-lane step, since the query's other half-lane takes part in the same
            // wave-wide ballot; only a rescale combines the halves.  m_true stays
            // lane-local and is combined once after the loop (bitwise the same result).
            const float mt = (FA_FWD_ABL & 4) ? sacc[u][0][0] : lane_max<NKB>(sacc[u]);
            m_true[u] = vmax(m_true[u], mt);
            if (__builtin_amdgcn_ballot_w64(mt > m_used[u] + thr_raw) != 0) {
                float m_new = fmaxf(m_used[u], swap_halves_max(mt));
                if constexpr (CAUSAL) {
                    // only the rows that passed the threshold themselves move (the others get
                    // alpha = 2^0 = 1, exact): a row's bits then depend on its own visible
                    // scores alone, not on what a later row of the wave sees
                    if (!(m_new > m_used[u] + thr_raw)) m_new = m_used[u];
                }
                float alpha = exp2_fast((m_used[u] - m_new) * c);
                if constexpr (LOCAL) {
                    // row-local as above; a row that stays gets alpha = 1 outright, since at
                    // m_used = -inf (no visible key yet) the exponent -inf - -inf is NaN
                    if (!(m_new > m_used[u] + thr_raw)) { m_new = m_used[u]; alpha = 1.0f; }
                }
                l_run[u] *= alpha;
#pragma unroll
                for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                    for (int x = 0; x < 16; ++x) oacc[u][cb][x] *= alpha;
                m_used[u] = m_new;
            }
            const float mc = m_used[u] * c;
            // LOCAL: the exponent is (s - m_used) c, not fma(s, c, -fl(m_used c)): the score that set
            // m_used then gets P = 2^0 = 1 exactly, where the fma leaves the product's rounding
            // residue in every P of the row (harmless in O, which divides it out, but l of a query
            // with one visible key must be 1 and its O that key's V, bit for bit).  A row with no
            // visible key yet (m_used = -inf; all its scores are -inf) subtracts 0: P = 2^-inf = 0.
            float msub = 0.0f;
            if constexpr (LOCAL) msub = m_used[u] == kNegInf ? 0.0f : m_used[u];
            float ps[4];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const float arg = LOCAL ? (sacc[u][kb][x] - msub) * c : fmaf(sacc[u][kb][x], c, -mc);
                    const float pv = (FA_FWD_ABL & 1) ? arg : exp2_fast(arg);
                    // first four seed the partial sums (no `0 + p` adds: without
                    // fast-math the compiler must keep them, -0 + 0 != -0)
                    if (kb == 0 && x < 4) ps[x] = pv; else if (!(FA_FWD_ABL & 2)) ps[x & 3] += pv;
                    pf[u][kb][x >> 3][x & 7] = (T)pv;
                }
            l_run[u] += (ps[0] + ps[1]) + (ps[2] + ps[3]);
        }
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const F8 va = *(const F8*)(vlds + voff + cb * 32 * VROW + (kb * 32 + 16 * s) * 2);
#pragma unroll
                    for (int u = 0; u < NQB; ++u) oacc[u][cb] = mfma32x32x16(va, pf[u][kb][s], oacc[u][cb]);
                }
    };

    char* const buf0 = smem;
    char* const buf1 = smem + STAGE;
    lstore(buf0, jt0);   // waits for the K/V loads only: the Q DMA issued after them is still in flight
    if constexpr (WIDE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's Q DMA landed
    FA_FWD_STAMP(6);
    __syncthreads();
    FA_FWD_STAMP(7);
    if constexpr (WIDE) {
#pragma unroll
        for (int u = 0; u < NQB; ++u)
#pragma unroll
            for (int s = 0; s < D / 16; ++s) {
                const int tb = ((wave * NQB + u) * 32 + 16 * kh + 4 * pp) * 2;
                const F4 lo = __builtin_bit_cast(F4, ds_read_tr16(qoimg + qo_at(16 * s + 8 * h + qq, tb)));
                const F4 hi = __builtin_bit_cast(F4, ds_read_tr16(qoimg + qo_at(16 * s + 8 * h + 4 + qq, tb)));
                qf[u][s] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
    }
    FA_FWD_STAMP(1);
    int wlast = 0;   // causal: the key limit (query row + off) of the wave's last query, a scalar
    if constexpr (CAUSAL) wlast = qb * BM + (__builtin_amdgcn_readfirstlane(wave) + 1) * NQB * 32 - 1 + (Nk - N);
    int wlo = 0, whi = 0;   // local: the first key of the wave's first query and the last key of its last query, scalars
    if constexpr (LOCAL) {
        wlo = qb * BM + __builtin_amdgcn_readfirstlane(wave) * NQB * 32 + FA_OFF - FA_WL;
        whi = qb * BM + (__builtin_amdgcn_readfirstlane(wave) + 1) * NQB * 32 - 1 + FA_OFF + FA_WR;
        if constexpr (VARLEN) {   // a wave whose rows are all past nq computes no tile
            if (qb * BM + __builtin_amdgcn_readfirstlane(wave) * NQB * 32 >= ve.nq) whi = -0x40000000;
        }
    }
    for (int j = jt0; j < jt1; j += 2) {
        gload(min(j + 1, jt1 - 1));
        if constexpr (CAUSAL) {   // only if some query of the wave sees the tile (wave-uniform)
            if (j * BN <= wlast) compute(buf0, buf0 + KBYTES, j);
        } else if constexpr (LOCAL) {   // ... on both sides
            if (j * BN <= whi && j * BN + BN - 1 >= wlo) compute(buf0, buf0 + KBYTES, j);
        } else {
            compute(buf0, buf0 + KBYTES, j);
        }
        lstore(buf1, min(j + 1, jt1 - 1));
        __syncthreads();
        if (j + 1 < jt1) {
            gload(min(j + 2, jt1 - 1));
            if constexpr (CAUSAL) {
                if ((j + 1) * BN <= wlast) compute(buf1, buf1 + KBYTES, j + 1);
            } else if constexpr (LOCAL) {
                if ((j + 1) * BN <= whi && (j + 1) * BN + BN - 1 >= wlo) compute(buf1, buf1 + KBYTES, j + 1);
            } else {
                compute(buf1, buf1 + KBYTES, j + 1);
            }
            lstore(buf0, min(j + 2, jt1 - 1));
            __syncthreads();
        }
    }
    FA_FWD_STAMP(2);
#pragma unroll
    for (int u = 0; u < NQB; ++u) m_true[u] = swap_halves_max(m_true[u]);   // the query's two half-lanes

    if constexpr (SPLIT) {   // partials: O, l relative to exp2(c (s - m_true)), m_true in raw units
        const int64_t sb = (int64_t)split * p.batch + b;
#pragma unroll
        for (int u = 0; u < NQB; ++u) {
            const int qi = qiv[u];
            const float sc = exp2_fast((m_used[u] - m_true[u]) * c);
            const float lt = swap_halves_sum(l_run[u]) * sc;
            if (qi < N) {
                float* Op = p.opart + sb * N * dv;
#pragma unroll
                for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int cc = cb * 32 + acc_row(x, h);
                        if (cc < dv) Op[(int64_t)cc * N + qi] = oacc[u][cb][x] * sc;
                    }
                if (h == 0) {
                    p.mpart[sb * N + qi] = m_true[u];
                    p.lpart[sb * N + qi] = lt;
                }
            }
        }
        return;
    }

    if constexpr (WIDE) {
        // O (normalised, T) into the Q/O image as token pairs.  Lanes r and r ^ 1 hold adjacent
        // tokens of the same features: a lane packs (feature f, feature f + 2) of its own
        // token, swaps the pair with its neighbour (DPP quad_perm [1,0,3,2]) and writes
        // (token r & ~1, token r | 1) of feature f (even lanes) or f + 2 (odd lanes) as one
        // b32: half the LDS writes, and every conversion's two halves are used.  Each value is
        // still (T)(oacc * inv) of its own token.  Rows f and f + 2 differ in bit 1 of the
        // block XOR, so the 32 lanes of a write group cover 32 distinct banks.
        const int odd = lane & 1;
        const unsigned sel = odd ? 0x03020706u : 0x05040100u;   // v_perm_b32: (nb.hi, own.hi) : (own.lo, nb.lo)
#pragma unroll
        for (int u = 0; u < NQB; ++u) {
            const int qi = qiv[u];
            const float lt = swap_halves_sum(l_run[u]);
            float inv = 1.0f / lt;
            // VARLEN: a row past nq or without a key leaves as O = 0, l = 0, m = -inf, by select
            // (its accumulators are zeroed first: 0 * inv = +0 whatever their sign was)
            if constexpr (VARLEN) {
                const bool live = qi < ve.nq && lt > 0.0f;
                inv = live ? inv : 0.0f;
                m_true[u] = live ? m_true[u] : kNegInf;   // m = -inf * scale; l below: 0 * 2^(...) needs its own select
                l_run[u] = live ? 1.0f : 0.0f;            // (reused as the row's live flag from here on)
#pragma unroll
                for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                    for (int x = 0; x < 16; ++x) oacc[u][cb][x] = live ? oacc[u][cb][x] : 0.0f;
            }
            const int tb = ((wave * NQB + u) * 32 + (r & ~1)) * 2;
            // acc_row(4 k + e, h) = 8 k + e + 4 h (e = 0, 1); + 2 for register 4 k + e + 2
            const int wb[2] = {qo_at(4 * h + 2 * odd, tb), qo_at(4 * h + 2 * odd + 1, tb)};
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int x = 4 * k + e;
                        const int ow = (int)pack_scaled<T>(oacc[u][cb][x], oacc[u][cb][x + 2], inv);
                        const int nb = __builtin_amdgcn_mov_dpp(ow, 0xB1, 0xF, 0xF, true);
                        *(unsigned*)(qoimg + wb[e] + (cb * 32 + 8 * k) * ROWB) =
                            __builtin_amdgcn_perm((unsigned)nb, (unsigned)ow, sel);
                    }
            if (qi < N && h == 0) {
                if constexpr (VARLEN) {
                    p.m[(int64_t)b * N + qi] = m_true[u] * p.scale;
                    p.l[(int64_t)b * N + qi] = l_run[u] != 0.0f ? lt * exp2_fast((m_used[u] - m_true[u]) * c) : 0.0f;
                } else {
                    p.m[(int64_t)b * N + qi] = m_true[u] * p.scale;
                    p.l[(int64_t)b * N + qi] = lt * exp2_fast((m_used[u] - m_true[u]) * c);
                }
            }
        }
        FA_FWD_STAMP(8);
        // Each wave stores the 16-B chunks of its own 32 * NQB tokens (with NQB = 2 one whole
        // 128-B line per feature row), so no other wave's image writes are read: the LDS
        // serves one wave's instructions in order and no workgroup barrier is needed; a wave
        // that finishes its tiles early stores and leaves.
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        FA_FWD_STAMP(9);
        const auto ors = slab_rsrc((T*)p.O + (int64_t)b * N * dv, (uint32_t)(N * dv * (int)sizeof(T)));
        constexpr int TPW = 32 * NQB, CPW = TPW / 8, RPI = 64 / CPW;   // tokens, chunks per row, rows per instruction
        static_assert(DV % RPI == 0, "O image store split");
        const int oc = lane % CPW, rs = lane / CPW;
        // 8 rows x 8 chunks per instruction: rows in the order 0 1 4 5 2 3 6 7, so that each
        // 16-lane group of the b128 read covers all 16 slots of a bank row; 16 rows x 4 chunks
        // are conflict-free in plain order
        const int fr = NQB == 2 ? ((rs & 1) | ((rs & 2) << 1) | ((rs & 4) >> 1)) : rs;
        const int lb = (wave * TPW + oc * 8) * 2;
        const int q = qb * BM + wave * TPW + oc * 8;
#pragma unroll
        for (int it = 0; it < DV / RPI; ++it) {
            const int f = it * RPI + fr;
            const u32x4 v4 = *(const u32x4*)(qoimg + qo_at(f, lb));
            // branch-free: a chunk outside (dv, N) gets an offset past the slab descriptor's
            // range, which the buffer store drops (no per-store exec-mask branch in the tail)
            const int off = (f < dv && q < N) ? (f * N + q) * 2 : 0x7FFFFFF0;
            __builtin_amdgcn_raw_buffer_store_b128(v4, ors, off, 0, FA_FWD_OAUX);
        }
        FA_FWD_STAMP(3);
        return;
    }
#pragma unroll
    for (int u = 0; u < NQB; ++u) {
        const int qi = qiv[u];
        const float lt = swap_halves_sum(l_run[u]);
        float inv = 1.0f / lt;
        if constexpr (VARLEN) {   // as in the WIDE epilogue above
            const bool live = qi < ve.nq && lt > 0.0f;
            inv = live ? inv : 0.0f;
            m_true[u] = live ? m_true[u] : kNegInf;
            l_run[u] = live ? 1.0f : 0.0f;
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int x = 0; x < 16; ++x) oacc[u][cb][x] = live ? oacc[u][cb][x] : 0.0f;
        }
        if (qi < N) {
            T* Ob = (T*)p.O + (int64_t)b * N * dv;
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int cc = cb * 32 + acc_row(x, h);
                    if (cc < dv) Ob[(int64_t)cc * N + qi] = (T)(oacc[u][cb][x] * inv);
                }
            if (h == 0) {
                if constexpr (VARLEN) {
                    p.m[(int64_t)b * N + qi] = m_true[u] * p.scale;
                    p.l[(int64_t)b * N + qi] = l_run[u] != 0.0f ? lt * exp2_fast((m_used[u] - m_true[u]) * c) : 0.0f;
                } else {
                    p.m[(int64_t)b * N + qi] = m_true[u] * p.scale;
                    p.l[(int64_t)b * N + qi] = lt * exp2_fast((m_used[u] - m_true[u]) * c);
                }
            }
        }
    }
}

#undef FA_NKE
#undef FA_OFF
#undef FA_WL
#undef FA_WR

// the four default geometries under a mask (a masked launch never splits, never runs fa_fwd_p4)
template <class T, int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(512, 1) void dense_fwd_w8b64(FwdParams p) { dense_fwd_tiled<T, D, DV, 8, 64, 1, false, false, MASK>(p); }
template <class T, int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(512, 1) void dense_fwd_w8q2(FwdParams p) { dense_fwd_tiled<T, D, DV, 8, 64, 2, false, false, MASK>(p); }
// ... with LDS-staged Q / O (N % 8 == 0, Q and O 16-B aligned)
template <class T, int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(512, 1) void dense_fwd_w8q2_wide(FwdParams p) {
    dense_fwd_tiled<T, D, DV, 8, 64, 2, false, (D <= 64 && DV <= 64), MASK>(p);   // the launcher picks it only there
}
template <class T, int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(512, 1) void dense_fwd_w8b64_wide(FwdParams p) { dense_fwd_tiled<T, D, DV, 8, 64, 1, false, true, MASK>(p); }
// split-KV instantiations of the two default geometries (small grids; dense only)
template <class T, int D, int DV>
__global__ __launch_bounds__(512, 1) void dense_fwd_w8q2_split(FwdParams p) { dense_fwd_tiled<T, D, DV, 8, 64, 2, true>(p); }
template <class T, int D, int DV>
__global__ __launch_bounds__(512, 1) void dense_fwd_w8b64_split(FwdParams p) { dense_fwd_tiled<T, D, DV, 8, 64, 1, true>(p); }

// Split-KV combine: O = Σ_s o_s·2^(c(m_s − m)) / Σ_s l_s·2^(c(m_s − m)), m = max_s m_s
// (fixed split order: deterministic).  One thread per output element.
template <class T>
__global__ __launch_bounds__(256) void fwd_split_combine(FwdParams p, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int N = p.N, dv = p.dv, B = p.batch;
    const int n = (int)(e % N);
    const int64_t rest = e / N;
    const int cc = (int)(rest % dv);
    const int b = (int)(rest / dv);
    const float c = p.scale_log2;
    float mx = kNegInf;
    for (int sp = 0; sp < p.nsplit; ++sp) mx = vmax(mx, p.mpart[((int64_t)sp * B + b) * N + n]);
    float L = 0.0f, acc = 0.0f;
    for (int sp = 0; sp < p.nsplit; ++sp) {
        const int64_t sb = (int64_t)sp * B + b;
        const float w = exp2_fast((p.mpart[sb * N + n] - mx) * c);
        L = fmaf(p.lpart[sb * N + n], w, L);
        acc = fmaf(p.opart[(sb * dv + cc) * N + n], w, acc);
    }
    ((T*)p.O)[((int64_t)b * dv + cc) * N + n] = (T)(acc / L);
    if (cc == 0) {
        p.m[(int64_t)b * N + n] = mx * p.scale;
        p.l[(int64_t)b * N + n] = L;
    }
}

// dst (Np, C, B) <- src (N, C, B), zero rows n >= N
template <class T>
__global__ __launch_bounds__(256) void fwd_pad_keys(const T* __restrict__ src, T* __restrict__ dst, int N, int Np,
                                                    int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int n = (int)(e % Np);
    const int64_t cb = e / Np;                  // c + C·b
    dst[e] = n < N ? src[cb * N + n] : (T)0.0f;
}

// --------------------------------------------------------------------------
// launcher: dense_fwd_plan (fa_dense_plan.h) names the kernel, its grid and the
// workspace offsets; nothing below decides any of them again
// --------------------------------------------------------------------------
static_assert(kBM == kFwdGenericRows && kThreads == kFwdGenericThreads && kBN == kFwdKeyTile, "the plan's constants");

hipError_t launch_dense_fwd_p4(const FwdParams& p, int Dc, int dtype, dim3 grid, hipStream_t s);

// The bf16 / fp16 kernel of a plan at head-dim classes (Dc, DVc) under the plan's mask.  Every
// kernel is instantiated for the nine class pairs, the d = 128 forms of w8q2 included (a forced
// kFwdW8Q2 reaches them), except the masked two-query-block kernels: d, dv <= 64 only (they
// spill above, and the plan picks them only there).
template <class T>
static hipError_t launch_16bit(const DenseFwdPlan& pl, const FwdParams& p, int Dc, int DVc, hipStream_t s) {
    const dim3 grid((unsigned)pl.grid), blk(pl.block);
    auto go = [&](void (*kernel)(FwdParams)) { hipLaunchKernelGGL(kernel, grid, blk, 0, s, p); };
    hipError_t e = hipErrorInvalidValue;   // stays when a class or the kernel is not one of ours
    by_mask(pl.mask, [&](auto M) {
        by_dim_class(Dc, [&](auto Dk) {
            by_dim_class(DVc, [&](auto DVk) {
                constexpr DenseMask MASK = decltype(M)::value;
                constexpr int D = decltype(Dk)::value, DV = decltype(DVk)::value;
                constexpr bool q2 = MASK == kMaskNone || (D <= 64 && DV <= 64);   // w8q2 exists here
                switch (pl.kernel) {
                    case kDenseFwdGeneric: go(dense_fwd_generic<T, D, DV, MASK>); break;
                    case kDenseFwdW8B64: go(dense_fwd_w8b64<T, D, DV, MASK>); break;
                    case kDenseFwdW8B64Wide: go(dense_fwd_w8b64_wide<T, D, DV, MASK>); break;
                    case kDenseFwdW8Q2:
                        if constexpr (q2) go(dense_fwd_w8q2<T, D, DV, MASK>);
                        else return;   // never planned
                        break;
                    case kDenseFwdW8Q2Wide:
                        if constexpr (q2) go(dense_fwd_w8q2_wide<T, D, DV, MASK>);
                        else return;
                        break;
                    case kDenseFwdW8B64Split: go(dense_fwd_w8b64_split<T, D, DV>); break;
                    case kDenseFwdW8Q2Split: go(dense_fwd_w8q2_split<T, D, DV>); break;
                    default: return;
                }
                if (pl.nsplit > 1) {
                    const int64_t total = (int64_t)p.N * p.dv * p.batch;
                    hipLaunchKernelGGL(fwd_split_combine<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, total);
                }
                e = hipGetLastError();
            });
        });
    });
    return e;
}
static hipError_t launch_f32(const DenseFwdPlan& pl, const FwdParams& p, int Dc, int DVc, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    by_mask(pl.mask, [&](auto M) {
        by_dim_class(Dc, [&](auto Dk) {
            by_dim_class(DVc, [&](auto DVk) {
                hipLaunchKernelGGL((dense_fwd_generic_f32<decltype(Dk)::value, decltype(DVk)::value, decltype(M)::value>),
                                   dim3((unsigned)pl.grid), dim3(pl.block), 0, s, p);
                e = hipGetLastError();
            });
        });
    });
    return e;
}
template <class T>
static void pad_keys(const void* src, void* dst, int64_t Nk, int64_t ldk, int64_t C, int64_t B, hipStream_t s) {
    const int64_t total = ldk * C * B;
    hipLaunchKernelGGL(fwd_pad_keys<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const T*)src, (T*)dst,
                       (int)Nk, (int)ldk, total);
}

// The shape's own needs (aligned tensors, the auto variant, room for everything): the
// queries have no pointers, and the CU count does not change the total.
// (A masked launch never splits the keys: its total is the padded K / V copies only.)
size_t dense_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, DenseMask mask) {
    return dense_fwd_plan(dtype, N, Nk, d, dv, batch, mask, {kFwdAuto, 0}, true, true, SIZE_MAX, 0).total;
}

int launch_dense_fwd(const DenseArgs& a, hipStream_t s, const char** why) {
    g_fwd_last_path = 0;   // every path below that is not a persistent kernel leaves 0
    if (a.dtype == FA_DTYPE_F64) {   // kDenseFwdF64: it makes its own checks
        const int rc = launch_dense_fwd_f64(a, s, why);
        if (rc == FA_OK) g_dense_fwd_last[0] = kDenseFwdF64, g_dense_fwd_last[1] = a.mask, g_dense_fwd_last[2] = 0;
        return rc;
    }
    const int Dc = head_dim_class(a.d), DVc = head_dim_class(a.dv);
    if (!Dc || !DVc) {
        *why = "head dimension exceeds the compiled maximum (128)";
        return FA_ERR_UNSUPPORTED;
    }
    if (mask_lacks_keys(a.mask, a.N, a.Nk, why)) return FA_ERR_UNSUPPORTED;
    if (a.N > INT32_MAX / 2 || a.Nk > INT32_MAX / 2 || a.N * a.d > INT32_MAX ||
        a.Nk * a.d > INT32_MAX || a.Nk * a.dv > INT32_MAX || a.N * a.dv > INT32_MAX) {
        *why = "per-slab extent exceeds 2^31 elements";
        return FA_ERR_UNSUPPORTED;
    }
    if ((a.N + kBM - 1) / kBM * a.batch > INT32_MAX) {
        *why = "grid too large";
        return FA_ERR_UNSUPPORTED;
    }
    if (a.dtype != FA_DTYPE_F32 && !dense_16bit(a.dtype)) {
        *why = "unknown dtype";
        return FA_ERR_INVALID_ARG;
    }
    const DenseFwdPlan pl = dense_fwd_plan(a.dtype, a.N, a.Nk, a.d, a.dv, a.batch, a.mask,
                                           {g_fwd_variant, g_causal_rev}, aligned16(a.K) && aligned16(a.V),
                                           aligned16(a.Q) && aligned16(a.O), a.workspace ? a.workspace_bytes : 0,
                                           device_cus(s));
    char* const w = al256(a.workspace);
    FwdParams p;
    p.Q = a.Q; p.K = a.K; p.V = a.V; p.O = a.O; p.l = a.l; p.m = a.m;
    p.N = (int)a.N; p.Nk = (int)a.Nk; p.d = (int)a.d; p.dv = (int)a.dv;
    p.ldk = (int)pl.ldk;
    p.nqb = (int)pl.nqb;
    p.total_wg = (int)pl.total_wg;
    p.scale = a.scale;
    p.scale_log2 = a.scale * kLog2e;
    p.rescale_log2 = g_fwd_rescale_log2;
    p.batch = (int)a.batch;
    p.nsplit = pl.nsplit; p.tps = pl.tps; p.opart = p.lpart = p.mpart = nullptr;
    if (a.mask == kMaskLocal || a.mask == kMaskVarlen) {   // never split: the window rides in the split's two ints (fa_fwd_params.h)
        const MaskInts mi = mask_ints(a.mask, a.left, a.right, a.N, a.Nk);
        p.wleft = mi.left;
        p.wright = mi.right;
    }
    if (a.mask == kMaskVarlen) {   // ... and the lengths in its first two partial pointers (fwd_q_lens, fwd_k_lens)
        p.opart = (float*)a.q_lens;
        p.lpart = (float*)a.k_lens;
    }
    p.causal = pl.causal;
    p.fast = pl.kv_vec;
    p.wide = pl.wide;
    if (pl.pad) {
        void* const kp = w + pl.off_k;
        void* const vp = w + pl.off_v;
        if (a.dtype == FA_DTYPE_F16) {
            pad_keys<f16>(a.K, kp, a.Nk, pl.ldk, a.d, a.batch, s);
            pad_keys<f16>(a.V, vp, a.Nk, pl.ldk, a.dv, a.batch, s);
        } else {
            pad_keys<bf16>(a.K, kp, a.Nk, pl.ldk, a.d, a.batch, s);
            pad_keys<bf16>(a.V, vp, a.Nk, pl.ldk, a.dv, a.batch, s);
        }
        p.K = kp;
        p.V = vp;
    }
    if (pl.nsplit > 1) {
        p.opart = (float*)(w + pl.off_opart);
        p.lpart = (float*)(w + pl.off_lpart);
        p.mpart = (float*)(w + pl.off_mpart);
    }
    hipError_t e;
    switch (pl.kernel) {
        case kDenseFwdGenericF32: e = launch_f32(pl, p, Dc, DVc, s); break;
        case kDenseFwdP4:
            e = launch_dense_fwd_p4(p, Dc, a.dtype, dim3((unsigned)pl.grid), s);
            g_fwd_last_path = 30;
            break;
        default:
            e = a.dtype == FA_DTYPE_F16 ? launch_16bit<f16>(pl, p, Dc, DVc, s) : launch_16bit<bf16>(pl, p, Dc, DVc, s);
    }
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    g_dense_fwd_last[0] = pl.kernel, g_dense_fwd_last[1] = pl.mask, g_dense_fwd_last[2] = pl.pad;
    return FA_OK;
}

}  // namespace fa
