// fa_bwd_dq.hip — dense backward, the dQ pass of the MFMA fast path: bwd_dq_fast, each wave
// 32 queries over all key tiles (the forward's shape), and fused_combine, the add it makes for
// the wrapped slices a single pass (fa_bwd_fused.hip) left to it.  Exports launch_dq_fast.
#include "fa_bwd_common.h"
#include "fa_bwd_params.h"

namespace fa {

// --------------------------------------------------------------------------
// 2./3. MFMA fast path (bf16 / fp16; d, dv in {32, 64, 128}; N, Nk % 8 == 0;
// 16-B aligned).  Token tiles of 64 are staged by LDS-DMA (buffer_load … lds)
// into the swizzled [rows][64 tokens] images of fa_bwd_common.h (img_chunk for the
// writers here, ImgReader for the MFMA operands).
// --------------------------------------------------------------------------

// dQ of the wrapped slices of query block qb (slices 2qb, 2qb + 1) of slab b whose two
// chain tails both stored their totals (fin == 2, bwd_fused): dQ = (A + B)·τ, the same
// single add — so the same bits — as chain B's tail makes when A is done first.  The
// totals are in bwd_fused's running-sum layout: per slice NTQ tiles of 32 x 32 fp32,
// lane l's 16-B pieces c4 at l·16 + c4·1024, element 4 c4 + e = dQᵀ row (feature)
// 32 cb + acc_row(4 c4 + e, l >> 5), column (query) 32 u + sig32(l & 31), tile = u·D/32 + cb.
template <class T, int D>
__device__ void fused_combine(const BwdParams& p, int b, int qb) {
    constexpr int NTQ = D / 16;
    const int NS = p.nqt, N = p.N;
    const float* const partb = p.part + (int64_t)b * 2 * NS * NTQ * 1024;
    const int64_t pchain = (int64_t)NS * NTQ * 1024;
    T* const dQb = (T*)p.dQ + (int64_t)b * N * D;
    for (int t = 2 * qb; t < 2 * qb + 2 && t < NS; ++t) {
        if (ld_agent((gu32*)(uintptr_t)(p.fin + (int64_t)b * NS + t)) != 2u) continue;
        for (int idx = threadIdx.x; idx < NTQ * 64; idx += 256) {
            const int w = idx >> 6, l = idx & 63;
            const int cb = w % (D / 32), u = w / (D / 32);
            const int q = t * 64 + 32 * u + sig32(l & 31);
            const float* a = partb + (int64_t)(t * NTQ + w) * 1024 + l * 4;
            const float* bb = a + pchain;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const f32x4 va = *(const f32x4*)(a + c4 * 256), vb = *(const f32x4*)(bb + c4 * 256);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int x = 4 * c4 + e;
                    const int f = cb * 32 + acc_row(x, l >> 5);
                    if (q < N) dQb[(int64_t)f * N + q] = (T)((va[e] + vb[e]) * p.scale);
                }
            }
        }
    }
}

// CAUSAL (fa_causal_bwd, never after bwd_fused: no guard, no combine): the key tiles end at
// the block's last query's last visible tile, a wave skips the tiles past its own last query,
// and S is selected to -inf on the tiles that straddle the wave's diagonal.
//
// LOCAL (fa_local_bwd, likewise never after bwd_fused): the key tiles run from the block's first
// query's left edge to its last query's right edge, a wave skips the tiles wholly outside
// its own band, and S is selected to -inf on the tiles that straddle either of its diagonals.
template <class T, int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(256, 2) void bwd_dq_fast(BwdParams p) {
    constexpr bool CAUSAL = MASK == kMaskCausal, LOCAL = MASK == kMaskLocal || MASK == kMaskVarlen, VARLEN = MASK == kMaskVarlen;
    typedef typename Frag8<T>::type F8;
    constexpr int KB = D * 128, VB = DV * 128, STAGE = KB + VB;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    // after bwd_fused: recompute dQ only on the slabs whose hand-off gave up, and make
    // dQ = A + B of the wrapped slices whose two chain tails both stored their totals
    const bool give_up = p.guard && ld_agent((gu32*)(uintptr_t)p.guard) != 0u;
    const bool combine = p.cguard && ld_agent((gu32*)(uintptr_t)p.cguard) != 0u;
    if (p.guard && !give_up && !combine) return;
    const int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int b = lid / p.nblk, qb = lid - b * p.nblk;
    if (p.sguard && (!give_up || ld_agent((gu32*)(uintptr_t)(p.sguard + b)) == 0u)) {
        if (combine) fused_combine<T, D>(p, b, qb);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int N = p.N, Nk = p.Nk;
    // key tiles [tbeg, NT) of the block, from the slab's extents (bwd_ext).  VARLEN: a block past
    // nq, or whose queries see no key, stores zeros and leaves before any load or barrier
    const VarlenExt e = bwd_ext<VARLEN>(p, b);
    int vtbeg = 0, vNT = 0;   // VARLEN: the tile range, here; the other masks compute theirs below, as before
    if constexpr (VARLEN) {
        const int hi = min(qb * 128 + 127, e.nq - 1) + e.off + e.right;
        vtbeg = max(0, qb * 128 + e.off - e.left) / 64;
        vNT = hi < 0 ? 0 : min((e.nk + 63) / 64, hi / 64 + 1);
        if (qb * 128 >= e.nq || vtbeg >= vNT) {
            zero_rows((T*)p.dQ + (int64_t)b * N * D, N, D, qb * 128, 128, 256);
            return;
        }
    }
    auto NKV = [&] { if constexpr (VARLEN) return e.nk; else return p.nkv; };
    const auto qrs = bslab<T>(p.Q, (int64_t)b * N * D, (int64_t)N * D);
    const auto ors = bslab<T>(p.dO, (int64_t)b * N * DV, (int64_t)N * DV);
    const auto krs = bslab<T>(p.K, (int64_t)b * Nk * D, (int64_t)Nk * D);
    const auto vrs = bslab<T>(p.V, (int64_t)b * Nk * DV, (int64_t)Nk * DV);
    const int qi = qb * 128 + wave * 32 + r;
    F8 qf[D / 16], df[DV / 16];
#pragma unroll
    for (int s = 0; s < D / 16; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            qf[s][e] = __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b16(qrs, ((16 * s + 8 * h + e) * N + qi) * 2, 0, 0));
#pragma unroll
    for (int s = 0; s < DV / 16; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            df[s][e] = __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b16(ors, ((16 * s + 8 * h + e) * N + qi) * 2, 0, 0));
    const int qc = qi < N ? qi : N - 1;
    const float c = p.scale_log2;
    const float cnl = c * p.nlse[(int64_t)b * N + qc];
    const float nDq = p.nD[(int64_t)b * N + qc];

    const ImgReader<T> rd(tid);

    f32x16 dq[D / 32];
#pragma unroll
    for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) dq[cb][x] = 0.0f;

    auto fill = [&](char* st, int t) {
        dma_image<D>(krs, st, Nk, t * 64, wave, lane);
        dma_image<DV>(vrs, st + KB, Nk, t * 64, wave, lane);
    };
    int wlim0 = 0;   // causal: the key limit (query row + off) of the wave's first query, a scalar
    if constexpr (CAUSAL || LOCAL) wlim0 = qb * 128 + __builtin_amdgcn_readfirstlane(wave) * 32 + e.off;
    auto compute = [&](const char* st, int t) {
        if constexpr (CAUSAL) {
            if (t * 64 > wlim0 + 31) return;   // wave-uniform: no query of the wave sees the tile
        }
        if constexpr (LOCAL) {   // ... on either side
            if (t * 64 > wlim0 + 31 + e.right || t * 64 + 63 < wlim0 - e.left) return;
        }
        const char* kimg = st;
        const char* vimg = st + KB;
        const bool partial = (t + 1) * 64 > NKV();
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x16 sa, dp;
#pragma unroll
            for (int x = 0; x < 16; ++x) { sa[x] = 0.0f; dp[x] = 0.0f; }
#pragma unroll
            for (int s = 0; s < D / 16; ++s) sa = mfma32x32x16(rd.tr(kimg, kb, s), qf[s], sa);
#pragma unroll
            for (int s = 0; s < DV / 16; ++s) dp = mfma32x32x16(rd.tr(vimg, kb, s), df[s], dp);
            if (partial) {
#pragma unroll
                for (int x = 0; x < 16; ++x)
                    if (t * 64 + kb * 32 + (x & 7) + 8 * h + 16 * (x >> 3) >= NKV()) sa[x] = kNegInf;
            }
            if constexpr (CAUSAL) {
                const int w0 = wlim0 - t * 64 - kb * 32;   // ... relative to the 32-key block
                if (31 > w0) {
                    const int lr = r - 8 * h + w0;           // key (x & 7) + 16 (x >> 3) + 8 h is hidden when > r + w0
#pragma unroll
                    for (int x = 0; x < 16; ++x)
                        if ((x & 7) + 16 * (x >> 3) > lr) sa[x] = kNegInf;
                }
            }
            if constexpr (LOCAL) {
                // wr, wl: the right and left key limits of the wave's first query, relative to the 32-key block
                const int wr = wlim0 + e.right - t * 64 - kb * 32, wl = wlim0 - e.left - t * 64 - kb * 32;
                if (31 > wr) {           // a key past the first query's right limit
                    const int lr = r - 8 * h + wr;
#pragma unroll
                    for (int x = 0; x < 16; ++x)
                        if ((x & 7) + 16 * (x >> 3) > lr) sa[x] = kNegInf;
                }
                if (wl + 31 > 0) {       // a key before the last query's left limit
                    const int ll = r - 8 * h + wl;
#pragma unroll
                    for (int x = 0; x < 16; ++x)
                        if ((x & 7) + 16 * (x >> 3) < ll) sa[x] = kNegInf;
                }
            }
            F8 dsf[2];
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pr = exp2_fast(fmaf(sa[x], c, cnl));
                dsf[x >> 3][x & 7] = (T)(pr * (dp[x] + nDq));
            }
#pragma unroll
            for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) dq[cb] = mfma32x32x16(rd.row(kimg, cb, kb, s2), dsf[s2], dq[cb]);
        }
    };

    int NT = (Nk + 63) / 64;
    if constexpr (CAUSAL) NT = min(NT, (min(qb * 128 + 127, N - 1) + p.off) / 64 + 1);
    int tbeg = 0;   // local: key tiles [tbeg, NT), never empty (the key i + off of the first query lies in both)
    if constexpr (LOCAL && !VARLEN) {
        tbeg = max(0, qb * 128 + p.off - p.left) / 64;
        NT = min(NT, (min(qb * 128 + 127, N - 1) + p.off + p.right) / 64 + 1);
    }
    if constexpr (VARLEN) { tbeg = vtbeg; NT = vNT; }
    char* const st0 = smem;
    char* const st1 = smem + STAGE;
    fill(st0, tbeg);
    __syncthreads();
    for (int t = tbeg; t < NT; t += 2) {
        fill(st1, min(t + 1, NT - 1));
        compute(st0, t);
        __syncthreads();
        if (t + 1 < NT) {
            fill(st0, min(t + 2, NT - 1));
            compute(st1, t + 1);
            __syncthreads();
        }
    }
    if (qi < N) {
        T* dQb = (T*)p.dQ + (int64_t)b * N * D;
#pragma unroll
        for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x)
                dQb[(int64_t)(cb * 32 + acc_row(x, h)) * N + qi] = (T)(dq[cb][x] * p.scale);
    }
}

template <class T>
hipError_t launch_dq_fast(const BwdParams& p, DenseMask mask, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    by_dim_class(p.d, [&](auto D) {
        by_dim_class(p.dv, [&](auto DV) {
            by_mask(mask, [&](auto M) {
                hipLaunchKernelGGL((bwd_dq_fast<T, decltype(D)::value, decltype(DV)::value, decltype(M)::value>),
                                   dim3((unsigned)p.total_wg), dim3(256), 0, s, p);
            });
            e = hipGetLastError();
        });
    });
    return e;
}
template hipError_t launch_dq_fast<bf16>(const BwdParams&, DenseMask, hipStream_t);
template hipError_t launch_dq_fast<f16>(const BwdParams&, DenseMask, hipStream_t);

}  // namespace fa
