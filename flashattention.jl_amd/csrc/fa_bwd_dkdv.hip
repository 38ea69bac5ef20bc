// fa_bwd_dkdv.hip — dense backward, the dK/dV pass of the MFMA fast path (bf16 / fp16; d, dv
// in {32, 64, 128}; N, Nk % 8 == 0; 16-B aligned; images and DMA as in fa_bwd_dq.hip):
// bwd_dkdv_fast, each wave 32 keys over all query tiles, dKᵀ and dVᵀ in registers and written
// once.  Exports launch_dkdv_fast.
#include "fa_bwd_common.h"
#include "fa_bwd_params.h"

namespace fa {

// CAUSAL: the query tiles (and the row-constant double buffer) begin at the first tile that
// sees the block's first key, a wave skips the tiles before its own first key, and S is
// selected to -inf after the MFMA chain (the accumulators start from the row constants) on
// the tiles that straddle the wave's diagonal.
//
// LOCAL: key j is seen by the queries j - off - right <= i <= j - off + left, so the block's
// query tiles are [t0, t1) of that range over its 128 keys.  The range is EMPTY for a block
// whose keys lie left of every window (Nk > N + left: a KV cache longer than the window): the
// whole pipeline (row constants, DMA, barriers) is then skipped, block-uniformly, and the
// zero accumulators are stored.  A wave skips the tiles outside its own keys' range and
// selects on the tiles that straddle either diagonal.
template <class T, int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(256, 2) void bwd_dkdv_fast(BwdParams p) {
    constexpr bool CAUSAL = MASK == kMaskCausal, LOCAL = MASK == kMaskLocal || MASK == kMaskVarlen, VARLEN = MASK == kMaskVarlen;
    typedef typename Frag8<T>::type F8;
    constexpr int QB = D * 128, OB = DV * 128, STAGE = QB + OB + 512;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int b = lid / p.nblk, kblk = lid - b * p.nblk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int N = p.N, Nk = p.Nk;
    const auto qrs = bslab<T>(p.Q, (int64_t)b * N * D, (int64_t)N * D);
    const auto ors = bslab<T>(p.dO, (int64_t)b * N * DV, (int64_t)N * DV);
    const auto krs = bslab<T>(p.K, (int64_t)b * Nk * D, (int64_t)Nk * D);
    const auto vrs = bslab<T>(p.V, (int64_t)b * Nk * DV, (int64_t)Nk * DV);
    const VarlenExt e = bwd_ext<VARLEN>(p, b);
    const int kj = kblk * 128 + wave * 32 + r;   // this lane's key (column of S, dP)
    F8 kf[D / 16], vf[DV / 16];
#pragma unroll
    for (int s = 0; s < D / 16; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            kf[s][e] = __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b16(krs, ((16 * s + 8 * h + e) * Nk + kj) * 2, 0, 0));
#pragma unroll
    for (int s = 0; s < DV / 16; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            vf[s][e] = __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b16(vrs, ((16 * s + 8 * h + e) * Nk + kj) * 2, 0, 0));
    const float c = p.scale_log2;
    const float* nlse = p.nlse + (int64_t)b * N;
    const float* nDg = p.nD + (int64_t)b * N;

    const ImgReader<T> rd(tid);

    f32x16 dk[D / 32], dv[DV / 32];
#pragma unroll
    for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) dk[cb][x] = 0.0f;
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) dv[cb][x] = 0.0f;

    // per-tile row constants: threads 0-63 carry −lse (−inf past N), 64-127 −D
    float rowc = 0.0f;
    auto load_rowc = [&](int t) {
        const int q = t * 64 + (tid & 63);
        if (tid < 64) rowc = q < N ? nlse[q] : kNegInf;
        else if (tid < 128) rowc = q < N ? nDg[q] : 0.0f;
    };
    auto store_rowc = [&](char* st) {
        if (tid < 128) ((float*)(st + QB + OB))[tid] = rowc;
    };
    auto fill = [&](char* st, int t) {
        dma_image<D>(qrs, st, N, t * 64, wave, lane);
        dma_image<DV>(ors, st + QB, N, t * 64, wave, lane);
    };
    int wk0 = 0;   // causal: the wave's first key minus off (the first query that sees it), a scalar
    if constexpr (CAUSAL || LOCAL) wk0 = kblk * 128 + __builtin_amdgcn_readfirstlane(wave) * 32 - e.off;
    auto compute = [&](const char* st, int t) {
        if constexpr (CAUSAL) {
            if (t * 64 + 63 < wk0) return;   // wave-uniform: no query of the tile sees the wave's keys
        }
        if constexpr (LOCAL) {
            if (t * 64 + 63 < wk0 - e.right || t * 64 > wk0 + 31 + e.left) return;
        }
        const char* qimg = st;
        const char* oimg = st + QB;
        const float* rl = (const float*)(st + QB + OB);      // −lse[64], then −D[64]
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            // rows of S / dP (queries) map to 8h + {0..7} and 16 + 8h + {0..7}
            f32x16 sa, dp;
            const f32x4* Lq = (const f32x4*)(rl + u * 32 + 8 * h);
            const f32x4* Dq = (const f32x4*)(rl + 64 + u * 32 + 8 * h);
            const f32x4 l0 = Lq[0], l1 = Lq[1], l2 = Lq[4], l3 = Lq[5];
            const f32x4 d0 = Dq[0], d1 = Dq[1], d2 = Dq[4], d3 = Dq[5];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sa[e] = l0[e]; sa[4 + e] = l1[e]; sa[8 + e] = l2[e]; sa[12 + e] = l3[e];
                dp[e] = d0[e]; dp[4 + e] = d1[e]; dp[8 + e] = d2[e]; dp[12 + e] = d3[e];
            }
#pragma unroll
            for (int s = 0; s < D / 16; ++s) sa = mfma32x32x16(rd.tr(qimg, u, s), kf[s], sa);
#pragma unroll
            for (int s = 0; s < DV / 16; ++s) dp = mfma32x32x16(rd.tr(oimg, u, s), vf[s], dp);
            if constexpr (CAUSAL) {
                const int q0 = t * 64 + u * 32 - wk0;   // the 32-query block's first row, relative to the wave's first key
                if (q0 < 31) {                          // that row misses the wave's last key
                    // query row (x & 7) + 16 (x >> 3) + 8 h misses key r when < r - q0; r and h rebuilt
                    // from the lane id here (7 fewer spilled registers at d = dv = 128 than from r, h)
                    const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                    const int lk = (ln & 31) - 8 * (ln >> 5) - q0;
#pragma unroll
                    for (int x = 0; x < 16; ++x)
                        if ((x & 7) + 16 * (x >> 3) < lk) sa[x] = kNegInf;
                }
            }
            if constexpr (LOCAL) {
                // query row q0 + ql (relative to the wave's first key minus off) sees key r iff
                // q0 + ql - left <= r <= q0 + ql + right; lane terms rebuilt from the lane id as above
                const int q0 = t * 64 + u * 32 - wk0;
                if (q0 + e.right < 31) {            // the block's first row misses the wave's last key on the right
                    const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                    const int lk = (ln & 31) - 8 * (ln >> 5) - q0 - e.right;
#pragma unroll
                    for (int x = 0; x < 16; ++x)
                        if ((x & 7) + 16 * (x >> 3) < lk) sa[x] = kNegInf;
                }
                if (q0 + 31 > e.left) {             // its last row misses the wave's first key on the left
                    const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                    const int lk = (ln & 31) - 8 * (ln >> 5) - q0 + e.left;
#pragma unroll
                    for (int x = 0; x < 16; ++x)
                        if ((x & 7) + 16 * (x >> 3) > lk) sa[x] = kNegInf;
                }
            }
            if constexpr (VARLEN) {
                // the key column at nk: these rows are the caller's and are written, so a key
                // >= nk gets P = 0 in every row (only in the wave that holds nk: wave-uniform test;
                // rows >= nq carry -lse = -inf from the pre-pass)
                const int wkey = kblk * 128 + __builtin_amdgcn_readfirstlane(wave) * 32;
                if (wkey + 31 >= e.nk) {
                    const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                    if (wkey + (ln & 31) >= e.nk) {
#pragma unroll
                        for (int x = 0; x < 16; ++x) sa[x] = kNegInf;
                    }
                }
            }
            F8 pf[2], dsf[2];
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pr = exp2_fast(sa[x] * c);
                pf[x >> 3][x & 7] = (T)pr;
                dsf[x >> 3][x & 7] = (T)(pr * dp[x]);
            }
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) dv[cb] = mfma32x32x16(rd.row(oimg, cb, u, s2), pf[s2], dv[cb]);
#pragma unroll
            for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) dk[cb] = mfma32x32x16(rd.row(qimg, cb, u, s2), dsf[s2], dk[cb]);
        }
    };

    const int NT = ((VARLEN ? e.nq : N) + 63) / 64;
    char* const st0 = smem;
    char* const st1 = smem + STAGE;
    int t0 = 0;   // causal: the first query tile that sees the block's first key (< NT: see DESIGN §2.7)
    if constexpr (CAUSAL) t0 = min(max(0, kblk * 128 - p.off) / 64, NT - 1);
    int t1 = NT;   // local: query tiles [t0, t1), possibly none
    if constexpr (LOCAL) {
        const int qhi = kblk * 128 + 127 - e.off + e.left;   // the last query that sees the block's last key
        t0 = max(0, kblk * 128 - e.off - e.right) / 64;
        t1 = qhi < 0 ? 0 : min(NT, qhi / 64 + 1);
        if (VARLEN && kblk * 128 >= e.nk) t1 = 0;   // a block past nk: no tile, zeros are stored
    }
    if (!LOCAL || t0 < t1) {   // (block-uniform: no prefetch of a tile that does not exist, no uneven barrier)
        load_rowc(t0);
        fill(st0, t0);
        store_rowc(st0);
        __syncthreads();
        for (int t = t0; t < t1; t += 2) {
            load_rowc(min(t + 1, t1 - 1));
            fill(st1, min(t + 1, t1 - 1));
            compute(st0, t);
            store_rowc(st1);
            __syncthreads();
            if (t + 1 < t1) {
                load_rowc(min(t + 2, t1 - 1));
                fill(st0, min(t + 2, t1 - 1));
                compute(st1, t + 1);
                store_rowc(st0);
                __syncthreads();
            }
        }
    }
    if (kj < Nk) {
        T* dKb = (T*)p.dK + (int64_t)b * Nk * D;
        T* dVb = (T*)p.dV + (int64_t)b * Nk * DV;
#pragma unroll
        for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x)
                dKb[(int64_t)(cb * 32 + acc_row(x, h)) * Nk + kj] = (T)(dk[cb][x] * p.scale);
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x)
                dVb[(int64_t)(cb * 32 + acc_row(x, h)) * Nk + kj] = (T)dv[cb][x];
    }
}

template <class T>
hipError_t launch_dkdv_fast(const BwdParams& p, DenseMask mask, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    by_dim_class(p.d, [&](auto D) {
        by_dim_class(p.dv, [&](auto DV) {
            by_mask(mask, [&](auto M) {
                hipLaunchKernelGGL((bwd_dkdv_fast<T, decltype(D)::value, decltype(DV)::value, decltype(M)::value>),
                                   dim3((unsigned)p.total_wg), dim3(256), 0, s, p);
            });
            e = hipGetLastError();
        });
    });
    return e;
}
template hipError_t launch_dkdv_fast<bf16>(const BwdParams&, DenseMask, hipStream_t);
template hipError_t launch_dkdv_fast<f16>(const BwdParams&, DenseMask, hipStream_t);

}  // namespace fa
