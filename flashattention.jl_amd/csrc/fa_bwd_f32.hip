// fa_bwd_f32.hip — dense backward, the fp32 MFMA path: bwd_dkdv_f32 and bwd_dq_f32, the
// dK/dV pass and the dQ pass of fa_bwd.hip's structure in exact fp32 products.  Exports
// launch_f32_mfma.
#include "fa_common.h"
#include "fa_bwd_params.h"

namespace fa {

// --------------------------------------------------------------------------
// 2./3. fp32 MFMA path (v_mfma_f32_32x32x2_f32: exact fp32 products, the same
// arithmetic as an fmaf chain; d, dv <= 128 (classes 32 / 64 / 128), any N, Nk).  Each lane keeps its
// own key's (dK/dV kernel) or query's (dQ kernel) K, V (resp. Q, dO) features in
// registers as the B operand of the score products; the tile of the other side
// sits in LDS ([feature][33] rows: conflict-free for both the column and the
// row access).  The score accumulators are used directly as the B operand of
// the gradient products: register x of lane (r, h) holds row acc_row(x, h), which
// is exactly what a 32x32x2 B operand with k = h needs (cf. the fp32 forward).
//   dK/dV: S = Q Kᵀ (queries on rows, keys on lanes), dVᵀ += dOᵀ P, dKᵀ += Qᵀ dS;
//   dQ   : Sᵀ = K Qᵀ (keys on rows, queries on lanes), dQᵀ += Kᵀ dSᵀ.
// Keys past Nk are zero rows whose own rows are not stored; the dQ kernel selects their
// scores to −inf (P = 0: with lse < −88 their exp(0 − lse) would be inf, and inf · 0 NaN);
// queries past N carry nlse = −inf (P = 0) and dO = 0.
// --------------------------------------------------------------------------
constexpr int kF32T = 32;   // tile of the streamed side
constexpr int kF32R = 33;   // LDS row (floats)

template <int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(256) void bwd_dkdv_f32(BwdParams p) {
    constexpr bool CAUSAL = MASK == kMaskCausal, LOCAL = MASK == kMaskLocal || MASK == kMaskVarlen, VARLEN = MASK == kMaskVarlen;
    __shared__ float sQ[D * kF32R], sdO[DV * kF32R], sL[kF32T], sD[kF32T];
    const int N = p.N, Nk = p.Nk, d = p.d, dv = p.dv;
    const int nkb = (Nk + 127) / 128;
    const int b = blockIdx.x / nkb, k0 = (blockIdx.x % nkb) * 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const float* Qb = (const float*)p.Q + (int64_t)b * N * d;
    const float* dOb = (const float*)p.dO + (int64_t)b * N * dv;
    const float* Kb = (const float*)p.K + (int64_t)b * Nk * d;
    const float* Vb = (const float*)p.V + (int64_t)b * Nk * dv;
    const int key = k0 + wave * 32 + r;
    float kf[D / 2], vf[DV / 2];
#pragma unroll
    for (int t = 0; t < D / 2; ++t) kf[t] = (key < Nk && 2 * t + h < d) ? Kb[(int64_t)(2 * t + h) * Nk + key] : 0.0f;
#pragma unroll
    for (int t = 0; t < DV / 2; ++t) vf[t] = (key < Nk && 2 * t + h < dv) ? Vb[(int64_t)(2 * t + h) * Nk + key] : 0.0f;
    f32x16 aK[D / 32], aV[DV / 32];
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) aK[i][x] = 0.0f;
#pragma unroll
    for (int i = 0; i < DV / 32; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) aV[i][x] = 0.0f;
    const float c = p.scale_log2;
    const float* nD = p.nD + (int64_t)b * N;
    const float* nL = p.nlse + (int64_t)b * N;
    int qbeg = 0;   // causal: the first query tile that sees the block's first key
    if constexpr (CAUSAL) qbeg = max(0, k0 - p.off) / kF32T * kF32T;
    int qend = N;   // local: the queries that see some key of the block (none: zeros are stored)
    const VarlenExt e = bwd_ext<VARLEN>(p, b);
    if constexpr (LOCAL) {
        qbeg = max(0, k0 - e.off - e.right) / kF32T * kF32T;
        qend = min(e.nq, k0 + 127 - e.off + e.left + 1);
        if (VARLEN && k0 >= e.nk) qend = 0;   // a block past nk: zeros are stored
    }
    for (int q0 = qbeg; q0 < qend; q0 += kF32T) {
        __syncthreads();
        for (int i = tid; i < D * kF32T; i += 256) {
            const int q = i % kF32T, f = i / kF32T;
            sQ[f * kF32R + q] = (q0 + q < N && f < d) ? Qb[(int64_t)f * N + q0 + q] : 0.0f;
        }
        for (int i = tid; i < DV * kF32T; i += 256) {
            const int q = i % kF32T, f = i / kF32T;
            sdO[f * kF32R + q] = (q0 + q < N && f < dv) ? dOb[(int64_t)f * N + q0 + q] : 0.0f;
        }
        if (tid < kF32T) {
            sL[tid] = q0 + tid < N ? nL[q0 + tid] : kNegInf;
            sD[tid] = q0 + tid < N ? nD[q0 + tid] : 0.0f;
        }
        __syncthreads();
        f32x16 sa, pa;
#pragma unroll
        for (int x = 0; x < 16; ++x) { sa[x] = 0.0f; pa[x] = 0.0f; }
#pragma unroll
        for (int t = 0; t < D / 2; ++t) sa = mfma32x32x2(sQ[(2 * t + h) * kF32R + r], kf[t], sa);
#pragma unroll
        for (int t = 0; t < DV / 2; ++t) pa = mfma32x32x2(sdO[(2 * t + h) * kF32R + r], vf[t], pa);
        // lane (r, h): key r; register x: query acc_row(x, h)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int q = acc_row(x, h);
            if constexpr (CAUSAL) {              // select after the chain: P = exp2(-inf) = 0
                if (key > q0 + q + p.off) sa[x] = kNegInf;
            }
            if constexpr (LOCAL) {
                if (key > q0 + q + e.off + e.right || key < q0 + q + e.off - e.left) sa[x] = kNegInf;
            }
            if constexpr (VARLEN) {   // the key column past nk (rows past nq carry sL = -inf)
                if (key >= e.nk) sa[x] = kNegInf;
            }
            const float pr = exp2f((sa[x] + sL[q]) * c);
            sa[x] = pr;                          // P
            pa[x] = pr * (pa[x] + sD[q]);        // dS
        }
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int q = acc_row(x, h);
#pragma unroll
            for (int i = 0; i < DV / 32; ++i) aV[i] = mfma32x32x2(sdO[(i * 32 + r) * kF32R + q], sa[x], aV[i]);
#pragma unroll
            for (int i = 0; i < D / 32; ++i) aK[i] = mfma32x32x2(sQ[(i * 32 + r) * kF32R + q], pa[x], aK[i]);
        }
    }
    if (key < Nk) {
        float* dKb = (float*)p.dK + (int64_t)b * Nk * d;
        float* dVb = (float*)p.dV + (int64_t)b * Nk * dv;
#pragma unroll
        for (int i = 0; i < D / 32; ++i)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = i * 32 + acc_row(x, h);
                if (f < d) dKb[(int64_t)f * Nk + key] = aK[i][x] * p.scale;
            }
#pragma unroll
        for (int i = 0; i < DV / 32; ++i)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = i * 32 + acc_row(x, h);
                if (f < dv) dVb[(int64_t)f * Nk + key] = aV[i][x];
            }
    }
}

template <int D, int DV, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(256) void bwd_dq_f32(BwdParams p) {
    constexpr bool CAUSAL = MASK == kMaskCausal, LOCAL = MASK == kMaskLocal || MASK == kMaskVarlen, VARLEN = MASK == kMaskVarlen;
    __shared__ float sK[D * kF32R], sV[DV * kF32R];
    const int N = p.N, Nk = p.Nk, d = p.d, dv = p.dv;
    const int nqb = (N + 127) / 128;
    const int b = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const float* Qb = (const float*)p.Q + (int64_t)b * N * d;
    const float* dOb = (const float*)p.dO + (int64_t)b * N * dv;
    const float* Kb = (const float*)p.K + (int64_t)b * Nk * d;
    const float* Vb = (const float*)p.V + (int64_t)b * Nk * dv;
    const int qi = q0 + wave * 32 + r;
    float qf[D / 2], df[DV / 2];
#pragma unroll
    for (int t = 0; t < D / 2; ++t) qf[t] = (qi < N && 2 * t + h < d) ? Qb[(int64_t)(2 * t + h) * N + qi] : 0.0f;
#pragma unroll
    for (int t = 0; t < DV / 2; ++t) df[t] = (qi < N && 2 * t + h < dv) ? dOb[(int64_t)(2 * t + h) * N + qi] : 0.0f;
    const float nlq = qi < N ? p.nlse[(int64_t)b * N + qi] : kNegInf;
    const float ndq = qi < N ? p.nD[(int64_t)b * N + qi] : 0.0f;
    const float c = p.scale_log2;
    f32x16 aQ[D / 32];
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) aQ[i][x] = 0.0f;
    int kend = Nk;   // causal: keys up to the block's last real query's limit
    if constexpr (CAUSAL) kend = min(Nk, min(q0 + 127, N - 1) + p.off + 1);
    int kbeg = 0;   // local: from the block's first query's left edge to its last real query's right edge
    const VarlenExt e = bwd_ext<VARLEN>(p, b);
    if constexpr (LOCAL) {   // (VARLEN: possibly no step; zeros are stored)
        kbeg = max(0, q0 + e.off - e.left) / kF32T * kF32T;
        kend = min(e.nk, min(q0 + 127, e.nq - 1) + e.off + e.right + 1);
    }
    for (int k0 = kbeg; k0 < kend; k0 += kF32T) {
        __syncthreads();
        for (int i = tid; i < D * kF32T; i += 256) {
            const int k = i % kF32T, f = i / kF32T;
            sK[f * kF32R + k] = (k0 + k < Nk && f < d) ? Kb[(int64_t)f * Nk + k0 + k] : 0.0f;
        }
        for (int i = tid; i < DV * kF32T; i += 256) {
            const int k = i % kF32T, f = i / kF32T;
            sV[f * kF32R + k] = (k0 + k < Nk && f < dv) ? Vb[(int64_t)f * Nk + k0 + k] : 0.0f;
        }
        __syncthreads();
        f32x16 sa, pa;
#pragma unroll
        for (int x = 0; x < 16; ++x) { sa[x] = 0.0f; pa[x] = 0.0f; }
#pragma unroll
        for (int t = 0; t < D / 2; ++t) sa = mfma32x32x2(sK[(2 * t + h) * kF32R + r], qf[t], sa);
#pragma unroll
        for (int t = 0; t < DV / 2; ++t) pa = mfma32x32x2(sV[(2 * t + h) * kF32R + r], df[t], pa);
        // lane (r, h): query r; register x: key acc_row(x, h)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            if constexpr (CAUSAL) {
                if (k0 + acc_row(x, h) > qi + p.off) sa[x] = kNegInf;
            }
            if constexpr (LOCAL) {
                if (k0 + acc_row(x, h) > qi + e.off + e.right || k0 + acc_row(x, h) < qi + e.off - e.left) sa[x] = kNegInf;
            }
            if (k0 + kF32T > e.nk && k0 + acc_row(x, h) >= e.nk) sa[x] = kNegInf;   // the ragged last tile
            const float pr = exp2f((sa[x] + nlq) * c);
            pa[x] = pr * (pa[x] + ndq);          // dSᵀ
        }
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int k = acc_row(x, h);
#pragma unroll
            for (int i = 0; i < D / 32; ++i) aQ[i] = mfma32x32x2(sK[(i * 32 + r) * kF32R + k], pa[x], aQ[i]);
        }
    }
    if (qi < N) {
        float* dQb = (float*)p.dQ + (int64_t)b * N * d;
#pragma unroll
        for (int i = 0; i < D / 32; ++i)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = i * 32 + acc_row(x, h);
                if (f < d) dQb[(int64_t)f * N + qi] = aQ[i][x] * p.scale;
            }
    }
}

template <int D, int DV>
static hipError_t launch_f32_dd(const BwdParams& p, DenseMask mask, hipStream_t s) {
    const int64_t nq = ((int64_t)p.N + 127) / 128 * p.batch, nk = ((int64_t)p.Nk + 127) / 128 * p.batch;
    by_mask(mask, [&](auto M) {
        hipLaunchKernelGGL((bwd_dq_f32<D, DV, decltype(M)::value>), dim3((unsigned)nq), dim3(256), 0, s, p);
        hipLaunchKernelGGL((bwd_dkdv_f32<D, DV, decltype(M)::value>), dim3((unsigned)nk), dim3(256), 0, s, p);
    });
    return hipGetLastError();
}
// (five class pairs, not nine: any d or dv above 64 runs the 128 x 128 kernels)
hipError_t launch_f32_mfma(const BwdParams& p, DenseMask mask, hipStream_t s) {
    if (p.d > 64 || p.dv > 64) return launch_f32_dd<128, 128>(p, mask, s);
    const int Dc = p.d <= 32 ? 32 : 64, DVc = p.dv <= 32 ? 32 : 64;
    if (Dc == 32 && DVc == 32) return launch_f32_dd<32, 32>(p, mask, s);
    if (Dc == 32) return launch_f32_dd<32, 64>(p, mask, s);
    if (DVc == 32) return launch_f32_dd<64, 32>(p, mask, s);
    return launch_f32_dd<64, 64>(p, mask, s);
}

}  // namespace fa
