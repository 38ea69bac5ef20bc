// fa_bwd_simt_dkdv.hip — dense backward, the dK/dV pass of the LDS-tiled SIMT path (see
// fa_bwd_simt_dq.hip: the same 32 x 32 tiles in LDS, arithmetic in A, rows of d + 1 elements).
// Exports launch_generic_dkdv.
#include "fa_common.h"
#include "fa_bwd_params.h"

namespace fa {

// dK, dV: one block per (b, 32-key tile).
template <class T, class A, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(kGThreads) void bwd_generic_dkdv(BwdParams p) {
    constexpr bool CAUSAL = MASK == kMaskCausal, LOCAL = MASK == kMaskLocal || MASK == kMaskVarlen, VARLEN = MASK == kMaskVarlen;
    extern __shared__ __attribute__((aligned(16))) char gsm_raw[];
    A* const gsm = (A*)gsm_raw;
    const int d = p.d, dv = p.dv, N = p.N, Nk = p.Nk, ld = d + 1, ldv = dv + 1;
    A* sK = gsm;                         // [32][d+1]
    A* sV = sK + kGT * ld;               // [32][dv+1]
    A* sQ = sV + kGT * ldv;              // [32][d+1]
    A* sdO = sQ + kGT * ld;              // [32][dv+1]
    A* sP = sdO + kGT * ldv;             // [32 q][33]
    A* sdS = sP + kGT * (kGT + 1);       // [32 q][33]
    const int nkt = (Nk + kGT - 1) / kGT;
    const int b = blockIdx.x / nkt, k0 = (blockIdx.x % nkt) * kGT;
    const int tid = threadIdx.x;
    const T* Qb = (const T*)p.Q + (int64_t)b * N * d;
    const T* Kb = (const T*)p.K + (int64_t)b * Nk * d;
    const T* Vb = (const T*)p.V + (int64_t)b * Nk * dv;
    const T* dOb = (const T*)p.dO + (int64_t)b * N * dv;
    for (int i = tid; i < kGT * d; i += kGThreads) {
        const int k = i % kGT, f = i / kGT;
        sK[k * ld + f] = (k0 + k < Nk) ? (A)Kb[(int64_t)f * Nk + k0 + k] : (A)0;
    }
    for (int i = tid; i < kGT * dv; i += kGThreads) {
        const int k = i % kGT, f = i / kGT;
        sV[k * ldv + f] = (k0 + k < Nk) ? (A)Vb[(int64_t)f * Nk + k0 + k] : (A)0;
    }
    constexpr int kMaxPer = 128 * kGT / kGThreads;
    A accK[kMaxPer], accV[kMaxPer];
#pragma unroll
    for (int t = 0; t < kMaxPer; ++t) { accK[t] = (A)0; accV[t] = (A)0; }
    const A* nD = (const A*)p.nD + (int64_t)b * N;
    const A* nL = (const A*)p.nlse + (int64_t)b * N;
    const A sl2 = scale_log2_a<A>(p.scale_log2, p.scale64);
    int qbeg = 0;   // causal: the first query tile that sees the block's first key
    if constexpr (CAUSAL) qbeg = max(0, k0 - p.off) / kGT * kGT;
    // local: the queries i that see some key of the tile, k0 - off - right <= i <= k0 + 31 - off + left;
    // none for keys left of every window (the loop then runs no step and zeros are stored)
    int qend = N;
    const VarlenExt x = bwd_ext<VARLEN>(p, b);
    if constexpr (LOCAL) {
        qbeg = max(0, k0 - x.off - x.right) / kGT * kGT;
        qend = min(x.nq, k0 + kGT - 1 - x.off + x.left + 1);
        if (VARLEN && k0 >= x.nk) qend = 0;   // a tile past nk: zeros are stored
    }
    for (int q0 = qbeg; q0 < qend; q0 += kGT) {
        __syncthreads();
        for (int i = tid; i < kGT * d; i += kGThreads) {
            const int q = i % kGT, f = i / kGT;
            sQ[q * ld + f] = (q0 + q < N) ? (A)Qb[(int64_t)f * N + q0 + q] : (A)0;
        }
        for (int i = tid; i < kGT * dv; i += kGThreads) {
            const int q = i % kGT, f = i / kGT;
            sdO[q * ldv + f] = (q0 + q < N) ? (A)dOb[(int64_t)f * N + q0 + q] : (A)0;
        }
        __syncthreads();
        for (int e = tid; e < kGT * kGT; e += kGThreads) {
            const int q = e / kGT, k = e % kGT;
            A pr = (A)0, ds = (A)0;
            bool vis = q0 + q < N && k0 + k < Nk;
            if constexpr (CAUSAL) vis = vis && k0 + k <= q0 + q + p.off;
            if constexpr (LOCAL) vis = vis && k0 + k <= q0 + q + x.off + x.right && k0 + k >= q0 + q + x.off - x.left;
            if constexpr (VARLEN) vis = vis && q0 + q < x.nq && k0 + k < x.nk;
            if (vis) {
                A s = (A)0, dp = (A)0;
                for (int f = 0; f < d; ++f) s = fma_a(sQ[q * ld + f], sK[k * ld + f], s);
                for (int f = 0; f < dv; ++f) dp = fma_a(sdO[q * ldv + f], sV[k * ldv + f], dp);
                pr = exp2_a((s + nL[q0 + q]) * sl2);
                ds = pr * (dp + nD[q0 + q]);
            }
            sP[q * (kGT + 1) + k] = pr;
            sdS[q * (kGT + 1) + k] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kMaxPer; ++t) {
            const int i = tid + kGThreads * t, k = i % kGT, f = i / kGT;
            if (f < d) {
                A a = accK[t];
                for (int q = 0; q < kGT; ++q) a = fma_a(sdS[q * (kGT + 1) + k], sQ[q * ld + f], a);
                accK[t] = a;
            }
            if (f < dv) {
                A a = accV[t];
                for (int q = 0; q < kGT; ++q) a = fma_a(sP[q * (kGT + 1) + k], sdO[q * ldv + f], a);
                accV[t] = a;
            }
        }
    }
    T* dKb = (T*)p.dK + (int64_t)b * Nk * d;
    T* dVb = (T*)p.dV + (int64_t)b * Nk * dv;
    const A sc = scale_a<A>(p.scale, p.scale64);
#pragma unroll
    for (int t = 0; t < kMaxPer; ++t) {
        const int i = tid + kGThreads * t, k = i % kGT, f = i / kGT;
        if (k0 + k < Nk) {
            if (f < d) dKb[(int64_t)f * Nk + k0 + k] = (T)(accK[t] * sc);
            if (f < dv) dVb[(int64_t)f * Nk + k0 + k] = (T)accV[t];
        }
    }
}

template <class T, class A>
hipError_t launch_generic_dkdv(const BwdParams& p, DenseMask mask, hipStream_t s) {
    const int64_t nk = ((int64_t)p.Nk + kGT - 1) / kGT * p.batch;
    const size_t sm_kv = sizeof(A) * (kGT * (2 * (p.d + 1) + 2 * (p.dv + 1)) + 2 * kGT * (kGT + 1));
    by_mask(mask, [&](auto M) {
        void (*dkdv)(BwdParams) = bwd_generic_dkdv<T, A, decltype(M)::value>;
        // > 64 KiB of dynamic LDS at d = dv = 128 (gfx950 has 160 KiB per CU)
        (void)hipFuncSetAttribute((const void*)dkdv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm_kv);
        hipLaunchKernelGGL(dkdv, dim3((unsigned)nk), dim3(kGThreads), sm_kv, s, p);
    });
    return hipGetLastError();
}
template hipError_t launch_generic_dkdv<bf16, float>(const BwdParams&, DenseMask, hipStream_t);
template hipError_t launch_generic_dkdv<f16, float>(const BwdParams&, DenseMask, hipStream_t);
template hipError_t launch_generic_dkdv<float, float>(const BwdParams&, DenseMask, hipStream_t);
template hipError_t launch_generic_dkdv<double, double>(const BwdParams&, DenseMask, hipStream_t);

}  // namespace fa
