// fa_bwd_simt_dq.hip — dense backward, the dQ pass of the LDS-tiled SIMT path: ragged or
// unaligned shapes of every dtype, Float64, and the parity reference of the MFMA paths.  (The
// SIMT dK/dV pass, fa_bwd_simt_dkdv.hip, is the same tiling from the keys' side; the two are
// separate files because each takes a minute to compile.)  Exports launch_generic_dq.
#include "fa_common.h"
#include "fa_bwd_params.h"

namespace fa {

// --------------------------------------------------------------------------
// 2./3. generic SIMT path.  Tiles (kGT, fa_bwd_params.h) of 32 queries x 32 keys in LDS, arithmetic in
// A: float for the 16/32-bit types, double for Float64 (whose row statistics
// nD / nlse are double too, fa_f64.hip).  LDS rows hold d + 1 (dv + 1) elements,
// so the per-key / per-query row reads of 32 lanes fall in distinct banks.
// --------------------------------------------------------------------------

// dQ: one block per (b, 32-query tile).
template <class T, class A, DenseMask MASK = kMaskNone>
__global__ __launch_bounds__(kGThreads) void bwd_generic_dq(BwdParams p) {
    constexpr bool CAUSAL = MASK == kMaskCausal, LOCAL = MASK == kMaskLocal || MASK == kMaskVarlen, VARLEN = MASK == kMaskVarlen;
    extern __shared__ __attribute__((aligned(16))) char gsm_raw[];
    A* const gsm = (A*)gsm_raw;
    const int d = p.d, dv = p.dv, N = p.N, Nk = p.Nk, ld = d + 1, ldv = dv + 1;
    A* sQ = gsm;                         // [32][d+1]
    A* sdO = sQ + kGT * ld;              // [32][dv+1]
    A* sK = sdO + kGT * ldv;             // [32][d+1]
    A* sV = sK + kGT * ld;               // [32][dv+1]
    A* sdS = sV + kGT * ldv;             // [32 q][33]
    const int nqt = (N + kGT - 1) / kGT;
    const int b = blockIdx.x / nqt, q0 = (blockIdx.x % nqt) * kGT;
    const int tid = threadIdx.x;
    const T* Qb = (const T*)p.Q + (int64_t)b * N * d;
    const T* Kb = (const T*)p.K + (int64_t)b * Nk * d;
    const T* Vb = (const T*)p.V + (int64_t)b * Nk * dv;
    const T* dOb = (const T*)p.dO + (int64_t)b * N * dv;
    for (int i = tid; i < kGT * d; i += kGThreads) {
        const int q = i % kGT, f = i / kGT;
        sQ[q * ld + f] = (q0 + q < N) ? (A)Qb[(int64_t)f * N + q0 + q] : (A)0;
    }
    for (int i = tid; i < kGT * dv; i += kGThreads) {
        const int q = i % kGT, f = i / kGT;
        sdO[q * ldv + f] = (q0 + q < N) ? (A)dOb[(int64_t)f * N + q0 + q] : (A)0;
    }
    // each thread owns dQ entries (q, f) = (i % 32, i / 32) for i = tid + 256·t
    constexpr int kMaxPer = 128 * kGT / kGThreads;   // d <= 128
    A acc[kMaxPer];
#pragma unroll
    for (int t = 0; t < kMaxPer; ++t) acc[t] = (A)0;
    const A* nD = (const A*)p.nD + (int64_t)b * N;
    const A* nL = (const A*)p.nlse + (int64_t)b * N;
    const A sl2 = scale_log2_a<A>(p.scale_log2, p.scale64);
    const VarlenExt x = bwd_ext<VARLEN>(p, b);   // VARLEN: the slab's extents (else N, Nk, p.off, the window)
    int kend = Nk;   // causal: keys up to the tile's last real query's limit
    if constexpr (CAUSAL) kend = min(Nk, min(q0 + kGT - 1, N - 1) + p.off + 1);
    int kbeg = 0;    // local: from the tile's first query's left edge to its last real query's right edge
    if constexpr (LOCAL) {   // (VARLEN: no step for a tile past nq or whose queries see no key; zeros are stored)
        kbeg = max(0, q0 + x.off - x.left) / kGT * kGT;
        kend = min(x.nk, min(q0 + kGT - 1, x.nq - 1) + x.off + x.right + 1);
    }
    for (int k0 = kbeg; k0 < kend; k0 += kGT) {
        __syncthreads();
        for (int i = tid; i < kGT * d; i += kGThreads) {
            const int k = i % kGT, f = i / kGT;
            sK[k * ld + f] = (k0 + k < Nk) ? (A)Kb[(int64_t)f * Nk + k0 + k] : (A)0;
        }
        for (int i = tid; i < kGT * dv; i += kGThreads) {
            const int k = i % kGT, f = i / kGT;
            sV[k * ldv + f] = (k0 + k < Nk) ? (A)Vb[(int64_t)f * Nk + k0 + k] : (A)0;
        }
        __syncthreads();
        for (int e = tid; e < kGT * kGT; e += kGThreads) {
            const int q = e / kGT, k = e % kGT;
            A ds = (A)0;
            bool vis = q0 + q < N && k0 + k < Nk;
            if constexpr (CAUSAL) vis = vis && k0 + k <= q0 + q + p.off;
            if constexpr (LOCAL) vis = vis && k0 + k <= q0 + q + x.off + x.right && k0 + k >= q0 + q + x.off - x.left;
            if constexpr (VARLEN) vis = vis && q0 + q < x.nq && k0 + k < x.nk;
            if (vis) {
                A s = (A)0, dp = (A)0;
                for (int f = 0; f < d; ++f) s = fma_a(sQ[q * ld + f], sK[k * ld + f], s);
                for (int f = 0; f < dv; ++f) dp = fma_a(sdO[q * ldv + f], sV[k * ldv + f], dp);
                const A pr = exp2_a((s + nL[q0 + q]) * sl2);
                ds = pr * (dp + nD[q0 + q]);
            }
            sdS[q * (kGT + 1) + k] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kMaxPer; ++t) {
            const int i = tid + kGThreads * t, q = i % kGT, f = i / kGT;
            if (f < d) {
                A a = acc[t];
                for (int k = 0; k < kGT; ++k) a = fma_a(sdS[q * (kGT + 1) + k], sK[k * ld + f], a);
                acc[t] = a;
            }
        }
    }
    T* dQb = (T*)p.dQ + (int64_t)b * N * d;
    const A sc = scale_a<A>(p.scale, p.scale64);
#pragma unroll
    for (int t = 0; t < kMaxPer; ++t) {
        const int i = tid + kGThreads * t, q = i % kGT, f = i / kGT;
        if (f < d && q0 + q < N) dQb[(int64_t)f * N + q0 + q] = (T)(acc[t] * sc);
    }
}

template <class T, class A>
hipError_t launch_generic_dq(const BwdParams& p, DenseMask mask, hipStream_t s) {
    const int64_t nq = ((int64_t)p.N + kGT - 1) / kGT * p.batch;
    const size_t sm_dq = sizeof(A) * (kGT * (2 * (p.d + 1) + 2 * (p.dv + 1)) + kGT * (kGT + 1));
    by_mask(mask, [&](auto M) {
        void (*dq)(BwdParams) = bwd_generic_dq<T, A, decltype(M)::value>;
        // > 64 KiB of dynamic LDS at d = dv = 128 (gfx950 has 160 KiB per CU)
        (void)hipFuncSetAttribute((const void*)dq, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm_dq);
        hipLaunchKernelGGL(dq, dim3((unsigned)nq), dim3(kGThreads), sm_dq, s, p);
    });
    return hipGetLastError();
}
template hipError_t launch_generic_dq<bf16, float>(const BwdParams&, DenseMask, hipStream_t);
template hipError_t launch_generic_dq<f16, float>(const BwdParams&, DenseMask, hipStream_t);
template hipError_t launch_generic_dq<float, float>(const BwdParams&, DenseMask, hipStream_t);
template hipError_t launch_generic_dq<double, double>(const BwdParams&, DenseMask, hipStream_t);

}  // namespace fa
