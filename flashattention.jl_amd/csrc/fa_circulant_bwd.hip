// fa_circulant_bwd.hip — gradients of circulant (periodic banded) flash attention
// (fa_circulant.hip) for gfx950.  The reference has no backward for circulant_fa!;
// the math is the dense backward's restricted to the band:
//   key(i, t) = (i − p + t) mod N, t = 0..W−1, p = (W−1) ÷ 2
//   s = τ q_i·k_j   P = exp(s − m_i) / l_i   dP = dO_i·v_j   D_i = dO_i·O_i   dS = P (dP − D_i)
//   dQ_i = τ Σ_t dS k_j    dK_j = τ Σ_{(i,t)→j} dS q_i    dV_j = Σ_{(i,t)→j} P dO_i
// W > N repeats keys; every band entry counts once, as in the forward.
//
// Three launches, no sum across workgroups (so no atomics and bitwise reproducible
// gradients):
//  1. circ_bwd_prepass: −D_i and −(m_i + ln l_i)/τ per query into the workspace.
//  2. dQ, query-stationary.  A workgroup owns consecutive queries and streams the
//     union of their bands, consecutive circular key positions, through LDS.
//  3. dK / dV, key-stationary.  Key j is attended by the queries i = j + p − t, so a
//     workgroup of consecutive keys streams the consecutive circular QUERY positions
//     starting at (j0 + p − W + 1) mod N, with their row constants.
// S and dP are computed in both passes (7 products against the minimal 5): the band
// is HBM-bound below W ≈ 600 and an ordered dQ hand-off across the ⌈W/128⌉ + 1 key
// blocks of a query costs more than the two products.
//
// Kernels:
//  * circ_bwd_dq_tiled / circ_bwd_dkdv_tiled (bf16 / fp16, N % 8 == 0, 16-B aligned
//    inputs): 4 waves x 32 queries (keys), 64-position tiles in the dense backward's
//    swizzled [feature][64 tokens] LDS images and MFMA fragments (fa_bwd_common.h);
//    tiles are staged through registers (buffer loads return 0 past the slab, which
//    zero-fills the features d..D−1 of a head dim inside a class) and double-buffered.
//    A wave computes only the tiles that intersect its 32 bands and applies the
//    forward's per-element band test only on tiles not inside every one of them.
//  * circ_bwd_dq_simt / circ_bwd_dkdv_simt (every dtype, any N / alignment): 32 x 32
//    tiles in LDS, arithmetic in A = float (exact fp32 dot products) or, for Float64,
//    double with the row statistics recomputed in double by the pre-pass.
#include "fa_bwd_common.h"
#include "fa_circulant_plan.h"
#include "fa_internal.h"
#include "../../include/fa_hip.h"

namespace fa {

thread_local int g_circ_bwd_last_kernel = 0;   // 0 none, 1 MFMA tiled, 2 SIMT, 3 Float64

struct CircBwdParams {
    const void *Q, *K, *V, *O, *dO;
    const float *l, *m;
    void *dQ, *dK, *dV;
    void* nD;     // workspace: −rowsum(dO ∘ O)           [batch][N], float (double: Float64)
    void* nlse;   // workspace: −(m + ln l)/τ (raw units)  [batch][N]
    int N, d, dv, W, p;
    int nblk, total_wg;          // tiled path: 128-token blocks per slab, workgroups
    int64_t batch;
    float scale, scale_log2;
    double scale64;
};

// (x mod N) in [0, N) for any sign of x
__device__ __forceinline__ int cb_mod(int64_t x, int N) {
    const int64_t r = x % N;
    return (int)(r < 0 ? r + N : r);
}

// --------------------------------------------------------------------------
// 1. pre-pass: one thread per (b, n), coalesced along n.  Float64 recomputes the
// row statistics in double from Q, K (the float32 l, m are not read), as the dense
// Float64 backward does.
// --------------------------------------------------------------------------
template <class T, class A>
__global__ __launch_bounds__(256) void circ_bwd_prepass(CircBwdParams p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int N = p.N;
    if (idx >= (int64_t)N * p.batch) return;
    const int64_t b = idx / N;
    const int n = (int)(idx - b * N);
    const T* O = (const T*)p.O + b * (int64_t)N * p.dv + n;
    const T* dO = (const T*)p.dO + b * (int64_t)N * p.dv + n;
    A acc = (A)0;
    for (int c = 0; c < p.dv; ++c) acc = fma_a((A)dO[(int64_t)c * N], (A)O[(int64_t)c * N], acc);
    ((A*)p.nD)[idx] = -acc;
    if constexpr (sizeof(A) == 8) {
        const T* Q = (const T*)p.Q + b * (int64_t)N * p.d + n;
        const T* K = (const T*)p.K + b * (int64_t)N * p.d;
        double mx = -__builtin_huge_val(), l = 0.0;
        int key = cb_mod((int64_t)n - p.p, N);
        for (int t = 0; t < p.W; ++t) {
            double s = 0.0;
            for (int f = 0; f < p.d; ++f) s = fma((double)Q[(int64_t)f * N], (double)K[(int64_t)f * N + key], s);
            s *= p.scale64;
            const double mn = __builtin_elementwise_maximum(mx, s);
            l = l * exp(mx - mn) + exp(s - mn);   // mx = −inf first: exp(−inf) = 0
            mx = mn;
            key = key + 1 == N ? 0 : key + 1;
        }
        ((double*)p.nlse)[idx] = -(mx + log(l)) / p.scale64;
    } else {
        ((float*)p.nlse)[idx] = -(p.m[idx] + logf(p.l[idx])) / p.scale;
    }
}

// 16-B variant (bf16 / fp16, N % 8 == 0, O and dO 16-B aligned): 8 queries per thread.
template <class T>
__global__ __launch_bounds__(256) void circ_bwd_prepass_v(CircBwdParams p) {
    const int64_t g8 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g8 >= (int64_t)p.N * p.batch / 8) return;
    prepass_rows8((const T*)p.O, (const T*)p.dO, p.l, p.m, (float*)p.nD, (float*)p.nlse, g8 * 8, p.N, p.dv, p.scale);
}

// W = 1: the softmax over a single band entry is exactly 1, so dS = P (dP − D) = 0:
// dQ = dK = 0 and dV = dO (key(i, 0) = i), written as such.  The general arithmetic
// can only approximate P = 1, since the float32 m = fl(τ s) does not give s back.
template <class T>
__global__ __launch_bounds__(256) void circ_bwd_w1(CircBwdParams p, int64_t nqk, int64_t nv) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nqk || i < nv; i += step) {
        if (i < nqk) {
            ((T*)p.dQ)[i] = (T)0.0f;
            ((T*)p.dK)[i] = (T)0.0f;
        }
        if (i < nv) ((T*)p.dV)[i] = ((const T*)p.dO)[i];
    }
}

// --------------------------------------------------------------------------
// 2./3. SIMT path.  Tiles of 32 queries x 32 keys in LDS (rows of d + 1 / dv + 1
// elements: the per-key / per-query row reads of 32 lanes fall in distinct banks),
// as the dense generic backward; the streamed side walks the band union and each
// (query, position) pair is tested against the band.
// --------------------------------------------------------------------------
constexpr int kCT = 32;
constexpr int kCThreads = 256;

// dQ: one block per (b, 32-query tile); union position u <-> key (base + u) mod N,
// base = q0 − p; query q0 + q attends u in [q, q + W).
template <class T, class A>
__global__ __launch_bounds__(kCThreads) void circ_bwd_dq_simt(CircBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char csm_raw[];
    A* const csm = (A*)csm_raw;
    const int d = p.d, dv = p.dv, N = p.N, W = p.W, ld = d + 1, ldv = dv + 1;
    A* sQ = csm;                         // [32][d+1]
    A* sdO = sQ + kCT * ld;              // [32][dv+1]
    A* sK = sdO + kCT * ldv;             // [32][d+1]
    A* sV = sK + kCT * ld;               // [32][dv+1]
    A* sdS = sV + kCT * ldv;             // [32 q][33]
    const int nqt = (N + kCT - 1) / kCT;
    const int b = blockIdx.x / nqt, q0 = (blockIdx.x % nqt) * kCT;
    const int tid = threadIdx.x;
    const T* Qb = (const T*)p.Q + (int64_t)b * N * d;
    const T* Kb = (const T*)p.K + (int64_t)b * N * d;
    const T* Vb = (const T*)p.V + (int64_t)b * N * dv;
    const T* dOb = (const T*)p.dO + (int64_t)b * N * dv;
    for (int i = tid; i < kCT * d; i += kCThreads) {
        const int q = i % kCT, f = i / kCT;
        sQ[q * ld + f] = (q0 + q < N) ? (A)Qb[(int64_t)f * N + q0 + q] : (A)0;
    }
    for (int i = tid; i < kCT * dv; i += kCThreads) {
        const int q = i % kCT, f = i / kCT;
        sdO[q * ldv + f] = (q0 + q < N) ? (A)dOb[(int64_t)f * N + q0 + q] : (A)0;
    }
    // each thread owns dQ entries (q, f) = (i % 32, i / 32) for i = tid + 256·t
    constexpr int kMaxPer = 128 * kCT / kCThreads;   // d <= 128
    A acc[kMaxPer];
#pragma unroll
    for (int t = 0; t < kMaxPer; ++t) acc[t] = (A)0;
    const A* nD = (const A*)p.nD + (int64_t)b * N;
    const A* nL = (const A*)p.nlse + (int64_t)b * N;
    const A sl2 = scale_log2_a<A>(p.scale_log2, p.scale64);
    const int base = cb_mod((int64_t)q0 - p.p, N);
    const int64_t U = (int64_t)kCT + W - 1;
    for (int64_t u0 = 0; u0 < U; u0 += kCT) {
        const int kb0 = cb_mod(base + u0, N);
        __syncthreads();
        for (int i = tid; i < kCT * d; i += kCThreads) {
            const int k = i % kCT, f = i / kCT;
            sK[k * ld + f] = (A)Kb[(int64_t)f * N + (kb0 + k) % N];
        }
        for (int i = tid; i < kCT * dv; i += kCThreads) {
            const int k = i % kCT, f = i / kCT;
            sV[k * ldv + f] = (A)Vb[(int64_t)f * N + (kb0 + k) % N];
        }
        __syncthreads();
        for (int e = tid; e < kCT * kCT; e += kCThreads) {
            const int q = e / kCT, k = e % kCT;
            const int64_t t = u0 + k - q;   // band entry of (query, position)
            A ds = (A)0;
            if (q0 + q < N && t >= 0 && t < W) {
                A s = (A)0, dp = (A)0;
                for (int f = 0; f < d; ++f) s = fma_a(sQ[q * ld + f], sK[k * ld + f], s);
                for (int f = 0; f < dv; ++f) dp = fma_a(sdO[q * ldv + f], sV[k * ldv + f], dp);
                const A pr = exp2_a((s + nL[q0 + q]) * sl2);
                ds = pr * (dp + nD[q0 + q]);
            }
            sdS[q * (kCT + 1) + k] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kMaxPer; ++t) {
            const int i = tid + kCThreads * t, q = i % kCT, f = i / kCT;
            if (f < d) {
                A a = acc[t];
                for (int k = 0; k < kCT; ++k) a = fma_a(sdS[q * (kCT + 1) + k], sK[k * ld + f], a);
                acc[t] = a;
            }
        }
    }
    T* dQb = (T*)p.dQ + (int64_t)b * N * d;
    const A sc = scale_a<A>(p.scale, p.scale64);
#pragma unroll
    for (int t = 0; t < kMaxPer; ++t) {
        const int i = tid + kCThreads * t, q = i % kCT, f = i / kCT;
        if (f < d && q0 + q < N) dQb[(int64_t)f * N + q0 + q] = (T)(acc[t] * sc);
    }
}

// dK, dV: one block per (b, 32-key tile); union position u <-> query (base + u) mod N,
// base = k0 + p − W + 1; key k0 + k is attended from u in [k, k + W) (band entry
// t = W − 1 − (u − k)).
template <class T, class A>
__global__ __launch_bounds__(kCThreads) void circ_bwd_dkdv_simt(CircBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char csm_raw[];
    A* const csm = (A*)csm_raw;
    const int d = p.d, dv = p.dv, N = p.N, W = p.W, ld = d + 1, ldv = dv + 1;
    A* sK = csm;                         // [32][d+1]
    A* sV = sK + kCT * ld;               // [32][dv+1]
    A* sQ = sV + kCT * ldv;              // [32][d+1]
    A* sdO = sQ + kCT * ld;              // [32][dv+1]
    A* sP = sdO + kCT * ldv;             // [32 q][33]
    A* sdS = sP + kCT * (kCT + 1);       // [32 q][33]
    A* sRow = sdS + kCT * (kCT + 1);     // −lse[32], −D[32] of the tile's queries
    const int nkt = (N + kCT - 1) / kCT;
    const int b = blockIdx.x / nkt, k0 = (blockIdx.x % nkt) * kCT;
    const int tid = threadIdx.x;
    const T* Qb = (const T*)p.Q + (int64_t)b * N * d;
    const T* Kb = (const T*)p.K + (int64_t)b * N * d;
    const T* Vb = (const T*)p.V + (int64_t)b * N * dv;
    const T* dOb = (const T*)p.dO + (int64_t)b * N * dv;
    for (int i = tid; i < kCT * d; i += kCThreads) {
        const int k = i % kCT, f = i / kCT;
        sK[k * ld + f] = (k0 + k < N) ? (A)Kb[(int64_t)f * N + k0 + k] : (A)0;
    }
    for (int i = tid; i < kCT * dv; i += kCThreads) {
        const int k = i % kCT, f = i / kCT;
        sV[k * ldv + f] = (k0 + k < N) ? (A)Vb[(int64_t)f * N + k0 + k] : (A)0;
    }
    constexpr int kMaxPer = 128 * kCT / kCThreads;
    A accK[kMaxPer], accV[kMaxPer];
#pragma unroll
    for (int t = 0; t < kMaxPer; ++t) { accK[t] = (A)0; accV[t] = (A)0; }
    const A* nD = (const A*)p.nD + (int64_t)b * N;
    const A* nL = (const A*)p.nlse + (int64_t)b * N;
    const A sl2 = scale_log2_a<A>(p.scale_log2, p.scale64);
    const int base = cb_mod((int64_t)k0 + p.p - W + 1, N);
    const int64_t U = (int64_t)kCT + W - 1;
    for (int64_t u0 = 0; u0 < U; u0 += kCT) {
        const int qb0 = cb_mod(base + u0, N);
        __syncthreads();
        for (int i = tid; i < kCT * d; i += kCThreads) {
            const int q = i % kCT, f = i / kCT;
            sQ[q * ld + f] = (A)Qb[(int64_t)f * N + (qb0 + q) % N];
        }
        for (int i = tid; i < kCT * dv; i += kCThreads) {
            const int q = i % kCT, f = i / kCT;
            sdO[q * ldv + f] = (A)dOb[(int64_t)f * N + (qb0 + q) % N];
        }
        if (tid < kCT) sRow[tid] = nL[(qb0 + tid) % N];
        else if (tid < 2 * kCT) sRow[tid] = nD[(qb0 + tid - kCT) % N];
        __syncthreads();
        for (int e = tid; e < kCT * kCT; e += kCThreads) {
            const int q = e / kCT, k = e % kCT;
            const int64_t t = u0 + q - k;
            A pr = (A)0, ds = (A)0;
            if (k0 + k < N && t >= 0 && t < W) {
                A s = (A)0, dp = (A)0;
                for (int f = 0; f < d; ++f) s = fma_a(sQ[q * ld + f], sK[k * ld + f], s);
                for (int f = 0; f < dv; ++f) dp = fma_a(sdO[q * ldv + f], sV[k * ldv + f], dp);
                pr = exp2_a((s + sRow[q]) * sl2);
                ds = pr * (dp + sRow[kCT + q]);
            }
            sP[q * (kCT + 1) + k] = pr;
            sdS[q * (kCT + 1) + k] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kMaxPer; ++t) {
            const int i = tid + kCThreads * t, k = i % kCT, f = i / kCT;
            if (f < d) {
                A a = accK[t];
                for (int q = 0; q < kCT; ++q) a = fma_a(sdS[q * (kCT + 1) + k], sQ[q * ld + f], a);
                accK[t] = a;
            }
            if (f < dv) {
                A a = accV[t];
                for (int q = 0; q < kCT; ++q) a = fma_a(sP[q * (kCT + 1) + k], sdO[q * ldv + f], a);
                accV[t] = a;
            }
        }
    }
    T* dKb = (T*)p.dK + (int64_t)b * N * d;
    T* dVb = (T*)p.dV + (int64_t)b * N * dv;
    const A sc = scale_a<A>(p.scale, p.scale64);
#pragma unroll
    for (int t = 0; t < kMaxPer; ++t) {
        const int i = tid + kCThreads * t, k = i % kCT, f = i / kCT;
        if (k0 + k < N) {
            if (f < d) dKb[(int64_t)f * N + k0 + k] = (T)(accK[t] * sc);
            if (f < dv) dVb[(int64_t)f * N + k0 + k] = (T)accV[t];
        }
    }
}

// --------------------------------------------------------------------------
// 2./3. MFMA path.  LDS images and fragments are the dense backward's, the swizzled
// [rows][64 tokens] image of fa_bwd_common.h (img_chunk, ImgReader).  Here a tile's
// 8-token chunks are loaded to registers (a chunk never straddles N: the union start
// is rounded down to 8 and N % 8 == 0) and written to LDS one iteration later.
// --------------------------------------------------------------------------
constexpr int kOobOffset = 0x7FFFFFF0;   // past every slab (extent < INT32_MAX): reads 0

// Registers <- the [R rows][64 tokens] tile whose first token is tok0 (< N, % 8 == 0)
// of a [rows][N] slab; 256 threads, chunk P = 256·it + tid is the image's P-th 16 B.
template <class T, int R>
__device__ __forceinline__ void cb_gload(u32x4 (&reg)[R / 32], __amdgpu_buffer_rsrc_t rs, int rows, int N,
                                         int tok0, int tid) {
#pragma unroll
    for (int it = 0; it < R / 32; ++it) {
        const ImgChunk ch = img_chunk(it * 256 + tid);
        const int tok = (tok0 + 8 * ch.c) % N;
        reg[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, ch.f < rows ? (ch.f * N + tok) * (int)sizeof(T) : kOobOffset, 0, 0);
    }
}
template <int R>
__device__ __forceinline__ void cb_lstore(char* img, const u32x4 (&reg)[R / 32], int tid) {
#pragma unroll
    for (int it = 0; it < R / 32; ++it) *(u32x4*)(img + (it * 256 + tid) * 16) = reg[it];
}

// B-operand fragments of the stationary side: element e of step s is feature
// 16 s + 8 h + e of token tok (zero past the head dim or past N).
template <class T, int D>
__device__ __forceinline__ void cb_load_frag(typename Frag8<T>::type (&fr)[D / 16], __amdgpu_buffer_rsrc_t rs,
                                             int rows, int N, int tok, int h) {
#pragma unroll
    for (int s = 0; s < D / 16; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int f = 16 * s + 8 * h + e;
            fr[s][e] = __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b16(
                                                 rs, (f < rows && tok < N) ? (f * N + tok) * 2 : kOobOffset, 0, 0));
        }
}

// Band union of a 128-token workgroup whose first band position is s0 (mod N):
// positions u <-> tokens (k0 + u) mod N with k0 = s0 rounded down to an 8-token
// chunk; stationary token c (0..127) meets u in [c + off, c + off + W − 1].
struct CbUnion {
    int k0, off, NT;
};
__device__ __forceinline__ CbUnion cb_union(int s0, int W) {
    CbUnion u;
    u.k0 = s0 & ~7;
    u.off = s0 - u.k0;
    u.NT = (128 + u.off + W - 1 + 63) / 64;
    return u;
}

template <class T, int D, int DV>
__global__ __launch_bounds__(256, (D + DV > 192) ? 1 : 2) void circ_bwd_dq_tiled(CircBwdParams p) {
    typedef typename Frag8<T>::type F8;
    constexpr int KB = D * 128, VB = DV * 128, STAGE = KB + VB;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int b = lid / p.nblk, qb = lid - b * p.nblk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int N = p.N, d = p.d, dv = p.dv, W = p.W;
    const auto qrs = slab_rsrc((const T*)p.Q + (int64_t)b * N * d, (uint32_t)(N * d * 2));
    const auto ors = slab_rsrc((const T*)p.dO + (int64_t)b * N * dv, (uint32_t)(N * dv * 2));
    const auto krs = slab_rsrc((const T*)p.K + (int64_t)b * N * d, (uint32_t)(N * d * 2));
    const auto vrs = slab_rsrc((const T*)p.V + (int64_t)b * N * dv, (uint32_t)(N * dv * 2));
    const int q0 = qb * 128;
    const CbUnion un = cb_union(cb_mod((int64_t)q0 - p.p, N), W);
    const int off = un.off, NT = un.NT;
    // this wave's queries 32·wave + r attend u in [32·wave + r + off, … + W − 1]
    const int tlo = (32 * wave + off) / 64;
    const int thi = min(NT - 1, (32 * wave + 31 + off + W - 1) / 64);
    const int qi = q0 + wave * 32 + r;
    F8 qf[D / 16], df[DV / 16];
    cb_load_frag<T, D>(qf, qrs, d, N, qi, h);
    cb_load_frag<T, DV>(df, ors, dv, N, qi, h);
    const int qc = qi < N ? qi : N - 1;
    const float c = p.scale_log2;
    const float cnl = c * ((const float*)p.nlse)[(int64_t)b * N + qc];
    const float nDq = ((const float*)p.nD)[(int64_t)b * N + qc];

    const ImgReader<T> rd(tid);

    f32x16 dq[D / 32];
#pragma unroll
    for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) dq[cb][x] = 0.0f;

    u32x4 kreg[D / 32], vreg[DV / 32];
    auto gload = [&](int t) {
        const int tok0 = (int)(((int64_t)un.k0 + (int64_t)t * 64) % N);
        cb_gload<T, D>(kreg, krs, d, N, tok0, tid);
        cb_gload<T, DV>(vreg, vrs, dv, N, tok0, tid);
    };
    auto lstore = [&](char* st) {
        cb_lstore<D>(st, kreg, tid);
        cb_lstore<DV>(st + KB, vreg, tid);
    };
    const int rq = 32 * wave + r + off;   // first band position of this lane's query
    auto compute = [&](const char* st, int t) {
        const char* kimg = st;
        const char* vimg = st + KB;
        // inside every band of the wave: [64 t, 64 t + 63] ⊂ [32w + 31 + off, 32w + off + W − 1]
        const bool full = t * 64 >= 32 * wave + 31 + off && t * 64 + 63 <= 32 * wave + off + W - 1;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x16 sa, dp;
#pragma unroll
            for (int x = 0; x < 16; ++x) { sa[x] = 0.0f; dp[x] = 0.0f; }
#pragma unroll
            for (int s = 0; s < D / 16; ++s) sa = mfma32x32x16(rd.tr(kimg, kb, s), qf[s], sa);
#pragma unroll
            for (int s = 0; s < DV / 16; ++s) dp = mfma32x32x16(rd.tr(vimg, kb, s), df[s], dp);
            float pr[16];
#pragma unroll
            for (int x = 0; x < 16; ++x) pr[x] = exp2_fast(fmaf(sa[x], c, cnl));
            if (!full) {
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int kt = kb * 32 + (x & 7) + 8 * h + 16 * (x >> 3);
                    if ((unsigned)(t * 64 + kt - rq) >= (unsigned)W) pr[x] = 0.0f;
                }
            }
            F8 dsf[2];
#pragma unroll
            for (int x = 0; x < 16; ++x) dsf[x >> 3][x & 7] = (T)(pr[x] * (dp[x] + nDq));
#pragma unroll
            for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) dq[cb] = mfma32x32x16(rd.row(kimg, cb, kb, s2), dsf[s2], dq[cb]);
        }
    };

    // tile t sits in LDS buffer t % 2; its loads are issued one iteration ahead
    char* const st0 = smem;
    char* const st1 = smem + STAGE;
    gload(0);
    lstore(st0);
    if (NT > 1) gload(1);
    __syncthreads();
    for (int t = 0; t < NT; t += 2) {
        if (t >= tlo && t <= thi) compute(st0, t);
        if (t + 1 < NT) {
            lstore(st1);
            if (t + 2 < NT) gload(t + 2);
        }
        __syncthreads();
        if (t + 1 < NT) {
            if (t + 1 >= tlo && t + 1 <= thi) compute(st1, t + 1);
            if (t + 2 < NT) {
                lstore(st0);
                if (t + 3 < NT) gload(t + 3);
            }
            __syncthreads();
        }
    }
    if (qi < N) {
        T* dQb = (T*)p.dQ + (int64_t)b * N * d;
#pragma unroll
        for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = cb * 32 + acc_row(x, h);
                if (f < d) dQb[(int64_t)f * N + qi] = (T)(dq[cb][x] * p.scale);
            }
    }
}

template <class T, int D, int DV>
__global__ __launch_bounds__(256, (D + DV > 128) ? 1 : 2) void circ_bwd_dkdv_tiled(CircBwdParams p) {
    typedef typename Frag8<T>::type F8;
    constexpr int QB = D * 128, OB = DV * 128, STAGE = QB + OB + 512;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int b = lid / p.nblk, kblk = lid - b * p.nblk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int N = p.N, d = p.d, dv = p.dv, W = p.W;
    const auto qrs = slab_rsrc((const T*)p.Q + (int64_t)b * N * d, (uint32_t)(N * d * 2));
    const auto ors = slab_rsrc((const T*)p.dO + (int64_t)b * N * dv, (uint32_t)(N * dv * 2));
    const auto krs = slab_rsrc((const T*)p.K + (int64_t)b * N * d, (uint32_t)(N * d * 2));
    const auto vrs = slab_rsrc((const T*)p.V + (int64_t)b * N * dv, (uint32_t)(N * dv * 2));
    const int j0 = kblk * 128;
    // key j is attended by the queries j + p − t, t = 0..W−1: union start j0 + p − W + 1
    const CbUnion un = cb_union(cb_mod((int64_t)j0 + p.p - W + 1, N), W);
    const int off = un.off, NT = un.NT;
    const int tlo = (32 * wave + off) / 64;
    const int thi = min(NT - 1, (32 * wave + 31 + off + W - 1) / 64);
    const int kj = j0 + wave * 32 + r;   // this lane's key (column of S, dP)
    F8 kf[D / 16], vf[DV / 16];
    cb_load_frag<T, D>(kf, krs, d, N, kj, h);
    cb_load_frag<T, DV>(vf, vrs, dv, N, kj, h);
    const float c = p.scale_log2;
    const float* nlse = (const float*)p.nlse + (int64_t)b * N;
    const float* nDg = (const float*)p.nD + (int64_t)b * N;

    const ImgReader<T> rd(tid);

    f32x16 dk[D / 32], dvv[DV / 32];
#pragma unroll
    for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) dk[cb][x] = 0.0f;
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) dvv[cb][x] = 0.0f;

    // per-tile row constants: threads 0-63 carry −lse, 64-127 −D of the tile's queries
    u32x4 qreg[D / 32], oreg[DV / 32];
    float rowc = 0.0f;
    auto gload = [&](int t) {
        const int tok0 = (int)(((int64_t)un.k0 + (int64_t)t * 64) % N);
        cb_gload<T, D>(qreg, qrs, d, N, tok0, tid);
        cb_gload<T, DV>(oreg, ors, dv, N, tok0, tid);
        const int q = (tok0 + (tid & 63)) % N;
        if (tid < 64) rowc = nlse[q];
        else if (tid < 128) rowc = nDg[q];
    };
    auto lstore = [&](char* st) {
        cb_lstore<D>(st, qreg, tid);
        cb_lstore<DV>(st + QB, oreg, tid);
        if (tid < 128) ((float*)(st + QB + OB))[tid] = rowc;
    };
    const int cq = 32 * wave + r + off;   // first union position that attends this lane's key
    auto compute = [&](const char* st, int t) {
        const char* qimg = st;
        const char* oimg = st + QB;
        const float* rl = (const float*)(st + QB + OB);      // −lse[64], then −D[64]
        const bool full = t * 64 >= 32 * wave + 31 + off && t * 64 + 63 <= 32 * wave + off + W - 1;
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
            float pr[16];
#pragma unroll
            for (int x = 0; x < 16; ++x) pr[x] = exp2_fast(sa[x] * c);
            if (!full) {
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int qt = u * 32 + (x & 7) + 8 * h + 16 * (x >> 3);
                    if ((unsigned)(t * 64 + qt - cq) >= (unsigned)W) pr[x] = 0.0f;
                }
            }
            F8 pf[2], dsf[2];
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                pf[x >> 3][x & 7] = (T)pr[x];
                dsf[x >> 3][x & 7] = (T)(pr[x] * dp[x]);
            }
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) dvv[cb] = mfma32x32x16(rd.row(oimg, cb, u, s2), pf[s2], dvv[cb]);
#pragma unroll
            for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) dk[cb] = mfma32x32x16(rd.row(qimg, cb, u, s2), dsf[s2], dk[cb]);
        }
    };

    char* const st0 = smem;
    char* const st1 = smem + STAGE;
    gload(0);
    lstore(st0);
    if (NT > 1) gload(1);
    __syncthreads();
    for (int t = 0; t < NT; t += 2) {
        if (t >= tlo && t <= thi) compute(st0, t);
        if (t + 1 < NT) {
            lstore(st1);
            if (t + 2 < NT) gload(t + 2);
        }
        __syncthreads();
        if (t + 1 < NT) {
            if (t + 1 >= tlo && t + 1 <= thi) compute(st1, t + 1);
            if (t + 2 < NT) {
                lstore(st0);
                if (t + 3 < NT) gload(t + 3);
            }
            __syncthreads();
        }
    }
    if (kj < N) {
        T* dKb = (T*)p.dK + (int64_t)b * N * d;
        T* dVb = (T*)p.dV + (int64_t)b * N * dv;
#pragma unroll
        for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = cb * 32 + acc_row(x, h);
                if (f < d) dKb[(int64_t)f * N + kj] = (T)(dk[cb][x] * p.scale);
            }
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = cb * 32 + acc_row(x, h);
                if (f < dv) dVb[(int64_t)f * N + kj] = (T)dvv[cb][x];
            }
    }
}

// --------------------------------------------------------------------------
// launcher: circ_bwd_plan (fa_circulant_plan.h) names the kernels, their grids and LDS sizes
// and the workspace layout; nothing below decides any of them again
// --------------------------------------------------------------------------
static_assert(kCT == kCircBwdSimtTile && kCThreads == kCircBwdThreads, "the plan's constants");

size_t circulant_bwd_workspace(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W) {
    return circ_bwd_plan(dtype, N, d, dv, batch, W, kCircAuto, true, true, true).total;
}

// T: the tensors' element type; A: the SIMT kernels' arithmetic (double for Float64)
template <class T, class A>
static void launch_cb_typed(const CircBwdPlan& pl, const CircBwdParams& p, hipStream_t s) {
    const dim3 grid((unsigned)pl.grid), blk(kCircBwdThreads);
    if (pl.w1) {
        const int64_t total = (int64_t)p.N * p.batch;
        hipLaunchKernelGGL(circ_bwd_w1<T>, dim3((unsigned)pl.w1_grid), blk, 0, s, p, total * p.d, total * p.dv);
        return;
    }
    if constexpr (sizeof(T) == 2) {
        if (pl.prepass_vec) hipLaunchKernelGGL(circ_bwd_prepass_v<T>, dim3((unsigned)pl.prepass_grid), blk, 0, s, p);
    }
    if (!pl.prepass_vec) hipLaunchKernelGGL((circ_bwd_prepass<T, A>), dim3((unsigned)pl.prepass_grid), blk, 0, s, p);
    if (pl.family == kCircBwdMfma) {
        if constexpr (sizeof(T) == 2)   // (never planned for fp32, Float64)
            by_dim_class(pl.Dc, [&](auto D) {
                by_dim_class(pl.DVc, [&](auto DV) {
                    hipLaunchKernelGGL((circ_bwd_dq_tiled<T, decltype(D)::value, decltype(DV)::value>), grid, blk, 0, s, p);
                    hipLaunchKernelGGL((circ_bwd_dkdv_tiled<T, decltype(D)::value, decltype(DV)::value>), grid, blk, 0, s, p);
                });
            });
        return;
    }
    // > 64 KiB of dynamic LDS at d = dv = 128 (gfx950 has 160 KiB per CU)
    (void)hipFuncSetAttribute((const void*)circ_bwd_dq_simt<T, A>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_dq);
    (void)hipFuncSetAttribute((const void*)circ_bwd_dkdv_simt<T, A>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_dkdv);
    hipLaunchKernelGGL((circ_bwd_dq_simt<T, A>), grid, blk, pl.lds_dq, s, p);
    hipLaunchKernelGGL((circ_bwd_dkdv_simt<T, A>), grid, blk, pl.lds_dkdv, s, p);
}

int launch_circulant_bwd(const CircBwdArgs& a, hipStream_t s, const char** why) {
    const CircBwdPlan pl = circ_bwd_plan(a.dtype, a.N, a.d, a.dv, a.batch, a.W, g_circ_force_generic,
                                         aligned16(a.Q) && aligned16(a.K) && aligned16(a.V), aligned16(a.O), aligned16(a.dO));
    if (pl.family == kCircBwdNone) {
        *why = pl.why;
        return pl.status;
    }
    if (!a.workspace || a.workspace_bytes < pl.total) {
        *why = "workspace missing or smaller than fa_circulant_bwd_workspace()";
        return FA_ERR_WORKSPACE;
    }
    char* const w = al256(a.workspace);
    CircBwdParams p;
    p.Q = a.Q; p.K = a.K; p.V = a.V; p.O = a.O; p.dO = a.dO; p.l = a.l; p.m = a.m;
    p.dQ = a.dQ; p.dK = a.dK; p.dV = a.dV;
    p.nD = w + pl.off_nD; p.nlse = w + pl.off_nlse;
    p.N = (int)a.N; p.d = (int)a.d; p.dv = (int)a.dv; p.W = (int)a.W; p.p = (int)((a.W - 1) / 2);
    p.nblk = (int)pl.nblk; p.total_wg = (int)pl.total_wg; p.batch = a.batch;
    p.scale = a.scale;
    p.scale_log2 = a.scale * kLog2e;
    p.scale64 = a.scale64 > 0.0 ? a.scale64 : (double)a.scale;
    switch (a.dtype) {
        case FA_DTYPE_BF16: launch_cb_typed<bf16, float>(pl, p, s); break;
        case FA_DTYPE_F16: launch_cb_typed<f16, float>(pl, p, s); break;
        case FA_DTYPE_F32: launch_cb_typed<float, float>(pl, p, s); break;
        case FA_DTYPE_F64: launch_cb_typed<double, double>(pl, p, s); break;
        default: *why = "unknown dtype"; return FA_ERR_INVALID_ARG;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    g_circ_bwd_last_kernel = pl.family;
    return FA_OK;
}

}  // namespace fa
