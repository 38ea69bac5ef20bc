// fa_bwd.hip — dense flash-attention backward for gfx950.
//
// Replaces dense_fa_backward(Q, K, V, O, dO, l, m) (reference
// src/dense.jl:104-167, not executable as committed — Appendix A.2; the
// executable spec is OneDFastBack, src_cpp/FlashAttention.cpp:194-252):
//   P = exp(τ Q Kᵀ − m)/l,  dV = Pᵀ dO,  dP = dO Vᵀ,  D = rowsum(dO ∘ O),
//   dS = P ∘ (dP − D),  dQ = τ dS K,  dK = τ dSᵀ Q.
//
// Structure (FA-2 style, deterministic: no float atomics):
//   1. pre-pass   : D[b][n] = Σ_c dO∘O (fp32) and lse2[b][n] = (m + ln l)·log2 e
//                   into the caller's workspace (8·N·B bytes);
//   2. dK/dV pass : each wave owns 32 keys, sweeps all query tiles;
//   3. dQ pass    : each wave owns 32 queries, sweeps all key tiles.
// P is recomputed from lse, so neither pass needs an online max.
//
// This file is the host side: launch_dense_bwd asks dense_bwd_plan (fa_dense_plan.h) once and
// launches what it names; plus the kernels every route shares, the pre-passes and the pad /
// unpad copies of the padded route.  The passes themselves are in fa_bwd_simt_dq.hip,
// fa_bwd_simt_dkdv.hip (SIMT), fa_bwd_f32.hip (fp32 MFMA), fa_bwd_dq.hip, fa_bwd_dkdv.hip (the
// 16-bit MFMA passes) and fa_bwd_fused.hip (2. and 3. in one sweep), each behind one launch
// function of fa_bwd_params.h.
#include <cstdlib>
#include <type_traits>

#include "fa_bwd_common.h"
#include "fa_bwd_params.h"
#include "fa_dense_plan.h"

namespace fa {

// The pre-pass runs first on the stream in every 16/32-bit backward: its thread 0
// (re)writes the workspace header, so the timeout word starts each call at hdr_err.
__device__ __forceinline__ void write_bwd_header(const BwdParams& p) {
    if (p.hdr) {
        p.hdr[0] = kBwdHdrMagic | p.hdr_plan;
        p.hdr[1] = p.hdr_err;
        p.hdr[3] = 0u;   // set by a chain-B tail that left its slice to the combine (read by tests)
    }
}

// --------------------------------------------------------------------------
// 1. pre-pass (HBM-bound): one thread per (b, n), coalesced along n.
// --------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void bwd_prepass(BwdParams p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)p.N * p.batch;
    if (idx >= total) return;
    if (idx == 0) write_bwd_header(p);
    const int64_t b = idx / p.N, n = idx - b * p.N;
    const T* O = (const T*)p.O + b * (int64_t)p.N * p.dv + n;
    const T* dO = (const T*)p.dO + b * (int64_t)p.N * p.dv + n;
    float acc = 0.0f;
    for (int c = 0; c < p.dv; ++c) acc = fmaf((float)dO[(int64_t)c * p.N], (float)O[(int64_t)c * p.N], acc);
    p.nD[idx] = -acc;
    p.nlse[idx] = -(p.m[idx] + logf(p.l[idx])) / p.scale;
}

// 16-B variant (bf16 / fp16, N % 8 == 0, O and dO 16-B aligned): a thread owns 8
// consecutive queries and keeps 16 row loads in flight; the scalar kernel above
// issues one 2-byte load pair per feature and leaves HBM half idle (88 µs at
// configs[3]).
template <class T>
__global__ __launch_bounds__(256) void bwd_prepass_v(BwdParams p) {
    const int64_t g8 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g8 >= (int64_t)p.N * p.batch / 8) return;
    if (g8 == 0) write_bwd_header(p);
    prepass_rows8((const T*)p.O, (const T*)p.dO, p.l, p.m, p.nD, p.nlse, g8 * 8, p.N, p.dv, p.scale);
}

// Varlen pre-pass (every 16/32-bit fa_varlen_bwd; one thread per (b, n) as bwd_prepass).  A row
// n >= nq, or a query that sees no key (its window [n + off - left, n + off + right] misses
// [0, nk)), gets nD = 0 and nlse = -inf, chosen from the lengths and the window, never from the
// caller's l: (s + nlse) c is then -inf for any finite score and P = exp2(-inf) = 0 exactly,
// where -(m + ln l)/tau of the empty-row state (-inf, 0) would be +inf.
template <class T>
__global__ __launch_bounds__(256) void bwd_prepass_varlen(BwdParams p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)p.N * p.batch;
    if (idx >= total) return;
    if (idx == 0) write_bwd_header(p);
    const int64_t b = idx / p.N, n = idx - b * p.N;
    const VarlenExt e = varlen_extents(p.q_lens, p.k_lens, (int)b, p.nqv, p.nkv, p.left, p.right);
    const int i = (int)n;
    if (i >= e.nq || max(0, i + e.off - e.left) > min(e.nk - 1, i + e.off + e.right)) {
        p.nD[idx] = 0.0f;
        p.nlse[idx] = kNegInf;
        return;
    }
    const T* O = (const T*)p.O + b * (int64_t)p.N * p.dv + n;
    const T* dO = (const T*)p.dO + b * (int64_t)p.N * p.dv + n;
    float acc = 0.0f;
    for (int c = 0; c < p.dv; ++c) acc = fmaf((float)dO[(int64_t)c * p.N], (float)O[(int64_t)c * p.N], acc);
    p.nD[idx] = -acc;
    p.nlse[idx] = -(p.m[idx] + logf(p.l[idx])) / p.scale;
}

thread_local int g_bwd_force_generic = 0;   // benchmark knob
thread_local int g_bwd_mode = kBwdAuto;     // a DenseBwdMode (fa_dense_plan.h)
thread_local int g_bwd_l2local = -1;        // bwd_fused: L2-local hand-off when a slab sits on one XCD
                                            // (-1 auto: at d, dv <= 64; 0 never; 1 always)
thread_local int g_bwd_hoff = 3;            // bwd_fused: step offset between consecutive members
thread_local int g_bwd_stall_us = kStallUs; // bwd_fused: no-progress bound of a poll (us)
thread_local int g_bwd_nodirect = 0;         // bwd_fused (tests): every wrapped slice left to bwd_dq_fast's combine
thread_local int g_bwd_xcd = -1;            // bwd_fused: one XCD per slab where eligible (-1 auto, 0 never)

// dst (Np, Cp, B) <- src (N, C, B), zero-filled
template <class T>
__global__ __launch_bounds__(256) void bwd_pad(const T* __restrict__ src, T* __restrict__ dst, int N, int C,
                                               int Np, int Cp, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int n = (int)(e % Np);
    const int64_t bc = e / Np;
    const int c = (int)(bc % Cp);
    const int64_t b = bc / Cp;
    dst[e] = (n < N && c < C) ? src[(b * C + c) * N + n] : (T)0.0f;
}
// dst (N, C, B) <- src (Np, Cp, B)
template <class T>
__global__ __launch_bounds__(256) void bwd_unpad(const T* __restrict__ src, T* __restrict__ dst, int N, int C,
                                                 int Np, int Cp, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int n = (int)(e % N);
    const int64_t bc = e / N;
    const int c = (int)(bc % C);
    const int64_t b = bc / C;
    dst[e] = src[(b * Cp + c) * Np + n];
}
// l, m (N, 1, B) -> (Np, 1, B); padded queries get l = 1, m = 0
__global__ __launch_bounds__(256) void bwd_pad_lm(const float* __restrict__ l, const float* __restrict__ m,
                                                  float* __restrict__ lp, float* __restrict__ mp, int N, int Np,
                                                  int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int n = (int)(e % Np);
    const int64_t b = e / Np;
    lp[e] = n < N ? l[b * N + n] : 1.0f;
    mp[e] = n < N ? m[b * N + n] : 0.0f;
}

// --------------------------------------------------------------------------
// launcher: dense_bwd_plan (fa_dense_plan.h) names the kernel, the extents it runs on
// and the workspace offsets; nothing below decides any of them again
// --------------------------------------------------------------------------
template <class T>
static hipError_t pad_launch(const void* src, void* dst, int64_t N, int64_t C, int64_t Np, int64_t Cp, int64_t B,
                             hipStream_t s) {
    const int64_t total = Np * Cp * B;
    hipLaunchKernelGGL(bwd_pad<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const T*)src, (T*)dst,
                       (int)N, (int)C, (int)Np, (int)Cp, total);
    return hipGetLastError();
}
template <class T>
static hipError_t unpad_launch(const void* src, void* dst, int64_t N, int64_t C, int64_t Np, int64_t Cp, int64_t B,
                               hipStream_t s) {
    const int64_t total = N * C * B;
    hipLaunchKernelGGL(bwd_unpad<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const T*)src, (T*)dst,
                       (int)N, (int)C, (int)Np, (int)Cp, total);
    return hipGetLastError();
}

// kDenseBwdTwoPass / kDenseBwdSinglePass: the single pass if the plan names it, the dQ pass,
// the dK/dV pass
template <class T>
static hipError_t launch_fast(const DenseBwdPlan& pl, BwdParams p, DenseMask mask, hipStream_t s) {
    // a pass of 128-row blocks over `rows`
    auto blocks = [&](int rows) {
        p.nblk = (rows + 127) / 128;
        p.total_wg = p.nblk * p.batch;
    };
    hipError_t e;
    const bool single = pl.kernel == kDenseBwdSinglePass;
    if (single) {   // dQ pass below only after a hand-off timeout
        p.total_wg = p.nkb * p.batch;
        if ((e = launch_fused<T>(p, s)) != hipSuccess) return e;
        const FusedFlags ff = fused_flags(p.batch, p.nqt, p.nkb);
        p.guard = p.err;
        p.sguard = p.flags + ff.serr;
        p.cguard = p.hdr + 3;
        p.fin = p.flags + ff.fin;
    }
    // (a masked backward is always the two passes: no atomics, no hand-off)
    blocks(p.N);
    if ((e = launch_dq_fast<T>(p, mask, s)) != hipSuccess || single) return e;
    blocks(p.Nk);
    return launch_dkdv_fast<T>(p, mask, s);
}

// both SIMT passes
template <class T, class A = float>
static hipError_t launch_generic(const BwdParams& p, DenseMask mask, hipStream_t s) {
    const hipError_t e = launch_generic_dq<T, A>(p, mask, s);
    return e != hipSuccess ? e : launch_generic_dkdv<T, A>(p, mask, s);
}

// the pre-pass, then the plan's kernel
template <class T>
static hipError_t launch_typed(const DenseBwdPlan& pl, const BwdParams& p, DenseMask mask, hipStream_t s) {
    const int64_t total = (int64_t)p.N * p.batch;
    if (mask == kMaskVarlen) {   // its own pre-pass: the empty rows come from the lengths (bwd_prepass_varlen)
        hipLaunchKernelGGL(bwd_prepass_varlen<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    } else {
        bool vec = false;
        if constexpr (sizeof(T) == 2) {
            vec = p.N % 8 == 0 && aligned16(p.O) && aligned16(p.dO);
            if (vec) hipLaunchKernelGGL(bwd_prepass_v<T>, dim3((unsigned)((total / 8 + 255) / 256)), dim3(256), 0, s, p);
        }
        if (!vec) hipLaunchKernelGGL(bwd_prepass<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (the plan never names the single pass under a mask)
    if constexpr (std::is_same<T, float>::value) {
        if (pl.kernel == kDenseBwdF32Mfma) return launch_f32_mfma(p, mask, s);
    } else {
        if (pl.kernel == kDenseBwdTwoPass || pl.kernel == kDenseBwdSinglePass) return launch_fast<T>(pl, p, mask, s);
    }
    return launch_generic<T>(p, mask, s);
}

thread_local int g_dense_bwd_last[3] = {-1, -1, -1};   // fa_debug_dense_last_launch: kernel, mask, padded

static DenseBwdKnobs bwd_knobs() { return {g_bwd_force_generic, g_bwd_mode, g_bwd_hoff, g_bwd_xcd}; }

// The shape's own needs under the thread's knobs on the current device: aligned tensors, room
// for everything (the queries have no pointers).
// A masked backward: header, row statistics, padded slabs; never the single pass's part, and so
// no device query.
size_t dense_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, DenseMask mask) {
    const int cus = mask == kMaskNone ? device_cus(nullptr) : 0;
    return dense_bwd_plan(dtype, N, Nk, d, dv, batch, mask, bwd_knobs(), true, SIZE_MAX, cus).total;
}

// Single-pass state in the workspace: per-slice counters (zeroed here), then the running dQ
// sums.  The status word is hdr[1], which the pre-pass sets to hdr_err.
static hipError_t fused_setup(BwdParams& p, const DenseBwdPlan& pl, int mode, char* w, hipStream_t s) {
    p.flags = (unsigned*)(w + pl.off_flags);
    p.part = (float*)(w + pl.off_part);
    p.nkb = pl.nkb; p.nqt = pl.nqt; p.xcd = pl.xcd;
    p.hdr_plan = 1;
    // kBwdSinglePassGiveUp (tests): the timeout word starts set, so every poll gives up and
    // the guarded dQ pass must recompute dQ of every slab
    p.hdr_err = mode == kBwdSinglePassGiveUp ? 1u : 0u;
    // L2-local hand-off: +6 % at d = dv = 64, -1 % at 128, where a slice's running
    // sums (32 KB) in flight over three steps fill most of the 4-MB L2 that also
    // serves the slab's Q / dO (profiles/r04_bwd_handoff_modes.log)
    p.l2local = g_bwd_l2local >= 0 ? g_bwd_l2local : (pl.d <= 64 && pl.dv <= 64 ? 1 : 0);
    p.hoff = g_bwd_hoff;
    p.stall_ticks = g_bwd_stall_us * 100;
    p.nodirect = g_bwd_nodirect;
#ifdef FA_BWD_ABL
    p.ablate = bwd_ablate_bits(mode);
#endif
    hipError_t e = hipMemsetAsync(p.flags, 0, pl.flag_bytes, s);
    if (e == hipSuccess && mode == kBwdSinglePassGiveUp)
        e = hipMemsetD32Async((hipDeviceptr_t)(p.flags + fused_flags(p.batch, pl.nqt, pl.nkb).serr), 1u, (size_t)p.batch, s);
    return e;
}

int dense_bwd_handoff_status(const void* workspace, size_t workspace_bytes, hipStream_t s, int* status,
                             const char** why) {
    const char* const hdr = al256((void*)workspace) + DenseBwdPlan{}.off_hdr;
    if (!workspace || (uintptr_t)hdr + 8 > (uintptr_t)workspace + workspace_bytes) {
        *why = "workspace missing or smaller than its header";
        return FA_ERR_INVALID_ARG;
    }
    unsigned h[2] = {0u, 0u};
    hipError_t e = hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    if ((h[0] & 0xFFFFFF00u) != kBwdHdrMagic) {
        *why = "workspace holds no fa_dense_bwd header (not the workspace of an fa_dense_bwd call)";
        return FA_ERR_INVALID_ARG;
    }
    *status = (h[0] & 0xFFu) == 1u ? (h[1] != 0u ? 1 : 0) : -1;
    return FA_OK;
}

int launch_dense_bwd(const DenseBwdArgs& a, hipStream_t s, const char** why) {
    if (a.d > kMaxHeadDim || a.dv > kMaxHeadDim) {
        *why = "head dimension exceeds the compiled maximum (128)";
        return FA_ERR_UNSUPPORTED;
    }
    if (mask_lacks_keys(a.mask, a.N, a.Nk, why)) return FA_ERR_UNSUPPORTED;
    if (a.N * a.d > INT32_MAX || a.Nk * a.d > INT32_MAX || a.N * a.dv > INT32_MAX ||
        a.Nk * a.dv > INT32_MAX || a.N * a.batch > INT32_MAX / 2 || a.Nk * a.batch > INT32_MAX / 2) {
        *why = "extent exceeds 2^31 elements";
        return FA_ERR_UNSUPPORTED;
    }
    const DenseBwdKnobs kn = bwd_knobs();
    char* const w = al256(a.workspace);
    const size_t slack = (size_t)(w - (char*)a.workspace);
    const DenseBwdPlan pl = dense_bwd_plan(a.dtype, a.N, a.Nk, a.d, a.dv, a.batch, a.mask, kn,
                                           aligned16(a.Q) && aligned16(a.K) && aligned16(a.V) && aligned16(a.dO),
                                           a.workspace_bytes > slack ? a.workspace_bytes - slack : 0, device_cus(s));
    // causal, local and Float64 totals depend on the shape alone: the whole of it must be there.
    // (A padded call checks its slabs below; the single pass's part is optional.)
    if ((a.mask != kMaskNone || a.dtype == FA_DTYPE_F64) && a.workspace_bytes < pl.total) {
        *why = a.mask == kMaskVarlen   ? "workspace smaller than fa_varlen_bwd_workspace()"
               : a.mask == kMaskLocal  ? "workspace smaller than fa_local_bwd_workspace()"
               : a.mask == kMaskCausal ? "workspace smaller than fa_causal_bwd_workspace()"
                                       : "workspace smaller than fa_dense_bwd_workspace()";
        return FA_ERR_WORKSPACE;
    }
    BwdParams p;
    const MaskInts mi = mask_ints(a.mask, a.left, a.right, a.N, a.Nk);   // from the caller's extents, also on the padded path
    p.causal = mi.causal; p.off = mi.off; p.local = mi.local; p.left = mi.left; p.right = mi.right;
    p.Q = a.Q; p.K = a.K; p.V = a.V; p.O = a.O; p.dO = a.dO; p.l = a.l; p.m = a.m;
    p.dQ = a.dQ; p.dK = a.dK; p.dV = a.dV;
    p.hdr = (unsigned*)(w + pl.off_hdr);
    p.err = p.hdr + 1;
    p.nD = (float*)(w + pl.off_nD);
    p.nlse = (float*)(w + pl.off_nlse);
    p.N = (int)a.N; p.Nk = (int)a.Nk; p.d = (int)a.d; p.dv = (int)a.dv; p.batch = (int)a.batch;
    p.nkv = (int)a.Nk;   // stays the caller's on the padded path
    p.nqv = (int)a.N;    // likewise
    p.q_lens = a.q_lens; p.k_lens = a.k_lens;
    p.scale = a.scale;
    p.scale_log2 = a.scale * kLog2e;
    hipError_t e;
    if (pl.kernel == kDenseBwdF64) {
        // Float64: row statistics recomputed in double (not from the float32 l, m),
        // then the SIMT passes in double.
        // plan 0; word 3 (a chain-B tail left its slice to the combine) belongs to the
        // current call like word 0, so it is cleared wherever word 0 is written; word 2
        // (the sticky give-up count) is left alone
        if ((e = hipMemsetD32Async((hipDeviceptr_t)p.hdr, kBwdHdrMagic, 1, s)) != hipSuccess ||
            (e = hipMemsetD32Async((hipDeviceptr_t)(p.hdr + 3), 0, 1, s)) != hipSuccess) {
            *why = hipGetErrorString(e);
            return FA_ERR_HIP;
        }
        p.scale64 = a.scale64 > 0.0 ? a.scale64 : (double)a.scale;
        const int rc = launch_f64_bwd_stats(a, (double*)p.nD, (double*)p.nlse, s, why);
        if (rc != FA_OK) return rc;
        if ((e = launch_generic<double, double>(p, a.mask, s)) != hipSuccess) {
            *why = hipGetErrorString(e);
            return FA_ERR_HIP;
        }
        g_dense_bwd_last[0] = pl.kernel, g_dense_bwd_last[1] = a.mask, g_dense_bwd_last[2] = pl.padded;
        return FA_OK;
    }
    if (pl.padded && !pl.slabs_fit) {
        *why = "workspace smaller than fa_dense_bwd_workspace()";
        return FA_ERR_WORKSPACE;
    }
    if (pl.kernel == kDenseBwdSinglePass && (e = fused_setup(p, pl, kn.mode, w, s)) != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    if (pl.padded) {
        // the kernels run on zero-padded copies in the workspace slabs; dQ, dK, dV are copied back
        const int64_t B = a.batch;
        const bool half = a.dtype == FA_DTYPE_F16;
        auto slab = [&](BwdSlab i) { return (void*)(w + pl.off_slab[i]); };
        auto pad = [&](const void* src, BwdSlab dst, int64_t N, int64_t C, int64_t Np, int64_t Cp) {
            return half ? pad_launch<f16>(src, slab(dst), N, C, Np, Cp, B, s) : pad_launch<bf16>(src, slab(dst), N, C, Np, Cp, B, s);
        };
        auto unpad = [&](BwdSlab src, void* dst, int64_t N, int64_t C, int64_t Np, int64_t Cp) {
            return half ? unpad_launch<f16>(slab(src), dst, N, C, Np, Cp, B, s) : unpad_launch<bf16>(slab(src), dst, N, C, Np, Cp, B, s);
        };
        const int64_t tlm = pl.N * B;
        if ((e = pad(a.Q, kSlabQ, a.N, a.d, pl.N, pl.d)) != hipSuccess ||
            (e = pad(a.K, kSlabK, a.Nk, a.d, pl.Nk, pl.d)) != hipSuccess ||
            (e = pad(a.V, kSlabV, a.Nk, a.dv, pl.Nk, pl.dv)) != hipSuccess ||
            (e = pad(a.O, kSlabO, a.N, a.dv, pl.N, pl.dv)) != hipSuccess ||
            (e = pad(a.dO, kSlabDO, a.N, a.dv, pl.N, pl.dv)) != hipSuccess) {
            *why = hipGetErrorString(e);
            return FA_ERR_HIP;
        }
        hipLaunchKernelGGL(bwd_pad_lm, dim3((unsigned)((tlm + 255) / 256)), dim3(256), 0, s, a.l, a.m,
                           (float*)slab(kSlabL), (float*)slab(kSlabM), (int)a.N, (int)pl.N, tlm);
        p.Q = slab(kSlabQ); p.K = slab(kSlabK); p.V = slab(kSlabV); p.O = slab(kSlabO); p.dO = slab(kSlabDO);
        p.l = (const float*)slab(kSlabL); p.m = (const float*)slab(kSlabM);
        p.dQ = slab(kSlabDQ); p.dK = slab(kSlabDK); p.dV = slab(kSlabDV);
        p.N = (int)pl.N; p.Nk = (int)pl.Nk; p.d = (int)pl.d; p.dv = (int)pl.dv;
        e = half ? launch_typed<f16>(pl, p, a.mask, s) : launch_typed<bf16>(pl, p, a.mask, s);
        if (e == hipSuccess && (e = unpad(kSlabDQ, a.dQ, a.N, a.d, pl.N, pl.d)) == hipSuccess &&
            (e = unpad(kSlabDK, a.dK, a.Nk, a.d, pl.Nk, pl.d)) == hipSuccess)
            e = unpad(kSlabDV, a.dV, a.Nk, a.dv, pl.Nk, pl.dv);
    } else {
        switch (a.dtype) {
            case FA_DTYPE_BF16: e = launch_typed<bf16>(pl, p, a.mask, s); break;
            case FA_DTYPE_F16: e = launch_typed<f16>(pl, p, a.mask, s); break;
            case FA_DTYPE_F32: e = launch_typed<float>(pl, p, a.mask, s); break;
            default: *why = "unknown dtype"; return FA_ERR_INVALID_ARG;
        }
    }
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    g_dense_bwd_last[0] = pl.kernel, g_dense_bwd_last[1] = a.mask, g_dense_bwd_last[2] = pl.padded;
    return FA_OK;
}

}  // namespace fa
