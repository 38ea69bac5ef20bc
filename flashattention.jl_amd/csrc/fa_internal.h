// fa_internal.h — host-side launcher interface between api.cpp (argument
// validation, C ABI) and the kernel translation units.  Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace fa {

// The mask of a dense-family call (dense, causal, local attention are one kernel family under
// three masks).  ONE value travels from the extern "C" entry points (api.cpp) through
// DenseArgs / DenseBwdArgs and the plans (fa_dense_plan.h) to the kernels' single MASK
// template parameter, which by_mask below turns into a compile-time constant.
// kMaskVarlen (fa_varlen_fwd / fa_varlen_bwd) is the local mask with per-slab extents: the
// kernels read q_lens[b], k_lens[b] and run the local bodies on the leading (nq, nk) rows.
enum DenseMask : int { kMaskNone = 0, kMaskCausal = 1, kMaskLocal = 2, kMaskVarlen = 3 };

struct DenseArgs {
    int dtype;                 // fa_dtype
    const void *Q, *K, *V;
    void* O;
    float *l, *m;
    int64_t N, Nk, d, dv, batch;
    float scale;               // already resolved (> 0)
    void* workspace = nullptr; // optional: padded K / V copies for ragged Nk (fa_dense_fwd_workspace)
    size_t workspace_bytes = 0;
    double scale64 = 0.0;      // Float64 kernels: τ resolved in double (0: use scale)
    // kMaskCausal (fa_causal_fwd): query i sees keys j <= i + off, off = Nk - N.  kMaskLocal
    // (fa_local_fwd): keys i + off - left <= j <= i + off + right; a negative side is unbounded
    // (mask_ints clamps).  left / right are read under kMaskLocal only.
    DenseMask mask = kMaskNone;
    int64_t left = -1, right = -1;
    // kMaskVarlen only: device pointers to `batch` int32 lengths (nullptr: every slab is full on
    // that side); clamped on the device (varlen_clamp), never read on the host
    const int32_t *q_lens = nullptr, *k_lens = nullptr;
};

struct DenseBwdArgs {
    int dtype;
    const void *Q, *K, *V, *O, *dO;
    const float *l, *m;
    void *dQ, *dK, *dV;
    int64_t N, Nk, d, dv, batch;
    float scale;
    void* workspace;
    size_t workspace_bytes;
    double scale64 = 0.0;      // Float64 kernels: τ resolved in double (0: use scale)
    DenseMask mask = kMaskNone;   // as DenseArgs::mask (a masked backward is always the two-pass form)
    int64_t left = -1, right = -1;
    const int32_t *q_lens = nullptr, *k_lens = nullptr;   // as DenseArgs (kMaskVarlen only)
};

struct WindowGeom {
    int nsp;                   // spatial rank 1..3
    int64_t S[3];              // spatial extents (first = fastest)
    int64_t O[3];              // windows per dim
    int64_t ws, stride, pad;
    int64_t T;                 // ws^nsp tokens per window
    int64_t L;                 // windows per image
    int64_t P;                 // pixels per image
};

struct WindowedArgs {
    int dtype;
    const void *q, *k, *v;
    void* y;
    float *l, *m;
    WindowGeom g;
    int64_t d, dv, batch;
    float scale;
    void* workspace;
    size_t workspace_bytes;
    double scale64 = 0.0;
};

struct WindowedBwdArgs {
    int dtype;
    const void *q, *k, *v, *y, *dy;
    const float *l, *m;
    void *dq, *dk, *dv_;
    WindowGeom g;
    int64_t d, dv, batch;
    float scale;
    void* workspace;
    size_t workspace_bytes;
    double scale64 = 0.0;
};

struct CircArgs {
    int dtype;
    const void *Q, *K, *V;
    void* O;
    float *l, *m;
    int64_t N, d, dv, batch, W;
    float scale;
    double scale64 = 0.0;      // Float64 kernel: τ resolved in double (0: use scale)
};

struct CircBwdArgs {
    int dtype;
    const void *Q, *K, *V, *O, *dO;
    const float *l, *m;
    void *dQ, *dK, *dV;
    int64_t N, d, dv, batch, W;
    float scale;
    void* workspace;
    size_t workspace_bytes;
    double scale64 = 0.0;      // Float64 kernels: τ resolved in double (0: use scale)
};

struct SoftmaxArgs {
    int dtype;
    const void* S;
    void* P;
    int64_t M, N, batch;
    int dims;                  // 1: over M (contiguous), 2: over N (stride M)
    void* workspace;
    size_t workspace_bytes;
};

// Each returns a hipError_t-like code through *err and a fa_status.
int launch_dense_fwd(const DenseArgs& a, hipStream_t s, const char** why);
int launch_dense_bwd(const DenseBwdArgs& a, hipStream_t s, const char** why);
// The workspace a shape needs under a mask.  Causal and local (the same answers, whatever the
// window): the forward's padded K / V copies only (no split-KV part); the backward's header,
// row statistics and pad plan, never the single pass's running sums, so only the dense
// backward query asks the device for its CU count.  (The windowed composed path asks for the
// dense answers.)
size_t dense_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, DenseMask mask = kMaskNone);
size_t dense_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, DenseMask mask = kMaskNone);
int dense_bwd_handoff_status(const void* workspace, size_t workspace_bytes, hipStream_t s, int* status,
                             const char** why);
// Float64 (fa_f64.hip): the forward, and the backward's row statistics in double
// (nD = −rowsum(dO ∘ O), nlse = −(m + ln l)/τ recomputed from Q, K; [batch][N] each)
int launch_dense_fwd_f64(const DenseArgs& a, hipStream_t s, const char** why);
int launch_f64_bwd_stats(const DenseBwdArgs& a, double* nD, double* nlse, hipStream_t s, const char** why);
// element size of a fa_dtype (0: unknown)
// CUs of the device the work runs on: the stream's device (the current device for
// the NULL stream, and for fa_dense_bwd_workspace, which takes no stream); 0 on error.
inline int device_cus(hipStream_t s) {
    int dev = 0, cus = 0;
    if (s != nullptr) {
        if (hipStreamGetDevice(s, &dev) != hipSuccess) return 0;
    } else if (hipGetDevice(&dev) != hipSuccess) {
        return 0;
    }
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
}

inline size_t dtype_size(int dtype) { return dtype == 0 ? 4 : dtype == 1 || dtype == 2 ? 2 : dtype == 3 ? 8 : 0; }
size_t windowed_workspace(int dtype, const WindowGeom& g, int64_t d, int64_t dv, int64_t batch);
size_t windowed_fwd_workspace(int dtype, const WindowGeom& g, int64_t d, int64_t dv, int64_t batch);
int launch_windowed_fwd(const WindowedArgs& a, hipStream_t s, const char** why);
int launch_windowed_bwd(const WindowedBwdArgs& a, hipStream_t s, const char** why);
// circulant attention (fa_circulant.hip, fa_circulant_bwd.hip): each launcher asks its plan
// (fa_circulant_plan.h: circ_fwd_plan, circ_bwd_plan) once, with the thread's circulant
// knob and the tensors' 16-B alignment facts, refuses with the plan's status
// and message (head dims, then the 32-bit extents), and launches what the plan names.  The
// backward then checks the workspace against the plan's total, which is what
// circulant_bwd_workspace returns for the shape, before the first launch.
int launch_circulant_fwd(const CircArgs& a, hipStream_t s, const char** why);
size_t circulant_bwd_workspace(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W);
int launch_circulant_bwd(const CircBwdArgs& a, hipStream_t s, const char** why);
// window (unfold) / unwindow (fold, sum over overlaps) of one tensor (S..., C, B) <-> (T, C, L, B)
int launch_window(int dtype, const void* src, void* dst, const WindowGeom& g, int64_t C, int64_t batch,
                  bool unwindow, hipStream_t s, const char** why);
size_t softmax_workspace(int64_t M, int64_t N, int64_t batch, int dims);
int launch_softmax(const SoftmaxArgs& a, hipStream_t s, const char** why);

// Padded head-dim class a kernel is compiled for: 32, 64 or 128 (0 = none).
inline int head_dim_class(int64_t d) {
    if (d <= 32) return 32;
    if (d <= 64) return 64;
    if (d <= 128) return 128;
    return 0;
}

constexpr int kMaxHeadDim = 128;

// "causal" / "local": the mask's word in messages and entry-point names ("dense" for kMaskNone)
inline const char* mask_word(DenseMask mask) {
    return mask == kMaskVarlen ? "varlen" : mask == kMaskLocal ? "local" : mask == kMaskCausal ? "causal" : "dense";
}
// A masked call needs Nk >= N: true, with the mask's message in *why, when it has fewer keys.
inline bool mask_lacks_keys(DenseMask mask, int64_t N, int64_t Nk, const char** why) {
    if (mask == kMaskNone || Nk >= N) return false;
    *why = mask == kMaskVarlen  ? "varlen attention needs Nk >= N (a query would see no key)"
           : mask == kMaskLocal ? "local attention needs Nk >= N (a query would see no key)"
                                : "causal attention needs Nk >= N (a query would see no key)";
    return true;
}
// The mask as the five ints of the device parameter structs (BwdParams, F64Params; FwdParams
// takes the window only).  off = Nk - N of the caller's extents.  A side of the local window
// lands in [0, Nk], where Nk binds nowhere (negative = unbounded, and a value >= Nk is the
// same), clamped on the 64-bit value before it becomes a 32-bit int.
// kMaskVarlen: off is per slab (nk - nq, anywhere in [-N, Nk]) and the kernels compute it; `off`
// here stays 0.  Nk as "no bound" relies on off >= 0 (i + off + Nk >= Nk), so the varlen window
// is clamped in two steps that bind nowhere for any off: here left to [0, Nk] and right to
// [0, N], and per slab (varlen_extents) left to nk and right to nq.  For a query i < nq,
// i + off - nk = i - nq < 0 and i + off + nq = i + nk >= nk; and i + off + right <= nk + nq
// stays a 32-bit int.
struct MaskInts {
    int causal = 0, off = 0, local = 0, left = 0, right = 0;
};
inline MaskInts mask_ints(DenseMask mask, int64_t left, int64_t right, int64_t N, int64_t Nk) {
    MaskInts r;
    if (mask == kMaskNone) return r;
    r.off = (int)(Nk - N);
    r.causal = mask == kMaskCausal;
    if (mask == kMaskLocal) {
        r.local = 1;
        r.left = (int)(left < 0 || left > Nk ? Nk : left);
        r.right = (int)(right < 0 || right > Nk ? Nk : right);
    }
    if (mask == kMaskVarlen) {
        r.off = 0;
        r.local = 1;
        r.left = (int)(left < 0 || left > Nk ? Nk : left);
        r.right = (int)(right < 0 || right > N ? N : right);
    }
    return r;
}

// A caller's length as the kernels use it: clamped to [0, n].  Lengths are device data and the
// ABI does not synchronise, so this clamp, not a host check, is what keeps every index in
// bounds (fa_debug_varlen_clamp exposes it to the host tests).
__host__ __device__ inline int varlen_clamp(int len, int n) { return len < 0 ? 0 : len > n ? n : len; }
// The extents of slab b under kMaskVarlen: the leading nq queries and nk keys (N, Nk: the
// caller's extents; a null array means full), off = nk - nq, and the window with each side
// clamped where it binds nowhere (mask_ints).
struct VarlenExt {
    int nq, nk, off, left, right;
};
__host__ __device__ inline VarlenExt varlen_extents(const int32_t* q_lens, const int32_t* k_lens, int b, int N, int Nk,
                                                    int left, int right) {
    VarlenExt e;
    e.nq = q_lens ? varlen_clamp(q_lens[b], N) : N;
    e.nk = k_lens ? varlen_clamp(k_lens[b], Nk) : Nk;
    e.off = e.nk - e.nq;
    e.left = left < e.nk ? left : e.nk;
    e.right = right < e.nq ? right : e.nq;
    return e;
}

// Workspace regions start on 256-B boundaries; the vector paths want 16-B aligned tensors.
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline char* al256(void* p) { return (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// A run-time head-dim class as a compile-time constant for the launchers: by_dim_class calls
// f(dim_c<C>{}) with the class c (32, 64 or 128; false, and no call, for anything else).  f
// is a generic lambda, [&](auto D), that names kernel<..., D> or decltype(D)::value.
// by_mask does the same for a DenseMask: f(mask_c<M>{}), [&](auto M) names
// kernel<..., decltype(M)::value>.
template <int N>
using dim_c = std::integral_constant<int, N>;
template <class F>
inline bool by_dim_class(int c, F&& f) {
    switch (c) {
        case 32: f(dim_c<32>{}); return true;
        case 64: f(dim_c<64>{}); return true;
        case 128: f(dim_c<128>{}); return true;
    }
    return false;
}
template <DenseMask M>
using mask_c = std::integral_constant<DenseMask, M>;
template <class F>
inline bool by_mask(DenseMask mask, F&& f) {
    switch (mask) {
        case kMaskNone: f(mask_c<kMaskNone>{}); return true;
        case kMaskCausal: f(mask_c<kMaskCausal>{}); return true;
        case kMaskLocal: f(mask_c<kMaskLocal>{}); return true;
        case kMaskVarlen: f(mask_c<kMaskVarlen>{}); return true;
    }
    return false;
}

// Debug / benchmark knobs (fa_debug_set_*; not part of include/fa_hip.h and not
// ABI state).  They are THREAD-LOCAL: a knob set on one host thread changes only
// the kernels that thread launches, so concurrent callers on other threads stay
// on the default paths and the public entry points remain stateless for them.
extern thread_local int g_fwd_variant;        // forward kernel variant (a DenseFwdVariant, fa_dense_plan.h)
extern thread_local int g_fwd_last_path;      // 30 when the last fast forward launch ran fa_fwd_p4
// fa_debug_dense_last_launch: what the last dense-family forward / backward of this thread launched:
// {a DenseFwdKernel / DenseBwdKernel, the DenseMask, pad / padded}; {-1, -1, -1} before the first
extern thread_local int g_dense_fwd_last[3], g_dense_bwd_last[3];
extern thread_local float g_fwd_rescale_log2; // forward fast kernels: lazy-rescale threshold (log2 units)
extern thread_local int g_causal_rev;         // causal fast forward: launch order of the query blocks (0, 1, 2: fa_debug_set_causal_order)
extern thread_local int g_bwd_force_generic;  // backward: force the generic SIMT path
extern thread_local int g_bwd_mode;           // backward MFMA path (a DenseBwdMode, fa_dense_plan.h: kBwdAuto, kBwdTwoPass, kBwdSinglePass, ...)
extern thread_local int g_bwd_l2local;        // single pass: running sums handed over in the XCD's L2
extern thread_local int g_bwd_hoff;           // single pass: step offset between consecutive members
extern thread_local int g_bwd_stall_us;       // single pass: no-progress bound of a poll (us)
extern thread_local int g_bwd_nodirect;       // single pass (tests): chain-B tails never add A's total themselves
extern thread_local int g_bwd_xcd;            // single pass: one XCD per slab where eligible (-1 auto, 0 never)
extern thread_local int g_win_force_composed; // windowed: forced path (a WinMode, fa_windowed.h)
extern thread_local int g_win_bwd_grid;       // windowed: strip backward workgroups (0: one per CU)
extern thread_local int g_circ_force_generic; // circulant: forced kernel (a CircKnob, fa_circulant_plan.h)
extern thread_local int g_circ_fwd_last_kernel; // circulant forward: kernel of the last launch (1 tiled MFMA, 2 one wave per query, 3 LDS-tiled SIMT, 4 Float64)
extern thread_local int g_circ_bwd_last_kernel; // circulant backward: family of the last launch (1 MFMA, 2 SIMT, 3 Float64)

}  // namespace fa
