// api.cpp — the extern "C" boundary declared in include/fa_hip.h.
//
// Validates arguments the way the reference's Julia methods would fail
// (DimensionMismatch → FA_ERR_INVALID_ARG), resolves the default scale
// τ = 1/√d (src/dense.jl:43), and dispatches to the kernel launchers.  No
// process-global state: the error string and the fa_debug_set_* knobs are
// thread-local (the knobs are test/benchmark hooks, not ABI); never allocates,
// synchronises or aborts.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/fa_hip.h"
#include "fa_circulant_plan.h"   // the circulant plans (host functions)
#include "fa_dense_plan.h"   // the dense plans (host functions)
#include "fa_internal.h"
#include "fa_windowed.h"   // the windowed plans (host functions; no kernel is instantiated here)

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fn, const char* msg) {
    g_last_error = std::string(fn) + ": " + msg;
    return code;
}

int ok() {
    g_last_error.clear();
    return FA_OK;
}

bool valid_dtype(int dt) {
    return dt == FA_DTYPE_F32 || dt == FA_DTYPE_BF16 || dt == FA_DTYPE_F16 || dt == FA_DTYPE_F64;
}

float resolve_scale(float scale, int64_t d) {
    if (!(scale > 0.0f) || !std::isfinite(scale)) return (float)(1.0 / std::sqrt((double)d));
    return scale;
}
// τ for the Float64 kernels: the default 1/√d in double (src/dense.jl:43), else the
// caller's float scale widened.
double resolve_scale64(float scale, int64_t d) {
    if (!(scale > 0.0f) || !std::isfinite(scale)) return 1.0 / std::sqrt((double)d);
    return (double)scale;
}

// Empty inputs, as dense_fa! (src/dense.jl:21-102) treats them: N = 0 or batch = 0
// runs no tile (nothing to write); Nk = 0 leaves the initial O = 0, l = 0,
// m = −Inf (:58-60).  Returns true when the call is complete.
bool dense_fwd_empty(int dtype, void* O, float* l, float* m, int64_t N, int64_t Nk, int64_t dv, int64_t batch,
                     hipStream_t s, int* rc) {
    *rc = FA_OK;
    if (N == 0 || batch == 0) return true;
    if (Nk != 0) return false;
    const size_t esz = fa::dtype_size(dtype);
    if (!O || !l || !m) { *rc = FA_ERR_INVALID_ARG; return true; }
    if (hipMemsetAsync(O, 0, (size_t)(N * dv * batch) * esz, s) != hipSuccess ||
        hipMemsetAsync(l, 0, (size_t)(N * batch) * 4, s) != hipSuccess ||
        hipMemsetD32Async((hipDeviceptr_t)m, 0xFF800000u, (size_t)(N * batch), s) != hipSuccess)
        *rc = FA_ERR_HIP;
    return true;
}

// Window geometry of NNlib.unfold(x, (ws…, d, 1); stride, pad) (src/utils.jl:40).
int make_geom(fa::WindowGeom& g, int nspatial, const int64_t* spatial, int64_t ws, int64_t stride,
              int64_t pad, const char** why) {
    if (nspatial < 1 || nspatial > 3 || !spatial) { *why = "nspatial must be 1, 2 or 3"; return FA_ERR_INVALID_ARG; }
    if (ws < 1) { *why = "window size must be >= 1"; return FA_ERR_INVALID_ARG; }
    if (stride < 1) { *why = "stride must be >= 1"; return FA_ERR_INVALID_ARG; }
    if (pad < 0) pad = (ws - 1) / 2;
    g.nsp = nspatial;
    g.ws = ws;
    g.stride = stride;
    g.pad = pad;
    g.T = 1;
    g.L = 1;
    g.P = 1;
    for (int i = 0; i < 3; ++i) { g.S[i] = 1; g.O[i] = 1; }
    for (int i = 0; i < nspatial; ++i) {
        if (spatial[i] < 1) { *why = "spatial extents must be >= 1"; return FA_ERR_INVALID_ARG; }
        const int64_t span = spatial[i] + 2 * pad - ws;
        if (span < 0) { *why = "window larger than the padded input"; return FA_ERR_INVALID_ARG; }
        g.S[i] = spatial[i];
        g.O[i] = span / stride + 1;
        g.T *= ws;
        g.L *= g.O[i];
        g.P *= spatial[i];
    }
    return FA_OK;
}

}  // namespace

extern "C" {

const char* fa_last_error(void) { return g_last_error.c_str(); }

int fa_abi_version(void) { return FA_HIP_ABI_VERSION; }

int fa_max_head_dim(void) { return fa::kMaxHeadDim; }

// Not part of the public header: selects the forward kernel variant for A/B
// benchmarking, a fa::DenseFwdVariant (fa_dense_plan.h): 0 kFwdAuto (per head-dim class),
// 5 kFwdW8B64 / 7 kFwdW8Q2 = 8 waves x {1, 2} query blocks per wave on 32x32x16 MFMA;
// 20 kFwdNarrow = the default geometries with per-element Q gathers and O stores;
// 30 kFwdP4 = the one-wave-per-SIMD persistent kernel (fa_fwd_p4.hip) where its shape
// rules allow.  (The measured-and-rejected 4-wave, 16x16x32 and
// 4-waves-per-SIMD geometries were removed in round 4, the persistent 8-wave d <= 64
// kernel, a measured tie, in round 6; git history keeps them.)
int fa_debug_set_fwd_variant(int v) {
    const int old = fa::g_fwd_variant;
    if (v == fa::kFwdAuto || v == fa::kFwdW8B64 || v == fa::kFwdW8Q2 || v == fa::kFwdNarrow || v == fa::kFwdP4)
        fa::g_fwd_variant = v;
    return old;
}

// Not part of the public header: 30 when the calling thread's last forward ran the
// one-wave-per-SIMD kernel (fa_fwd_p4.hip), 0 otherwise (tests, bench labels).
int fa_debug_fwd_last_path(void) { return fa::g_fwd_last_path; }

// Not part of the public header (tests): what the calling thread's last dense-family forward
// and backward (dense, causal, local, varlen) launched, as recorded by the launchers after a
// successful launch: out[0..2] the forward's fa::DenseFwdKernel, fa::DenseMask and pad flag (K / V
// ran from the zero-padded copies), out[3..5] the backward's fa::DenseBwdKernel, fa::DenseMask
// and padded flag (the kernels ran on the padded slabs).  -1 in all three of a direction that
// has not launched on this thread.  Returns 0 (-1: out is null).
int fa_debug_dense_last_launch(int* out) {
    if (!out) return -1;
    for (int i = 0; i < 3; ++i) {
        out[i] = fa::g_dense_fwd_last[i];
        out[3 + i] = fa::g_dense_bwd_last[i];
    }
    return 0;
}

// Not part of the public header: lazy-rescale threshold of the bf16/f16 forward
// kernels in log2 units (default 8; 0 = rescale on every max increase, the
// textbook order).  Accuracy tests only; returns the previous value.
float fa_debug_set_rescale_threshold(float t) {
    const float old = fa::g_fwd_rescale_log2;
    if (t >= 0.0f && t <= 16.0f) fa::g_fwd_rescale_log2 = t;
    return old;
}

// Not part of the public header: 1 forces the generic (SIMT) backward.
int fa_debug_set_bwd_generic(int v) {
    const int old = fa::g_bwd_force_generic;
    fa::g_bwd_force_generic = v != 0;
    return old;
}

// Not part of the public header: backward MFMA path, a fa::DenseBwdMode (fa_dense_plan.h):
// 0 kBwdAuto, 1 kBwdTwoPass the dK/dV + dQ passes, 2 kBwdSinglePass the single pass wherever
// its shape conditions hold, 3 kBwdSinglePassGiveUp as 2 with the hand-off's timeout word
// preset, which exercises the dQ fallback pass.  Builds with -DFA_BWD_ABL also accept the
// timing-only ablations of the single pass (kBwdAbl*), which compute a WRONG dQ: 4, 5, 6 no
// waits, no running-sum traffic, neither; 7, 8 no running-sum loads / stores; 9 no dS image
// writes; 10 no next-slice Q/dO DMA; 11 = 10 + 6.  Any other value is rejected (returns -1,
// the mode is unchanged).
int fa_debug_set_bwd_mode(int v) {
    const int old = fa::g_bwd_mode;
#ifdef FA_BWD_ABL
    constexpr int kMaxMode = fa::kBwdAblNoNextDmaNoWaitsNoSums;
#else
    constexpr int kMaxMode = fa::kBwdSinglePassGiveUp;
#endif
    if (v < 0 || v > kMaxMode) return -1;
    fa::g_bwd_mode = v;
    return old;
}

// Not part of the public header: the single-pass backward hands its running dQ sums
// over in the XCD's L2 when all of a slab's members run on one XCD (plain stores instead
// of sc1 write-through): -1 auto (d, dv <= 64), 0 never, 1 always; returns the previous
// value (-2 for an invalid argument).
int fa_debug_set_bwd_l2local(int v) {
    const int old = fa::g_bwd_l2local;
    if (v < -1 || v > 1) return -2;
    fa::g_bwd_l2local = v;
    return old;
}

// Not part of the public header: the single-pass backward's slab placement: -1 auto (a
// slab's members on one XCD when they fit), 0 members dealt over the whole chip;
// returns the previous value (-2 for an invalid argument).
int fa_debug_set_bwd_xcd(int v) {
    const int old = fa::g_bwd_xcd;
    if (v < -1 || v > 0) return -2;
    fa::g_bwd_xcd = v;
    return old;
}

// Not part of the public header: the single-pass backward's step offset between
// consecutive members of a slice's chain (1..4, default 3); returns the previous value
// (-2 for an invalid argument).
int fa_debug_set_bwd_hoff(int v) {
    const int old = fa::g_bwd_hoff;
    if (v < 1 || v > 4) return -2;
    fa::g_bwd_hoff = v;
    return old;
}

// Not part of the public header: the single-pass backward's no-progress bound in
// microseconds (a poll gives up when the launch published nothing for this long;
// 10..10000000, default 100000); returns the previous value (-2 for an invalid argument).
int fa_debug_set_bwd_stall_us(int v) {
    const int old = fa::g_bwd_stall_us;
    if (v < 10 || v > 10000000) return -2;
    fa::g_bwd_stall_us = v;
    return old;
}

// Not part of the public header (tests): 1 makes every chain-B tail of the single-pass
// backward store its total and leave dQ = A + B of the wrapped slices to the guarded dQ
// pass's combine (the path a co-tenant can force), 0 the default; returns the previous
// value (-2 for an invalid argument).
int fa_debug_set_bwd_nodirect(int v) {
    const int old = fa::g_bwd_nodirect;
    if (v < 0 || v > 1) return -2;
    fa::g_bwd_nodirect = v;
    return old;
}

// Not part of the public header: circulant kernel override (1 one-wave-per-query,
// 2 LDS-tiled SIMT; 0 auto).
int fa_debug_set_circ_generic(int v) {
    const int old = fa::g_circ_force_generic;
    fa::g_circ_force_generic = (v == 1 || v == 2) ? v : 0;
    return old;
}

// Not part of the public header: which kernel the calling thread's last fa_circulant_fwd
// launched: 0 none, 1 tiled MFMA, 2 one wave per query, 3 LDS-tiled SIMT, 4 Float64 (tests).
int fa_debug_last_circ_fwd_kernel(void) { return fa::g_circ_fwd_last_kernel; }

// Not part of the public header: which kernel family the calling thread's last
// fa_circulant_bwd launched: 0 none, 1 MFMA tiled, 2 SIMT, 3 Float64 (tests).
int fa_debug_last_circ_bwd_kernel(void) { return fa::g_circ_bwd_last_kernel; }

// Not part of the public header (tests): the plan of a circulant forward / backward,
// fa::circ_fwd_plan / fa::circ_bwd_plan (fa_circulant_plan.h).  Returns the kernel, a
// fa::CircFwdKernel (the codes of fa_debug_last_circ_fwd_kernel), or the family, a
// fa::CircBwdFamily (those of fa_debug_last_circ_bwd_kernel); -1 for invalid arguments (out
// is left alone) and for a shape the launcher refuses.  Writes the plan's other fields to out
// (may be null).  Every input is an argument, the knob (a fa_debug_set_circ_generic value) and
// the 16-B alignment facts included: nothing is read from the thread's knobs or the device.
// forward out[9]: Dc, DVc, simt_class, simt_kt, nqb, total_wg, grid, block, status.
int fa_debug_circ_fwd_plan(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W, int knob,
                           int kv_aligned16, int64_t* out) {
    if (!valid_dtype(dtype) || N < 1 || d < 1 || dv < 1 || batch < 1 || W < 1) return -1;
    const fa::CircFwdPlan pl = fa::circ_fwd_plan(dtype, N, d, dv, batch, W, knob, kv_aligned16 != 0);
    if (out) {
        const int64_t f[9] = {pl.Dc, pl.DVc, pl.simt_class, pl.simt_kt, pl.nqb, pl.total_wg, pl.grid, pl.block, pl.status};
        for (int i = 0; i < 9; ++i) out[i] = f[i];
    }
    return pl.kernel;
}
// backward out[15]: w1, w1_grid, prepass_vec, prepass_grid, Dc, DVc, nblk, total_wg, grid, lds_dq,
// lds_dkdv, off_nD, off_nlse, total, status.
int fa_debug_circ_bwd_plan(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W, int knob,
                           int qkv_aligned16, int o_aligned16, int do_aligned16, int64_t* out) {
    if (!valid_dtype(dtype) || N < 1 || d < 1 || dv < 1 || batch < 1 || W < 1) return -1;
    const fa::CircBwdPlan pl = fa::circ_bwd_plan(dtype, N, d, dv, batch, W, knob, qkv_aligned16 != 0, o_aligned16 != 0,
                                                 do_aligned16 != 0);
    if (out) {
        const int64_t f[15] = {pl.w1, pl.w1_grid, pl.prepass_vec, pl.prepass_grid, pl.Dc, pl.DVc, pl.nblk, pl.total_wg,
                               pl.grid, (int64_t)pl.lds_dq, (int64_t)pl.lds_dkdv, (int64_t)pl.off_nD,
                               (int64_t)pl.off_nlse, (int64_t)pl.total, pl.status};
        for (int i = 0; i < 15; ++i) out[i] = f[i];
    }
    return pl.family;
}

// Not part of the public header: windowed forward path override (1 composed,
// 2 register-gather fused, 3 one-window row-shift (ws <= 7) / row-scatter, 4 four-window
// row-scatter, 5 one-window row-scatter, 6 two-window row-shift (the auto choice at ws <= 7),
// 10 eight-window strip (stride == ws), 12 three-window row-shift, where eligible; 13: the
// per-window backward with two windows per workgroup; 0 auto).  Modes 7-9 (rejected
// experimental kernels) were removed; they now select the auto path.
int fa_debug_set_win_composed(int v) {
    const int old = fa::g_win_force_composed;
    fa::g_win_force_composed = ((v >= 1 && v <= 6) || v == 10 || v == 12 || v == 13) ? v : 0;
    return old;
}

// Not part of the public header (tests): the kernel the windowed forward / backward picks
// for a shape, as a fa::WinFwdKernel / fa::WinBwdKernel value (-1: invalid arguments).  The
// mode (a fa_debug_set_win_composed value), the 16-B alignment facts of the tensors and the
// CU count are arguments: nothing is read from the thread's knobs or the device.
int fa_debug_win_fwd_plan(int dtype, int nspatial, const int64_t* spatial, int64_t d, int64_t dv, int64_t batch,
                          int64_t ws, int64_t stride, int64_t pad, int mode, int qkv_aligned16, int y_aligned16) {
    fa::WindowGeom g;
    const char* why = "";
    if (!valid_dtype(dtype) || d < 1 || dv < 1 || batch < 1) return -1;
    if (make_geom(g, nspatial, spatial, ws, stride, pad, &why) != FA_OK) return -1;
    return fa::win_fwd_plan(dtype, g, d, dv, batch, mode, qkv_aligned16 != 0, y_aligned16 != 0);
}
int fa_debug_win_bwd_plan(int dtype, int nspatial, const int64_t* spatial, int64_t d, int64_t dv, int64_t batch,
                          int64_t ws, int64_t stride, int64_t pad, int mode, int in_aligned16, int grad_aligned16,
                          int cus) {
    fa::WindowGeom g;
    const char* why = "";
    if (!valid_dtype(dtype) || d < 1 || dv < 1 || batch < 1) return -1;
    if (make_geom(g, nspatial, spatial, ws, stride, pad, &why) != FA_OK) return -1;
    return fa::win_bwd_plan(dtype, g, d, dv, batch, mode, in_aligned16 != 0, grad_aligned16 != 0, fa::win_cus(cus));
}

// The argument checks the four plan hooks below share (mask: a fa::DenseMask value; a masked
// plan needs Nk >= N; the backward plans also a head dimension within the compiled maximum).
static bool plan_args_ok(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, int mask, bool bwd) {
    return valid_dtype(dtype) && N >= 1 && Nk >= 1 && d >= 1 && dv >= 1 && batch >= 1 && mask >= fa::kMaskNone &&
           mask <= fa::kMaskLocal && !(mask != fa::kMaskNone && Nk < N) &&
           !(bwd && (d > fa::kMaxHeadDim || dv > fa::kMaxHeadDim));
}

// Not part of the public header (tests): the plan of a dense-family forward / backward,
// fa::dense_fwd_plan / fa::dense_bwd_plan (fa_dense_plan.h); the argument `causal` is the
// fa::DenseMask value (0 dense, 1 causal, 2 local).  Returns the kernel, a
// fa::DenseFwdKernel / fa::DenseBwdKernel value (-1: invalid arguments, or a head dimension
// above the compiled maximum), and writes the plan's other fields to out (may be null).
// Every input is an argument, the knob values, the 16-B alignment facts, the workspace bytes
// and the CU count included: nothing is read from the thread's knobs or the device.
// forward out[17]: causal bits, pad, ldk, nsplit, tps, rows, nqb, total_wg, grid, block, wide,
// off_k, off_v, off_opart, off_lpart, off_mpart, total.
int fa_debug_dense_fwd_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, int causal,
                            int variant, int causal_order, int kv_aligned16, int qo_aligned16, size_t ws_bytes,
                            int cus, int64_t* out) {
    if (!plan_args_ok(dtype, N, Nk, d, dv, batch, causal, false)) return -1;
    const fa::DenseFwdPlan pl = fa::dense_fwd_plan(dtype, N, Nk, d, dv, batch, (fa::DenseMask)causal, {variant, causal_order},
                                                   kv_aligned16 != 0, qo_aligned16 != 0, ws_bytes, cus);
    if (out) {
        const int64_t f[17] = {pl.causal, pl.pad, pl.ldk, pl.nsplit, pl.tps, pl.rows, pl.nqb, pl.total_wg, pl.grid,
                               pl.block, pl.wide, (int64_t)pl.off_k, (int64_t)pl.off_v, (int64_t)pl.off_opart,
                               (int64_t)pl.off_lpart, (int64_t)pl.off_mpart, (int64_t)pl.total};
        for (int i = 0; i < 17; ++i) out[i] = f[i];
    }
    return pl.kernel;
}
// backward out[25]: padded, N, Nk, d, dv as run, slabs_fit, nkb, nqt, xcd, off_nD, off_nlse,
// off_slab[10] (Q dQ K dK V dV O dO l m), off_flags, off_part, flag_bytes, total.
int fa_debug_dense_bwd_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, int causal,
                            int force_generic, int mode, int hoff, int xcd, int qkvdo_aligned16, size_t ws_bytes,
                            int cus, int64_t* out) {
    if (!plan_args_ok(dtype, N, Nk, d, dv, batch, causal, true)) return -1;
    const fa::DenseBwdPlan pl = fa::dense_bwd_plan(dtype, N, Nk, d, dv, batch, (fa::DenseMask)causal,
                                                   {force_generic, mode, hoff, xcd}, qkvdo_aligned16 != 0, ws_bytes, cus);
    if (out) {
        int64_t* o = out;
        for (int64_t v : {(int64_t)pl.padded, pl.N, pl.Nk, pl.d, pl.dv, (int64_t)pl.slabs_fit, (int64_t)pl.nkb,
                          (int64_t)pl.nqt, (int64_t)pl.xcd, (int64_t)pl.off_nD, (int64_t)pl.off_nlse})
            *o++ = v;
        for (size_t v : pl.off_slab) *o++ = (int64_t)v;
        for (size_t v : {pl.off_flags, pl.off_part, pl.flag_bytes, pl.total}) *o++ = (int64_t)v;
    }
    return pl.kernel;
}
// The plans of a local call under the default knobs, with fewer arguments and fields than the
// two hooks above at mask 2 (which agree with them: tests/test_local_host.py).  The window is
// not an argument: no plan depends on it.  forward out[8]: local, causal bits, pad, ldk,
// nsplit, rows, grid, total; backward out[6]: padded, N, Nk, d, dv as run, total.
int fa_debug_local_fwd_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                            int kv_aligned16, int qo_aligned16, size_t ws_bytes, int cus, int64_t* out) {
    if (!plan_args_ok(dtype, N, Nk, d, dv, batch, fa::kMaskLocal, false)) return -1;
    const fa::DenseFwdPlan pl = fa::dense_fwd_plan(dtype, N, Nk, d, dv, batch, fa::kMaskLocal, {fa::kFwdAuto, 0},
                                                   kv_aligned16 != 0, qo_aligned16 != 0, ws_bytes, cus);
    if (out) {
        const int64_t f[8] = {pl.mask == fa::kMaskLocal, pl.causal, pl.pad, pl.ldk, pl.nsplit, pl.rows, pl.grid, (int64_t)pl.total};
        for (int i = 0; i < 8; ++i) out[i] = f[i];
    }
    return pl.kernel;
}
int fa_debug_local_bwd_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                            int qkvdo_aligned16, size_t ws_bytes, int cus, int64_t* out) {
    if (!plan_args_ok(dtype, N, Nk, d, dv, batch, fa::kMaskLocal, true)) return -1;
    const fa::DenseBwdPlan pl = fa::dense_bwd_plan(dtype, N, Nk, d, dv, batch, fa::kMaskLocal,
                                                   {0, fa::kBwdAuto, 3, -1}, qkvdo_aligned16 != 0, ws_bytes, cus);
    if (out) {
        const int64_t f[6] = {pl.padded, pl.N, pl.Nk, pl.d, pl.dv, (int64_t)pl.total};
        for (int i = 0; i < 6; ++i) out[i] = f[i];
    }
    return pl.kernel;
}

// The plans of a varlen call, in the shape of the local hooks: the plans treat kMaskVarlen
// exactly as kMaskLocal (the class's default geometry, never a variant, never split, never p4,
// never the single pass), and no plan depends on the lengths or the window.  forward out[8]:
// varlen, causal bits, pad, ldk, nsplit, rows, grid, total; backward out[6] as the local hook.
int fa_debug_varlen_fwd_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                             int kv_aligned16, int qo_aligned16, size_t ws_bytes, int cus, int64_t* out) {
    if (!plan_args_ok(dtype, N, Nk, d, dv, batch, fa::kMaskLocal, false)) return -1;
    const fa::DenseFwdPlan pl = fa::dense_fwd_plan(dtype, N, Nk, d, dv, batch, fa::kMaskVarlen, {fa::kFwdAuto, 0},
                                                   kv_aligned16 != 0, qo_aligned16 != 0, ws_bytes, cus);
    if (out) {
        const int64_t f[8] = {pl.mask == fa::kMaskVarlen, pl.causal, pl.pad, pl.ldk, pl.nsplit, pl.rows, pl.grid, (int64_t)pl.total};
        for (int i = 0; i < 8; ++i) out[i] = f[i];
    }
    return pl.kernel;
}
int fa_debug_varlen_bwd_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                             int qkvdo_aligned16, size_t ws_bytes, int cus, int64_t* out) {
    if (!plan_args_ok(dtype, N, Nk, d, dv, batch, fa::kMaskLocal, true)) return -1;
    const fa::DenseBwdPlan pl = fa::dense_bwd_plan(dtype, N, Nk, d, dv, batch, fa::kMaskVarlen,
                                                   {0, fa::kBwdAuto, 3, -1}, qkvdo_aligned16 != 0, ws_bytes, cus);
    if (out) {
        const int64_t f[6] = {pl.padded, pl.N, pl.Nk, pl.d, pl.dv, (int64_t)pl.total};
        for (int i = 0; i < 6; ++i) out[i] = f[i];
    }
    return pl.kernel;
}
static_assert(std::is_same<int32_t, int>::value, "include/fa_hip.h declares the varlen lengths as const int*");
// Not part of the public header (tests): the clamp the varlen kernels apply to a caller's
// length, fa::varlen_clamp(len, n) = min(max(len, 0), n).
int fa_debug_varlen_clamp(int len, int n) { return fa::varlen_clamp(len, n); }

// Not part of the public header: workgroups of the persistent strip backward (0 = one per
// CU, the default; 1..4096 caps the grid).  Benchmark knob; returns the previous value.
int fa_debug_set_win_bwd_grid(int v) {
    const int old = fa::g_win_bwd_grid;
    if (v >= 0 && v <= 4096) fa::g_win_bwd_grid = v;
    return old;
}

// ---------------------------------------------------------------------------------------
// The dense family: dense, causal and local attention are one forward body, one backward
// body and one workspace query under a fa::DenseMask.  The public functions below are
// one-line forwards, and every place where the masks' contracts differ is an
// `if (mask == fa::kMaskNone)` here or a name looked up from the mask.
// ---------------------------------------------------------------------------------------

// "workspace missing or smaller than fa_<mask>_<fwd|bwd>_workspace()": each mask names its own query
static int fail_workspace(const char* fn, fa::DenseMask mask, const char* dir) {
    const std::string msg = std::string("workspace missing or smaller than fa_") + fa::mask_word(mask) + "_" + dir + "_workspace()";
    return fail(FA_ERR_WORKSPACE, fn, msg.c_str());
}

// The checks the causal and local entry points make after the null-pointer and DimensionMismatch
// ones, in order: head dims and Nk >= N, then the kernels' 32-bit extents (the launchers'
// own conditions, repeated here so that they precede the workspace check and any launch).
// The dense entry points make none: their launchers refuse, in their own words, after the
// workspace check.
static int masked_shape_check(fa::DenseMask mask, int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv,
                              int64_t batch, bool bwd, const char** why) {
    if (mask == fa::kMaskNone) return FA_OK;
    if (d > fa::kMaxHeadDim || dv > fa::kMaxHeadDim) {
        *why = "head dimension exceeds the compiled maximum (128)";
        return FA_ERR_UNSUPPORTED;
    }
    if (fa::mask_lacks_keys(mask, N, Nk, why)) return FA_ERR_UNSUPPORTED;
    const bool big = N > INT32_MAX / 2 || Nk > INT32_MAX / 2 || N * d > INT32_MAX || Nk * d > INT32_MAX ||
                     Nk * dv > INT32_MAX || N * dv > INT32_MAX ||
                     (bwd && (N * batch > INT32_MAX / 2 || Nk * batch > INT32_MAX / 2)) ||
                     (dtype == FA_DTYPE_F64 && (N + 63) / 64 * batch > INT32_MAX);
    if (big) {
        *why = "extent exceeds the kernels' 32-bit addressing";
        return FA_ERR_UNSUPPORTED;
    }
    return FA_OK;
}

// The six workspace queries.  Dense answers 0 only for non-positive extents; a masked call
// with Nk < N is refused, so its query answers 0 as well.
static size_t dense_family_workspace(fa::DenseMask mask, bool bwd, int dtype, int64_t N, int64_t Nk, int64_t d,
                                     int64_t dv, int64_t batch) {
    if (!valid_dtype(dtype) || N < 1 || Nk < (mask == fa::kMaskNone ? 1 : N) || d < 1 || dv < 1 || batch < 1) return 0;
    return bwd ? fa::dense_bwd_workspace(dtype, N, Nk, d, dv, batch, mask)
               : fa::dense_fwd_workspace(dtype, N, Nk, d, dv, batch, mask);
}

// fn: the public function's name.  The window (left, right) is read under kMaskLocal and kMaskVarlen; it
// stays int64_t down to the launchers (fa::mask_ints clamps it to [0, Nk] before it becomes a
// 32-bit int) and changes neither a check nor a workspace answer.  takes_ws: false for
// fa_dense_fwd, which has no workspace argument and runs what needs none.
static int dense_family_fwd(fa::DenseMask mask, const char* fn, int dtype, const void* Q, const void* K,
                            const void* V, void* O, float* l, float* m, int64_t N, int64_t Nk, int64_t d,
                            int64_t dv, int64_t batch, int64_t left, int64_t right, float scale, bool takes_ws,
                            void* workspace, size_t workspace_bytes, void* hip_stream,
                            const int32_t* q_lens = nullptr, const int32_t* k_lens = nullptr) {
    if (!valid_dtype(dtype)) return fail(FA_ERR_INVALID_ARG, fn, "unknown dtype");
    if (N < 0 || Nk < 0 || d < 1 || dv < 1 || batch < 0)
        return fail(FA_ERR_INVALID_ARG, fn, "DimensionMismatch: N, Nk, batch must be >= 0 and d, dv >= 1");
    if (mask == fa::kMaskNone) {   // no query: nothing to write; no key: O = 0, l = 0, m = -Inf
        int erc;
        if (dense_fwd_empty(dtype, O, l, m, N, Nk, dv, batch, (hipStream_t)hip_stream, &erc))
            return erc == FA_OK ? ok() : fail(erc, fn, erc == FA_ERR_HIP ? "hipMemsetAsync failed" : "null pointer");
    } else if (N == 0 || batch == 0) {
        return ok();   // no query: nothing to write (Nk = 0 < N is refused below)
    }
    if (!Q || !K || !V || !O || !l || !m) return fail(FA_ERR_INVALID_ARG, fn, "null pointer");
    const char* why = "";
    int rc = masked_shape_check(mask, dtype, N, Nk, d, dv, batch, false, &why);
    if (rc != FA_OK) return fail(rc, fn, why);
    if (takes_ws) {
        const size_t need = fa::dense_fwd_workspace(dtype, N, Nk, d, dv, batch, mask);
        if (need > 0 && (!workspace || workspace_bytes < need))
            return fail_workspace(fn, mask, "fwd");
    }
    fa::DenseArgs a{dtype, Q, K, V, O, l, m, N, Nk, d, dv, batch, resolve_scale(scale, d)};
    a.scale64 = resolve_scale64(scale, d);
    a.workspace = workspace;
    a.workspace_bytes = workspace_bytes;
    a.mask = mask;
    a.left = left;
    a.right = right;
    a.q_lens = q_lens;   // device data, kMaskVarlen only: never read here
    a.k_lens = k_lens;
    rc = fa::launch_dense_fwd(a, (hipStream_t)hip_stream, &why);
    return rc == FA_OK ? ok() : fail(rc, fn, why);
}

static int dense_family_bwd(fa::DenseMask mask, const char* fn, int dtype, const void* Q, const void* K,
                            const void* V, const void* O, const void* dO, const float* l, const float* m, void* dQ,
                            void* dK, void* dV, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                            int64_t left, int64_t right, float scale, void* workspace, size_t workspace_bytes,
                            void* hip_stream, const int32_t* q_lens = nullptr, const int32_t* k_lens = nullptr) {
    if (!valid_dtype(dtype)) return fail(FA_ERR_INVALID_ARG, fn, "unknown dtype");
    if (N < 0 || Nk < 0 || d < 1 || dv < 1 || batch < 0)
        return fail(FA_ERR_INVALID_ARG, fn, "DimensionMismatch: N, Nk, batch must be >= 0 and d, dv >= 1");
    if (mask == fa::kMaskNone) {
        if (N == 0 || Nk == 0 || batch == 0) {   // empty sums: every gradient element is 0
            const size_t esz = fa::dtype_size(dtype);
            const hipStream_t s = (hipStream_t)hip_stream;
            const size_t nq = (size_t)(N * d * batch), nk = (size_t)(Nk * d * batch), nv = (size_t)(Nk * dv * batch);
            if ((nq && !dQ) || (nk && (!dK || !dV))) return fail(FA_ERR_INVALID_ARG, fn, "null pointer");
            if ((nq && hipMemsetAsync(dQ, 0, nq * esz, s) != hipSuccess) ||
                (nk && hipMemsetAsync(dK, 0, nk * esz, s) != hipSuccess) ||
                (nv && hipMemsetAsync(dV, 0, nv * esz, s) != hipSuccess))
                return fail(FA_ERR_HIP, fn, "hipMemsetAsync failed");
            return ok();
        }
    } else if (N == 0 || batch == 0) {
        return ok();   // no query (and, with Nk >= N required, no call with keys only)
    }
    if (!Q || !K || !V || !O || !dO || !l || !m || !dQ || !dK || !dV)
        return fail(FA_ERR_INVALID_ARG, fn, "null pointer");
    const char* why = "";
    int rc = masked_shape_check(mask, dtype, N, Nk, d, dv, batch, true, &why);
    if (rc != FA_OK) return fail(rc, fn, why);
    const size_t need = fa::dense_bwd_workspace(dtype, N, Nk, d, dv, batch, mask);
    // a masked backward rejects a null workspace whatever `need` is
    if ((mask != fa::kMaskNone || need > 0) && (!workspace || workspace_bytes < need))
        return fail_workspace(fn, mask, "bwd");
    fa::DenseBwdArgs a{dtype, Q, K, V, O, dO, l, m, dQ, dK, dV, N, Nk, d, dv, batch,
                       resolve_scale(scale, d), workspace, workspace_bytes};
    a.scale64 = resolve_scale64(scale, d);
    a.mask = mask;
    a.left = left;
    a.right = right;
    a.q_lens = q_lens;
    a.k_lens = k_lens;
    rc = fa::launch_dense_bwd(a, (hipStream_t)hip_stream, &why);
    return rc == FA_OK ? ok() : fail(rc, fn, why);
}

size_t fa_dense_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    return dense_family_workspace(fa::kMaskNone, false, dtype, N, Nk, d, dv, batch);
}
size_t fa_dense_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    return dense_family_workspace(fa::kMaskNone, true, dtype, N, Nk, d, dv, batch);
}
size_t fa_causal_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    return dense_family_workspace(fa::kMaskCausal, false, dtype, N, Nk, d, dv, batch);
}
size_t fa_causal_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    return dense_family_workspace(fa::kMaskCausal, true, dtype, N, Nk, d, dv, batch);
}
size_t fa_local_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    return dense_family_workspace(fa::kMaskLocal, false, dtype, N, Nk, d, dv, batch);
}
size_t fa_local_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    return dense_family_workspace(fa::kMaskLocal, true, dtype, N, Nk, d, dv, batch);
}
size_t fa_varlen_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    return dense_family_workspace(fa::kMaskVarlen, false, dtype, N, Nk, d, dv, batch);
}
size_t fa_varlen_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    return dense_family_workspace(fa::kMaskVarlen, true, dtype, N, Nk, d, dv, batch);
}

int fa_dense_fwd_ws(int dtype, const void* Q, const void* K, const void* V, void* O, float* l, float* m,
                    int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, float scale,
                    void* workspace, size_t workspace_bytes, void* hip_stream) {
    return dense_family_fwd(fa::kMaskNone, "fa_dense_fwd_ws", dtype, Q, K, V, O, l, m, N, Nk, d, dv, batch, -1, -1, scale,
                            true, workspace, workspace_bytes, hip_stream);
}
int fa_dense_fwd(int dtype, const void* Q, const void* K, const void* V, void* O, float* l, float* m,
                 int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, float scale,
                 void* hip_stream) {
    return dense_family_fwd(fa::kMaskNone, "fa_dense_fwd", dtype, Q, K, V, O, l, m, N, Nk, d, dv, batch, -1, -1, scale,
                            false, nullptr, 0, hip_stream);
}
int fa_causal_fwd(int dtype, const void* Q, const void* K, const void* V, void* O, float* l, float* m,
                  int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, float scale,
                  void* workspace, size_t workspace_bytes, void* hip_stream) {
    return dense_family_fwd(fa::kMaskCausal, "fa_causal_fwd", dtype, Q, K, V, O, l, m, N, Nk, d, dv, batch, -1, -1, scale,
                            true, workspace, workspace_bytes, hip_stream);
}
int fa_local_fwd(int dtype, const void* Q, const void* K, const void* V, void* O, float* l, float* m,
                 int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, int64_t left, int64_t right,
                 float scale, void* workspace, size_t workspace_bytes, void* hip_stream) {
    return dense_family_fwd(fa::kMaskLocal, "fa_local_fwd", dtype, Q, K, V, O, l, m, N, Nk, d, dv, batch, left, right,
                            scale, true, workspace, workspace_bytes, hip_stream);
}

int fa_varlen_fwd(int dtype, const void* Q, const void* K, const void* V, void* O, float* l, float* m,
                  int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, const int32_t* q_lens,
                  const int32_t* k_lens, int64_t left, int64_t right, float scale, void* workspace,
                  size_t workspace_bytes, void* hip_stream) {
    return dense_family_fwd(fa::kMaskVarlen, "fa_varlen_fwd", dtype, Q, K, V, O, l, m, N, Nk, d, dv, batch, left, right,
                            scale, true, workspace, workspace_bytes, hip_stream, q_lens, k_lens);
}

int fa_dense_bwd(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* dO,
                 const float* l, const float* m, void* dQ, void* dK, void* dV, int64_t N, int64_t Nk,
                 int64_t d, int64_t dv, int64_t batch, float scale, void* workspace,
                 size_t workspace_bytes, void* hip_stream) {
    return dense_family_bwd(fa::kMaskNone, "fa_dense_bwd", dtype, Q, K, V, O, dO, l, m, dQ, dK, dV, N, Nk, d, dv, batch,
                            -1, -1, scale, workspace, workspace_bytes, hip_stream);
}
int fa_causal_bwd(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* dO,
                  const float* l, const float* m, void* dQ, void* dK, void* dV, int64_t N, int64_t Nk,
                  int64_t d, int64_t dv, int64_t batch, float scale, void* workspace,
                  size_t workspace_bytes, void* hip_stream) {
    return dense_family_bwd(fa::kMaskCausal, "fa_causal_bwd", dtype, Q, K, V, O, dO, l, m, dQ, dK, dV, N, Nk, d, dv, batch,
                            -1, -1, scale, workspace, workspace_bytes, hip_stream);
}
int fa_local_bwd(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* dO,
                 const float* l, const float* m, void* dQ, void* dK, void* dV, int64_t N, int64_t Nk,
                 int64_t d, int64_t dv, int64_t batch, int64_t left, int64_t right, float scale,
                 void* workspace, size_t workspace_bytes, void* hip_stream) {
    return dense_family_bwd(fa::kMaskLocal, "fa_local_bwd", dtype, Q, K, V, O, dO, l, m, dQ, dK, dV, N, Nk, d, dv, batch,
                            left, right, scale, workspace, workspace_bytes, hip_stream);
}

int fa_varlen_bwd(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* dO,
                  const float* l, const float* m, void* dQ, void* dK, void* dV, int64_t N, int64_t Nk,
                  int64_t d, int64_t dv, int64_t batch, const int32_t* q_lens, const int32_t* k_lens,
                  int64_t left, int64_t right, float scale, void* workspace, size_t workspace_bytes,
                  void* hip_stream) {
    return dense_family_bwd(fa::kMaskVarlen, "fa_varlen_bwd", dtype, Q, K, V, O, dO, l, m, dQ, dK, dV, N, Nk, d, dv, batch,
                            left, right, scale, workspace, workspace_bytes, hip_stream, q_lens, k_lens);
}

// Not part of the public header: launch order of the causal fast forward's query blocks
// 0 in order; 1 slab by slab, a slab's heaviest (last) block first; 2 block-major inside each
// XCD's share of the grid, heaviest blocks of all its slabs first (where that share holds
// whole slabs, else as 1): the default.  Benchmark knob; returns the previous value (-2 for an invalid
// argument).
int fa_debug_set_causal_order(int v) {
    const int old = fa::g_causal_rev;
    if (v < 0 || v > 2) return -2;
    fa::g_causal_rev = v;
    return old;
}

int fa_dense_bwd_handoff_status(const void* workspace, size_t workspace_bytes, void* hip_stream, int* status) {
    static const char* fn = "fa_dense_bwd_handoff_status";
    if (!status) return fail(FA_ERR_INVALID_ARG, fn, "null status pointer");
    const char* why = "";
    const int rc = fa::dense_bwd_handoff_status(workspace, workspace_bytes, (hipStream_t)hip_stream, status, &why);
    return rc == FA_OK ? ok() : fail(rc, fn, why);
}

size_t fa_windowed_workspace(int dtype, int nspatial, const int64_t* spatial, int64_t d, int64_t dv,
                             int64_t batch, int64_t ws, int64_t stride, int64_t pad) {
    fa::WindowGeom g;
    const char* why = "";
    if (!valid_dtype(dtype) || d < 1 || dv < 1 || batch < 1) return 0;
    if (make_geom(g, nspatial, spatial, ws, stride, pad, &why) != FA_OK) return 0;
    return fa::windowed_workspace(dtype, g, d, dv, batch);
}

size_t fa_windowed_fwd_workspace(int dtype, int nspatial, const int64_t* spatial, int64_t d, int64_t dv,
                                 int64_t batch, int64_t ws, int64_t stride, int64_t pad) {
    fa::WindowGeom g;
    const char* why = "";
    if (!valid_dtype(dtype) || d < 1 || dv < 1 || batch < 1) return 0;
    if (make_geom(g, nspatial, spatial, ws, stride, pad, &why) != FA_OK) return 0;
    return fa::windowed_fwd_workspace(dtype, g, d, dv, batch);
}

int fa_windowed_fwd(int dtype, const void* q, const void* k, const void* v, void* y, float* l, float* m,
                    int nspatial, const int64_t* spatial, int64_t d, int64_t dv, int64_t batch,
                    int64_t ws, int64_t stride, int64_t pad, float scale, void* workspace,
                    size_t workspace_bytes, void* hip_stream) {
    static const char* fn = "fa_windowed_fwd";
    if (!valid_dtype(dtype)) return fail(FA_ERR_INVALID_ARG, fn, "unknown dtype");
    if (d < 1 || dv < 1 || batch < 0)
        return fail(FA_ERR_INVALID_ARG, fn, "DimensionMismatch: d, dv must be >= 1, batch >= 0");
    fa::WindowedArgs a{};
    const char* why = "";
    int rc = make_geom(a.g, nspatial, spatial, ws, stride, pad, &why);
    if (rc != FA_OK) return fail(rc, fn, why);
    if (batch == 0) return ok();   // no image: windowed_fa on an empty batch computes nothing
    if (!q || !k || !v || !y || !l || !m) return fail(FA_ERR_INVALID_ARG, fn, "null pointer");
    a.dtype = dtype; a.q = q; a.k = k; a.v = v; a.y = y; a.l = l; a.m = m;
    a.d = d; a.dv = dv; a.batch = batch;
    a.scale = resolve_scale(scale, d);
    a.scale64 = resolve_scale64(scale, d);
    const size_t need = fa::windowed_fwd_workspace(dtype, a.g, d, dv, batch);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(FA_ERR_WORKSPACE, fn, "workspace missing or smaller than fa_windowed_fwd_workspace()");
    a.workspace = workspace;
    a.workspace_bytes = workspace_bytes;
    rc = fa::launch_windowed_fwd(a, (hipStream_t)hip_stream, &why);
    return rc == FA_OK ? ok() : fail(rc, fn, why);
}

static int window_common(const char* fn, int dtype, const void* src, void* dst, int nspatial,
                         const int64_t* spatial, int64_t C, int64_t batch, int64_t ws, int64_t stride,
                         int64_t pad, bool unwindow, void* hip_stream) {
    if (!valid_dtype(dtype)) return fail(FA_ERR_INVALID_ARG, fn, "unknown dtype");
    if (C < 1 || batch < 0) return fail(FA_ERR_INVALID_ARG, fn, "DimensionMismatch: C must be >= 1, batch >= 0");
    fa::WindowGeom g{};
    const char* why = "";
    int rc = make_geom(g, nspatial, spatial, ws, stride, pad, &why);
    if (rc != FA_OK) return fail(rc, fn, why);
    if (batch == 0) return ok();   // empty batch: nothing to move
    if (!src || !dst) return fail(FA_ERR_INVALID_ARG, fn, "null pointer");
    rc = fa::launch_window(dtype, src, dst, g, C, batch, unwindow, (hipStream_t)hip_stream, &why);
    return rc == FA_OK ? ok() : fail(rc, fn, why);
}

int fa_window(int dtype, const void* x, void* xw, int nspatial, const int64_t* spatial, int64_t C,
              int64_t batch, int64_t ws, int64_t stride, int64_t pad, void* hip_stream) {
    return window_common("fa_window", dtype, x, xw, nspatial, spatial, C, batch, ws, stride, pad, false,
                         hip_stream);
}

int fa_unwindow(int dtype, const void* xw, void* x, int nspatial, const int64_t* spatial, int64_t C,
                int64_t batch, int64_t ws, int64_t stride, int64_t pad, void* hip_stream) {
    return window_common("fa_unwindow", dtype, xw, x, nspatial, spatial, C, batch, ws, stride, pad, true,
                         hip_stream);
}

int fa_windowed_bwd(int dtype, const void* q, const void* k, const void* v, const void* y, const void* dy,
                    const float* l, const float* m, void* dq, void* dk, void* dv_, int nspatial,
                    const int64_t* spatial, int64_t d, int64_t dv, int64_t batch, int64_t ws,
                    int64_t stride, int64_t pad, float scale, void* workspace, size_t workspace_bytes,
                    void* hip_stream) {
    static const char* fn = "fa_windowed_bwd";
    if (!valid_dtype(dtype)) return fail(FA_ERR_INVALID_ARG, fn, "unknown dtype");
    if (d < 1 || dv < 1 || batch < 0)
        return fail(FA_ERR_INVALID_ARG, fn, "DimensionMismatch: d, dv must be >= 1, batch >= 0");
    fa::WindowedBwdArgs a{};
    const char* why = "";
    int rc = make_geom(a.g, nspatial, spatial, ws, stride, pad, &why);
    if (rc != FA_OK) return fail(rc, fn, why);
    if (batch == 0) return ok();   // no image, no gradient element
    if (!q || !k || !v || !y || !dy || !l || !m || !dq || !dk || !dv_)
        return fail(FA_ERR_INVALID_ARG, fn, "null pointer");
    const size_t need = fa::windowed_workspace(dtype, a.g, d, dv, batch);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(FA_ERR_WORKSPACE, fn, "workspace missing or smaller than fa_windowed_workspace()");
    a.dtype = dtype; a.q = q; a.k = k; a.v = v; a.y = y; a.dy = dy; a.l = l; a.m = m;
    a.dq = dq; a.dk = dk; a.dv_ = dv_;
    a.d = d; a.dv = dv; a.batch = batch;
    a.scale = resolve_scale(scale, d);
    a.scale64 = resolve_scale64(scale, d);
    a.workspace = workspace;
    a.workspace_bytes = workspace_bytes;
    rc = fa::launch_windowed_bwd(a, (hipStream_t)hip_stream, &why);
    return rc == FA_OK ? ok() : fail(rc, fn, why);
}

// The checks fa_circulant_fwd and fa_circulant_bwd share, in their order.  True when the call
// is complete, with its status in *rc: an argument refused, or an empty input (circulant_fa!
// loops over no row / slab; no query, no key: no gradient element), which dereferences
// nothing, so the null-pointer check (null_ptr: one of the call's tensors is null) comes after.
static bool circ_call_done(const char* fn, int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W,
                           bool null_ptr, int* rc) {
    if (!valid_dtype(dtype)) *rc = fail(FA_ERR_INVALID_ARG, fn, "unknown dtype");
    else if (N < 0 || d < 1 || dv < 1 || batch < 0)
        *rc = fail(FA_ERR_INVALID_ARG, fn, "DimensionMismatch: d, dv must be >= 1, N, batch >= 0");
    else if (W < 1) *rc = fail(FA_ERR_INVALID_ARG, fn, "DimensionMismatch: window size W must be >= 1");
    else if (N == 0 || batch == 0) *rc = ok();
    else if (null_ptr) *rc = fail(FA_ERR_INVALID_ARG, fn, "null pointer");
    else return false;
    return true;
}

int fa_circulant_fwd(int dtype, const void* Q, const void* K, const void* V, void* O, float* l, float* m,
                     int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W, float scale,
                     void* hip_stream) {
    static const char* fn = "fa_circulant_fwd";
    int rc;
    if (circ_call_done(fn, dtype, N, d, dv, batch, W, !Q || !K || !V || !O || !l || !m, &rc)) return rc;
    fa::CircArgs a{dtype, Q, K, V, O, l, m, N, d, dv, batch, W, resolve_scale(scale, d)};
    a.scale64 = resolve_scale64(scale, d);
    const char* why = "";
    rc = fa::launch_circulant_fwd(a, (hipStream_t)hip_stream, &why);
    return rc == FA_OK ? ok() : fail(rc, fn, why);
}

size_t fa_circulant_bwd_workspace(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W) {
    if (!valid_dtype(dtype) || N < 1 || d < 1 || dv < 1 || batch < 1 || W < 1) return 0;
    return fa::circulant_bwd_workspace(dtype, N, d, dv, batch, W);
}

int fa_circulant_bwd(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* dO,
                     const float* l, const float* m, void* dQ, void* dK, void* dV, int64_t N, int64_t d,
                     int64_t dv, int64_t batch, int64_t W, float scale, void* workspace,
                     size_t workspace_bytes, void* hip_stream) {
    static const char* fn = "fa_circulant_bwd";
    int rc;
    if (circ_call_done(fn, dtype, N, d, dv, batch, W, !Q || !K || !V || !O || !dO || !l || !m || !dQ || !dK || !dV, &rc))
        return rc;
    fa::CircBwdArgs a{dtype, Q, K, V, O, dO, l, m, dQ, dK, dV, N, d, dv, batch, W,
                      resolve_scale(scale, d), workspace, workspace_bytes};
    a.scale64 = resolve_scale64(scale, d);
    const char* why = "";
    rc = fa::launch_circulant_bwd(a, (hipStream_t)hip_stream, &why);
    return rc == FA_OK ? ok() : fail(rc, fn, why);
}

size_t fa_softmax_workspace(int64_t M, int64_t N, int64_t batch, int dims) {
    if (M < 1 || N < 1 || batch < 1 || (dims != 1 && dims != 2)) return 0;
    return fa::softmax_workspace(M, N, batch, dims);
}

int fa_softmax(int dtype, const void* S, void* P, int64_t M, int64_t N, int64_t batch, int dims,
               void* workspace, size_t workspace_bytes, void* hip_stream) {
    static const char* fn = "fa_softmax";
    if (!valid_dtype(dtype)) return fail(FA_ERR_INVALID_ARG, fn, "unknown dtype");
    if (dims != 1 && dims != 2) return fail(FA_ERR_INVALID_ARG, fn, "only softmax in dims 1 or 2 supported");
    if (M < 1 || N < 1 || batch < 0)
        return fail(FA_ERR_INVALID_ARG, fn, "DimensionMismatch: M, N must be >= 1, batch >= 0");
    if (batch == 0) return ok();   // no matrix to normalise
    if (!S || !P) return fail(FA_ERR_INVALID_ARG, fn, "null pointer");
    const size_t need = fa::softmax_workspace(M, N, batch, dims);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(FA_ERR_WORKSPACE, fn, "workspace missing or smaller than fa_softmax_workspace()");
    fa::SoftmaxArgs a{dtype, S, P, M, N, batch, dims, workspace, workspace_bytes};
    const char* why = "";
    const int rc = fa::launch_softmax(a, (hipStream_t)hip_stream, &why);
    return rc == FA_OK ? ok() : fail(rc, fn, why);
}

}  // extern "C"
