// fa_bwd_params.h — what the translation units of the dense backward share: the kernels'
// by-value parameters, the two device helpers every kernel path uses, and the host launch
// functions the kernel files export to fa_bwd.hip.  No kernel lives here.
//   fa_bwd.hip        host side (plan -> launches, workspace, knobs), pre-passes, pad / unpad
//   fa_bwd_simt_dq.hip, fa_bwd_simt_dkdv.hip   bwd_generic_dq, bwd_generic_dkdv (SIMT, every dtype)
//   fa_bwd_f32.hip    bwd_dq_f32, bwd_dkdv_f32 (fp32 MFMA)
//   fa_bwd_dq.hip     bwd_dq_fast, with fused_combine (16-bit MFMA)
//   fa_bwd_dkdv.hip   bwd_dkdv_fast
//   fa_bwd_fused.hip  bwd_fused (the single pass)
// (the device helpers of the three MFMA files are in fa_bwd_common.h)
#pragma once

#include "fa_internal.h"
#include "../../include/fa_hip.h"

namespace fa {

// bwd_fused: a poll gives up only when the whole launch has published nothing for this
// long (fa_debug_set_bwd_stall_us): a safety net, not a scheduling decision (§ bwd_fused).
// The boundary header states the same bound (tests/test_abi.py checks they agree).
constexpr int kStallUs = FA_BWD_HANDOFF_STALL_US;

// (the single pass's hand-off words, FusedFlags, are laid out in fa_dense_plan.h)

struct BwdParams {
    const void *Q, *K, *V, *O, *dO;
    const float *l, *m;
    void *dQ, *dK, *dV;
    float* nD;     // workspace: −rowsum(dO ∘ O)          [batch][N]
    float* nlse;   // workspace: −(m + ln l)/τ (raw units) [batch][N]
    int N, Nk, d, dv, batch;
    // the caller's key count.  The padded path runs on Nk rounded up to 8: the zero rows
    // j >= nkv are masked (P = 0) where a dQ is summed, not left to P * 0: with every real
    // score far below 0 their P = exp(0 - lse) overflows (fp16 dS from lse < -11 on)
    int nkv = 0;
    int nblk, total_wg;          // fast path: row blocks per slab, workgroups
    float scale, scale_log2;
    double scale64 = 0.0;        // Float64 generic path: τ in double
    // single-pass kernel (bwd_fused): dQ hand-off state, all in the caller's workspace
    unsigned* flags = nullptr;   // hand-off words (FusedFlags, zeroed per call)
    unsigned* err = nullptr;     // hand-off timeout word = hdr[1] (set per call by the pre-pass)
    // workspace header (first 256 B of the aligned workspace; fa_dense_bwd_handoff_status):
    // hdr[0] = kBwdHdrMagic | plan (1 = single pass), hdr[1] = the timeout word,
    // hdr[2] = give-ups counted over every call on this workspace (never reset here),
    // hdr[3] = some chain-B tail of this call left its slice to bwd_dq_fast's combine
    unsigned* hdr = nullptr;
    unsigned hdr_plan = 0, hdr_err = 0;
    float* part = nullptr;       // [batch][2 chains][nqt][D/16 tiles][16 x 64] fp32 running dQ sums
    int nkb = 0, nqt = 0, hoff = 3, xcd = 0;   // key blocks, 64-query slices, step offset, XCD mapping
    int stall_ticks = kStallUs * 100;   // no-progress bound of a poll in s_memrealtime ticks (100 MHz)
    int nodirect = 0;                   // tests: chain-B tails store, bwd_dq_fast adds A + B (fa_debug_set_bwd_nodirect)
    int l2local = 0;  // 1: hand the running sums over in the XCD's L2 when a slab's members share one
    int ablate = 0;   // timing-only ablations (wrong dQ): 1 no waits, 2 no sum traffic, 8 no sum loads, 16 no sum stores, 32 no dS image writes
    const unsigned* guard = nullptr;           // bwd_dq_fast runs only if *guard != 0 (nullptr: always)
    const unsigned* sguard = nullptr;          // ... and then only on the slabs b with sguard[b] != 0
    const unsigned* cguard = nullptr;          // bwd_dq_fast: combine the wrapped slices bwd_fused left (*cguard != 0)
    const unsigned* fin = nullptr;             // ... those with fin[b][t] == 2
    // causal (fa_causal_bwd; read by the CAUSAL instantiations only): query i sees keys
    // j <= i + off, off = Nk - N of the caller's extents (the padded path rounds N and Nk up
    // separately and keeps this off)
    int causal = 0, off = 0;
    // local (fa_local_bwd; read by the LOCAL instantiations only, which also read off): query i
    // sees keys i + off - left <= j <= i + off + right, both sides clamped to [0, Nk] of the
    // caller's extents, where Nk binds nowhere (mask_ints)
    int local = 0, left = 0, right = 0;
    // varlen (fa_varlen_bwd; read by the kMaskVarlen instantiations only, which are LOCAL bodies):
    // `batch` int32 lengths on the device (null = full), clamped to the caller's extents nqv / nkv
    // (the padded path rounds N and Nk up); off is then per slab, nk - nq (bwd_ext)
    const int32_t *q_lens = nullptr, *k_lens = nullptr;
    int nqv = 0;
};

// The extents of slab b in the bounds of a masked kernel: the launch's own (N, Nk as run, off
// and the window from the host), or under VARLEN the slab's (varlen_extents).  Strides stay
// p.N / p.Nk.  Rows >= nq carry nlse = -inf from the varlen pre-pass (P = 0 exactly), so the
// kernels only trim their loops at nq; keys >= nk are selected to -inf where S is formed.
template <bool VARLEN>
__device__ __forceinline__ VarlenExt bwd_ext(const BwdParams& p, int b) {
    if constexpr (VARLEN) return varlen_extents(p.q_lens, p.k_lens, b, p.nqv, p.nkv, p.left, p.right);
    return VarlenExt{p.N, p.Nk, p.off, p.left, p.right};
}
// `rows` zero rows of a [C][ld] slab from row r0 (clipped at ld), by the whole workgroup
template <class T>
__device__ __forceinline__ void zero_rows(T* slab, int ld, int C, int r0, int rows, int nthreads) {
    const int n = min(rows, ld - r0);
    for (int i = threadIdx.x; i < n * C; i += nthreads) slab[(int64_t)(i / n) * ld + r0 + i % n] = (T)0.0f;
}

constexpr unsigned kBwdHdrMagic = 0x46414200u;   // "FAB\0"

// the SIMT kernels' tile (fa_bwd_simt_dq.hip, fa_bwd_simt_dkdv.hip)
constexpr int kGT = 32;          // tile edge
constexpr int kGThreads = 256;

// --------------------------------------------------------------------------
// Host launch functions, one per kernel family, each defined (and instantiated for the
// types named) in the file that holds the kernels: a kernel is launched from its own
// translation unit.  Each picks the instantiation for (T, p.d, p.dv, mask) with by_dim_class /
// by_mask and launches it on the grid p states; which of them run, in what order and on what
// grid is fa_bwd.hip's business.
// --------------------------------------------------------------------------
// fa_bwd_simt_dq.hip, fa_bwd_simt_dkdv.hip: one SIMT pass each;
// (T, A) = (bf16 | f16 | float, float), (double, double)
template <class T, class A = float>
hipError_t launch_generic_dq(const BwdParams& p, DenseMask mask, hipStream_t s);
template <class T, class A = float>
hipError_t launch_generic_dkdv(const BwdParams& p, DenseMask mask, hipStream_t s);
// fa_bwd_f32.hip: both fp32 MFMA passes
hipError_t launch_f32_mfma(const BwdParams& p, DenseMask mask, hipStream_t s);
// fa_bwd_dq.hip, fa_bwd_dkdv.hip: one pass of p.total_wg 128-row blocks; T = bf16 | f16
template <class T>
hipError_t launch_dq_fast(const BwdParams& p, DenseMask mask, hipStream_t s);
template <class T>
hipError_t launch_dkdv_fast(const BwdParams& p, DenseMask mask, hipStream_t s);
// fa_bwd_fused.hip: the single pass on p.total_wg 256-key members (no mask); T = bf16 | f16
template <class T>
hipError_t launch_fused(const BwdParams& p, hipStream_t s);

}  // namespace fa
