// fa_fwd_params.h — launch parameters of the dense forward kernels
// (fa_fwd.hip: generic / tiled / split-KV kernels).  The struct is pinned at 136 bytes with
// no padding left, so the local (sliding-window) launches carry their clamped window in the
// two split-KV ints, which they never use (anonymous unions below), rather than in a params
// type of their own.
#pragma once

#include <hip/hip_runtime.h>

namespace fa {

struct FwdParams {
    const void* Q;
    const void* K;
    const void* V;
    void* O;
    float* l;
    float* m;
    int N, Nk, d, dv;
    int ldk;   // K / V row stride in elements (= Nk, or Nk rounded up to 8 in padded workspace copies)
    int nqb, total_wg;
    // split-KV (small grids): nsplit key ranges of tps tiles each; partial results
    // (fp32, unnormalised, relative to the split's max) go to opart / lpart / mpart,
    // indexed by (split * batch + b)
    // Local (sliding-window) launches never split the keys, so their clamped window rides in
    // these two ints (the struct has no padding left for new fields): wleft / wright, each in
    // [0, Nk], Nk meaning no bound on that side (fa_local_fwd; read by the LOCAL
    // instantiations only, which never read nsplit / tps / the partial pointers).
    union { int nsplit; int wleft; };
    union { int tps; int wright; };
    int batch;
    // Varlen launches (fa_varlen_fwd) never split either: their two length arrays (device
    // pointers to `batch` int32, null = full) ride in the first two partial pointers, opart and
    // lpart, and are read through fwd_q_lens / fwd_k_lens by the kMaskVarlen instantiations only.
    // (A cast at the two accessors, not a union: a union member changes the split kernels' code.)
    float *opart, *lpart, *mpart;
    float scale, scale_log2;
    float rescale_log2;   // lazy-rescale threshold (log2 units): kRescaleLog2, or the debug knob
    int fast;  // K/V rows 16-B aligned and Nk a multiple of the chunk width
    int wide = 0;     // N % 8 == 0, Q and O 16-B aligned: Q / O staged through LDS (16-B accesses)
    // causal launches (0: dense): bit 0 set, query i sees keys j <= i + off with off = Nk - N
    // (N and Nk here are always the caller's extents: padded K / V copies change ldk only);
    // bit 1: a slab's query blocks run last (heaviest) first; bit 2: block-major inside an
    // XCD's share of the grid, heaviest first (dense_fwd_tiled).  One int, in the struct's tail
    // padding: sizeof(FwdParams) and every existing kernel's argument layout stay as they were.
    int causal = 0;
};
__host__ __device__ inline const int32_t* fwd_q_lens(const FwdParams& p) { return (const int32_t*)p.opart; }
__host__ __device__ inline const int32_t* fwd_k_lens(const FwdParams& p) { return (const int32_t*)p.lpart; }
static_assert(sizeof(FwdParams) == 136, "fwd_split_combine's second argument follows the struct: keep its size");

}  // namespace fa
