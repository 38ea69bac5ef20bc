// fa_dense_plan.h — the HOST PLANS of the dense (and causal, and local) attention forward
// (fa_fwd.hip, fa_fwd_p4.hip) and backward (fa_bwd.hip): which kernel a call gets, on what
// grid, and where every region of its workspace lies.  dense_fwd_plan and dense_bwd_plan
// are pure functions of the shape, a snapshot of the debug knobs, the pointer-alignment
// facts, the workspace bytes and the CU count: no device query, no thread-local read.  The
// launchers ask once and switch on the answer, the workspace entry points return the same
// plan's total, fa_debug_dense_fwd_plan / fa_debug_dense_bwd_plan (api.cpp) return it for
// tests, and tests/test_dense_plan_host.py pins the choice.
//
// The mask is one DenseMask (fa_internal.h) from the entry points on: both plans take it, the
// forward plan hands it on (DenseFwdPlan::mask) and the launchers instantiate the plan's
// kernel with it as the kernel's MASK template argument (by_mask).
#pragma once

#include <algorithm>

#include "fa_internal.h"
#include "../../include/fa_hip.h"

namespace fa {

inline bool dense_16bit(int dtype) { return dtype == FA_DTYPE_BF16 || dtype == FA_DTYPE_F16; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ==========================================================================
// Forward
// ==========================================================================

// Values of fa_debug_set_fwd_variant (g_fwd_variant).  They apply to the fast (MFMA) kernels
// of dense launches only: causal launches and the generic kernels ignore them.
enum DenseFwdVariant : int {
    kFwdAuto = 0,      // per head-dim class: w8q2 at d, dv <= 64, w8b64 above; p4 at d = dv = 128
    kFwdW8B64 = 5,     // 8 waves x 1 query block (256 rows per workgroup), never split, never p4
    kFwdW8Q2 = 7,      // 8 waves x 2 query blocks (512 rows), never split, never p4
    kFwdNarrow = 20,   // the auto geometries with per-element Q gathers / O stores (no LDS staging)
    kFwdP4 = 30,       // the one-wave-per-SIMD persistent kernel wherever its shape rules allow
};

// A causal or local launch is the same enumerator with DenseFwdPlan::mask: the kernel named
// here, instantiated with MASK = kMaskCausal / kMaskLocal.
enum DenseFwdKernel : int {
    kDenseFwdNone = -1,        // a head dimension above kMaxHeadDim: the launcher refuses
    kDenseFwdGeneric = 0,      // dense_fwd_generic (SIMT, any shape and alignment)
    kDenseFwdGenericF32 = 1,   // dense_fwd_generic_f32
    kDenseFwdF64 = 2,          // fa_f64.hip
    kDenseFwdW8B64 = 3,        // dense_fwd_w8b64
    kDenseFwdW8B64Wide = 4,    // dense_fwd_w8b64_wide (Q / O staged through LDS)
    kDenseFwdW8Q2 = 5,         // dense_fwd_w8q2
    kDenseFwdW8Q2Wide = 6,     // dense_fwd_w8q2_wide
    kDenseFwdW8B64Split = 7,   // dense_fwd_w8b64_split, then fwd_split_combine
    kDenseFwdW8Q2Split = 8,    // dense_fwd_w8q2_split, then fwd_split_combine
    kDenseFwdP4 = 9,           // dense_fwd_p4 (fa_fwd_p4.hip) on a grid of one workgroup per CU
};

struct DenseFwdKnobs {
    int variant;        // a DenseFwdVariant
    int causal_order;   // fa_debug_set_causal_order: 0, 1, 2
};

struct DenseFwdPlan {
    DenseFwdKernel kernel = kDenseFwdNone;
    // FwdParams::causal: 0 dense; bit 0 causal, bit 1 a slab's heaviest query block first,
    // bit 2 block-major inside an XCD's share of the grid (dense_fwd_tiled)
    int causal = 0;
    DenseMask mask = kMaskNone;   // the kernel's MASK (causal bits only under kMaskCausal; a masked launch never splits, never p4)
    bool kv_vec = false;   // FwdParams::fast: K / V rows take 16-B loads (after padding, if any)
    bool wide = false;     // FwdParams::wide: N % 8 == 0, Q and O 16-B aligned
    bool pad = false;      // K / V are first copied to zero-padded slabs of row stride ldk
    int64_t ldk = 0;       // K / V row stride in elements
    int nsplit = 1, tps = 0;       // split-KV: key ranges, 64-key tiles per range
    int rows = 0;                  // query rows per workgroup (p4: per block)
    int64_t nqb = 0, total_wg = 0; // FwdParams::nqb, total_wg: row blocks per slab, blocks in all
    int64_t grid = 0;              // workgroups launched (p4: the CU count; else total_wg)
    int block = 0;                 // threads per workgroup
    // workspace, in bytes from its 256-B aligned base: the padded K and V slabs, the split-KV
    // partial O, l and m; total is what fa_dense_fwd_workspace / fa_causal_fwd_workspace
    // reserve for the shape (plus the slabs when misaligned K / V take them)
    size_t off_k = 0, off_v = 0, off_opart = 0, off_lpart = 0, off_mpart = 0, total = 0;
};

constexpr int kFwdKeyTile = 64;    // keys per tile (kBN)
constexpr int kFwdGenericRows = 128, kFwdGenericThreads = 256;   // dense_fwd_generic: kBM, kThreads
constexpr int kFwdP4Rows = 256, kFwdP4Threads = 256;             // dense_fwd_p4: kP4Rows
// The split-KV rule aims at this many workgroups for grids below kFwdSplitBelow (an
// MI355X's CU count: the workspace query cannot ask the device).
constexpr int64_t kFwdSplitBelow = 256, kFwdSplitTarget = 512;

// Split-KV by shape: grids of fewer than kFwdSplitBelow workgroups split the key range so
// that about kFwdSplitTarget run, each on at least 2 key tiles.  nsplit 1: no split.
struct DenseFwdSplit {
    int nsplit = 1, tps = 0;
};
inline DenseFwdSplit dense_fwd_split(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    DenseFwdSplit sp;
    const int Dc = head_dim_class(d), DVc = head_dim_class(dv);
    if (!dense_16bit(dtype) || !Dc || !DVc) return sp;
    const int64_t rows = (Dc <= 64 && DVc <= 64) ? 512 : 256;
    const int64_t wgs = ceil_div(N, rows) * batch;
    const int64_t NT = ceil_div(Nk, kFwdKeyTile);
    if (wgs >= kFwdSplitBelow || NT < 4) return sp;
    int64_t ns = std::min<int64_t>(ceil_div(kFwdSplitTarget, wgs), NT / 2);
    if (ns < 2) return sp;
    const int64_t tps = ceil_div(NT, ns);
    ns = ceil_div(NT, tps);
    if (ns < 2 || ns * wgs > INT32_MAX) return sp;
    sp.nsplit = (int)ns;
    sp.tps = (int)tps;
    return sp;
}

// kv_aligned16: K and V are 16-B aligned; qo_aligned16: Q and O are.  ws_bytes: the
// caller's workspace (0: none).  cus: the device's CU count (0: unknown; only p4 asks).
//
// Padded K / V: bf16 / fp16 K and V whose rows the fast kernels cannot load 16 B at a time
// (Nk % 8 != 0, or a misaligned pointer) are copied into zero-padded slabs of row stride
// roundup(Nk, 8) when the workspace holds them; the kernels mask keys >= Nk as for any
// ragged last tile.  The workspace query reserves the slabs only when the SHAPE needs them
// (it has no pointers); without room for them those calls run the generic kernel.
inline DenseFwdPlan dense_fwd_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                                   DenseMask mask, DenseFwdKnobs kn, bool kv_aligned16, bool qo_aligned16,
                                   size_t ws_bytes, int cus) {
    DenseFwdPlan pl;
    const bool causal = mask == kMaskCausal;
    pl.mask = mask;
    if (dtype == FA_DTYPE_F64) {
        pl.kernel = kDenseFwdF64;
        return pl;
    }
    const bool f32 = dtype == FA_DTYPE_F32;
    const int Dc = head_dim_class(d), DVc = head_dim_class(dv);
    const int64_t nk8 = ceil_div(Nk, 8) * 8;
    const bool pad_fits = dense_16bit(dtype) && nk8 * d * 2 < INT32_MAX && nk8 * dv * 2 < INT32_MAX &&
                          nk8 * (d > dv ? d : dv) * batch < ((int64_t)1 << 40);
    const size_t kbytes = al256((size_t)(nk8 * d * batch) * 2), vbytes = al256((size_t)(nk8 * dv * batch) * 2);
    const size_t pad_bytes = kbytes + vbytes + 256;
    const DenseFwdSplit shape_split = mask != kMaskNone ? DenseFwdSplit{} : dense_fwd_split(dtype, N, Nk, d, dv, batch);
    const size_t obytes = al256((size_t)(shape_split.nsplit * batch * N * dv) * 4);
    const size_t lmbytes = al256((size_t)(shape_split.nsplit * batch * N) * 4);
    const size_t split_bytes = obytes + 2 * lmbytes + 256;

    // what the kernels can load
    bool fast = Nk % (f32 ? 4 : 8) == 0 && kv_aligned16;
    pl.wide = N % 8 == 0 && qo_aligned16;
    pl.ldk = Nk;
    if (!fast && pad_fits && N * d * 2 < (int64_t)INT32_MAX && ws_bytes >= pad_bytes) {
        pl.pad = true;
        pl.ldk = nk8;
        fast = true;
    }
    // buffer descriptors address a slab with 32-bit byte offsets
    const int64_t esz = f32 ? 4 : 2;
    if (N * d * esz >= (int64_t)INT32_MAX || pl.ldk * d * esz >= (int64_t)INT32_MAX ||
        pl.ldk * dv * esz >= (int64_t)INT32_MAX)
        fast = false;
    pl.kv_vec = fast;
    pl.causal = causal ? (kn.causal_order ? 3 : 1) : 0;

    // the layout: [K slab | V slab] (256 B of slack for the base's alignment), then
    // [opart | lpart | mpart] (and their slack)
    const bool slabs = pl.pad || (Nk % 8 != 0 && pad_fits);
    pl.off_k = 0;
    pl.off_v = kbytes;
    pl.off_opart = slabs ? kbytes + vbytes : 0;
    pl.off_lpart = pl.off_opart + obytes;
    pl.off_mpart = pl.off_lpart + lmbytes;
    pl.total = (slabs ? pad_bytes : 0) + (shape_split.nsplit > 1 ? split_bytes : 0);

    // the generic kernels' grid, which every kernel below replaces
    pl.rows = kFwdGenericRows;
    pl.nqb = ceil_div(N, pl.rows);
    pl.grid = pl.total_wg = pl.nqb * batch;
    pl.block = kFwdGenericThreads;
    if (f32) {
        pl.kernel = kDenseFwdGenericF32;
        return pl;
    }
    if (!Dc || !DVc) return pl;
    pl.kernel = kDenseFwdGeneric;
    if (!fast) return pl;

    // geometry per head-dim class (measured on MI355X):
    // <= 64: 8 waves x 2 query blocks (512 rows / workgroup); 128: 8 waves x 1
    const bool q2_class = Dc <= 64 && DVc <= 64;
    pl.block = 512;
    if (mask != kMaskNone) {   // the class's default geometry: no variant, no split, no p4
        pl.rows = q2_class ? 512 : 256;
        pl.nqb = ceil_div(N, pl.rows);
        pl.grid = pl.total_wg = pl.nqb * batch;
        // order 2 needs every XCD's share of the grid to hold whole slabs
        // (local launches keep the default order: a bounded band makes the blocks near-uniform)
        if (causal && kn.causal_order == 2 && pl.total_wg % 8 == 0 && (pl.total_wg / 8) % pl.nqb == 0) pl.causal = 1 | 4;
        pl.kernel = q2_class ? (pl.wide ? kDenseFwdW8Q2Wide : kDenseFwdW8Q2) : (pl.wide ? kDenseFwdW8B64Wide : kDenseFwdW8B64);
        return pl;
    }
    const int v = kn.variant;
    // One wave per SIMD, persistent (fa_fwd_p4.hip): the default at d = dv = 128 (5-8 % over
    // the 8-wave kernel, bitwise equal: profiles/r04_fwd_p4_default_d128_ab.log); at 64 the
    // 8-wave kernel stays (p4 is 15 % slower there).  It runs when its 256-row blocks fill the
    // chip and the shape is its own: Q / O staged, d = dv equal to their class (64 or 128),
    // whole key tiles, enough of them for the Q prefetch (phases B(0 .. d/8 - 1) of the
    // previous block; whole tiles also mean ldk = Nk).  Where it is asked for and its blocks
    // fill the chip the keys are never split, even if p4 then refuses the shape.
    const int64_t p4_blocks = ceil_div(N, kFwdP4Rows) * batch;
    const bool p4_asked = v == kFwdP4 || (v == kFwdAuto && Dc == 128 && DVc == 128);
    const bool p4_fills = p4_asked && p4_blocks >= cus;
    if (p4_fills && cus > 0 && pl.wide && Dc == DVc && Dc >= 64 && d == Dc && dv == DVc && Nk % kFwdKeyTile == 0 &&
        Nk / kFwdKeyTile >= Dc / 8 + 1 && p4_blocks <= INT32_MAX / 2) {
        pl.kernel = kDenseFwdP4;
        pl.rows = kFwdP4Rows;
        pl.nqb = ceil_div(N, kFwdP4Rows);
        pl.total_wg = p4_blocks;
        pl.grid = cus;
        pl.block = kFwdP4Threads;
        return pl;
    }
    // split-KV for small grids: the auto geometries only, and only with room for the partials
    if ((v == kFwdAuto || v == kFwdP4) && !p4_fills && shape_split.nsplit > 1 &&
        ws_bytes >= (pl.pad ? pad_bytes : 0) + split_bytes) {
        pl.nsplit = shape_split.nsplit;
        pl.tps = shape_split.tps;
    }
    const bool q2 = v == kFwdW8Q2 || (v != kFwdW8B64 && q2_class);
    // kFwdNarrow: the same geometries with per-element Q gathers / O stores, for A/B
    const bool wide = pl.wide && v != kFwdNarrow;
    pl.rows = q2 ? 512 : 256;
    pl.nqb = ceil_div(N, pl.rows);
    pl.grid = pl.total_wg = pl.nqb * batch * pl.nsplit;
    if (pl.nsplit > 1) pl.kernel = q2 ? kDenseFwdW8Q2Split : kDenseFwdW8B64Split;
    else if (q2) pl.kernel = wide ? kDenseFwdW8Q2Wide : kDenseFwdW8Q2;
    else pl.kernel = wide ? kDenseFwdW8B64Wide : kDenseFwdW8B64;
    return pl;
}

// ==========================================================================
// Backward
// ==========================================================================

// Values of fa_debug_set_bwd_mode (g_bwd_mode).  Everything from kBwdSinglePass up runs the
// single pass wherever its shape conditions hold; kBwdAbl* (builds with -DFA_BWD_ABL only)
// are its timing-only ablations, which compute a WRONG dQ.
enum DenseBwdMode : int {
    kBwdAuto = 0,             // the single pass where it also fills the chip evenly
    kBwdTwoPass = 1,          // always the dK/dV + dQ passes
    kBwdSinglePass = 2,
    kBwdSinglePassGiveUp = 3, // the hand-off's timeout word preset: exercises the dQ fallback pass
    kBwdAblNoWaits = 4,
    kBwdAblNoSums = 5,        // no running-sum traffic
    kBwdAblNoWaitsNoSums = 6,
    kBwdAblNoSumLoads = 7,
    kBwdAblNoSumStores = 8,
    kBwdAblNoDsWrites = 9,    // no dS image writes
    kBwdAblNoNextDma = 10,    // no next-slice Q / dO DMA
    kBwdAblNoNextDmaNoWaitsNoSums = 11,
};
// BwdParams::ablate of a mode (0 below kBwdAblNoWaits)
inline int bwd_ablate_bits(int mode) {
    constexpr int bits[] = {1, 2, 3, 8, 16, 32, 64, 64 | 3};   // kBwdAblNoWaits .. kBwdAblNoNextDmaNoWaitsNoSums
    return mode >= kBwdAblNoWaits && mode <= kBwdAblNoNextDmaNoWaitsNoSums ? bits[mode - kBwdAblNoWaits] : 0;
}

enum DenseBwdKernel : int {
    kDenseBwdF64 = 0,         // double row statistics (fa_f64.hip), then the SIMT passes in double
    kDenseBwdGeneric = 1,     // bwd_generic_dq + bwd_generic_dkdv (SIMT, any shape and alignment)
    kDenseBwdF32Mfma = 2,     // bwd_dq_f32 + bwd_dkdv_f32
    kDenseBwdTwoPass = 3,     // bwd_dq_fast + bwd_dkdv_fast
    kDenseBwdSinglePass = 4,  // bwd_fused, then bwd_dq_fast guarded by the hand-off's timeout word
};

struct DenseBwdKnobs {
    int force_generic;   // fa_debug_set_bwd_generic
    int mode;            // a DenseBwdMode
    int hoff;            // fa_debug_set_bwd_hoff: step offset between consecutive members
    int xcd;             // fa_debug_set_bwd_xcd: -1 auto, 0 never one XCD per slab
};

// Single-pass hand-off words in the workspace (zeroed per call), in 32-bit words from
// BwdParams::flags, for `batch` slabs of NS slices and KM members:
struct FusedFlags {
    int64_t cnt;    // [2 chains][batch][NS]: members of the chain that have published slice t
    int64_t fin;    // [batch][NS]: tails of a wrapped slice's two chains that stored their sums
    int64_t serr;   // [batch]: the slab gave up (its dQ is recomputed by bwd_dq_fast)
    int64_t xcc;    // [batch][KM]: XCD of each member + 1 (L2-local hand-off)
    int64_t prog;   // [batch][KM]: each member's count of publishes (plain stores, no contention)
    int64_t garr;   // the launch's arrival count (one add per workgroup)
    int64_t words;  // (a wrapped slice left to bwd_dq_fast's combine is flagged in hdr[3])
};
__host__ __device__ inline FusedFlags fused_flags(int64_t batch, int64_t NS, int64_t KM) {
    FusedFlags f;
    f.cnt = 0;
    f.fin = 2 * batch * NS;
    f.serr = 3 * batch * NS;
    f.xcc = f.serr + batch;
    f.prog = f.xcc + batch * KM;
    f.garr = f.prog + batch * KM;
    f.words = f.garr + 1;
    return f;
}

// the ten padded slabs, in workspace order
enum BwdSlab : int { kSlabQ, kSlabDQ, kSlabK, kSlabDK, kSlabV, kSlabDV, kSlabO, kSlabDO, kSlabL, kSlabM, kBwdSlabs };

constexpr size_t kBwdHdrBytes = 256;   // the workspace header (fa_dense_bwd_handoff_status), at the aligned base

struct DenseBwdPlan {
    DenseBwdKernel kernel = kDenseBwdGeneric;
    // the extents the kernels run on: the caller's, or with `padded` N, Nk rounded up to 8 and
    // d, dv to their class, on zero-padded copies in the workspace slabs
    bool padded = false;
    int64_t N = 0, Nk = 0, d = 0, dv = 0;
    bool slabs_fit = true;        // padded: the workspace holds the slabs (else FA_ERR_WORKSPACE)
    int nkb = 0, nqt = 0, xcd = 0;   // single pass: members (256-key blocks) per slab, 64-query slices, one XCD per slab
    // workspace, in bytes from its 256-B aligned base: header | nD | nlse | ten padded slabs |
    // hand-off words (flag_bytes of them) | the two chains' running dQ sums.  total is what
    // fa_dense_bwd_workspace / fa_causal_bwd_workspace return: it keeps the slabs of a shape
    // that pads even when force_generic leaves them unused.
    size_t off_hdr = 0, off_nD = 0, off_nlse = 0, off_slab[kBwdSlabs] = {}, off_flags = 0, off_part = 0;
    size_t flag_bytes = 0, total = 0;
};

// The MFMA kernels' own shapes: bf16 / fp16, d and dv exactly a class, N and Nk multiples of 8,
// slabs within 32-bit byte offsets.
inline bool bwd_cls_dim(int64_t x) { return x == 32 || x == 64 || x == 128; }
inline bool bwd_shape_fast(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv) {
    return dense_16bit(dtype) && bwd_cls_dim(d) && bwd_cls_dim(dv) && N % 8 == 0 && Nk % 8 == 0 &&
           N * d * 2 < INT32_MAX && Nk * d * 2 < INT32_MAX && N * dv * 2 < INT32_MAX && Nk * dv * 2 < INT32_MAX;
}

// qkvdo_aligned16: Q, K, V and dO are 16-B aligned.  ws_bytes: what the caller's workspace
// holds from its 256-B aligned base on.  cus: the device's CU count (0: unknown, never the
// single pass).
//
// Padded fast path: 16-bit shapes the MFMA kernels do not take directly (N or Nk not a
// multiple of 8, d or dv not 32 / 64 / 128) are copied into zero-padded workspace slabs and
// run on the fast kernels.  The zero keys past the caller's Nk are masked where a dQ is summed
// (BwdParams::nkv: P = 0; left to P·0 they break once exp(0 − lse) overflows, which fp16's dS
// does from lse < −11 on), and their own dK / dV rows are dropped; zero features add 0 to every
// product; padded queries carry dO = O = 0 (so dS = 0) and l = 1, m = 0 (finite P, no NaN).  A fast shape with a misaligned
// tensor is NOT padded: it runs the generic kernels.
//
// Single pass (bwd_fused) on the extents the fast kernels run: K = ceil(Nk/256) members per
// slab, T = ceil(N/64) slices, step offset hoff (needs hoff·K <= T); K <= CUs, one XCD per
// slab when K <= CUs/8 and the slab count is a multiple of 8 (a slab's members then run
// together: speed, not correctness, which needs no co-residency); in kBwdAuto only when the
// grid fills the chip and K divides the CUs a slab's members are dealt over (one XCD's, or
// the chip's), so no slab waits part-resident behind another.  Never for causal or local
// launches (no atomics, no hand-off there).  A workspace too small for its part gets the two passes.
inline DenseBwdPlan dense_bwd_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                                   DenseMask mask, DenseBwdKnobs kn, bool qkvdo_aligned16, size_t ws_bytes, int cus) {
    DenseBwdPlan pl;
    pl.N = N; pl.Nk = Nk; pl.d = d; pl.dv = dv;
    pl.off_hdr = 0;
    pl.off_nD = kBwdHdrBytes;
    if (dtype == FA_DTYPE_F64) {   // nD, nlse in double
        pl.kernel = kDenseBwdF64;
        pl.off_nlse = pl.off_nD + (size_t)(N * batch) * sizeof(double);
        pl.total = kBwdHdrBytes + (size_t)(2 * N * batch * sizeof(double) + 256);
        return pl;
    }
    const bool shape_fast = bwd_shape_fast(dtype, N, Nk, d, dv);
    const int64_t Np = ceil_div(N, 8) * 8, Nkp = ceil_div(Nk, 8) * 8;
    const int64_t Dp = head_dim_class(d), DVp = head_dim_class(dv);
    // the shape pads (whatever the knobs say: the workspace keeps its slabs)
    const bool pads = dense_16bit(dtype) && d <= kMaxHeadDim && dv <= kMaxHeadDim && !shape_fast &&
                      bwd_shape_fast(dtype, Np, Nkp, Dp, DVp) && Np * batch <= INT32_MAX / 2 &&
                      Nkp * batch <= INT32_MAX / 2;
    const bool fast = !kn.force_generic && shape_fast && qkvdo_aligned16;
    pl.padded = pads && !kn.force_generic;
    if (pl.padded) { pl.N = Np; pl.Nk = Nkp; pl.d = Dp; pl.dv = DVp; }

    // the layout
    const int64_t rows = pads ? Np : N;   // rows the row statistics are sized for
    pl.off_nlse = pl.off_nD + (size_t)(pl.N * batch) * sizeof(float);
    size_t end = kBwdHdrBytes + al256((size_t)(2 * pl.N * batch) * sizeof(float));
    pl.total = kBwdHdrBytes + (size_t)(2 * rows * batch * sizeof(float) + 256);
    if (pads) {
        const size_t q = al256((size_t)(Np * Dp * batch) * 2), k = al256((size_t)(Nkp * Dp * batch) * 2);
        const size_t v = al256((size_t)(Nkp * DVp * batch) * 2), o = al256((size_t)(Np * DVp * batch) * 2);
        const size_t lm = al256((size_t)(Np * batch) * 4);
        const size_t bytes[kBwdSlabs] = {q, q, k, k, v, v, o, o, lm, lm};
        pl.total += 2 * q + 2 * k + 2 * v + 2 * o + 2 * lm + 256;
        if (pl.padded) {
            for (int i = 0; i < kBwdSlabs; ++i) {
                pl.off_slab[i] = end;
                end += bytes[i];
            }
            pl.slabs_fit = end <= ws_bytes;
        }
    }
    pl.off_flags = pl.off_part = end;

    // the kernel
    if (dtype == FA_DTYPE_F32) {   // fp32 MFMA kernels (exact fp32 products)
        pl.kernel = !kn.force_generic && N * batch < INT32_MAX / 2 && Nk * batch < INT32_MAX / 2 ? kDenseBwdF32Mfma
                                                                                                   : kDenseBwdGeneric;
        return pl;
    }
    if (!fast && !pl.padded) return pl;   // kDenseBwdGeneric
    pl.kernel = kDenseBwdTwoPass;
    const int64_t K = ceil_div(pl.Nk, 256), T = ceil_div(pl.N, 64);
    if (mask != kMaskNone || kn.mode == kBwdTwoPass || cus < 8 || kn.hoff * K > T || K > cus || batch * K > INT32_MAX / 2 ||
        2 * T * (pl.d / 16) * 4096 >= INT32_MAX || T >= (1 << 20))   // a slice index fits the 20 bits bwd_fused packs it in
        return pl;
    const int xcd = (K <= cus / 8 && batch % 8 == 0 && kn.xcd != 0) ? 1 : 0;
    if (kn.mode == kBwdAuto && (batch * K < cus || (xcd ? cus / 8 : cus) % K != 0)) return pl;
    const size_t flag_bytes = al256((size_t)fused_flags(batch, T, K).words * 4);
    const size_t part_bytes = flag_bytes + al256((size_t)(2 * batch * T * (pl.d / 16)) * 4096) + 256;
    if (end + part_bytes > ws_bytes) return pl;
    pl.kernel = kDenseBwdSinglePass;
    pl.nkb = (int)K; pl.nqt = (int)T; pl.xcd = xcd;
    pl.flag_bytes = flag_bytes;
    pl.off_part = end + flag_bytes;
    pl.total += part_bytes;
    return pl;
}

}  // namespace fa
