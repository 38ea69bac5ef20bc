// fa_circulant_plan.h — the HOST PLANS of circulant attention, forward (fa_circulant.hip) and
// backward (fa_circulant_bwd.hip): which kernel a call gets, on what grid, with how much
// dynamic LDS, and where the backward's two workspace regions lie.  circ_fwd_plan and
// circ_bwd_plan are pure functions of the shape, a snapshot of the debug knob
// (fa_debug_set_circ_generic) and the pointer-alignment facts: no device query, no
// thread-local read.  The launchers ask once and switch on the answer, the workspace query
// returns the backward plan's total, fa_debug_circ_fwd_plan / fa_debug_circ_bwd_plan (api.cpp)
// return the plans for tests, and tests/test_circulant_plan_host.py pins the choice.
#pragma once

#include "fa_internal.h"
#include "../../include/fa_hip.h"

namespace fa {

// Values of fa_debug_set_circ_generic.  Either forced value also keeps
// both directions off the MFMA kernels.
enum CircKnob : int {
    kCircAuto = 0,
    kCircWave = 1,   // forward: one wave per query
    kCircSimt = 2,   // forward: the LDS-tiled SIMT kernel
};

inline bool circ_16bit(int dtype) { return dtype == FA_DTYPE_BF16 || dtype == FA_DTYPE_F16; }
inline int64_t circ_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// What both directions refuse before anything else, head dimensions first: FA_OK, or the
// status with its message in *why.
inline int circ_refusal(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W, const char** why) {
    if (!head_dim_class(d) || !head_dim_class(dv)) {
        *why = "head dimension exceeds the compiled maximum (128)";
        return FA_ERR_UNSUPPORTED;
    }
    const int64_t esz = (int64_t)dtype_size(dtype);
    if (N * d * esz >= (int64_t)INT32_MAX || N * dv * esz >= (int64_t)INT32_MAX || W > INT32_MAX / 2 ||
        N * batch > (int64_t)INT32_MAX * 2) {
        *why = "per-slab extent or band width exceeds the 32-bit addressing of the kernels";
        return FA_ERR_UNSUPPORTED;
    }
    return FA_OK;
}

// The MFMA kernels of either direction take 16-bit slabs of whole 8-token chunks, 128 tokens
// per workgroup, under the auto knob (and 16-B aligned tensors: each plan names its own).
inline bool circ_mfma_shape(int dtype, int64_t N, int64_t batch, int knob) {
    return circ_16bit(dtype) && N % 8 == 0 && circ_ceil_div(N, 128) * batch <= INT32_MAX && knob == kCircAuto;
}

// ==========================================================================
// Forward
// ==========================================================================

// The codes of fa_debug_last_circ_fwd_kernel.
enum CircFwdKernel : int {
    kCircFwdNone = -1,    // refused: status, why
    kCircFwdTiled = 1,    // circ_fwd_tiled<T, Dc, DVc> (MFMA), 128 queries per workgroup
    kCircFwdWave = 2,     // circ_fwd_generic<T>, one wave per query
    kCircFwdSimt = 3,     // circ_fwd_simt<T, simt_class, simt_class, KT>, 256 queries per workgroup
    kCircFwdF64 = 4,      // circ_fwd_f64, one wave per query
};

constexpr int kCircFwdTiledRows = 128, kCircFwdSimtRows = 256, kCircFwdThreads = 256;
// Grids below this many SIMT workgroups keep one wave per query: more parallelism there
// (N 4096, d 32, one slab, W 129 fp32: 72 vs 137 us).
constexpr int64_t kCircFwdSimtFrom = 128;
// keys per LDS tile of the SIMT kernel at a (square) head-dim class
constexpr int circ_simt_kt(int cls) { return cls == 128 ? 8 : 32; }

struct CircFwdPlan {
    CircFwdKernel kernel = kCircFwdNone;
    int status = FA_OK;      // of a refusal, with its message
    const char* why = "";
    int Dc = 0, DVc = 0;                // tiled: the head-dim classes of d, dv
    int simt_class = 0, simt_kt = 0;    // SIMT: the larger of the two classes, for both D and DV, and its KT
    // CircParams::nqb (tiled: 128-query blocks per slab), CircParams::total_wg (tiled: nqb·batch;
    // wave: the slab count; SIMT: ceil(N/256)·batch), workgroups launched, threads of each
    int64_t nqb = 0, total_wg = 0, grid = 0;
    int block = kCircFwdThreads;
};

// kv_aligned16: K and V are 16-B aligned.
inline CircFwdPlan circ_fwd_plan(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W, int knob,
                                 bool kv_aligned16) {
    CircFwdPlan pl;
    pl.status = circ_refusal(dtype, N, d, dv, batch, W, &pl.why);
    if (pl.status != FA_OK) return pl;
    const int Dc = head_dim_class(d), DVc = head_dim_class(dv);
    const int64_t waves = N * batch;   // one wave per query, 4 to a workgroup
    if (dtype == FA_DTYPE_F64) {
        pl.kernel = kCircFwdF64;
        pl.grid = circ_ceil_div(waves, 4);
        return pl;
    }
    if (circ_mfma_shape(dtype, N, batch, knob) && kv_aligned16) {
        pl.kernel = kCircFwdTiled;
        pl.Dc = Dc;
        pl.DVc = DVc;
        pl.nqb = circ_ceil_div(N, kCircFwdTiledRows);
        pl.grid = pl.total_wg = pl.nqb * batch;
        return pl;
    }
    const int64_t simt_wg = circ_ceil_div(N, kCircFwdSimtRows) * batch;
    if (knob == kCircWave || (knob != kCircSimt && simt_wg < kCircFwdSimtFrom)) {
        pl.kernel = kCircFwdWave;
        pl.total_wg = batch;
        pl.grid = circ_ceil_div(waves, 4);
        return pl;
    }
    pl.kernel = kCircFwdSimt;
    pl.simt_class = Dc > DVc ? Dc : DVc;
    pl.simt_kt = circ_simt_kt(pl.simt_class);
    pl.grid = pl.total_wg = simt_wg;
    return pl;
}

// ==========================================================================
// Backward
// ==========================================================================

// The codes of fa_debug_last_circ_bwd_kernel.
enum CircBwdFamily : int {
    kCircBwdNone = -1,   // refused: status, why
    kCircBwdMfma = 1,    // circ_bwd_dq_tiled + circ_bwd_dkdv_tiled <T, Dc, DVc>
    kCircBwdSimt = 2,    // circ_bwd_dq_simt + circ_bwd_dkdv_simt <T, float>
    kCircBwdF64 = 3,     // the SIMT kernels in double, row statistics recomputed by the pre-pass
};

constexpr int kCircBwdTiledRows = 128, kCircBwdSimtTile = 32, kCircBwdThreads = 256;
constexpr int64_t kCircBwdW1MaxGrid = 1 << 20;   // circ_bwd_w1 strides over the rest

struct CircBwdPlan {
    CircBwdFamily family = kCircBwdNone;
    int status = FA_OK;      // of a refusal, with its message
    const char* why = "";
    // W == 1: circ_bwd_w1 alone on w1_grid workgroups, no pre-pass; family kCircBwdSimt
    // (kCircBwdF64 for Float64) whatever the shape
    bool w1 = false;
    int64_t w1_grid = 0;
    bool prepass_vec = false;   // circ_bwd_prepass_v (8 queries per thread) instead of circ_bwd_prepass
    int64_t prepass_grid = 0;
    int Dc = 0, DVc = 0;                 // MFMA: the head-dim classes of d, dv
    int64_t nblk = 0, total_wg = 0;      // MFMA: CircBwdParams::nblk, total_wg (128-token blocks per slab, in all)
    int64_t grid = 0;                    // workgroups of the dQ and of the dK / dV launch
    size_t lds_dq = 0, lds_dkdv = 0;     // SIMT, Float64: dynamic LDS of the two kernels, bytes
    // workspace, in bytes from its 256-B aligned base: nD | nlse, [batch][N] floats (doubles for
    // Float64); total is what fa_circulant_bwd_workspace returns (256 B of slack for the base)
    size_t off_nD = 0, off_nlse = 0, total = 0;
};

// qkv_aligned16: Q, K and V are 16-B aligned; o_aligned16, do_aligned16: O, dO.
inline CircBwdPlan circ_bwd_plan(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W, int knob,
                                 bool qkv_aligned16, bool o_aligned16, bool do_aligned16) {
    CircBwdPlan pl;
    // the layout first: the workspace query answers for a shape the launcher refuses, too
    const bool f64 = dtype == FA_DTYPE_F64;
    const size_t asz = f64 ? sizeof(double) : sizeof(float);
    const size_t part = al256((size_t)N * (size_t)batch * asz);
    pl.off_nD = 0;
    pl.off_nlse = part;
    pl.total = 256 + 2 * part;
    pl.status = circ_refusal(dtype, N, d, dv, batch, W, &pl.why);
    if (pl.status != FA_OK) return pl;

    const int64_t total = N * batch;
    if (W == 1) {
        const int64_t elems = total * (d > dv ? d : dv);
        const int64_t blocks = circ_ceil_div(elems, 256);
        pl.family = f64 ? kCircBwdF64 : kCircBwdSimt;
        pl.w1 = true;
        pl.w1_grid = blocks < kCircBwdW1MaxGrid ? blocks : kCircBwdW1MaxGrid;
        return pl;
    }
    pl.prepass_vec = circ_16bit(dtype) && N % 8 == 0 && o_aligned16 && do_aligned16;
    pl.prepass_grid = circ_ceil_div(pl.prepass_vec ? total / 8 : total, 256);
    if (circ_mfma_shape(dtype, N, batch, knob) && qkv_aligned16 && do_aligned16) {
        pl.family = kCircBwdMfma;
        pl.Dc = head_dim_class(d);
        pl.DVc = head_dim_class(dv);
        pl.nblk = circ_ceil_div(N, kCircBwdTiledRows);
        pl.grid = pl.total_wg = pl.nblk * batch;
        return pl;
    }
    // 32 x 32 tiles: Q, dO, K, V rows of d + 1 / dv + 1 elements, then dS (dQ) or P, dS and the
    // 64 row constants (dK / dV), each [32][33]: above 64 KiB at d = dv = 128
    constexpr size_t T = kCircBwdSimtTile;
    const size_t rows = T * (2 * (size_t)(d + 1) + 2 * (size_t)(dv + 1));
    pl.family = f64 ? kCircBwdF64 : kCircBwdSimt;
    pl.grid = circ_ceil_div(N, kCircBwdSimtTile) * batch;
    pl.lds_dq = asz * (rows + T * (T + 1));
    pl.lds_dkdv = asz * (rows + 2 * T * (T + 1) + 2 * T);
    return pl;
}

}  // namespace fa
