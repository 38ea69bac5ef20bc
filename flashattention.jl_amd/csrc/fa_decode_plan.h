// fa_decode_plan.h — the HOST PLAN of decode attention (fa_decode.hip): how many key ranges
// a call is split into, which instantiation runs, on what grid, and how large the workspace of
// partials is.  decode_plan is a pure function of the shape, the forced range count
// (fa_debug_set_decode_nsplit) and the K / V alignment fact: no device query, no thread-local
// read, nothing from the lengths or the window (they are device data; the kernel cuts each
// slab's own visible range into the plan's nsplit shares).  The launcher asks once, the
// workspace entry point returns the same plan's total, fa_debug_decode_plan (api.cpp) returns
// it for tests/test_decode_host.py.  decode_fp8_plan, below, is the same plan for the fp8 cache
// (fa_decode_fp8.hip, fa_debug_decode_fp8_plan, tests/test_decode_fp8_host.py).
#pragma once

#include <algorithm>

#include "fa_dense_plan.h"

namespace fa {

struct DecodeArgs {
    int dtype;                 // FA_DTYPE_BF16 or FA_DTYPE_F16
    const void *Q, *K, *V;
    void* O;
    float *l, *m;
    int64_t N, Nk, d, dv, batch, group;   // batch: KV slabs; Q, O, l, m have batch * group slabs
    const int32_t *q_lens, *k_lens;       // device, `batch` values each, or nullptr (full)
    int64_t left, right;
    float scale;               // already resolved (> 0)
    void* workspace;
    size_t workspace_bytes;
};

constexpr int kDecodeRows = 32;       // rows of the one MFMA row tile: N * group <= 32
constexpr int kDecodeKeyTile = 64;    // keys per tile
constexpr int kDecodeThreads = 256;   // 4 waves, each on alternate key tiles of the workgroup's range

enum DecodeKernel : int {
    kDecodeNone = -1,     // refused (dtype, head dims, rows)
    kDecodeVec = 0,       // decode_fwd<.., VEC = true>: 16-B K DMA into LDS, 16-B V loads
    kDecodeNarrow = 1,    // decode_fwd<.., VEC = false>: 2-byte loads (Nk % 8 != 0 or misaligned K / V); no copies
    kPagedTile = 2,       // decode_paged_fwd<.., TILE = true>: page_size % 64 == 0, a key tile lies in one page
    kPagedChunk = 3,      // decode_paged_fwd<.., TILE = false>: page_size % 8 == 0, each 8-key chunk lies in one page
    kPaged8Tile = 4,      // decode_paged8_fwd<.., TILE = true>: fp8 pages, page_size % 64 == 0
    kPaged8Chunk = 5,     // decode_paged8_fwd<.., TILE = false>: fp8 pages, page_size % 16 == 0, each 16-key chunk lies in one page
};

struct DecodePlan {
    DecodeKernel kernel = kDecodeNone;
    int nsplit = 1;          // key ranges per KV slab (1: the workgroup stores O, l, m itself)
    int64_t grid = 0;        // workgroups of decode_fwd: batch * nsplit
    int64_t combine_grid = 0;   // workgroups of decode_combine (0 when nsplit == 1)
    size_t total = 0;        // workspace bytes: [nsplit][batch * group][N][dv + 2] floats + 256 (0 when nsplit == 1)
};

// Split by shape, as dense_fwd_split: fewer than kFwdSplitBelow slabs split the keys so that
// about kFwdSplitTarget workgroups run, each range at least 2 key tiles.  force: 0 auto, n > 0
// that many ranges, clamped to the shape's tile count.
inline int decode_nsplit(int64_t Nk, int64_t batch, int force) {
    const int64_t NT = ceil_div(Nk, kDecodeKeyTile);
    if (force > 0) return (int)std::max<int64_t>(1, std::min<int64_t>(force, NT));
    if (batch >= kFwdSplitBelow || NT < 4) return 1;
    int64_t ns = std::min<int64_t>(ceil_div(kFwdSplitTarget, batch), NT / 2);
    if (ns < 2) return 1;
    ns = ceil_div(NT, ceil_div(NT, ns));
    return ns < 2 ? 1 : (int)ns;
}

inline DecodePlan decode_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, int64_t group,
                              int force_nsplit, bool kv_aligned16) {
    DecodePlan pl;
    if (!dense_16bit(dtype) || !head_dim_class(d) || !head_dim_class(dv) || N < 1 || group < 1 ||
        N * group > kDecodeRows || Nk < N || batch < 1)
        return pl;
    pl.kernel = Nk % 8 == 0 && kv_aligned16 ? kDecodeVec : kDecodeNarrow;
    pl.nsplit = decode_nsplit(Nk, batch, force_nsplit);
    pl.grid = batch * pl.nsplit;
    if (pl.nsplit > 1) {
        pl.combine_grid = ceil_div(batch * group * N * dv, kDecodeThreads);
        pl.total = (size_t)(pl.nsplit * batch * group * N * (dv + 2)) * sizeof(float) + 256;
    }
    return pl;
}

int launch_decode_fwd(const DecodeArgs& a, hipStream_t s, const char** why);

// The fp8 cache (fa_decode_fp8.hip, fa_decode_fp8_fwd): K and V are e4m3fn bytes, so a 16-B chunk
// is 16 keys and the wide loads need Nk % 16 == 0.  Everything else is decode_plan's: the
// same decode_nsplit, grid and workspace of fp32 partials (dtype is the type of Q and O).
// kernel: kDecodeVec is decode8_fwd<.., VEC = true>, kDecodeNarrow its single-byte loads.
inline DecodePlan decode_fp8_plan(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, int64_t group,
                                  int force_nsplit, bool kv_aligned16) {
    DecodePlan pl = decode_plan(dtype, N, Nk, d, dv, batch, group, force_nsplit, kv_aligned16);
    if (pl.kernel != kDecodeNone) pl.kernel = Nk % 16 == 0 && kv_aligned16 ? kDecodeVec : kDecodeNarrow;
    return pl;
}

struct DecodeFp8Args {
    DecodeArgs a;                      // K, V: e4m3fn bytes; dtype: the type of Q and O
    const float *k_scale, *v_scale;    // device, `batch` floats each, or nullptr (1.0)
};

int launch_decode_fp8_fwd(const DecodeFp8Args& a, hipStream_t s, const char** why);

// The paged cache (fa_decode_paged.hip, fa_decode_paged_fwd): K and V are pools of pages of
// page_size keys and a (max_pages, batch) table names each slab's pages.  The logical capacity
// cap = max_pages * page_size is decode_plan's Nk for nsplit, grids and workspace; the kernel is
// chosen by the page size alone (anything but a positive multiple of 8, or a cap past 32 bits,
// is refused).  fa_debug_decode_paged_plan, tests/test_decode_paged_host.py.
inline DecodePlan decode_paged_plan(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t group,
                                    int64_t page_size, int64_t max_pages, int force_nsplit) {
    DecodePlan pl;
    if (page_size < 8 || page_size % 8 != 0 || max_pages < 1 || max_pages > INT32_MAX / page_size) return pl;
    pl = decode_plan(dtype, N, page_size * max_pages, d, dv, batch, group, force_nsplit, true);
    if (pl.kernel != kDecodeNone) pl.kernel = page_size % kDecodeKeyTile == 0 ? kPagedTile : kPagedChunk;
    return pl;
}

struct DecodePagedArgs {
    DecodeArgs a;                  // K, V: the page pools; Nk: the logical capacity max_pages * page_size
    const int32_t* block_table;    // device, (max_pages, batch)
    int64_t page_size, num_pages, max_pages;
};

int launch_decode_paged_fwd(const DecodePagedArgs& a, hipStream_t s, const char** why);

// The paged fp8 cache (fa_decode_paged_fp8.hip, fa_decode_paged_fp8_fwd): pools of byte pages.
// decode_plan at Nk = cap as decode_paged_plan; a 16-B chunk is 16 keys, so the page size must be
// a positive multiple of 16.  fa_debug_decode_paged_fp8_plan, tests/test_decode_paged_fp8_host.py.
inline DecodePlan decode_paged_fp8_plan(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t group,
                                        int64_t page_size, int64_t max_pages, int force_nsplit) {
    DecodePlan pl;
    if (page_size < 16 || page_size % 16 != 0 || max_pages < 1 || max_pages > INT32_MAX / page_size) return pl;
    pl = decode_plan(dtype, N, page_size * max_pages, d, dv, batch, group, force_nsplit, true);
    if (pl.kernel != kDecodeNone) pl.kernel = page_size % kDecodeKeyTile == 0 ? kPaged8Tile : kPaged8Chunk;
    return pl;
}

struct DecodePagedFp8Args {
    DecodeArgs a;                      // K, V: the byte page pools; Nk: the logical capacity; dtype: the type of Q and O
    const float *k_scale, *v_scale;    // device, `batch` floats each, or nullptr (1.0)
    const int32_t* block_table;        // device, (max_pages, batch)
    int64_t page_size, num_pages, max_pages;
};

int launch_decode_paged_fp8_fwd(const DecodePagedFp8Args& a, hipStream_t s, const char** why);

// Chunked prefill over the paged cache (fa_prefill_paged.hip, fa_prefill_paged_fwd): decode_paged's
// arguments with any N * group.  The rows of a KV slab, position-major, are cut into blocks of
// kPrefillRows, one workgroup each; when batch * blocks is small each block's visible tile range
// is cut into nsplit shares by decode_nsplit's rule, with batch * blocks where decode has batch.
// The workspace and the combine grid are decode_plan's ([nsplit][batch * group][N][dv + 2] fp32),
// the kernel is chosen by the page size alone.  fa_debug_prefill_paged_plan,
// tests/test_prefill_paged_host.py.
constexpr int kPrefillRows = 128;      // rows of a block: 4 waves, one 32-row MFMA tile each
constexpr int kPrefillThreads = 256;
constexpr DecodeKernel kPrefillTile = (DecodeKernel)6;    // prefill_paged_fwd<.., TILE = true>: page_size % 64 == 0, LDS-DMA staging
constexpr DecodeKernel kPrefillChunk = (DecodeKernel)7;   // prefill_paged_fwd<.., TILE = false>: page_size % 8 == 0, 16-B chunks via registers

struct PrefillPlan : DecodePlan {
    int64_t blocks = 0;   // row blocks per KV slab; grid = batch * blocks * nsplit
};

inline PrefillPlan prefill_paged_plan(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t group,
                                      int64_t page_size, int64_t max_pages, int force_nsplit) {
    PrefillPlan pl;
    if (page_size < 8 || page_size % 8 != 0 || max_pages < 1 || max_pages > INT32_MAX / page_size) return pl;
    const int64_t cap = page_size * max_pages;
    if (!dense_16bit(dtype) || !head_dim_class(d) || !head_dim_class(dv) || N < 1 || group < 1 || batch < 1 || cap < N ||
        group > INT32_MAX / N)
        return pl;
    pl.kernel = page_size % kDecodeKeyTile == 0 ? kPrefillTile : kPrefillChunk;
    pl.blocks = ceil_div(N * group, kPrefillRows);
    pl.nsplit = decode_nsplit(cap, batch * pl.blocks, force_nsplit);
    pl.grid = batch * pl.blocks * pl.nsplit;
    if (pl.nsplit > 1) {
        pl.combine_grid = ceil_div(batch * group * N * dv, kDecodeThreads);
        pl.total = (size_t)(pl.nsplit * batch * group * N * (dv + 2)) * sizeof(float) + 256;
    }
    return pl;
}

int launch_prefill_paged_fwd(const DecodePagedArgs& a, hipStream_t s, const char** why);

// Chunked prefill over the paged fp8 cache (fa_prefill_paged_fp8.hip, fa_prefill_paged_fp8_fwd):
// prefill_paged_plan over pools of byte pages.  A 16-B chunk is 16 keys, so the page size must be a
// positive multiple of 16; blocks, nsplit, grids and workspace are prefill_paged_plan's (dtype is
// the type of Q and O).  fa_debug_prefill_paged_fp8_plan, tests/test_prefill_paged_fp8_host.py.
constexpr DecodeKernel kPrefill8Tile = (DecodeKernel)8;    // prefill_paged8_fwd<.., TILE = true>: page_size % 64 == 0, LDS-DMA staging
constexpr DecodeKernel kPrefill8Chunk = (DecodeKernel)9;   // prefill_paged8_fwd<.., TILE = false>: page_size % 16 == 0, 16-B chunks via registers

inline PrefillPlan prefill_paged_fp8_plan(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t group,
                                          int64_t page_size, int64_t max_pages, int force_nsplit) {
    if (page_size % 16 != 0) return PrefillPlan();
    PrefillPlan pl = prefill_paged_plan(dtype, N, d, dv, batch, group, page_size, max_pages, force_nsplit);
    if (pl.kernel != kDecodeNone) pl.kernel = pl.kernel == kPrefillTile ? kPrefill8Tile : kPrefill8Chunk;
    return pl;
}

int launch_prefill_paged_fp8_fwd(const DecodePagedFp8Args& a, hipStream_t s, const char** why);

extern thread_local int g_decode_nsplit;  // fa_debug_set_decode_nsplit: 0 auto, n forces n key ranges

}  // namespace fa
