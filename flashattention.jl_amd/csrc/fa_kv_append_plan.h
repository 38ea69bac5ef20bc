// fa_kv_append_plan.h — the HOST PLAN of the cache writers (fa_kv_append.hip): how
// fa_kv_append_paged / fa_kv_append_paged_fp8 cut a call into destination pieces, and how
// fa_kv_quantize_fp8 cuts a slab into the spans whose maxima it keeps in its workspace.  Pure
// functions of the shape: the lengths and the table are device data and are never read here, so
// the grid covers the most pages N rows can touch and a workgroup whose piece is empty leaves.
#pragma once

#include <algorithm>

#include "fa_dense_plan.h"

namespace fa {

struct KvAppendArgs {
    int dtype;                          // FA_DTYPE_BF16 or FA_DTYPE_F16: the type of K_new and V_new
    bool fp8;                           // the pools hold e4m3fn bytes
    const void *K_new, *V_new;          // (N, d, batch), (N, dv, batch)
    void *K_pages, *V_pages;            // (page_size, d, num_pages), (page_size, dv, num_pages)
    const float *k_scale, *v_scale;     // fp8: device, `batch` floats each, or nullptr (1.0)
    const int32_t* block_table;         // device, (max_pages, batch)
    int64_t N, d, dv, batch, page_size, num_pages, max_pages;
    const int32_t *q_lens, *k_lens;     // device, `batch` values each, or nullptr (full)
};

constexpr int kAppendThreads = 256;
constexpr int kAppendSegRows = 1024;    // rows of a page one workgroup covers: longer pages are cut into segments
constexpr int kAppendChunks = 512;      // 16-B destination chunks per workgroup, at most (two per thread)

struct KvAppendPlan {
    bool decode = false;     // N == 1: kv_append_row, one thread per feature of K and of V
    int chunk = 0;           // elements of a 16-B destination chunk: 8 (16-bit pools), 16 (byte pools)
    int64_t pages = 0;       // the most pages N consecutive rows can touch
    int64_t nseg = 0;        // segments per page
    int64_t feats = 0;       // features (of the d + dv of K and V) per workgroup
    int64_t nfsplit = 0;     // feature ranges
    int64_t grid = 0;        // decode: ceil(batch / slabs per workgroup); else batch * pages * nseg * nfsplit
};

// page_size must be a positive multiple of the chunk (api.cpp refuses anything else first).
inline KvAppendPlan kv_append_plan(bool fp8, int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t page_size,
                                   int64_t max_pages) {
    KvAppendPlan pl;
    pl.chunk = fp8 ? 16 : 8;
    if (N == 1) {
        pl.decode = true;
        pl.grid = ceil_div(batch, std::max<int64_t>(1, kAppendThreads / (d + dv)));
        return pl;
    }
    pl.pages = std::min<int64_t>(max_pages, (N + page_size - 2) / page_size + 1);
    pl.nseg = ceil_div(page_size, kAppendSegRows);
    const int64_t cmax = std::min<int64_t>(page_size, kAppendSegRows) / pl.chunk;
    pl.feats = std::min<int64_t>(d + dv, kAppendChunks / cmax);
    pl.nfsplit = ceil_div(d + dv, pl.feats);
    pl.grid = batch * pl.pages * pl.nseg * pl.nfsplit;
    return pl;
}

int launch_kv_append(const KvAppendArgs& a, hipStream_t s, const char** why);

// fa_kv_quantize_fp8: a slab of n = Nk * dim elements is cut into `parts` spans of `span` elements
// (a multiple of 16), at least kQuantSpan each and at most kQuantParts of them; K and V share the
// part count of the larger.  Workspace: the spans' maxima, [2][batch][parts] floats (+ 256).
constexpr int kQuantSpan = 16384;
constexpr int kQuantParts = 256;

struct KvQuantPlan {
    int64_t parts = 0, span = 0;
    size_t total = 0;
};

inline KvQuantPlan kv_quant_plan(int dtype, int64_t Nk, int64_t d, int64_t dv, int64_t batch) {
    KvQuantPlan pl;
    if (!dense_16bit(dtype) || Nk < 1 || d < 1 || dv < 1 || batch < 1 || Nk >= (1 << 30) / std::max(d, dv)) return pl;
    const int64_t n = Nk * std::max(d, dv);
    const int64_t want = std::max<int64_t>(kQuantSpan, ceil_div(n, kQuantParts));
    pl.span = ceil_div(want, 16) * 16;
    pl.parts = ceil_div(n, pl.span);
    pl.total = (size_t)(2 * batch * pl.parts) * sizeof(float) + 256;
    return pl;
}

struct KvQuantArgs {
    int dtype;
    const void *K, *V;        // (Nk, d, batch), (Nk, dv, batch)
    void *K8, *V8;            // e4m3fn bytes, the same shapes
    float *k_scale, *v_scale; // `batch` floats each
    int64_t Nk, d, dv, batch;
    void* workspace;
    size_t workspace_bytes;
};

int launch_kv_quantize_fp8(const KvQuantArgs& a, hipStream_t s, const char** why);

}  // namespace fa
