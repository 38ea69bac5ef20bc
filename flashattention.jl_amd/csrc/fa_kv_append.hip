// fa_kv_append.hip — the cache WRITERS for gfx950 (MI355X, CDNA4): new K / V rows into a paged
// cache, 16-bit or fp8 (fa_kv_append_paged, fa_kv_append_paged_fp8), and a contiguous 16-bit cache
// into e4m3fn bytes with one scale per slab (fa_kv_quantize_fp8).  No MFMA: these move bytes.
//
// A pool keeps keys contiguous per feature: element (row t, feature f, page p) lies at
// t + page_size * (f + dim * p).  New row i < nq of slab b is logical key j = nk - nq + i and goes
// to row j % page_size of page clamp(table[j / page_size, b]); the rows of one page are therefore
// one contiguous run per feature in the pool AND in the (N, dim, batch) source, but the two runs
// start at unrelated alignments (N, nk - nq and the source pointer are arbitrary).
//
//  * kv_append_pages (N > 1): the work is cut by DESTINATION.  A workgroup owns one piece:
//    (slab, touched page, segment of at most kAppendSegRows rows of it, a range of the d + dv
//    features of K and V together).  It clamps the lengths, leaves if its piece holds no written
//    row, reads and clamps its ONE table entry, then
//      1. loads, per feature, the 16-B ALIGNED source chunks that cover the run (a chunk that
//         sticks out of the source array is read element by element, so nothing outside it is
//         touched) and writes them to an LDS row as they are;
//      2. after one barrier a thread takes a 16-B destination chunk: 8 (or, for byte pools, 16)
//         consecutive source elements from the LDS row, at whatever 2-byte offset the two
//         alignments leave, as aligned dwords joined by v_alignbyte_b32; byte pools divide by the
//         slab's scale, clamp and convert (v_cvt_pk_fp8_f32); one 16-B store.  A chunk that the
//         run covers only in part (its ragged head and tail) is stored element by element, the
//         owned elements only.
//    Nothing of a pool is ever read.
//  * kv_append_row (N == 1, the decode step): one element per feature per slab, page_size apart.
//    One thread per feature of K and of V, 256 / (d + dv) slabs per workgroup, no LDS.
//  * kv_amax_parts, kv_quant_parts (fa_kv_quantize_fp8): a slab is cut into spans; the first
//    kernel writes each span's max |x| (compared as integers: exact, order-free) to the
//    workspace, the second reduces its slab's maxima, writes s = amax / 448 (1 for a zero slab)
//    and converts its span, 16 elements per 16-B store.
//
// The fp8 byte is e4m3fn_rne(clamp(float(x) / s, -448, 448)): an IEEE fp32 division, the clamp
// by v_med3_f32 (it keeps the sign of zero), the convert round-to-nearest-even with subnormals.
#include <type_traits>

#include "fa_common.h"
#include "fa_internal.h"
#include "fa_kv_append_plan.h"
#include "../../include/fa_hip.h"

namespace fa {

namespace {

struct KvAppendParams {
    const void *K_new, *V_new;
    void *K_pages, *V_pages;
    const float *k_scale, *v_scale;
    const int32_t *table, *q_lens, *k_lens;
    int N, d, dv, batch, page_size, num_pages, max_pages, cap;
    int nseg, feats, nfsplit, pages;
};

template <class T>
__device__ __forceinline__ float half_to_float(uint32_t bits) {
    if constexpr (std::is_same<T, bf16>::value) return __uint_as_float(bits << 16);
    else return (float)__builtin_bit_cast(f16, (uint16_t)bits);
}

__device__ __forceinline__ float fp8_prep(float x, float s) {
    return __builtin_amdgcn_fmed3f(__fdiv_rn(x, s), 448.0f, -448.0f);
}

// one 16-bit element as its e4m3fn byte
template <class T>
__device__ __forceinline__ uint8_t fp8_byte(uint32_t bits, float s) {
    const float q = fp8_prep(half_to_float<T>(bits), s);
    return (uint8_t)__builtin_amdgcn_cvt_pk_fp8_f32(q, q, 0, false);
}

// four 16-bit elements (two dwords) as four e4m3fn bytes
template <class T>
__device__ __forceinline__ uint32_t fp8_quad(uint32_t w0, uint32_t w1, float s) {
    const float a = fp8_prep(half_to_float<T>(w0 & 0xFFFFu), s), b = fp8_prep(half_to_float<T>(w0 >> 16), s);
    const float c = fp8_prep(half_to_float<T>(w1 & 0xFFFFu), s), e = fp8_prep(half_to_float<T>(w1 >> 16), s);
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, e, r, true);
    return (uint32_t)r;
}

// The 16 B at the 16-B aligned address a, of an array of 16-bit elements that occupies [lo, hi):
// one wide load when the chunk lies inside the array, else its elements one by one (0 outside).
__device__ __forceinline__ u32x4 source_chunk(uintptr_t a, uintptr_t lo, uintptr_t hi) {
    if (a >= lo && a + 16 <= hi) return *(const u32x4*)a;
    u32x4 w = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uintptr_t q = a + 2 * e;
        if (q >= lo && q + 2 <= hi) w[e >> 1] |= (uint32_t)(*(const uint16_t*)q) << (16 * (e & 1));
    }
    return w;
}

// The clamped lengths of slab b and its written range [lo, nk) of logical keys; false if empty.
struct AppendRange {
    int nq, nk, lo;
};
__device__ __forceinline__ bool append_range(const KvAppendParams& p, int b, AppendRange& r) {
    r.nq = p.q_lens ? varlen_clamp(p.q_lens[b], p.N) : p.N;
    r.nk = p.k_lens ? varlen_clamp(p.k_lens[b], p.cap) : p.cap;
    r.lo = max(r.nk - r.nq, 0);
    return r.nk > r.lo;
}

__device__ __forceinline__ int table_page(const KvAppendParams& p, int pg, int b) {
    const int raw = p.table[(int64_t)b * p.max_pages + pg];
    return min(max(raw, 0), p.num_pages - 1);
}

template <class T, bool FP8>
__global__ __launch_bounds__(kAppendThreads) void kv_append_pages(KvAppendParams p) {
    constexpr int E = FP8 ? 16 : 8;          // elements of a 16-B destination chunk
    constexpr int SPC = FP8 ? 2 : 1;         // 16-B source chunks under one of them
    // feats * (SPC * C + 1) source chunks with feats * C <= kAppendChunks and feats <= 256, and
    // 16 B that the last dword pair of the last row may read
    constexpr int LDS = (kAppendChunks * SPC + 2 * kMaxHeadDim) * 16 + 16;
    __shared__ __attribute__((aligned(16))) char smem[LDS];

    const int tid = threadIdx.x, ps = p.page_size;
    int bid = blockIdx.x;
    const int fs = bid % p.nfsplit;
    bid /= p.nfsplit;
    const int sg = bid % p.nseg;
    bid /= p.nseg;
    const int tp = bid % p.pages, b = bid / p.pages;

    AppendRange ar;
    if (!append_range(p, b, ar)) return;
    const int pg = ar.lo / ps + tp;                       // the logical page of this piece
    if (pg > (ar.nk - 1) / ps) return;
    const int pj0 = pg * ps;                              // its first logical key
    const int r0 = max(ar.lo - pj0, sg * kAppendSegRows), r1 = min(min(ar.nk - pj0, ps), (sg + 1) * kAppendSegRows);
    if (r1 <= r0) return;
    const int page = table_page(p, pg, b);
    const int i0 = pj0 + r0 - (ar.nk - ar.nq);            // the source row of page row r0 (>= 0: pj0 + r0 >= lo)

    const int f_lo = fs * p.feats, nf = min(p.d + p.dv, f_lo + p.feats) - f_lo;
    const int c_lo = r0 / E, C = (r1 + E - 1) / E - c_lo, SC = SPC * C + 1;
    const int N = p.N, d = p.d;

    // the source address of page row r0 of local feature fl, and the bounds of its array
    auto source_of = [&](int fl, uintptr_t& lo, uintptr_t& hi) -> uintptr_t {
        const int g = f_lo + fl;
        const bool isk = g < d;
        const int dim = isk ? d : p.dv, f = isk ? g : g - d;
        lo = (uintptr_t)(isk ? p.K_new : p.V_new);
        hi = lo + 2 * (uintptr_t)N * dim * p.batch;
        return lo + 2 * (((uintptr_t)b * dim + f) * N + i0);
    };

    for (int idx = tid; idx < nf * SC; idx += kAppendThreads) {
        const int fl = idx / SC, sc = idx - fl * SC;
        uintptr_t lo, hi;
        const uintptr_t sa = source_of(fl, lo, hi);
        const uintptr_t a = (sa & ~(uintptr_t)15) + 16 * sc;
        if (a < sa + 2 * (uintptr_t)(r1 - r0)) *(u32x4*)(smem + idx * 16) = source_chunk(a, lo, hi);
    }
    __syncthreads();

    for (int idx = tid; idx < nf * C; idx += kAppendThreads) {
        const int fl = idx / C, c = c_lo + (idx - fl * C);
        uintptr_t lo, hi;
        const uintptr_t sa = source_of(fl, lo, hi);
        const int g = f_lo + fl;
        const bool isk = g < d;
        const int dim = isk ? d : p.dv, f = isk ? g : g - d;
        const int ra = max(c * E, r0), rb = min(c * E + E, r1);
        // row ra of the feature: in the LDS row, and in the pool
        const int o = fl * SC * 16 + (int)(sa & 15) + 2 * (ra - r0);
        const int64_t de = ((int64_t)page * dim + f) * ps + ra;
        float s = 1.0f;
        if constexpr (FP8) {
            const float* const sp = isk ? p.k_scale : p.v_scale;
            if (sp) s = sp[b];
        }
        if (rb - ra == E) {
            const uint32_t* const w = (const uint32_t*)(smem + (o & ~3));
            const int sh = o & 3;
            uint32_t v[4 * SPC];
#pragma unroll
            for (int k = 0; k < 4 * SPC; ++k) v[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
            u32x4 out;
            if constexpr (FP8) {
#pragma unroll
                for (int k = 0; k < 4; ++k) out[k] = fp8_quad<T>(v[2 * k], v[2 * k + 1], s);
                *(u32x4*)((uint8_t*)(isk ? p.K_pages : p.V_pages) + de) = out;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) out[k] = v[k];
                *(u32x4*)((uint16_t*)(isk ? p.K_pages : p.V_pages) + de) = out;
            }
        } else {
            for (int r = ra; r < rb; ++r) {
                const uint16_t x = *(const uint16_t*)(smem + o + 2 * (r - ra));
                if constexpr (FP8) ((uint8_t*)(isk ? p.K_pages : p.V_pages))[de + (r - ra)] = fp8_byte<T>(x, s);
                else ((uint16_t*)(isk ? p.K_pages : p.V_pages))[de + (r - ra)] = x;
            }
        }
    }
}

template <class T, bool FP8>
__global__ __launch_bounds__(kAppendThreads) void kv_append_row(KvAppendParams p) {
    const int per = p.d + p.dv, spw = max(1, kAppendThreads / per);
    const int sl = threadIdx.x / per, g = threadIdx.x - sl * per;
    const int64_t bb = (int64_t)blockIdx.x * spw + sl;
    if (sl >= spw || bb >= p.batch) return;
    const int b = (int)bb;
    AppendRange ar;
    if (!append_range(p, b, ar)) return;                  // N == 1: nq == 1 and nk >= 1 from here on
    const int j = ar.nk - 1, pg = j / p.page_size, row = j - pg * p.page_size;
    const int page = table_page(p, pg, b);
    const bool isk = g < p.d;
    const int dim = isk ? p.d : p.dv, f = isk ? g : g - p.d;
    const uint16_t x = ((const uint16_t*)(isk ? p.K_new : p.V_new))[(int64_t)b * dim + f];
    const int64_t de = ((int64_t)page * dim + f) * p.page_size + row;
    if constexpr (FP8) {
        const float* const sp = isk ? p.k_scale : p.v_scale;
        ((uint8_t*)(isk ? p.K_pages : p.V_pages))[de] = fp8_byte<T>(x, sp ? sp[b] : 1.0f);
    } else {
        ((uint16_t*)(isk ? p.K_pages : p.V_pages))[de] = x;
    }
}

// ---- fa_kv_quantize_fp8 ----

struct KvQuantParams {
    const void *K, *V;
    uint8_t *K8, *V8;
    float *k_scale, *v_scale;
    float* part;      // [2][batch][parts]
    int Nk, d, dv, batch, parts, span;
};

// max over the workgroup of a non-negative value; every thread gets it
__device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return max(max(red[0], red[1]), max(red[2], red[3]));
}

// max |x| of two 16-bit elements in a dword, as the bits of |x| (ordered like the values)
__device__ __forceinline__ uint32_t abs_bits_max(uint32_t w) { return max(w & 0x7FFFu, (w >> 16) & 0x7FFFu); }

template <class T>
__global__ __launch_bounds__(kAppendThreads) void kv_amax_parts(KvQuantParams p) {
    __shared__ uint32_t red[4];
    const int tid = threadIdx.x, part = blockIdx.x % p.parts, b = blockIdx.x / p.parts, z = blockIdx.y;
    const int n = p.Nk * (z ? p.dv : p.d);
    const int e0 = part * p.span, e1 = min(n, e0 + p.span);
    uint32_t mx = 0;
    if (e0 < n) {
        const uint16_t* const src = (const uint16_t*)(z ? p.V : p.K) + (int64_t)b * n;
        const int lead = min(e1 - e0, (int)(((16 - ((uintptr_t)(src + e0) & 15)) & 15) >> 1));
        if (tid < lead) mx = src[e0 + tid] & 0x7FFFu;
        const int ng = (e1 - e0 - lead) / 8;
        for (int g = tid; g < ng; g += kAppendThreads) {
            const u32x4 w = *(const u32x4*)(src + e0 + lead + 8 * g);
            mx = max(max(mx, abs_bits_max(w[0])), max(abs_bits_max(w[1]), max(abs_bits_max(w[2]), abs_bits_max(w[3]))));
        }
        const int t0 = e0 + lead + 8 * ng;
        if (t0 + tid < e1) mx = max(mx, (uint32_t)(src[t0 + tid] & 0x7FFFu));
    }
    mx = block_max(mx, red);
    if (tid == 0) p.part[((int64_t)z * p.batch + b) * p.parts + part] = half_to_float<T>(mx);
}

template <class T>
__global__ __launch_bounds__(kAppendThreads) void kv_quant_parts(KvQuantParams p) {
    __shared__ uint32_t red[4];
    const int tid = threadIdx.x, part = blockIdx.x % p.parts, b = blockIdx.x / p.parts, z = blockIdx.y;
    const int n = p.Nk * (z ? p.dv : p.d);
    const int e0 = part * p.span, e1 = min(n, e0 + p.span);
    if (e0 >= n) return;
    // the slab's maxima, as the bits of non-negative floats (ordered like the values)
    const float* const pm = p.part + ((int64_t)z * p.batch + b) * p.parts;
    uint32_t mx = 0;
    for (int q = tid; q < p.parts; q += kAppendThreads) mx = max(mx, __float_as_uint(pm[q]));
    const float amax = __uint_as_float(block_max(mx, red));
    const float s = amax > 0.0f ? __fdiv_rn(amax, 448.0f) : 1.0f;
    if (part == 0 && tid == 0) (z ? p.v_scale : p.k_scale)[b] = s;

    const uint16_t* const src = (const uint16_t*)(z ? p.V : p.K) + (int64_t)b * n;
    uint8_t* const dst = (z ? p.V8 : p.K8) + (int64_t)b * n;
    const int lead = min(e1 - e0, (int)((16 - ((uintptr_t)(dst + e0) & 15)) & 15));
    if (tid < lead) dst[e0 + tid] = fp8_byte<T>(src[e0 + tid], s);
    const int ng = (e1 - e0 - lead) / 16;
    for (int g = tid; g < ng; g += kAppendThreads) {
        const int e = e0 + lead + 16 * g;
        uint32_t v[8];
        if (((uintptr_t)(src + e) & 15) == 0) {
            const u32x4 w0 = *(const u32x4*)(src + e), w1 = *(const u32x4*)(src + e + 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = w0[k], v[4 + k] = w1[k];
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (uint32_t)src[e + 2 * k] | (uint32_t)src[e + 2 * k + 1] << 16;
        }
        u32x4 out;
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = fp8_quad<T>(v[2 * k], v[2 * k + 1], s);
        *(u32x4*)(dst + e) = out;
    }
    const int t0 = e0 + lead + 16 * ng;
    if (t0 + tid < e1) dst[t0 + tid] = fp8_byte<T>(src[t0 + tid], s);
}

template <class T>
void launch_append_kernels(const KvAppendPlan& pl, const KvAppendParams& p, bool fp8, hipStream_t s) {
    const dim3 grid((unsigned)pl.grid), blk(kAppendThreads);
    if (pl.decode) {
        if (fp8) hipLaunchKernelGGL((kv_append_row<T, true>), grid, blk, 0, s, p);
        else hipLaunchKernelGGL((kv_append_row<T, false>), grid, blk, 0, s, p);
    } else {
        if (fp8) hipLaunchKernelGGL((kv_append_pages<T, true>), grid, blk, 0, s, p);
        else hipLaunchKernelGGL((kv_append_pages<T, false>), grid, blk, 0, s, p);
    }
}

template <class T>
void launch_quant_kernels(const KvQuantPlan& pl, const KvQuantParams& p, hipStream_t s) {
    const dim3 grid((unsigned)(pl.parts * p.batch), 2), blk(kAppendThreads);
    hipLaunchKernelGGL((kv_amax_parts<T>), grid, blk, 0, s, p);
    hipLaunchKernelGGL((kv_quant_parts<T>), grid, blk, 0, s, p);
}

}  // namespace

int launch_kv_append(const KvAppendArgs& a, hipStream_t s, const char** why) {
    const int64_t chunk = a.fp8 ? 16 : 8;
    if (!dense_16bit(a.dtype) || a.N < 1 || a.batch < 1 || a.d < 1 || a.dv < 1 || a.d > kMaxHeadDim || a.dv > kMaxHeadDim ||
        a.page_size < chunk || a.page_size % chunk != 0 || a.max_pages < 1 || a.max_pages > INT32_MAX / a.page_size ||
        a.num_pages < 1 || !aligned16(a.K_pages) || !aligned16(a.V_pages)) {
        *why = "shape outside the cache append kernels (api.cpp checks it first)";
        return FA_ERR_UNSUPPORTED;
    }
    const KvAppendPlan pl = kv_append_plan(a.fp8, a.N, a.d, a.dv, a.batch, a.page_size, a.max_pages);
    if (pl.grid > INT32_MAX) {
        *why = "grid too large";
        return FA_ERR_UNSUPPORTED;
    }
    KvAppendParams p;
    p.K_new = a.K_new; p.V_new = a.V_new; p.K_pages = a.K_pages; p.V_pages = a.V_pages;
    p.k_scale = a.k_scale; p.v_scale = a.v_scale;
    p.table = a.block_table; p.q_lens = a.q_lens; p.k_lens = a.k_lens;
    p.N = (int)a.N; p.d = (int)a.d; p.dv = (int)a.dv; p.batch = (int)a.batch;
    p.page_size = (int)a.page_size;
    p.num_pages = (int)std::min<int64_t>(a.num_pages, INT32_MAX);   // an entry is an int32: ids past it cannot be named
    p.max_pages = (int)a.max_pages;
    p.cap = (int)(a.max_pages * a.page_size);
    p.nseg = (int)pl.nseg; p.feats = (int)pl.feats; p.nfsplit = (int)pl.nfsplit; p.pages = (int)pl.pages;
    if (a.dtype == FA_DTYPE_F16) launch_append_kernels<f16>(pl, p, a.fp8, s);
    else launch_append_kernels<bf16>(pl, p, a.fp8, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    return FA_OK;
}

int launch_kv_quantize_fp8(const KvQuantArgs& a, hipStream_t s, const char** why) {
    const KvQuantPlan pl = kv_quant_plan(a.dtype, a.Nk, a.d, a.dv, a.batch);
    if (pl.parts < 1 || a.batch > INT32_MAX / pl.parts) {
        *why = "shape outside the cache quantise kernels (api.cpp checks it first)";
        return FA_ERR_UNSUPPORTED;
    }
    if (!a.workspace || a.workspace_bytes < pl.total) {
        *why = "workspace missing or smaller than fa_kv_quantize_fp8_workspace()";
        return FA_ERR_WORKSPACE;
    }
    KvQuantParams p;
    p.K = a.K; p.V = a.V; p.K8 = (uint8_t*)a.K8; p.V8 = (uint8_t*)a.V8;
    p.k_scale = a.k_scale; p.v_scale = a.v_scale;
    p.part = (float*)al256(a.workspace);
    p.Nk = (int)a.Nk; p.d = (int)a.d; p.dv = (int)a.dv; p.batch = (int)a.batch;
    p.parts = (int)pl.parts; p.span = (int)pl.span;
    if (a.dtype == FA_DTYPE_F16) launch_quant_kernels<f16>(pl, p, s);
    else launch_quant_kernels<bf16>(pl, p, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    return FA_OK;
}

}  // namespace fa
