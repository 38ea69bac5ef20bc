// fa_windowed.h — what the windowed / block-local attention forward
// (fa_windowed_fwd.hip) and backward (fa_windowed_bwd.hip) share: the window
// geometry, the composed path's gather / fold, the row-shift, LDS and strip-image
// device helpers, and the HOST PLANS that name the kernel a call gets
// (win_fwd_plan, win_bwd_plan, at the end of this file; api.cpp exposes them
// as debug entries, tests/test_windowed_plan_host.py pins them).
//
// Replaces windowed_fa(q, k, v, ws; stride, pad) (reference
// src/windowed.jl:3-23; block_fa = stride ws, :1) and adds its backward
// (README.md:36-37 claims it, the reference has no code).
//
// Window geometry is NNlib.unfold / fold's (src/utils.jl:36-54): per spatial
// dim O_i = (S_i + 2 pad − ws) / stride + 1 windows, window token t =
// (t_1, t_2, t_3) first-dim-fastest, pixel x_i = o_i·stride − pad + t_i, zero
// padding outside the image (padded tokens are ordinary, UNMASKED keys with
// k = v = 0, exactly as in the reference).  y = fold(window outputs) ./
// coverage count, so uncovered pixels are 0/0 = NaN (Appendix A.7).
//
// Composed path (every dtype, any window size):
//   gather  : q, k, v → (T, d, L·B) window batches in the workspace;
//   dense   : fa_dense_fwd / fa_dense_bwd on the window batch (l, m land
//             directly in the caller's (T, 1, L, B) arrays: same layout);
//   fold    : deterministic per-pixel sum over covering windows (÷ count).
// The backward is the exact chain rule: dyw = window(dy ./ count), dense
// backward per window, fold (sum) of dqw / dkw / dvw.
//
// The two .hip files are separate objects because they want different scheduler
// flags (Makefile).  win_gather / win_fold are templates here, so each object emits
// the instantiations its launchers use.
#pragma once
#include <type_traits>

#include "fa_common.h"
#include "fa_internal.h"
#include "../../include/fa_hip.h"

// Phase-timestamp hook for latency studies (tools/exp/win_stamp.hip defines it);
// compiled out of the product library.
#ifndef FA_STAMP
#define FA_STAMP(k)
#endif
#ifndef FA_BSTAMP   // the persistent strip backward's per-strip hook: 0 start, 1 + j load j landed,
                    // 9 + c dV chunk c, 11 + c dK chunk c, 13 + c dQ chunk c stored, 15 end
#define FA_BSTAMP(k)
#endif
// Timing-only ablations of win_rows1s (tools/exp/win_ablate.hip; 0 in the product):
// 1 = no y stores, 2 = every row load from one address; of win_strip
// (tools/exp/strip_stamp.py): 4 = no y strip-image writes, 8 = no y global stores,
// 16 = no 2-B stores of the chunks shared with a neighbour strip; of win_bwd_strip
// (tools/exp/bwd_strip_stamp.py): 32 = no gradient stores, 64 = no gradient image writes
#ifndef FA_WIN_ABL
#define FA_WIN_ABL 0
#endif

namespace fa {

struct WinDev {
    int nsp, ws, stride, pad, T, L, P;
    int S[3], O[3];
};

static WinDev to_dev(const WindowGeom& g) {
    WinDev w;
    w.nsp = g.nsp; w.ws = (int)g.ws; w.stride = (int)g.stride; w.pad = (int)g.pad;
    w.T = (int)g.T; w.L = (int)g.L; w.P = (int)g.P;
    for (int i = 0; i < 3; ++i) { w.S[i] = (int)g.S[i]; w.O[i] = (int)g.O[i]; }
    return w;
}

// pixel index of window w, token t (−1 = zero padding)
__device__ __forceinline__ int win_pixel(const WinDev& g, int w, int t) {
    int pix = 0, mul = 1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i < g.nsp) {
            const int o = w % g.O[i];
            w /= g.O[i];
            const int ti = t % g.ws;
            t /= g.ws;
            const int x = o * g.stride - g.pad + ti;
            if (x < 0 || x >= g.S[i]) return -1;
            pix += x * mul;
            mul *= g.S[i];
        }
    }
    return pix;
}

// number of windows covering pixel pix (for the divisor)
__device__ __forceinline__ int win_count(const WinDev& g, int pix) {
    int cnt = 1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i < g.nsp) {
            const int x = pix % g.S[i];
            pix /= g.S[i];
            const int num = x + g.pad - g.ws + 1;
            const int lo = num <= 0 ? 0 : (num + g.stride - 1) / g.stride;
            const int hi = min(g.O[i] - 1, (x + g.pad) / g.stride);
            cnt *= max(0, hi - lo + 1);
        }
    }
    return cnt;
}

// dst (T, C, L·B) ← window(src (S..., C, B)); DIVIDE scales by 1/coverage
template <class T, bool DIVIDE>
__global__ __launch_bounds__(256) void win_gather(const T* __restrict__ src, T* __restrict__ dst, int C,
                                                  int64_t total, WinDev g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int t = (int)(e % g.T);
    int64_t rest = e / g.T;
    const int c = (int)(rest % C);
    rest /= C;
    const int w = (int)(rest % g.L);
    const int64_t b = rest / g.L;
    const int pix = win_pixel(g, w, t);
    typedef typename std::conditional<sizeof(T) == 8, double, float>::type A;   // Float64 stays double
    A v = (A)0;
    if (pix >= 0) {
        v = (A)src[(b * C + c) * (int64_t)g.P + pix];
        if constexpr (DIVIDE) v /= (A)win_count(g, pix);
    }
    dst[e] = (T)v;
}

// dst (S..., C, B) ← fold(src (T, C, L·B)) [÷ coverage count, NaN if 0]
template <class T, bool DIVIDE>
__global__ __launch_bounds__(256) void win_fold(const T* __restrict__ src, T* __restrict__ dst, int C,
                                                int64_t total, WinDev g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int pix = (int)(e % g.P);
    const int64_t bc = e / g.P;             // b·C + c
    const int c = (int)(bc % C);
    const int64_t b = bc / C;
    int x[3] = {0, 0, 0}, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    int rem = pix;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i < g.nsp) {
            x[i] = rem % g.S[i];
            rem /= g.S[i];
            const int num = x[i] + g.pad - g.ws + 1;
            lo[i] = num <= 0 ? 0 : (num + g.stride - 1) / g.stride;
            hi[i] = min(g.O[i] - 1, (x[i] + g.pad) / g.stride);
        }
    }
    typedef typename std::conditional<sizeof(T) == 8, double, float>::type A;   // Float64 stays double
    A acc = (A)0;
    int cnt = 0;
    for (int o3 = lo[2]; o3 <= hi[2]; ++o3)
        for (int o2 = lo[1]; o2 <= hi[1]; ++o2)
            for (int o1 = lo[0]; o1 <= hi[0]; ++o1) {
                const int t1 = x[0] + g.pad - o1 * g.stride;
                const int t2 = g.nsp > 1 ? x[1] + g.pad - o2 * g.stride : 0;
                const int t3 = g.nsp > 2 ? x[2] + g.pad - o3 * g.stride : 0;
                const int w = o1 + g.O[0] * (o2 + g.O[1] * o3);
                const int t = t1 + g.ws * (t2 + g.ws * t3);
                acc += (A)src[t + (int64_t)g.T * (c + (int64_t)C * (w + (int64_t)g.L * b))];
                ++cnt;
            }
    if constexpr (DIVIDE) acc = acc / (A)cnt;   // 0/0 = NaN where uncovered (reference semantics)
    dst[e] = (T)acc;
}

static bool fully_covered(const WindowGeom& g) {
    for (int i = 0; i < g.nsp; ++i) {
        if (g.stride > g.ws) return false;                                  // gaps between windows
        if (-g.pad > 0) return false;
        if ((g.O[i] - 1) * g.stride - g.pad + g.ws - 1 < g.S[i] - 1) return false;   // uncovered tail
    }
    return true;
}

// --------------------------------------------------------------------------
// Row-shift staging helpers (win_rows1s in the forward file has the scheme; the
// per-window and strip backward stage their rows the same way).
// --------------------------------------------------------------------------
__device__ __forceinline__ unsigned pick_dword(const u32x4& in, int idx) {
    unsigned r = 0u;
    r = idx == 0 ? in[0] : r;
    r = idx == 1 ? in[1] : r;
    r = idx == 2 ? in[2] : r;
    r = idx == 3 ? in[3] : r;
    return r;
}
// out pixel t = in pixel (t + sh) (0 outside 0..7), sh in (-8, 8) wave-uniform,
// then AND-ed with the per-slot mask.  Interior windows (ax = xs rounded down to even)
// shift by 0 or 1 pixel: one v_alignbyte per dword (round 5; the runtime dword picks of
// the general case are kept for windows at the image's left and right edges).
__device__ __forceinline__ u32x4 shift_row(const u32x4& in, int sh, const unsigned (&mask)[4]) {
    const int s2 = sh >> 1;              // floor(sh / 2)
    u32x4 o;
    if (s2 == 0) {
        const unsigned ab = (sh & 1) ? 2u : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_alignbyte(j < 3 ? in[j + 1] : 0u, in[j], ab) & mask[j];
    } else if (sh & 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = __builtin_amdgcn_alignbyte(pick_dword(in, j + s2 + 1), pick_dword(in, j + s2), 2u) & mask[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pick_dword(in, j + s2) & mask[j];
    }
    return o;
}

// Workgroup barrier that orders LDS only (s_waitcnt lgkmcnt(0); s_barrier):
// outstanding global loads are not waited for.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_s_waitcnt(0xC07F);   // gfx9 encoding: vmcnt 63, expcnt 7, lgkmcnt 0
    __builtin_amdgcn_s_barrier();
}

// LDS accesses hidden from the compiler (inline asm).  hipcc makes every LDS access
// it can see wait for ALL outstanding LDS-DMA (s_waitcnt vmcnt(0)): it cannot tell
// the DMA's destination buffer from the one being read, so a multi-buffer DMA
// pipeline would drain at every step.  An asm read's result is NOT ready until
// lds_wait(); pass it through lds_fence() after that wait, before any use.
__device__ __forceinline__ uint32_t lds_off(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
__device__ __forceinline__ s16x4 lds_tr16(const void* p) {
    s16x4 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(lds_off(p)) : "memory");
    return r;
}
__device__ __forceinline__ u32x4 lds_b128(const void* p) {
    u32x4 r;
    asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(lds_off(p)) : "memory");
    return r;
}
__device__ __forceinline__ u32x2 lds_b64(const void* p) {
    u32x2 r;
    asm volatile("ds_read_b64 %0, %1" : "=v"(r) : "v"(lds_off(p)) : "memory");
    return r;
}
__device__ __forceinline__ float lds_b32(const void* p) {
    float r;
    asm volatile("ds_read_b32 %0, %1" : "=v"(r) : "v"(lds_off(p)) : "memory");
    return r;
}
__device__ __forceinline__ void lds_w16(void* p, unsigned v) {
    asm volatile("ds_write_b16 %0, %1" : : "v"(lds_off(p)), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void lds_w32u(void* p, unsigned v) {
    asm volatile("ds_write_b32 %0, %1" : : "v"(lds_off(p)), "v"(v) : "memory");
}
// Returning agent-scope atomic add, hidden from the compiler's waitcnt model (the
// caller counts it in its vmcnt bookkeeping and fences the result after the wait).
__device__ __forceinline__ unsigned atomic_add_ret(unsigned* p, unsigned v) {
    unsigned r;
    asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(r) : "v"(p), "v"(v) : "memory");
    return r;
}

template <class X>
__device__ __forceinline__ void lds_fence(X& x) { asm volatile("" : "+v"(x)); }

// Per-lane variant of shift_row (windows of one workgroup differ in shift; -8 < sh < 8,
// so the dword shift s2 = floor(sh / 2) is in [-4, 3]): three bit-select levels (1, 2, 4
// dwords) over the zero-extended row, with lane masks, then the odd pixel by
// v_alignbyte with the lane's byte shift.  (Written as selects of array elements, the
// compiler turned the levels into indexed scratch accesses.)
__device__ __forceinline__ u32x4 shift_row_lane(const u32x4& in, int sh, const unsigned (&mask)[4]) {
    const int u = (sh >> 1) + 4;                     // 0 .. 7: e[j] = ext[j + u] = in[j + s2]
    const unsigned m1 = 0u - (unsigned)(u & 1), m2 = 0u - (unsigned)((u >> 1) & 1), m4 = 0u - (unsigned)((u >> 2) & 1);
    auto bfi = [](unsigned m, unsigned x, unsigned y) { return (x & m) | (y & ~m); };
    unsigned ext[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) ext[i] = (i >= 4 && i < 8) ? in[i - 4] : 0u;
    unsigned a1[12], a2[10], e[5];
#pragma unroll
    for (int i = 0; i < 12; ++i) a1[i] = bfi(m1, ext[i + 1], ext[i]);
#pragma unroll
    for (int i = 0; i < 10; ++i) a2[i] = bfi(m2, a1[i + 2], a1[i]);
#pragma unroll
    for (int j = 0; j < 5; ++j) e[j] = bfi(m4, a2[j + 4], a2[j]);
    const unsigned ab = (sh & 1) ? 2u : 0u;
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_alignbyte(e[j + 1], e[j], ab) & mask[j];
    return o;
}

// --------------------------------------------------------------------------
// Strip kernels' LDS images (win_strip in the forward file describes the strip
// geometry, the rotated slots and the Q / K / V chunk swizzles; win_bwd_strip
// uses the same images).
// --------------------------------------------------------------------------
constexpr int kStripW = 8;                          // windows per strip workgroup
// Strip image [f][8 rows][64 px] (1 KB per feature): byte offset of pixel px.  The
// 16-B chunk index is XORed with (row & 3, f >> 2).  A 2-B write instruction of a
// wave covers, per 32-lane group, 4 slot rows x one window's 8 consecutive pixels of
// one feature; writes bank on 32 dwords (MI355X_MICROARCH §LDS), so the 128-B rows
// all start on bank 0 and only the XOR separates them: with row & 3 the 4 rows take
// 4 different 16-B chunks, and when a window's 8 pixels straddle two chunks (c, c + 1)
// the XOR swaps them so the rows' dwords stay complementary — conflict-free.  (Round 3
// used row >> 1: rows 2k and 2k + 1 met on the same banks, ~1.9 conflict cycles per
// write, profiles/r04_win_bwd_strip_lds_conflicts.txt.)  The 16-B chunk reads of the
// stores (ds_read_b128, 16-lane groups, 64 banks) stay conflict-free: an XOR below 4
// keeps each chunk in its half of the row.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// two fp32 -> a packed pair of T (v_cvt_pk_*), and back
template <class T>
__device__ __forceinline__ unsigned pk2(f32x2 v) {
    typedef T T2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, T2));
}
template <class T>
__device__ __forceinline__ f32x2 unpk2(unsigned u) {
    typedef T T2 __attribute__((ext_vector_type(2)));
    return __builtin_convertvector(__builtin_bit_cast(T2, u), f32x2);
}
__device__ __forceinline__ int simg_swz(int f, int row) { return (row & 3) | (((f >> 2) & 1) << 2); }
__device__ __forceinline__ int simg_pos(int f, int row, int px) {
    return f * 1024 + row * 128 + (((px >> 3) ^ simg_swz(f, row)) << 4) + (px & 7) * 2;
}
__device__ __forceinline__ int sqk_swz(int f, int c) { return (f & 7) ^ (((c >> 1) & 1) << 2); }
__device__ __forceinline__ int sqk_pos(int f, int c, int w) {   // byte offset in a Q / K chunk image
    return f * 1024 + c * 128 + ((w ^ sqk_swz(f, c)) << 4);
}
__device__ __forceinline__ int sv_pos(int f, int c, int w) {    // byte offset in a V chunk image
    return f * 1024 + ((c ^ ((f >> 3) & 1)) << 7) + ((w ^ (f & 7)) << 4);
}

// Windows of the first strip: the smallest k0 in 1..8 with k0 * ws = pad (mod 8),
// so that every later strip starts on a 16-B chunk of y (8 otherwise).
static int strip_first(const WindowGeom& g) {
    for (int k0 = 1; k0 <= kStripW; ++k0)
        if (((k0 * g.ws - g.pad) % 8 + 8) % 8 == 0) return k0;
    return kStripW;
}
static int64_t strip_count(const WindowGeom& g, int k0) {
    return g.O[0] <= k0 ? 1 : 1 + (g.O[0] - k0 + kStripW - 1) / kStripW;
}

static size_t esize(int dtype) { return dtype_size(dtype); }
static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

template <class T>
static hipError_t gather(const void* src, void* dst, int C, int64_t batch, const WinDev& g, bool divide,
                         hipStream_t s) {
    const int64_t total = (int64_t)g.T * C * g.L * batch;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (divide) hipLaunchKernelGGL((win_gather<T, true>), grid, dim3(256), 0, s, (const T*)src, (T*)dst, C, total, g);
    else hipLaunchKernelGGL((win_gather<T, false>), grid, dim3(256), 0, s, (const T*)src, (T*)dst, C, total, g);
    return hipGetLastError();
}
template <class T>
static hipError_t fold(const void* src, void* dst, int C, int64_t batch, const WinDev& g, bool divide,
                       hipStream_t s) {
    const int64_t total = (int64_t)g.P * C * batch;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (divide) hipLaunchKernelGGL((win_fold<T, true>), grid, dim3(256), 0, s, (const T*)src, (T*)dst, C, total, g);
    else hipLaunchKernelGGL((win_fold<T, false>), grid, dim3(256), 0, s, (const T*)src, (T*)dst, C, total, g);
    return hipGetLastError();
}

static bool geom_fits(const WindowGeom& g, int64_t d, int64_t dv, int64_t batch) {
    return g.T * g.L * batch * (d > dv ? d : dv) < (int64_t)INT32_MAX * 2 && g.P * batch * (d > dv ? d : dv) < INT32_MAX * 2LL &&
           g.T * g.L < INT32_MAX && g.P < INT32_MAX;
}

// what both launchers check first
static int win_args_fit(const WindowGeom& g, int64_t d, int64_t dv, int64_t batch, const char** why) {
    if (d > kMaxHeadDim || dv > kMaxHeadDim) {
        *why = "head dimension exceeds the compiled maximum (128)";
        return FA_ERR_UNSUPPORTED;
    }
    if (!geom_fits(g, d, dv, batch)) {
        *why = "windowed problem too large for 32-bit window indexing";
        return FA_ERR_UNSUPPORTED;
    }
    return FA_OK;
}

// fa_status of a HIP call, and of the launch just made
static int hip_status(hipError_t e, const char** why) {
    if (e == hipSuccess) return FA_OK;
    *why = hipGetErrorString(e);
    return FA_ERR_HIP;
}
static int launch_status(const char** why) { return hip_status(hipGetLastError(), why); }

// Calls f(D, DV) with the head-dim classes the d, dv <= 64 kernels are compiled for
// (32 or 64 each) as integral constants: f is a generic lambda, [&](auto D, auto DV),
// that names kernel<..., D, DV> (the constants, dim_c of fa_internal.h, convert to int at
// compile time).
template <class F>
static void by_head_class(int64_t d, int64_t dv, F&& f) {
    if (d <= 32) {
        if (dv <= 32) f(dim_c<32>{}, dim_c<32>{});
        else f(dim_c<32>{}, dim_c<64>{});
    } else if (dv <= 32) f(dim_c<64>{}, dim_c<32>{});
    else f(dim_c<64>{}, dim_c<64>{});
}

// --------------------------------------------------------------------------
// The plans: which kernel a call gets.  Pure host functions of the shape, the
// forced mode, the pointer-alignment facts and the CU count: the launchers switch
// on the result and make no choice of their own, fa_windowed_fwd_workspace asks the
// forward plan too, and fa_debug_win_fwd_plan / fa_debug_win_bwd_plan (api.cpp)
// return it for tests.
// --------------------------------------------------------------------------

// Values of fa_debug_set_win_composed (g_win_force_composed).  "Where eligible": a mode
// that does not apply to a shape falls through to the next rule.  7-9 (the rejected
// LDS-DMA and segment kernels, removed in round 4), 11 and anything else select auto.
enum WinMode : int {
    kWinAuto = 0,
    kWinComposed = 1,    // gather, dense, fold
    kWinGather = 2,      // win_fused (register gather): no row-staged kernel
    kWinOne = 3,         // one window per workgroup: win_rows1s x1 (ws <= 7), win_rows1 (ws 8)
    kWinScatter4 = 4,    // win_rows: four-window row scatter
    kWinScatter1 = 5,    // win_rows1: one-window row scatter, at ws <= 7 too
    kWinTwo = 6,         // win_rows1s x2 (the auto choice for small launches)
    kWinStrip = 10,      // win_strip / win_bwd_strip below kStripMin / kStripBwdMin strips too
    kWinThree = 12,      // win_rows1s x3
    kWinBwdPair = 13,    // win_bwd_rows x2 at any grid size (the forward: as kWinTwo)
};

enum WinFwdKernel : int {
    kWinFwdComposed = 0,   // gather, dense forward, fold
    kWinFwdFused = 1,      // win_fused, y stored directly
    kWinFwdFusedWs = 2,    // win_fused into the workspace, then fold (overlapping windows)
    kWinFwdRows = 3,       // win_rows
    kWinFwdRows1 = 4,      // win_rows1
    kWinFwdShift1 = 5,     // win_rows1s, one window per workgroup
    kWinFwdShift2 = 6,     // win_rows1s, two
    kWinFwdShift3 = 7,     // win_rows1s, three
    kWinFwdShift128 = 8,   // win_rows1s<128, 128>, one window per workgroup
    kWinFwdStrip = 9,      // win_strip
    kWinFwdF32 = 10,       // win_rows_f32
};

enum WinBwdKernel : int {
    kWinBwdComposed = 0,      // gather, dense forward + backward, fold
    kWinBwdRows1 = 1,         // win_bwd_rows, one window per workgroup
    kWinBwdRows2 = 2,         // win_bwd_rows, two
    kWinBwdRows128 = 3,       // win_bwd_rows<128, 128>
    kWinBwdStrip = 4,         // win_bwd_strip, every strip end on a 16-B chunk
    kWinBwdStripPartial = 5,  // win_bwd_strip<PARTIAL>
    kWinBwdF32 = 6,           // win_bwd_f32
};

// ws = 8 (row scatter): four windows per workgroup (win_rows) from kRows4Min windows up,
// one window per workgroup (win_rows1) below, where four per workgroup would leave CUs idle.
constexpr int64_t kRows4Min = 1024;
// Strip kernel (win_strip) from this many workgroups on: below it the eight-window
// workgroups leave CUs idle and the two-window kernel's latency wins (configs[2] at
// B = 1 is 57 strips).
constexpr int64_t kStripMin = 256;
// Window counts between which the row-shift forward runs three windows per workgroup
// (768 threads) instead of two (round 6, profiles/r06_win_nwin_ab.log, configs[2] shape:
// B = 2 8.09-8.14 vs 8.82-8.95 us, B = 3 11.67 vs 11.41, B = 4 a tie, B = 1 7.10 vs 6.23,
// r06_win_nwin_ab2.log; four windows per workgroup slower at every B): fewer, longer
// workgroups than two windows give, with one more window's row loads coalesced per
// (feature, row) line.
constexpr int64_t kRows3Min = 600, kRows3Max = 1000;
// The strip backward (win_bwd_strip) from this many strips on.
constexpr int64_t kStripBwdMin = 256;
// The per-window backward runs two adjacent windows per workgroup (their row loads share
// lines, as in win_rows1s) while the grid is at most about one round of CUs, up to this many
// windows per CU (1.5: configs[2] at B = 1 is 361 windows on 256 CUs); one window per
// workgroup, several per CU, above it (round 6).
constexpr double kBwdPairMaxPerCu = 1.5;
// The CU count the backward plans with: device_cus()'s answer, or an MI355X's when the
// device cannot be asked.
constexpr int64_t kCusUnknown = 256;
inline int64_t win_cus(int device_cus) { return device_cus > 0 ? device_cus : kCusUnknown; }

inline bool win_16bit(int dtype) { return dtype == FA_DTYPE_BF16 || dtype == FA_DTYPE_F16; }
inline int64_t win_dmax(int64_t d, int64_t dv) { return d > dv ? d : dv; }
// 2-D windows that do not overlap (every covered pixel has one owner: direct stores), at
// most wsmax pixels a side
inline bool win_direct2d(const WindowGeom& g, int wsmax) { return g.nsp == 2 && g.stride >= g.ws && g.ws <= wsmax; }
// the fp32 kernels' shapes, forward and backward
inline bool win_f32_ok(int dtype, const WindowGeom& g, int64_t d, int64_t dv) {
    return dtype == FA_DTYPE_F32 && win_direct2d(g, 8) && g.S[0] >= 8 && d <= 64 && dv <= 64 &&
           g.P * win_dmax(d, dv) * 4 < INT32_MAX - 64;
}
// the strip kernels' shapes, forward and backward (the strip count is the caller's check)
inline bool win_strip_shape(int dtype, const WindowGeom& g, int64_t d, int64_t dv, int mode) {
    return win_16bit(dtype) && g.nsp == 2 && g.stride == g.ws && g.ws <= 7 && g.S[0] % 8 == 0 && d <= 64 && dv <= 64 &&
           (mode == kWinAuto || mode == kWinStrip);
}
inline int64_t win_strips(const WindowGeom& g, int64_t batch) {
    return strip_count(g, strip_first(g)) * g.O[1] * batch;
}

// qkv_aligned16: q, k and v are 16-B aligned; y_aligned16: y is.
inline WinFwdKernel win_fwd_plan(int dtype, const WindowGeom& g, int64_t d, int64_t dv, int64_t batch, int mode,
                                 bool qkv_aligned16, bool y_aligned16) {
    if (mode == kWinComposed) return kWinFwdComposed;
    if (win_f32_ok(dtype, g, d, dv)) return kWinFwdF32;
    if (!win_16bit(dtype)) return kWinFwdComposed;
    const int64_t nw = g.L * batch, dmax = win_dmax(d, dv);
    // Row-staged kernels: 2-D, non-overlapping, ws <= 8, width % 8 == 0, 16-B aligned tensors
    const bool staged = mode != kWinGather && win_direct2d(g, 8) && g.S[0] % 8 == 0 && nw < INT32_MAX && qkv_aligned16;
    // d or dv in (64, 128]: the one-window row-shift kernel at 128 features (50 KB of LDS,
    // every wave runs two of the four 32-feature output chunks)
    if (staged && g.ws <= 7 && (d > 64 || dv > 64) && d <= 128 && dv <= 128 && g.P * 128 * 2 < INT32_MAX)
        return kWinFwdShift128;
    // win_fused's limits, which every kernel below shares
    if (g.T > 64 || d > 64 || dv > 64 || g.P * dmax * 2 >= INT32_MAX) return kWinFwdComposed;
    if (g.stride < g.ws) return kWinFwdFusedWs;
    if (!staged) return kWinFwdFused;
    const bool per_window = mode == kWinOne || mode >= kWinScatter1;
    if (mode == kWinScatter4 || (!per_window && g.ws == 8 && nw >= kRows4Min)) return kWinFwdRows;
    if (g.ws == 8 || mode == kWinScatter1) return kWinFwdRows1;
    // ws <= 7: the row-shift family beats the four-window row-scatter kernel at every batch
    // size (128x128x64, ws 7: B=1 6.8 vs 26.7 us, B=32 83-90 vs 123 us)
    if (y_aligned16 && win_strip_shape(dtype, g, d, dv, mode)) {
        const int64_t nstrip = win_strips(g, batch);
        if (nstrip < INT32_MAX && (mode == kWinStrip || nstrip >= kStripMin)) return kWinFwdStrip;
    }
    // win_rows1s addresses its NWIN windows by 32-bit byte offsets from the workgroup's first
    // image, over up to NWIN images (one window per image): those images' bytes stay below 2^31
    const bool two_img_ok = 2 * g.P * dmax * 2 < INT32_MAX, three_img_ok = 3 * g.P * dmax * 2 < INT32_MAX;
    // The auto rule looks at the window count only (kRows3Min's measurements), not at the
    // geometry: any windows-per-image count is right, since the kernel's descriptors span the
    // three images a triple can touch; images too large for that take two per workgroup.
    const bool three = mode == kWinThree || (mode == kWinAuto && nw >= kRows3Min && nw < kRows3Max);
    if (three && three_img_ok) return kWinFwdShift3;
    if (mode != kWinOne && two_img_ok) return kWinFwdShift2;
    return kWinFwdShift1;
}

// in_aligned16: q, k, v, y and dy are 16-B aligned; grad_aligned16: dq, dk and dv are;
// cus: win_cus() of the device's CU count.
inline WinBwdKernel win_bwd_plan(int dtype, const WindowGeom& g, int64_t d, int64_t dv, int64_t batch, int mode,
                                 bool in_aligned16, bool grad_aligned16, int64_t cus) {
    if (mode == kWinComposed) return kWinBwdComposed;
    // the row-shift forward's shapes
    if (win_16bit(dtype) && win_direct2d(g, 7) && g.S[0] % 8 == 0 && d <= 128 && dv <= 128 && in_aligned16 &&
        g.P * 128 * 2 < INT32_MAX && g.L * batch < INT32_MAX) {
        if (grad_aligned16 && win_strip_shape(dtype, g, d, dv, mode)) {
            const int64_t nstrip = win_strips(g, batch);
            if (nstrip < INT32_MAX && g.T * g.O[0] * 4 < INT32_MAX && (mode == kWinStrip || nstrip >= kStripBwdMin)) {
                // strip ends on 16-B chunks: every strip boundary (k0 aligns them) and the covered right end
                const int64_t xend = g.O[0] * g.ws - g.pad;
                const bool aligned = ((strip_first(g) * g.ws - g.pad) % 8 + 8) % 8 == 0 && (xend >= g.S[0] || xend % 8 == 0);
                return aligned ? kWinBwdStrip : kWinBwdStripPartial;
            }
        }
        if (d > 64 || dv > 64) return kWinBwdRows128;   // 83 KB of LDS: one workgroup per CU
        const bool pair = 2 * g.P * win_dmax(d, dv) * 2 < INT32_MAX &&
                          (mode == kWinBwdPair || (mode == kWinAuto && g.L * batch <= kBwdPairMaxPerCu * cus));
        return pair ? kWinBwdRows2 : kWinBwdRows1;
    }
    if (win_f32_ok(dtype, g, d, dv)) return kWinBwdF32;
    return kWinBwdComposed;
}

}  // namespace fa
