// fa_windowed_fwd.hip — the windowed attention forward on gfx950 (fa_windowed.h has the
// geometry, the composed path and the plan).
//
// Kernels: win_fused (register gather, any rank, T <= 64), win_rows / win_rows1 (row
// scatter, four / one window per workgroup), win_rows1s (row shift, 1-3 windows per
// workgroup, and at 128 features), win_strip (eight windows of a window row per
// workgroup), win_rows_f32, and win_nan_uncovered for the pixels no window covers.
// Host: the forward launcher (launch_windowed_fwd), launch_window (fa_window /
// fa_unwindow), both workspace queries, and the definition of g_win_force_composed.
// Built with the scheduler's register-pressure trackers (Makefile).
#include "fa_windowed.h"

namespace fa {

// --------------------------------------------------------------------------
// Fused single-pass windowed forward (bf16 / fp16, T <= 64 tokens per window,
// d, dv <= 64): one wave per window, 4 windows per workgroup.
//
// The window's pixel indices go to a 64-entry LDS table; Q, K and V are then
// gathered straight from the image into MFMA fragment registers with buffer
// loads (the zero-padding pixels read as 0 through an out-of-range offset), so
// no window batch is ever materialised in HBM.  Scores are the transposed
// tile Sᵀ = K·Qᵀ (keys on accumulator rows, natural key order), softmax is
// exact per window (all keys in registers: max over 2 key blocks + one
// permlane swap), and Oᵀ = Vᵀ·Pᵀ takes P straight from the accumulator.
// Query blocks of 32 are processed one after the other to bound registers.
// Output: stride >= ws (no overlap) stores y directly (each covered pixel has
// exactly one owner window; uncovered pixels are NaN-filled separately), else
// the window outputs go to the workspace and win_fold sums / divides.
// --------------------------------------------------------------------------
template <class T, int D, int DV, int NKB, bool DIRECT>
__global__ __launch_bounds__(256, 2) void win_fused(const T* __restrict__ q, const T* __restrict__ k,
                                                    const T* __restrict__ v, T* __restrict__ out,
                                                    float* __restrict__ lo, float* __restrict__ mo,
                                                    WinDev g, int d, int dv, int batch, float scale,
                                                    float scale_log2) {
    typedef typename Frag8<T>::type F8;
    __shared__ int ptab[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int64_t wid = (int64_t)blockIdx.x * 4 + wave;       // global window id (w + L·b)
    const bool live = wid < (int64_t)g.L * batch;
    const int w = live ? (int)(wid % g.L) : 0;
    const int b = live ? (int)(wid / g.L) : 0;
    ptab[wave][lane] = (live && lane < g.T) ? win_pixel(g, w, lane) : -1;
    __syncthreads();
    const int* tab = ptab[wave];
    constexpr unsigned kOOB = 0x7FFFFFF0u;                      // past any slab: buffer load → 0
    const auto qrs = __builtin_amdgcn_make_buffer_rsrc((void*)(q + (int64_t)b * d * g.P), (short)0, d * g.P * 2, 0x00020000);
    const auto krs = __builtin_amdgcn_make_buffer_rsrc((void*)(k + (int64_t)b * d * g.P), (short)0, d * g.P * 2, 0x00020000);
    const auto vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(v + (int64_t)b * dv * g.P), (short)0, dv * g.P * 2, 0x00020000);
    auto off = [&](int f, int pix) -> unsigned { return pix < 0 ? kOOB : (unsigned)((f * g.P + pix) * 2); };
    auto ld = [&](__amdgpu_buffer_rsrc_t rs, unsigned o) -> T {
        return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b16(rs, o, 0, 0));
    };

    // K: A operand of Sᵀ (row = key kb·32 + r), V: A operand of Oᵀ (row = feature)
    F8 kf[NKB][D / 16], vf[DV / 32][NKB][2];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        const int pk = tab[kb * 32 + r];
#pragma unroll
        for (int s = 0; s < D / 16; ++s)
#pragma unroll
            for (int e = 0; e < 8; ++e) kf[kb][s][e] = ld(krs, off(16 * s + 8 * h + e, pk));
    }
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // B-operand k order of the accumulator: element j of half h ↔ row 16s + 8(j>>2) + 4h + (j&3)
            int pv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) pv[j] = tab[kb * 32 + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)];
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int j = 0; j < 8; ++j) vf[cb][kb][s][j] = ld(vrs, off(cb * 32 + r, pv[j]));
        }

    const int T_ = g.T;
#pragma unroll
    for (int qb = 0; qb < NKB; ++qb) {
        const int tq = qb * 32 + r;                 // this lane's query token
        const int pq = tab[tq];
        F8 qf[D / 16];
#pragma unroll
        for (int s = 0; s < D / 16; ++s)
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[s][e] = ld(qrs, off(16 * s + 8 * h + e, pq));
        f32x16 sa[NKB];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
            for (int x = 0; x < 16; ++x) sa[kb][x] = 0.0f;
#pragma unroll
            for (int s = 0; s < D / 16; ++s) sa[kb] = mfma32x32x16(kf[kb][s], qf[s], sa[kb]);
#pragma unroll
            for (int x = 0; x < 16; ++x)
                if (kb * 32 + acc_row(x, h) >= T_) sa[kb][x] = kNegInf;   // tokens past the window
        }
        float pm[4] = {kNegInf, kNegInf, kNegInf, kNegInf};
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) pm[x & 3] = vmax(pm[x & 3], sa[kb][x]);
        const float mt = swap_halves_max(vmax(vmax(pm[0], pm[1]), vmax(pm[2], pm[3])));
        const float mc = mt * scale_log2;
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
        F8 pf[NKB][2];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pr = exp2_fast(fmaf(sa[kb][x], scale_log2, -mc));
                ps[x & 3] += pr;
                pf[kb][x >> 3][x & 7] = (T)pr;
            }
        const float lt = swap_halves_sum((ps[0] + ps[1]) + (ps[2] + ps[3]));
        const float inv = 1.0f / lt;
        f32x16 oa[DV / 32];
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb) {
#pragma unroll
            for (int x = 0; x < 16; ++x) oa[cb][x] = 0.0f;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int s = 0; s < 2; ++s) oa[cb] = mfma32x32x16(vf[cb][kb][s], pf[kb][s], oa[cb]);
        }
        if (live && tq < T_) {
            if (h == 0) {
                const int64_t li = tq + (int64_t)T_ * wid;
                mo[li] = mt * scale;
                lo[li] = lt;
            }
            if constexpr (DIRECT) {
                if (pq >= 0) {
                    T* yb = out + (int64_t)b * dv * g.P + pq;
#pragma unroll
                    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                        for (int x = 0; x < 16; ++x) {
                            const int cc = cb * 32 + acc_row(x, h);
                            if (cc < dv) yb[(int64_t)cc * g.P] = (T)(oa[cb][x] * inv);
                        }
                }
            } else {
                T* ob = out + (int64_t)T_ * dv * wid + tq;      // (T, dv, L·B) window batch
#pragma unroll
                for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int cc = cb * 32 + acc_row(x, h);
                        if (cc < dv) ob[(int64_t)cc * T_] = (T)(oa[cb][x] * inv);
                    }
            }
        }
    }
}

// NaN for pixels no window covers (reference 0/0, Appendix A.7); DIRECT mode only
template <class T>
__global__ __launch_bounds__(256) void win_nan_uncovered(T* __restrict__ y, int dv, int64_t total, WinDev g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int pix = (int)(e % g.P);
    if (win_count(g, pix) == 0) y[e] = (T)__builtin_nanf("");
}

// --------------------------------------------------------------------------
// Row-staged single-pass windowed forward (2-D, stride >= ws, ws <= 8,
// bf16/fp16, d, dv <= 64, image width % 8 == 0).  The register-gather kernel
// above is texture-addresser bound (2-byte gathers across 64 feature planes:
// profiles/r01_windowed_ta_counters.txt).  Here a workgroup owns 4 adjacent
// windows of one window row; lanes load IMAGE-ALIGNED 16-byte chunks along
// x (never straddling a row, no shifts, no negative offsets) and scatter the
// pixels into per-window token slots in LDS (slot = 8·ty + tx, the dense
// forward's swizzled [feature][slot] images).  Features stream in chunks (16
// for q, k — Sᵀ accumulates in registers across chunks; 32 for v), so the LDS
// footprint is one chunk.  Out-of-image pixels and padding slots stay zero
// (zero-filled image): the reference's zero padding.
// --------------------------------------------------------------------------
template <class T, int D, int DV>
__global__ __launch_bounds__(256, 2) void win_rows(const T* __restrict__ q, const T* __restrict__ k,
                                                   const T* __restrict__ v, T* __restrict__ out,
                                                   float* __restrict__ lo, float* __restrict__ mo,
                                                   WinDev g, int d, int dv, int batch, int ngx,
                                                   float scale, float scale_log2) {
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    constexpr int NWIN = 4, NTH = 256;
    constexpr int FQ = D < 32 ? D : 32, FV = 32;              // feature chunk: q/k, v
    constexpr int KROW = 128, VROW = 144;
    constexpr int QKIMG = FQ * KROW;                           // one window, one tensor, one q/k chunk
    constexpr int VIMG = FV * VROW;
    constexpr int REGION = (2 * NWIN * QKIMG > NWIN * VIMG) ? 2 * NWIN * QKIMG : NWIN * VIMG;
    __shared__ __attribute__((aligned(16))) char smem[REGION];
    auto kswz = [](int f) { return ((f >> 1) & 1) << 1; };

    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W_ = g.S[0], H_ = g.S[1], P_ = g.P, ws = g.ws, st = g.stride;
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int gx = bid % ngx; bid /= ngx;
    const int wy = bid % g.O[1];
    const int b = bid / g.O[1];
    const int wx0 = gx * NWIN;
    const int nwin = min(NWIN, g.O[0] - wx0);
    const int xs = wx0 * st - g.pad;                           // x of window 0, token 0
    const int xe = (wx0 + nwin - 1) * st - g.pad + ws;         // one past the last window's pixels
    const int y0 = wy * st - g.pad;
    const int c_lo = max(xs, 0) >> 3, c_hi = (min(xe, W_) + 7) >> 3;   // image-aligned 8-pixel chunks
    const int ncx = c_hi - c_lo;
    const int ylo = max(y0, 0), yhi = min(y0 + ws, H_);
    const int nrow = max(yhi - ylo, 0);

    // zero the staging region, then scatter nf features (from feature f0) of
    // tensor src into image base + wl·imgbytes with the given row layout
    auto zero_region = [&]() {
        for (int o = tid * 16; o < REGION; o += NTH * 16) *(u32x4*)(smem + o) = u32x4{0u, 0u, 0u, 0u};
    };
    auto stage = [&](const T* src, int C, int f0, int nf, int base, int imgbytes, bool vlayout) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(src + (int64_t)b * C * P_), (short)0, C * P_ * 2, 0x00020000);
        const int items = nf * nrow * ncx;
        for (int it = tid; it < items; it += NTH) {
            const int cx = it % ncx;
            const int rest = it / ncx;
            const int yy = rest % nrow, fl = rest / nrow;
            const int f = f0 + fl, y = ylo + yy, x8 = (c_lo + cx) * 8;
            u32x4 val = u32x4{0u, 0u, 0u, 0u};
            if (f < C) val = __builtin_amdgcn_raw_buffer_load_b128(rs, (f * P_ + y * W_ + x8) * 2, 0, 0);
            const int ty = y - y0;
            // (window, token column) of the chunk's first pixel; consecutive pixels
            // then advance incrementally (tx < 0: left of window 0)
            const int rel = x8 - xs;
            int wl = rel >= 0 ? rel / st : 0;
            int tx = rel >= 0 ? rel - wl * st : rel;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (tx >= 0 && tx < ws && wl < nwin) {
                    const unsigned wd = val[e >> 1];
                    const unsigned short px = (unsigned short)((e & 1) ? (wd >> 16) : (wd & 0xFFFFu));
                    const int slot = ty * 8 + tx;
                    const int o = vlayout ? fl * VROW + slot * 2
                                          : fl * KROW + (((slot >> 4) ^ kswz(fl)) * 32) + (slot & 15) * 2;
                    *(unsigned short*)(smem + base + wl * imgbytes + o) = px;
                }
                if (++tx == st) { tx = 0; ++wl; }
            }
        }
    };

    const int g4 = lane >> 4, kh = g4 & 1, qq = (lane & 15) >> 2, pp = lane & 3;
    const int sig = (pp == 1) ? 2 : (pp == 2) ? 1 : pp;
    f32x16 sa[2][2];                                           // [key block][query block]
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int x = 0; x < 16; ++x) sa[kb][qb][x] = 0.0f;

    // ---- Sᵀ = K·Qᵀ over feature chunks.  Every chunk writes the same slot
    //      positions (pixel validity does not depend on the feature), so the
    //      padding slots stay zero after one zero-fill per layout. ----
    zero_region();
    __syncthreads();
    for (int f0 = 0; f0 < D; f0 += FQ) {
        stage(q, d, f0, FQ, 0, QKIMG, false);
        stage(k, d, f0, FQ, NWIN * QKIMG, QKIMG, false);
        __syncthreads();
        if (wave < nwin) {
            const char* qimg = smem + wave * QKIMG;
            const char* kimg = smem + NWIN * QKIMG + wave * QKIMG;
#pragma unroll
            for (int s16 = 0; s16 < FQ / 16; ++s16) {          // 16-feature k-steps of the chunk
                F8 kf[2], qf[2];
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    const int o = (16 * s16 + 8 * h + qq) * KROW + (((blk * 2 + kh) ^ kswz(qq)) * 32);
                    kf[blk] = __builtin_shufflevector(__builtin_bit_cast(F4, ds_read_tr16(kimg + o + 8 * sig)),
                                                      __builtin_bit_cast(F4, ds_read_tr16(kimg + o + 8 * sig + 4 * KROW)), 0, 1, 2, 3, 4, 5, 6, 7);
                    qf[blk] = __builtin_shufflevector(__builtin_bit_cast(F4, ds_read_tr16(qimg + o + 8 * pp)),
                                                      __builtin_bit_cast(F4, ds_read_tr16(qimg + o + 8 * pp + 4 * KROW)), 0, 1, 2, 3, 4, 5, 6, 7);
                }
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb) sa[kb][qb] = mfma32x32x16(kf[kb], qf[qb], sa[kb][qb]);
            }
        }
        __syncthreads();
    }

    // ---- exact softmax per query (keys: the window's ws x ws real slots) ----
    F8 pf[2][2][2];                                            // [query block][key block][half]
    float mt[2], lt[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int kt = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
                if ((kt & 7) >= ws || (kt >> 3) >= ws) sa[kb][qb][x] = kNegInf;
            }
        float pm[4] = {sa[0][qb][0], sa[0][qb][1], sa[0][qb][2], sa[0][qb][3]};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = (kb == 0 ? 4 : 0); x < 16; ++x) pm[x & 3] = vmax(pm[x & 3], sa[kb][qb][x]);
        mt[qb] = swap_halves_max(vmax(vmax(pm[0], pm[1]), vmax(pm[2], pm[3])));
        const float mc = mt[qb] * scale_log2;
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pr = exp2_fast(fmaf(sa[kb][qb][x], scale_log2, -mc));
                ps[x & 3] += pr;
                pf[qb][kb][x >> 3][x & 7] = (T)pr;
            }
        lt[qb] = swap_halves_sum((ps[0] + ps[1]) + (ps[2] + ps[3]));
    }

    // ---- Oᵀ = Vᵀ·Pᵀ over feature chunks of 32, stored straight to the pixels ----
    const int wx = wx0 + wave;
    const int64_t wid = (int64_t)(wx + g.O[0] * wy) + (int64_t)g.L * b;
    zero_region();                                             // v layout (last barrier of the q/k loop passed)
    __syncthreads();
    for (int c0 = 0; c0 < DV; c0 += FV) {
        stage(v, dv, c0, FV, 0, VIMG, true);
        __syncthreads();
        if (wave < nwin) {
            const char* vimg = smem + wave * VIMG + r * VROW + 16 * h;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                f32x16 oa;
#pragma unroll
                for (int x = 0; x < 16; ++x) oa[x] = 0.0f;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2)
                        oa = mfma32x32x16(*(const F8*)(vimg + (kb * 32 + 16 * s2) * 2), pf[qb][kb][s2], oa);
                const int qslot = qb * 32 + r, qtx = qslot & 7, qty = qslot >> 3;
                const int px = wx * st - g.pad + qtx, py = y0 + qty;
                if (qtx < ws && qty < ws && px >= 0 && px < W_ && py >= 0 && py < H_) {
                    const float inv = 1.0f / lt[qb];
                    T* yb = out + (int64_t)b * dv * P_ + (int64_t)py * W_ + px;
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int cc = c0 + acc_row(x, h);
                        if (cc < dv) yb[(int64_t)cc * P_] = (T)(oa[x] * inv);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (wave < nwin && h == 0) {
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int qslot = qb * 32 + r, qtx = qslot & 7, qty = qslot >> 3;
            if (qtx < ws && qty < ws) {
                const int64_t li = qty * ws + qtx + (int64_t)g.T * wid;
                mo[li] = mt[qb] * scale;
                lo[li] = lt[qb];
            }
        }
    }
}

// --------------------------------------------------------------------------
// Row-staged kernel, one window per workgroup (small launches: B = 1 of
// configs[2] has 324 windows, so four windows per workgroup would leave most
// CUs idle).  q, k and v are staged in ONE phase: every thread issues all its
// image-aligned 16-B row loads before it scatters any of them (items decoded
// with fixed strides — 2 chunks per row, 8 rows per feature — so out-of-window
// items read an out-of-range offset, i.e. 0, and are skipped at the scatter),
// so the workgroup pays one HBM round trip instead of one per item.  The 4
// waves split the window: wave w computes query block (w & 1) and the 32-wide
// v feature chunk (w >> 1).
// --------------------------------------------------------------------------
template <class T, int D, int DV>
__global__ __launch_bounds__(256) void win_rows1(const T* __restrict__ q, const T* __restrict__ k,
                                                 const T* __restrict__ v, T* __restrict__ out,
                                                 float* __restrict__ lo, float* __restrict__ mo,
                                                 WinDev g, int d, int dv, float scale, float scale_log2) {
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    constexpr int NTH = 256, KROW = 128, VROW = 144;
    constexpr int QIMG = D * KROW, VIMG = DV * VROW, REGION = 2 * QIMG + VIMG;
    constexpr int NBQ = D * 16 / NTH, NBV = DV * 16 / NTH;    // items per thread: feature x 8 rows x 2 chunks
    static_assert(D * 16 % NTH == 0 && DV * 16 % NTH == 0, "item split");
    __shared__ __attribute__((aligned(16))) char smem[REGION];
    auto kswz = [](int f) { return ((f >> 1) & 1) << 1; };

    FA_STAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W_ = g.S[0], H_ = g.S[1], P_ = g.P, ws = g.ws, st = g.stride;
    const int bid = blockIdx.x;
    const int wx = bid % g.O[0], wy = (bid / g.O[0]) % g.O[1], b = bid / (g.O[0] * g.O[1]);
    const int xs = wx * st - g.pad, y0 = wy * st - g.pad;
    const int c_lo = max(xs, 0) >> 3;
    const int ncx = max(((min(xs + ws, W_) + 7) >> 3) - c_lo, 0);
    const int ylo = max(y0, 0), nrow = max(min(y0 + ws, H_) - ylo, 0);

    // item it -> (feature fl = it >> 4, row yy = (it >> 1) & 7, chunk cx = it & 1)
    auto item_off = [&](int it, int C) {
        const int cx = it & 1, yy = (it >> 1) & 7, fl = it >> 4;
        const bool ok = cx < ncx && yy < nrow && fl < C;
        return ok ? (fl * P_ + (ylo + yy) * W_ + (c_lo + cx) * 8) * 2 : 0x7FFFFFF0;
    };
    const auto qrs = slab_rsrc(q + (int64_t)b * d * P_, (uint32_t)(d * P_ * 2));
    const auto krs = slab_rsrc(k + (int64_t)b * d * P_, (uint32_t)(d * P_ * 2));
    const auto vrs = slab_rsrc(v + (int64_t)b * dv * P_, (uint32_t)(dv * P_ * 2));
    u32x4 rq[NBQ], rk[NBQ], rv[NBV];
#pragma unroll
    for (int j = 0; j < NBQ; ++j) {
        const int o = item_off(tid + NTH * j, d);
        rq[j] = __builtin_amdgcn_raw_buffer_load_b128(qrs, o, 0, 0);
        rk[j] = __builtin_amdgcn_raw_buffer_load_b128(krs, o, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NBV; ++j) rv[j] = __builtin_amdgcn_raw_buffer_load_b128(vrs, item_off(tid + NTH * j, dv), 0, 0);

    for (int o = tid * 16; o < REGION; o += NTH * 16) *(u32x4*)(smem + o) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    FA_STAMP(1);
    auto scatter = [&](const u32x4& val, int it, int C, char* base, bool vlayout) {
        const int cx = it & 1, yy = (it >> 1) & 7, fl = it >> 4;
        if (!(cx < ncx && yy < nrow && fl < C)) return;
        const int ty = ylo + yy - y0;
        int tx = (c_lo + cx) * 8 - xs;
#pragma unroll
        for (int e = 0; e < 8; ++e, ++tx) {
            if (tx >= 0 && tx < ws) {
                const unsigned wd = val[e >> 1];
                const unsigned short px = (unsigned short)((e & 1) ? (wd >> 16) : (wd & 0xFFFFu));
                const int slot = ty * 8 + tx;
                const int o = vlayout ? fl * VROW + slot * 2 : fl * KROW + (((slot >> 4) ^ kswz(fl)) * 32) + (slot & 15) * 2;
                *(unsigned short*)(base + o) = px;
            }
        }
    };
#pragma unroll
    for (int j = 0; j < NBQ; ++j) {
        scatter(rq[j], tid + NTH * j, d, smem, false);
        scatter(rk[j], tid + NTH * j, d, smem + QIMG, false);
    }
#pragma unroll
    for (int j = 0; j < NBV; ++j) scatter(rv[j], tid + NTH * j, dv, smem + 2 * QIMG, true);
    __syncthreads();
    FA_STAMP(2);

    // ---- Sᵀ = K·Qᵀ for this wave's query block ----
    const int qb = wave & 1, vc = wave >> 1;
    const int g4 = lane >> 4, kh = g4 & 1, qq = (lane & 15) >> 2, pp = lane & 3;
    const int sig = (pp == 1) ? 2 : (pp == 2) ? 1 : pp;
    f32x16 sa[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int x = 0; x < 16; ++x) sa[kb][x] = 0.0f;
#pragma unroll
    for (int s16 = 0; s16 < D / 16; ++s16) {
        const int orow = (16 * s16 + 8 * h + qq) * KROW;
        F8 kf[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const char* a = smem + QIMG + orow + (((blk * 2 + kh) ^ kswz(qq)) * 32) + 8 * sig;
            kf[blk] = __builtin_shufflevector(__builtin_bit_cast(F4, ds_read_tr16(a)),
                                              __builtin_bit_cast(F4, ds_read_tr16(a + 4 * KROW)), 0, 1, 2, 3, 4, 5, 6, 7);
        }
        const char* a = smem + orow + (((qb * 2 + kh) ^ kswz(qq)) * 32) + 8 * pp;
        const F8 qf = __builtin_shufflevector(__builtin_bit_cast(F4, ds_read_tr16(a)),
                                              __builtin_bit_cast(F4, ds_read_tr16(a + 4 * KROW)), 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) sa[kb] = mfma32x32x16(kf[kb], qf, sa[kb]);
    }

    FA_STAMP(3);
    // ---- exact softmax per query (keys: the window's ws x ws real slots) ----
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int kt = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
            if ((kt & 7) >= ws || (kt >> 3) >= ws) sa[kb][x] = kNegInf;
        }
    const float mt = swap_halves_max(lane_max<2>(sa));
    const float mc = mt * scale_log2;
    float ps[4] = {0.f, 0.f, 0.f, 0.f};
    F8 pf[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const float pr = exp2_fast(fmaf(sa[kb][x], scale_log2, -mc));
            ps[x & 3] += pr;
            pf[kb][x >> 3][x & 7] = (T)pr;
        }
    const float lt = swap_halves_sum((ps[0] + ps[1]) + (ps[2] + ps[3]));

    FA_STAMP(4);
    // ---- Oᵀ = Vᵀ·Pᵀ for this wave's 32-feature chunk, stored straight to the pixels ----
    const int qslot = qb * 32 + r, qtx = qslot & 7, qty = qslot >> 3;
    if (vc < DV / 32) {
        const char* vimg = smem + 2 * QIMG + (vc * 32 + r) * VROW + 16 * h;
        f32x16 oa;
#pragma unroll
        for (int x = 0; x < 16; ++x) oa[x] = 0.0f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) oa = mfma32x32x16(*(const F8*)(vimg + (kb * 32 + 16 * s2) * 2), pf[kb][s2], oa);
        const int px = xs + qtx, py = y0 + qty;
        if (qtx < ws && qty < ws && px >= 0 && px < W_ && py >= 0 && py < H_) {
            const float inv = 1.0f / lt;
            T* yb = out + (int64_t)b * dv * P_ + (int64_t)py * W_ + px;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int cc = vc * 32 + acc_row(x, h);
                if (cc < dv) yb[(int64_t)cc * P_] = (T)(oa[x] * inv);
            }
        }
    }
    if (vc == 0 && h == 0 && qtx < ws && qty < ws) {
        const int64_t wid = (int64_t)(wx + g.O[0] * wy) + (int64_t)g.L * b;
        const int64_t li = qty * ws + qtx + (int64_t)g.T * wid;
        mo[li] = mt * scale;
        lo[li] = lt;
    }
    FA_STAMP(5);
}

// --------------------------------------------------------------------------
// Row-SHIFT staging, ws <= 7 (the default row-staged kernel for ws <= 7 at
// every launch size; two windows per workgroup, below).  A window row of <= 7 pixels always
// fits in the 8 pixels that start at the dword-aligned pixel
//   a = clamp(xs & ~1, 0, W - 8),
// so every (feature, window row) item is ONE 16-B buffer load, a wave-uniform
// shift by sh = xs - a pixels (dword selects + v_alignbyte), a uniform mask
// (slot < ws, pixel inside the image) and ONE ds_write_b128 into the dense
// kernel's LDS layouts: 6 loads and 6 LDS writes per thread, no zero-fill and
// no 2-byte scatter (the scatter kernel above spent ~30 % of its time there,
// tools/exp/win_stamp.py).  Items cover all 8 slot rows and all D features,
// so padding slots are written as zeros.  Workgroups are dealt to XCDs in
// contiguous window runs (xcd_remap), so horizontally adjacent windows, which
// share cache lines, hit one XCD's L2: configs[2] B=1 12.2 -> 6.8 us.  Two
// windows per workgroup (their loads coalesce, below) took B=32 97 -> 83 us.
// --------------------------------------------------------------------------
// NWIN horizontally adjacent windows per workgroup (4 waves each).  Staging items
// interleave the windows on adjacent lanes, so the NWIN 16-B row loads of one
// (feature, row) — 14 B apart at stride 7 — fall in the same cache line and
// coalesce in the texture path (NWIN = 1: the wave-uniform shift above).
template <class T, int D, int DV, int NWIN>
__global__ __launch_bounds__(256 * NWIN) void win_rows1s(const T* __restrict__ q, const T* __restrict__ k,
                                                         const T* __restrict__ v, T* __restrict__ out,
                                                         float* __restrict__ lo, float* __restrict__ mo,
                                                         WinDev g, int d, int dv, int64_t nwin_total,
                                                         float scale, float scale_log2) {
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    constexpr int NTH = 256 * NWIN, KROW = 128, VROW = 144;
    constexpr int QIMG = D * KROW, VIMG = DV * VROW, REGION = 2 * QIMG + VIMG;
    constexpr int NIQ = D * 8 / 256, NIV = DV * 8 / 256;    // items per thread: window x feature x 8 slot rows
    static_assert(D * 8 % 256 == 0 && DV * 8 % 256 == 0, "item split");
    __shared__ __attribute__((aligned(16))) char smem[NWIN * REGION];
    auto kswz = [](int f) { return ((f >> 1) & 1) << 1; };

    FA_STAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W_ = g.S[0], H_ = g.S[1], P_ = g.P, ws = g.ws, st = g.stride;
    const int64_t wid0 = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * NWIN;
    const int nperimg = g.O[0] * g.O[1];
    struct Win { int wx, wy, b, xs, y0, ax; bool ok; };
    auto win_of = [&](int wl) {
        Win w;
        const int id = (int)wid0 + wl;   // 32-bit: the host keeps L·B < 2^31 on this path
        w.ok = id < (int)nwin_total;
        const int idc = w.ok ? id : 0;
        w.b = idc / nperimg;
        const int rem = idc - w.b * nperimg;
        w.wy = rem / g.O[0];
        w.wx = rem - w.wy * g.O[0];
        w.xs = w.wx * st - g.pad;
        w.y0 = w.wy * st - g.pad;
        w.ax = min(max(w.xs & ~1, 0), W_ - 8);
        return w;
    };

    // item it -> (window it % NWIN, feature f = (it / NWIN) >> 3, slot row yy = (it / NWIN) & 7)
    // descriptors over the images the workgroup's windows can span: NWIN of them when
    // every image holds one window, clamped to the batch; item offsets are relative to
    // image b0 (32-bit: win_fwd_plan keeps NWIN images' bytes below 2^31)
    const int b0 = win_of(0).b;
    const int nimg = min(NWIN, (int)nwin_total / nperimg - b0);
    // every item of a lane belongs to the same window (NTH is a multiple of NWIN)
    const int wl_me = NWIN == 1 ? 0 : (int)(tid % NWIN);
    const Win wme = win_of(wl_me);
    auto item_off = [&](int it, int C) {
        const Win& w = wme;
        const int rest = NWIN == 1 ? it : it / NWIN, yy = rest & 7, f = rest >> 3, y = w.y0 + yy;
        const bool ok = w.ok && yy < ws && y >= 0 && y < H_ && f < C;
        if (FA_WIN_ABL & 2) return 0;
        return ok ? (((w.b - b0) * C + f) * P_ + y * W_ + w.ax) * 2 : 0x7FFFFFF0;
    };
    const auto qrs = slab_rsrc(q + (int64_t)b0 * d * P_, (uint32_t)(nimg * d * P_ * 2));
    const auto krs = slab_rsrc(k + (int64_t)b0 * d * P_, (uint32_t)(nimg * d * P_ * 2));
    const auto vrs = slab_rsrc(v + (int64_t)b0 * dv * P_, (uint32_t)(nimg * dv * P_ * 2));
    u32x4 rq[NIQ], rk[NIQ], rv[NIV];
#pragma unroll
    for (int j = 0; j < NIQ; ++j) {
        const int o = item_off(tid + NTH * j, d);
        rq[j] = __builtin_amdgcn_raw_buffer_load_b128(qrs, o, 0, 0);
        rk[j] = __builtin_amdgcn_raw_buffer_load_b128(krs, o, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NIV; ++j) rv[j] = __builtin_amdgcn_raw_buffer_load_b128(vrs, item_off(tid + NTH * j, dv), 0, 0);

    // staging of one item: shift into slots, mask (slot < ws, pixel inside the image).
    // A lane's window, masks and shift are computed once.  Round 5: when no lane of the wave
    // shifts by 2 pixels or more (every window away from the image's left and right
    // edges: ax = xs rounded down to even, so the shift is 0 or 1), the shift is one
    // v_alignbyte per dword with the lane's byte shift instead of five runtime dword
    // picks (the staging was ~400 VALU, 163 of them v_cndmask, per lane before the barrier).
    unsigned mask_me[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t0 = 2 * j, t1 = 2 * j + 1;
        const bool v0 = t0 < ws && wme.xs + t0 >= 0 && wme.xs + t0 < W_;
        const bool v1 = t1 < ws && wme.xs + t1 >= 0 && wme.xs + t1 < W_;
        mask_me[j] = (v0 ? 0x0000FFFFu : 0u) | (v1 ? 0xFFFF0000u : 0u);
    }
    const int sh_me = wme.xs - wme.ax;
    const bool near_shift = NWIN > 1 && __builtin_amdgcn_ballot_w64((sh_me >> 1) != 0) == 0;
    const unsigned ab_me = (sh_me & 1) ? 2u : 0u;
    auto stage = [&](auto fast, const u32x4& val, int it, char* img, bool vlayout) {
        const int rest = NWIN == 1 ? it : it / NWIN, yy = rest & 7, f = rest >> 3;
        u32x4 o;
        if constexpr (NWIN == 1) {
            o = shift_row(val, sh_me, mask_me);
        } else if constexpr (decltype(fast)::value) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = __builtin_amdgcn_alignbyte(j < 3 ? val[j + 1] : 0u, val[j], ab_me) & mask_me[j];
        } else {
            o = shift_row_lane(val, sh_me, mask_me);
        }
        char* base = smem + wl_me * REGION + (img - smem);
        const int off = vlayout ? f * VROW + yy * 16 : f * KROW + (((yy >> 1) ^ kswz(f)) * 32) + (yy & 1) * 16;
        *(u32x4*)(base + off) = o;
    };
    // V staged before the one barrier too (round 5): its loads were issued with Q's and
    // K's, and staging it after the softmax put a second barrier and the staging on the
    // path to the stores
    auto stage_all = [&](auto fast) {
#pragma unroll
        for (int j = 0; j < NIQ; ++j) {
            stage(fast, rq[j], tid + NTH * j, smem, false);
            stage(fast, rk[j], tid + NTH * j, smem + QIMG, false);
        }
#pragma unroll
        for (int j = 0; j < NIV; ++j) stage(fast, rv[j], tid + NTH * j, smem + 2 * QIMG, true);
    };
    if (near_shift) stage_all(std::true_type{});
    else stage_all(std::false_type{});
    lds_barrier();
    FA_STAMP(2);

    // ---- this wave's window, query block and v chunk ----
    const int wl = wave >> 2;
    const Win w = win_of(wl);
    char* const wsm = smem + wl * REGION;
    const int qb = wave & 1, vc = (wave >> 1) & 1;
    const int g4 = lane >> 4, kh = g4 & 1, qq = (lane & 15) >> 2, pp = lane & 3;
    const int sig = (pp == 1) ? 2 : (pp == 2) ? 1 : pp;
    f32x16 sa[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int x = 0; x < 16; ++x) sa[kb][x] = 0.0f;
#pragma unroll
    for (int s16 = 0; s16 < D / 16; ++s16) {
        const int orow = (16 * s16 + 8 * h + qq) * KROW;
        F8 kf[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const char* a = wsm + QIMG + orow + (((blk * 2 + kh) ^ kswz(qq)) * 32) + 8 * sig;
            kf[blk] = __builtin_shufflevector(__builtin_bit_cast(F4, ds_read_tr16(a)),
                                              __builtin_bit_cast(F4, ds_read_tr16(a + 4 * KROW)), 0, 1, 2, 3, 4, 5, 6, 7);
        }
        const char* a = wsm + orow + (((qb * 2 + kh) ^ kswz(qq)) * 32) + 8 * pp;
        const F8 qf = __builtin_shufflevector(__builtin_bit_cast(F4, ds_read_tr16(a)),
                                              __builtin_bit_cast(F4, ds_read_tr16(a + 4 * KROW)), 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) sa[kb] = mfma32x32x16(kf[kb], qf, sa[kb]);
    }
    FA_STAMP(3);

    // ---- exact softmax per query (keys: the window's ws x ws real slots) ----
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int kt = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
            if ((kt & 7) >= ws || (kt >> 3) >= ws) sa[kb][x] = kNegInf;
        }
    const float mt = swap_halves_max(lane_max<2>(sa));
    const float mc = mt * scale_log2;
    float ps[4];
    F8 pf[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const float pr = exp2_fast(fmaf(sa[kb][x], scale_log2, -mc));
            if (kb == 0 && x < 4) ps[x] = pr; else ps[x & 3] += pr;
            pf[kb][x >> 3][x & 7] = (T)pr;
        }
    const float lt = swap_halves_sum((ps[0] + ps[1]) + (ps[2] + ps[3]));
    FA_STAMP(4);

    // ---- Oᵀ = Vᵀ·Pᵀ for this wave's 32-feature chunk, stored straight to the pixels ----
    const int qslot = qb * 32 + r, qtx = qslot & 7, qty = qslot >> 3;
#pragma unroll
    for (int cv = vc; cv < DV / 32 && w.ok; cv += 2) {   // DV = 128: chunks vc and vc + 2
        const char* vimg = wsm + 2 * QIMG + (cv * 32 + r) * VROW + 16 * h;
        f32x16 oa;
#pragma unroll
        for (int x = 0; x < 16; ++x) oa[x] = 0.0f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) oa = mfma32x32x16(*(const F8*)(vimg + (kb * 32 + 16 * s2) * 2), pf[kb][s2], oa);
        const int px = w.xs + qtx, py = w.y0 + qty;
        if (qtx < ws && qty < ws && px >= 0 && px < W_ && py >= 0 && py < H_) {
            const float inv = 1.0f / lt;
            T* yb = out + (int64_t)w.b * dv * P_ + (int64_t)py * W_ + px;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int cc = cv * 32 + acc_row(x, h);
                if (cc < dv && (!(FA_WIN_ABL & 1) || oa[x] == 1234.5f)) yb[(int64_t)cc * P_] = (T)(oa[x] * inv);
            }
        }
    }
    if (vc == 0 && h == 0 && qtx < ws && qty < ws && w.ok) {
        const int64_t wid = (int64_t)(w.wx + g.O[0] * w.wy) + (int64_t)g.L * w.b;
        const int64_t li = qty * ws + qtx + (int64_t)g.T * wid;
        mo[li] = mt * scale;
        lo[li] = lt;
    }
    FA_STAMP(5);
}

// --------------------------------------------------------------------------
// Strip kernel: NS = 8 horizontally adjacent windows of one window row per
// workgroup, one window per wave (bf16/f16, 2-D, stride == ws <= 7, d, dv <= 64,
// width % 8 == 0, q, k, v, y 16-B aligned; the default for large launches).
//
// Why: the per-window kernels move q, k, v and y in 14-B window-row segments, so
// every load / store instruction touches ~64 cache lines that ~9 windows of other
// workgroups share: ~14 M L2 requests of ~20 B per configs[2] B = 32 call
// (r02_windowed_fwd_pmc.txt), which sets their pace, not HBM.  Here the eight
// windows' rows sit side by side in every DMA instruction (8 lanes x 16 B per
// cache line) and y leaves as whole 16-B chunks of the strip's 56 contiguous
// pixels.  The first strip holds k0 <= 8 windows, k0 chosen so that every strip
// boundary falls on a 16-B chunk boundary (k0 * ws = pad mod 8, solvable for odd
// ws): then no chunk is shared with a neighbour strip.  When no k0 aligns them
// (even ws), the two strip ends are 2-B stores.
//
// Channels are streamed so the eight windows fit in LDS:
//   * two 32-KB buffers (64 KB: two workgroups per CU) take the image loads in
//     turn, each issued as soon as its buffer is free: Q / K chunks of 16 features
//     ([16 f][8 slot rows][8 windows] x 16 B, 16 KB each), then the two 32-feature
//     V chunks ([32 f][8][8] x 16 B), which land under the last QKᵀ steps;
//     Sᵀ = K·Qᵀ accumulates over the chunks (one 16-deep MFMA step per chunk,
//     64 x 64 slots per window, 2 x 2 blocks);
//   * y: per V chunk, each wave writes its window's normalised O into a strip
//     image [32 f][8 rows][64 px] over that V chunk, then the workgroup stores it
//     row by row.
// Slots are ROTATED: slot (yy, sx) of window w holds pixel
// (ax_w + sx, y0 + yy), ax_w = clamp(xs_w & ~1, 0, W - 8); padding columns enter
// the softmax analytically (npad zero keys), padding rows load as zeros.
// LDS-DMA writes lane-linearly, so the swizzles are applied through each lane's
// choice of (window, slot row):
//   Q / K: window position w ^ (f & 7) ^ ((c >> 1) & 1) << 2  (ds_read_b64_tr_b16: f & 4 is fixed per
//          instruction, so this is the conflict-free (f & 3, c) pattern; the 16-B row reads of the
//          strip backward's register stash, 16 features at a time, then meet 2-way conflicts, not 4);
//   V    : slot-row position c ^ ((f >> 3) & 1), window position w ^ (f & 7)  (ds_read_b128, conflict-free).
// --------------------------------------------------------------------------
template <class T, int D, int DV>
__global__ __launch_bounds__(512, 2) void win_strip(const T* __restrict__ q, const T* __restrict__ k,
                                                    const T* __restrict__ v, T* __restrict__ out,
                                                    float* __restrict__ lo, float* __restrict__ mo, WinDev g, int d,
                                                    int dv, int nsx, int k0, int nwg, float scale, float scale_log2) {
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    static_assert(D % 16 == 0 && D <= 64 && DV % 32 == 0 && DV <= 64, "head dims");
    constexpr int NQC = D / 16, NVC = DV / 32;       // Q/K chunks of 16 features, V chunks of 32
    constexpr int NLD = NQC + NVC;                   // image loads, alternating between the two buffers
    constexpr int BUF = 32768;
    // two separate LDS objects (not one array): the compiler's LDS-DMA wait tracking tells
    // them apart, so a read of one buffer does not wait for the DMA into the other
    __shared__ __attribute__((aligned(16))) char sbuf0[BUF], sbuf1[BUF];   // 64 KB: two workgroups per CU
    auto bufp = [&](int i) __attribute__((always_inline)) { return (i & 1) ? sbuf1 : sbuf0; };

    FA_STAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W_ = g.S[0], H_ = g.S[1], P_ = g.P, ws = g.ws, st = g.stride, nwx = g.O[0];
    const int lid = xcd_remap(blockIdx.x, nwg);
    const int sxi = lid % nsx, t0 = lid / nsx, wy = t0 % g.O[1], b = t0 / g.O[1];
    const int wx0 = sxi == 0 ? 0 : k0 + (sxi - 1) * kStripW, y0 = wy * st - g.pad;
    const int nvalid = min(sxi == 0 ? k0 : kStripW, nwx - wx0);
    auto ax_of = [&](int w) { return min(max(((wx0 + w) * st - g.pad) & ~1, 0), W_ - 8); };
    const auto qrs = slab_rsrc(q + (int64_t)b * d * P_, (uint32_t)(d * P_ * 2));
    const auto krs = slab_rsrc(k + (int64_t)b * d * P_, (uint32_t)(d * P_ * 2));
    const auto vrs = slab_rsrc(v + (int64_t)b * dv * P_, (uint32_t)(dv * P_ * 2));

    // one DMA instruction = one feature row f of an image: lane -> (slot row, window).
    // (buffer descriptors are passed, not captured: a lambda capturing one made
    // hipcc's host pass drop the kernel's launch stub, with no diagnostic)
    auto dma_qk = [&](__amdgpu_buffer_rsrc_t rs, char* img, int fl, int fg) {
        const int pc = lane >> 3, pw = lane & 7;
        const int w = pw ^ sqk_swz(fl, pc), y = y0 + pc;
        const bool ok = w < nvalid && pc < ws && y >= 0 && y < H_ && fg < d;
        const int off = ok ? (fg * P_ + y * W_ + ax_of(w)) * 2 : 0x7FFFFFF0;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(img + fl * 1024), 16,
                                                 off, 0, 0, 0);
    };
    auto dma_v = [&](__amdgpu_buffer_rsrc_t rs, char* img, int fl, int fg) {
        const int c = (lane >> 3) ^ ((fl >> 3) & 1), w = (lane & 7) ^ (fl & 7), y = y0 + c;
        const bool ok = w < nvalid && c < ws && y >= 0 && y < H_ && fg < dv;
        const int off = ok ? (fg * P_ + y * W_ + ax_of(w)) * 2 : 0x7FFFFFF0;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(img + fl * 1024), 16,
                                                 off, 0, 0, 0);
    };
    // image load i (QK chunk i, then V chunk i - NQC) into buffer i & 1: 32 DMA
    // instructions (one feature row each), 4 per wave
    auto issue = [&](__amdgpu_buffer_rsrc_t qr, __amdgpu_buffer_rsrc_t kr, __amdgpu_buffer_rsrc_t vr, int i) {
        char* buf = bufp(i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rr = j * 8 + wave;                  // 0..31
            if (i < NQC) {
                if (rr < 16) dma_qk(qr, buf, rr, i * 16 + rr);
                else dma_qk(kr, buf + 16384, rr - 16, i * 16 + rr - 16);
            } else {
                dma_v(vr, buf, rr, (i - NQC) * 32 + rr);
            }
        }
    };
    issue(qrs, krs, vrs, 0);
    issue(qrs, krs, vrs, 1);

    // ---- this wave's window ----
    const int wl = wave;
    const bool wok = wl < nvalid;
    const int wx = wx0 + wl, xs = wx * st - g.pad, ax = ax_of(wl);
    const int c0 = xs - ax, c1 = c0 + ws;
    const int ncols = min(c1, 8) - max(c0, 0);
    const float npad = (float)((ws - ncols) * ws);       // padding-column tokens (zero keys)
    const int g4 = lane >> 4, kh = g4 & 1, qq = (lane & 15) >> 2, pp = lane & 3;
    const int sig = (pp == 1) ? 2 : (pp == 2) ? 1 : pp;

    f32x16 sa[2][2];                                     // [key block][query block]
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int x = 0; x < 16; ++x) sa[kb][qb][x] = 0.0f;

    // Load cc is consumed at step cc; load cc + 1 is always the one issued after it,
    // so this wave waits with 4 DMA instructions in flight, then an LDS-only barrier
    // (a __syncthreads fence would drain those too) makes every wave's part visible.
#pragma unroll
    for (int cc = 0; cc < NQC; ++cc) {
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        lds_barrier();
        if (cc == 0) FA_STAMP(1);
        const char* buf = bufp(cc);
        // tr-read rows 8h + qq (+4): chunk-local features; slot rows 4blk + 2kh + (sig >> 1) / qb*4 + 2kh + (pp >> 1)
        // (asm reads: the next buffer's DMA stays in flight)
        s16x4 rk[2][2], rq[2][2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const char* a = buf + 16384 + sqk_pos(8 * h + qq, 4 * blk + 2 * kh + (sig >> 1), wl) + (sig & 1) * 8;
            rk[blk][0] = lds_tr16(a);
            rk[blk][1] = lds_tr16(buf + 16384 + sqk_pos(8 * h + qq + 4, 4 * blk + 2 * kh + (sig >> 1), wl) + (sig & 1) * 8);
            const char* aq = buf + sqk_pos(8 * h + qq, 4 * blk + 2 * kh + (pp >> 1), wl) + (pp & 1) * 8;
            rq[blk][0] = lds_tr16(aq);
            rq[blk][1] = lds_tr16(buf + sqk_pos(8 * h + qq + 4, 4 * blk + 2 * kh + (pp >> 1), wl) + (pp & 1) * 8);
        }
        lds_wait();
        F8 kf[2], qf[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { lds_fence(rk[blk][i]); lds_fence(rq[blk][i]); }
            kf[blk] = __builtin_shufflevector(__builtin_bit_cast(F4, rk[blk][0]), __builtin_bit_cast(F4, rk[blk][1]),
                                              0, 1, 2, 3, 4, 5, 6, 7);
            qf[blk] = __builtin_shufflevector(__builtin_bit_cast(F4, rq[blk][0]), __builtin_bit_cast(F4, rq[blk][1]),
                                              0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) sa[kb][qb] = mfma32x32x16(kf[kb], qf[qb], sa[kb][qb]);
        if (cc + 2 < NLD) {
            lds_barrier();                                // every wave is done with this buffer
            issue(qrs, krs, vrs, cc + 2);
        }
    }

    FA_STAMP(2);
    // ---- exact softmax per query over the window's real keys (+ npad zero keys) ----
    F8 pf[2][2][2];                                      // [query block][key block][16-key half]
    float mt[2], lt[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int kt = kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
                const int sx = kt & 7;
                if ((kt >> 3) >= ws || sx < c0 || sx >= c1) sa[kb][qb][x] = kNegInf;
            }
        f32x16 two[2] = {sa[0][qb], sa[1][qb]};
        float m = swap_halves_max(lane_max<2>(two));
        if (npad > 0.0f) m = vmax(m, 0.0f);
        const float mc = m * scale_log2;
        float ps[4];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pr = exp2_fast(fmaf(sa[kb][qb][x], scale_log2, -mc));
                if (kb == 0 && x < 4) ps[x] = pr; else ps[x & 3] += pr;
                pf[qb][kb][x >> 3][x & 7] = (T)pr;
            }
        float l = swap_halves_sum((ps[0] + ps[1]) + (ps[2] + ps[3]));
        if (npad > 0.0f) l = fmaf(npad, exp2_fast(-mc), l);
        mt[qb] = m;
        lt[qb] = l;
    }
    // l, m (window layout) and the padding-column query tokens
    if (wok) {
        const int64_t wbase = (int64_t)g.T * ((int64_t)(wx + nwx * wy) + (int64_t)g.L * b);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int qs = qb * 32 + r, qtx = qs & 7, qty = qs >> 3;
            if (h == 0 && qtx >= c0 && qtx < c1 && qty < ws) {
                const int64_t li = wbase + qty * ws + (qtx - c0);
                mo[li] = mt[qb] * scale;
                lo[li] = lt[qb];
            }
        }
        if (lane < g.T) {                                 // padding-column query tokens (q = 0): every score is 0
            const int px = xs + lane % ws;
            if (px < 0 || px >= W_) {
                mo[wbase + lane] = 0.0f;
                lo[wbase + lane] = (float)g.T;
            }
        }
    }
    // this wave's V DMA (and the l, m stores).  The builtin, not asm: hipcc then knows no
    // LDS-DMA is pending, and adds no vmcnt(0) of its own before the epilogue's LDS
    // accesses (which made chunk 1's image reads wait for chunk 0's y stores).
    __builtin_amdgcn_s_waitcnt(0x0F70);
    lds_barrier();                                       // every wave's V landed
    FA_STAMP(3);

    // ---- per 32-feature chunk: Oᵀ = Vᵀ·Pᵀ, then (over the V image) the strip image
    //      [32 f][8 rows][64 px] of normalised O, then 16-B stores of the strip's pixels ----
    const int xs0 = wx0 * st - g.pad, X0 = xs0 & ~7;     // strip start, its 16-B aligned base
    const int xlo = max(xs0, 0), xhi = min(xs0 + nvalid * ws, W_);
    const auto ors = slab_rsrc(out + (int64_t)b * dv * P_, (uint32_t)(dv * P_ * 2));
    unsigned vm[4];                                      // key-slot mask of a V fragment (one slot row)
#pragma unroll
    for (int j = 0; j < 4; ++j)
        vm[j] = ((2 * j >= c0 && 2 * j < c1) ? 0x0000FFFFu : 0u) | ((2 * j + 1 >= c0 && 2 * j + 1 < c1) ? 0xFFFF0000u : 0u);
#pragma unroll
    for (int vc = 0; vc < NVC; ++vc) {
        char* img = bufp(NQC + vc);
        f32x16 oa[2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int x = 0; x < 16; ++x) oa[qb][x] = 0.0f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                u32x4 vr = *(const u32x4*)(img + sv_pos(r, kb * 4 + s2 * 2 + h, wl));
#pragma unroll
                for (int j = 0; j < 4; ++j) vr[j] &= vm[j];
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) oa[qb] = mfma32x32x16(__builtin_bit_cast(F8, vr), pf[qb][kb][s2], oa[qb]);
            }
        lds_barrier();                                   // every wave has read this V chunk
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int qs = qb * 32 + r, qtx = qs & 7, qty = qs >> 3;
            const float inv = 1.0f / lt[qb];
            if (wok && qtx >= c0 && qtx < c1 && qty < ws && !(FA_WIN_ABL & 4)) {
                const int px = ax + qtx - X0;
#pragma unroll
                for (int x = 0; x < 16; ++x)
                    *(T*)(img + simg_pos(acc_row(x, h), qty, px)) = (T)(oa[qb][x] * inv);
            }
        }
        lds_barrier();
        constexpr int NU = 32 * 8 * 8;                   // (feature, row, 16-B chunk) units: a wave covers
#pragma unroll                                           // 8 rows x 8 chunks of one feature
        for (int it = 0; it < NU / 512; ++it) {
            const int u = it * 512 + tid, f = u >> 6, row = (u >> 3) & 7, j = u & 7;
            const int y = y0 + row, fg = vc * 32 + f, x0 = X0 + 8 * j;
            if (row >= ws || y < 0 || y >= H_ || fg >= dv || x0 + 8 <= xlo || x0 >= xhi || (FA_WIN_ABL & 8)) continue;
            const int go = ((fg * P_ + y * W_ + x0) * 2);
            const char* src = img + f * 1024 + row * 128 + ((j ^ simg_swz(f, row)) << 4);
            if (x0 >= xlo && x0 + 8 <= xhi) {
                __builtin_amdgcn_raw_buffer_store_b128(*(const u32x4*)src, ors, go, 0, 0);
            } else if (!(FA_WIN_ABL & 16)) {             // a chunk shared with the neighbour strip
                for (int e = 0; e < 8; ++e)
                    if (x0 + e >= xlo && x0 + e < xhi)
                        __builtin_amdgcn_raw_buffer_store_b16(*(const unsigned short*)(src + 2 * e), ors, go + 2 * e, 0, 0);
            }
        }
        if (vc == 0) FA_STAMP(4);
    }
    FA_STAMP(5);
}

// --------------------------------------------------------------------------
// fp32 fused windowed forward (2-D, stride >= ws, ws <= 8, d, dv <= 64, W >= 8):
// one window per workgroup on the exact-f32 MFMA v_mfma_f32_32x32x2_f32 (the
// arithmetic of an fmaf chain, like the fp32 dense path).  Staging: each
// (feature, window row) item is two 16-B loads of the 8 pixels starting at
// a = clamp(xs, 0, W - 8) (fp32 pixels are dword aligned, so the window-uniform
// shift xs - a is a dword select), masked (slot < ws, pixel in the image) and
// written to [feature][65-float] LDS rows (conflict-free for both the column
// reads of the score product and the row reads of the PV product).  Wave
// (qb, vc): Sᵀ = K·Qᵀ for query block qb, exact softmax per query, then
// Oᵀ = Vᵀ·Pᵀ for its 32-feature chunk with the score accumulators as the B
// operand (register x of lane (r, h) holds key acc_row(x, h): k = h).
// --------------------------------------------------------------------------
template <int D, int DV>
__global__ __launch_bounds__(256) void win_rows_f32(const float* __restrict__ q, const float* __restrict__ k,
                                                    const float* __restrict__ v, float* __restrict__ out,
                                                    float* __restrict__ lo, float* __restrict__ mo, WinDev g,
                                                    int d, int dv, float scale, float scale_log2) {
    constexpr int NTH = 256, ROW = 65;
    constexpr int QI = 0, KI = D * ROW, VI = 2 * D * ROW, REGION = (2 * D + DV) * ROW;
    constexpr int NIQ = D * 8 / NTH, NIV = DV * 8 / NTH;
    static_assert(D * 8 % NTH == 0 && DV * 8 % NTH == 0, "item split");
    __shared__ float sm[REGION];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W_ = g.S[0], H_ = g.S[1], P_ = g.P, ws = g.ws, st = g.stride;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int wx = bid % g.O[0], wy = (bid / g.O[0]) % g.O[1], b = bid / (g.O[0] * g.O[1]);
    const int xs = wx * st - g.pad, y0 = wy * st - g.pad;
    const int ax = min(max(xs, 0), W_ - 8);
    const int sh = xs - ax;                                    // slot t <- loaded pixel t + sh
    auto item_off = [&](int it, int C) {
        const int yy = it & 7, f = it >> 3, yr = y0 + yy;
        const bool ok = yy < ws && yr >= 0 && yr < H_ && f < C;
        return ok ? (f * P_ + yr * W_ + ax) * 4 : 0x7FFFFFE0;
    };
    const auto qrs = slab_rsrc(q + (int64_t)b * d * P_, (uint32_t)(d * P_ * 4));
    const auto krs = slab_rsrc(k + (int64_t)b * d * P_, (uint32_t)(d * P_ * 4));
    const auto vrs = slab_rsrc(v + (int64_t)b * dv * P_, (uint32_t)(dv * P_ * 4));
    u32x4 rq[NIQ][2], rk[NIQ][2], rv[NIV][2];
#pragma unroll
    for (int j = 0; j < NIQ; ++j) {
        const int o = item_off(tid + NTH * j, d);
        rq[j][0] = __builtin_amdgcn_raw_buffer_load_b128(qrs, o, 0, 0);
        rq[j][1] = __builtin_amdgcn_raw_buffer_load_b128(qrs, o + 16, 0, 0);
        rk[j][0] = __builtin_amdgcn_raw_buffer_load_b128(krs, o, 0, 0);
        rk[j][1] = __builtin_amdgcn_raw_buffer_load_b128(krs, o + 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NIV; ++j) {
        const int o = item_off(tid + NTH * j, dv);
        rv[j][0] = __builtin_amdgcn_raw_buffer_load_b128(vrs, o, 0, 0);
        rv[j][1] = __builtin_amdgcn_raw_buffer_load_b128(vrs, o + 16, 0, 0);
    }
    bool valid[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) valid[t] = t < ws && xs + t >= 0 && xs + t < W_;
    auto stage = [&](const u32x4 (&raw)[2], int it, int img) {
        const int yy = it & 7, f = it >> 3;
        unsigned px[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) px[t] = t < 4 ? raw[0][t] : raw[1][t - 4];
        float* dst = sm + img + f * ROW + yy * 8;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int src = t + sh;
            unsigned val = 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) val = src == e ? px[e] : val;
            dst[t] = valid[t] ? __uint_as_float(val) : 0.0f;
        }
    };
#pragma unroll
    for (int j = 0; j < NIQ; ++j) {
        stage(rq[j], tid + NTH * j, QI);
        stage(rk[j], tid + NTH * j, KI);
    }
#pragma unroll
    for (int j = 0; j < NIV; ++j) stage(rv[j], tid + NTH * j, VI);
    __syncthreads();

    const int qb = wave & 1, vc = wave >> 1;
    f32x16 sa[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int x = 0; x < 16; ++x) sa[kb][x] = 0.0f;
#pragma unroll
        for (int t = 0; t < D / 2; ++t)
            sa[kb] = mfma32x32x2(sm[KI + (2 * t + h) * ROW + kb * 32 + r], sm[QI + (2 * t + h) * ROW + qb * 32 + r], sa[kb]);
    }
    // mask padding key slots, exact softmax per query (lanes r and r + 32 share query r)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int kt = kb * 32 + acc_row(x, h);
            if ((kt & 7) >= ws || (kt >> 3) >= ws) sa[kb][x] = kNegInf;
        }
    const float mt = swap_halves_max(lane_max<2>(sa));
    const float mc = mt * scale_log2;
    float ps[4];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const float pr = exp2_fast(fmaf(sa[kb][x], scale_log2, -mc));
            if (kb == 0 && x < 4) ps[x] = pr; else ps[x & 3] += pr;
            sa[kb][x] = pr;
        }
    const float lt = swap_halves_sum((ps[0] + ps[1]) + (ps[2] + ps[3]));
    const int qslot = qb * 32 + r, qtx = qslot & 7, qty = qslot >> 3;
    if (vc < DV / 32) {
        f32x16 oa;
#pragma unroll
        for (int x = 0; x < 16; ++x) oa[x] = 0.0f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x)
                oa = mfma32x32x2(sm[VI + (vc * 32 + r) * ROW + kb * 32 + acc_row(x, h)], sa[kb][x], oa);
        const int px = xs + qtx, py = y0 + qty;
        if (qtx < ws && qty < ws && px >= 0 && px < W_ && py >= 0 && py < H_) {
            const float inv = 1.0f / lt;
            float* yb = out + (int64_t)b * dv * P_ + (int64_t)py * W_ + px;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int cc = vc * 32 + acc_row(x, h);
                if (cc < dv) yb[(int64_t)cc * P_] = oa[x] * inv;
            }
        }
    }
    if (vc == 0 && h == 0 && qtx < ws && qty < ws) {
        const int64_t wid = (int64_t)(wx + g.O[0] * wy) + (int64_t)g.L * b;
        const int64_t li = qty * ws + qtx + (int64_t)g.T * wid;
        mo[li] = mt * scale;
        lo[li] = lt;
    }
}

// --------------------------------------------------------------------------
// Host side.  win_fwd_plan (fa_windowed.h) names the kernel; the code below launches it.
// --------------------------------------------------------------------------
thread_local int g_win_force_composed = 0;   // benchmark knob (fa_debug_set_win_composed): a WinMode

static size_t composed_fwd_bytes(int dtype, const WindowGeom& g, int64_t d, int64_t dv, int64_t batch) {
    const size_t tok = (size_t)(g.T * g.L * batch);
    return align256(tok * d * esize(dtype)) * 2 + align256(tok * dv * esize(dtype)) * 2 +
           align256(dense_fwd_workspace(dtype, g.T, g.T, d, dv, g.L * batch)) + 256;
}

// The query cannot see the pointers, so it plans for unaligned ones: a 16-bit shape within
// win_fused's limits then gets win_fused, and whatever kernel aligned pointers will select
// needs no more.  Every other shape (the 128-wide and fp32 kernels' too) keeps the composed
// path's size.
size_t windowed_fwd_workspace(int dtype, const WindowGeom& g, int64_t d, int64_t dv, int64_t batch) {
    switch (win_fwd_plan(dtype, g, d, dv, batch, g_win_force_composed, false, false)) {
        case kWinFwdFused: return 0;   // direct stores
        case kWinFwdFusedWs: return align256((size_t)(g.T * g.L * batch) * dv * esize(dtype)) + 256;   // the window outputs
        default: return composed_fwd_bytes(dtype, g, d, dv, batch);
    }
}

size_t windowed_workspace(int dtype, const WindowGeom& g, int64_t d, int64_t dv, int64_t batch) {
    const size_t tok = (size_t)(g.T * g.L * batch);
    const size_t e = esize(dtype);
    return align256(tok * d * e) * 4 + align256(tok * dv * e) * 4 + align256(tok * 4) * 2 +
           align256(dense_bwd_workspace(dtype, g.T, g.T, d, dv, g.L * batch)) +
           align256(dense_fwd_workspace(dtype, g.T, g.T, d, dv, g.L * batch)) + 256;
}

// After a kernel that stores y directly: its launch status, then NaN for the pixels no
// window covers (reference 0/0, Appendix A.7).
template <class T>
static int finish_direct(const WindowedArgs& a, const WinDev& g, hipStream_t s, const char** why) {
    const int rc = launch_status(why);
    if (rc != FA_OK || fully_covered(a.g)) return rc;
    const int64_t total = a.g.P * a.dv * a.batch;
    hipLaunchKernelGGL(win_nan_uncovered<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (T*)a.y,
                       (int)a.dv, total, g);
    return launch_status(why);
}

template <class T, int NWIN, int D, int DV>
static void launch_rows1s(const WindowedArgs& a, const WinDev& g, hipStream_t s) {
    const int64_t nw = a.g.L * a.batch;
    hipLaunchKernelGGL((win_rows1s<T, D, DV, NWIN>), dim3((unsigned)((nw + NWIN - 1) / NWIN)), dim3(256 * NWIN), 0, s,
                       (const T*)a.q, (const T*)a.k, (const T*)a.v, (T*)a.y, a.l, a.m, g, (int)a.d, (int)a.dv, nw,
                       a.scale, a.scale * kLog2e);
}

// bf16 / f16: every plan but the composed one
template <class T>
static int windowed_fwd_16bit(const WindowedArgs& a, WinFwdKernel plan, const WinDev& g, hipStream_t s,
                              const char** why) {
    const int64_t nw = a.g.L * a.batch;
    const float c = a.scale * kLog2e;
    const bool direct = plan != kWinFwdFusedWs;
    void* const out = direct ? a.y : (void*)(((uintptr_t)a.workspace + 255) & ~(uintptr_t)255);
    switch (plan) {
        case kWinFwdFused:
        case kWinFwdFusedWs:
            by_head_class(a.d, a.dv, [&](auto D, auto DV) {
                auto fused = [&](auto NKB, auto DIRECT) {
                    hipLaunchKernelGGL((win_fused<T, D, DV, NKB, DIRECT>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s,
                                       (const T*)a.q, (const T*)a.k, (const T*)a.v, (T*)out, a.l, a.m, g, (int)a.d,
                                       (int)a.dv, (int)a.batch, a.scale, c);
                };
                if (a.g.T <= 32) { if (direct) fused(dim_c<1>{}, std::true_type{}); else fused(dim_c<1>{}, std::false_type{}); }
                else { if (direct) fused(dim_c<2>{}, std::true_type{}); else fused(dim_c<2>{}, std::false_type{}); }
            });
            if (direct) break;
            if (const int rc = launch_status(why); rc != FA_OK) return rc;
            return hip_status(fold<T>(out, a.y, (int)a.dv, a.batch, g, true, s), why);
        case kWinFwdRows: {
            const int ngx = (int)((a.g.O[0] + 3) / 4);
            const int64_t nwg = (int64_t)ngx * a.g.O[1] * a.batch;
            by_head_class(a.d, a.dv, [&](auto D, auto DV) {
                hipLaunchKernelGGL((win_rows<T, D, DV>), dim3((unsigned)nwg), dim3(256), 0, s, (const T*)a.q,
                                   (const T*)a.k, (const T*)a.v, (T*)a.y, a.l, a.m, g, (int)a.d, (int)a.dv,
                                   (int)a.batch, ngx, a.scale, c);
            });
            break;
        }
        case kWinFwdRows1:
            by_head_class(a.d, a.dv, [&](auto D, auto DV) {
                hipLaunchKernelGGL((win_rows1<T, D, DV>), dim3((unsigned)nw), dim3(256), 0, s, (const T*)a.q,
                                   (const T*)a.k, (const T*)a.v, (T*)a.y, a.l, a.m, g, (int)a.d, (int)a.dv, a.scale, c);
            });
            break;
        case kWinFwdShift1:
        case kWinFwdShift2:
        case kWinFwdShift3:
            by_head_class(a.d, a.dv, [&](auto D, auto DV) {
                if (plan == kWinFwdShift3) launch_rows1s<T, 3, D, DV>(a, g, s);
                else if (plan == kWinFwdShift2) launch_rows1s<T, 2, D, DV>(a, g, s);
                else launch_rows1s<T, 1, D, DV>(a, g, s);
            });
            break;
        case kWinFwdShift128:
            launch_rows1s<T, 1, 128, 128>(a, g, s);
            break;
        case kWinFwdStrip: {
            const int k0 = strip_first(a.g);
            const int64_t nsx = strip_count(a.g, k0), nstrip = nsx * a.g.O[1] * a.batch;
            by_head_class(a.d, a.dv, [&](auto D, auto DV) {
                hipLaunchKernelGGL((win_strip<T, D, DV>), dim3((unsigned)nstrip), dim3(512), 0, s, (const T*)a.q,
                                   (const T*)a.k, (const T*)a.v, (T*)a.y, a.l, a.m, g, (int)a.d, (int)a.dv, (int)nsx, k0,
                                   (int)nstrip, a.scale, c);
            });
            break;
        }
        default:
            *why = "windowed forward: no 16-bit kernel for this plan";
            return FA_ERR_UNSUPPORTED;
    }
    return finish_direct<T>(a, g, s, why);
}

template <class T>
static int windowed_fwd_composed(const WindowedArgs& a, const WinDev& g, hipStream_t s, const char** why) {
    const int64_t tok = a.g.T * a.g.L * a.batch;
    char* ws = (char*)(((uintptr_t)a.workspace + 255) & ~(uintptr_t)255);
    void* qw = ws;  ws += align256(tok * a.d * sizeof(T));
    void* kw = ws;  ws += align256(tok * a.d * sizeof(T));
    void* vw = ws;  ws += align256(tok * a.dv * sizeof(T));
    void* ow = ws;  ws += align256(tok * a.dv * sizeof(T));
    hipError_t e;
    if ((e = gather<T>(a.q, qw, (int)a.d, a.batch, g, false, s)) != hipSuccess ||
        (e = gather<T>(a.k, kw, (int)a.d, a.batch, g, false, s)) != hipSuccess ||
        (e = gather<T>(a.v, vw, (int)a.dv, a.batch, g, false, s)) != hipSuccess)
        return hip_status(e, why);
    // the window batch has T = ws^k tokens (49 at ws 7): the dense workspace lets
    // the fast kernels run on padded key copies (or split-KV) instead of the generic one
    DenseArgs da{a.dtype, qw, kw, vw, ow, a.l, a.m, a.g.T, a.g.T, a.d, a.dv, a.g.L * a.batch, a.scale};
    da.scale64 = a.scale64;
    da.workspace = ws;
    da.workspace_bytes = dense_fwd_workspace(a.dtype, a.g.T, a.g.T, a.d, a.dv, a.g.L * a.batch);
    const int rc = launch_dense_fwd(da, s, why);
    if (rc != FA_OK) return rc;
    return hip_status(fold<T>(ow, a.y, (int)a.dv, a.batch, g, true, s), why);
}

template <class T>
static int windowed_fwd_typed(const WindowedArgs& a, hipStream_t s, const char** why) {
    if (a.workspace_bytes < windowed_fwd_workspace(a.dtype, a.g, a.d, a.dv, a.batch)) {
        *why = "workspace smaller than fa_windowed_fwd_workspace()";
        return FA_ERR_WORKSPACE;
    }
    const WinDev g = to_dev(a.g);
    const WinFwdKernel plan = win_fwd_plan(a.dtype, a.g, a.d, a.dv, a.batch, g_win_force_composed,
                                           aligned16(a.q) && aligned16(a.k) && aligned16(a.v), aligned16(a.y));
    if constexpr (std::is_same<T, float>::value) {
        if (plan == kWinFwdF32) {
            by_head_class(a.d, a.dv, [&](auto D, auto DV) {
                hipLaunchKernelGGL((win_rows_f32<D, DV>), dim3((unsigned)(a.g.L * a.batch)), dim3(256), 0, s,
                                   (const float*)a.q, (const float*)a.k, (const float*)a.v, (float*)a.y, a.l, a.m, g,
                                   (int)a.d, (int)a.dv, a.scale, a.scale * kLog2e);
            });
            return finish_direct<float>(a, g, s, why);
        }
    }
    if constexpr (sizeof(T) == 2) {
        if (plan != kWinFwdComposed) return windowed_fwd_16bit<T>(a, plan, g, s, why);
    }
    return windowed_fwd_composed<T>(a, g, s, why);
}

int launch_window(int dtype, const void* src, void* dst, const WindowGeom& geom, int64_t C, int64_t batch,
                  bool unwindow, hipStream_t s, const char** why) {
    if (!geom_fits(geom, C, C, batch) || C > INT32_MAX) {
        *why = "window geometry exceeds the 32-bit index range";
        return FA_ERR_UNSUPPORTED;
    }
    const WinDev g = to_dev(geom);
    const int64_t total = unwindow ? geom.P * C * batch : geom.T * C * geom.L * batch;
    if (total == 0) return FA_OK;
    if ((total + 255) / 256 > INT32_MAX) {
        *why = "grid too large";
        return FA_ERR_UNSUPPORTED;
    }
    hipError_t e;
    switch (dtype) {
        case FA_DTYPE_BF16: e = unwindow ? fold<bf16>(src, dst, (int)C, batch, g, false, s)
                                         : gather<bf16>(src, dst, (int)C, batch, g, false, s); break;
        case FA_DTYPE_F16: e = unwindow ? fold<f16>(src, dst, (int)C, batch, g, false, s)
                                        : gather<f16>(src, dst, (int)C, batch, g, false, s); break;
        case FA_DTYPE_F32: e = unwindow ? fold<float>(src, dst, (int)C, batch, g, false, s)
                                        : gather<float>(src, dst, (int)C, batch, g, false, s); break;
        case FA_DTYPE_F64: e = unwindow ? fold<double>(src, dst, (int)C, batch, g, false, s)
                                        : gather<double>(src, dst, (int)C, batch, g, false, s); break;
        default: *why = "unknown dtype"; return FA_ERR_INVALID_ARG;
    }
    return hip_status(e, why);
}

int launch_windowed_fwd(const WindowedArgs& a, hipStream_t s, const char** why) {
    if (const int rc = win_args_fit(a.g, a.d, a.dv, a.batch, why); rc != FA_OK) return rc;
    switch (a.dtype) {
        case FA_DTYPE_BF16: return windowed_fwd_typed<bf16>(a, s, why);
        case FA_DTYPE_F16: return windowed_fwd_typed<f16>(a, s, why);
        case FA_DTYPE_F32: return windowed_fwd_typed<float>(a, s, why);
        case FA_DTYPE_F64: return windowed_fwd_typed<double>(a, s, why);
    }
    *why = "unknown dtype";
    return FA_ERR_INVALID_ARG;
}

}  // namespace fa
