// fa_decode.hip — decode attention for gfx950 (MI355X, CDNA4): a few queries per KV slab
// against a long cache, with G query heads sharing each K / V slab (fa_decode_fwd).
//
// The masked dense forward gives a decode call one workgroup per slab, 8 waves of which at
// most one holds a real row, and no way to share a cache between heads.  This kernel is built
// the other way round:
//
//  * the G * N <= 32 query rows of a KV slab (row g * N + i = query i of head g) are ONE
//    32-row MFMA tile, so K and V are read once for all heads of the group;
//  * the keys are what is split: a slab's VISIBLE tile range (from its lengths and window,
//    read on the device) is cut into nsplit equal shares, one workgroup each, and inside a
//    workgroup each of the 4 waves takes alternate 64-key tiles;
//  * every wave keeps its own double-buffered K image in LDS, filled by LDS-DMA (no VGPRs, no
//    workgroup barrier in the key loop: a wave waits for its own loads only) and read with the
//    transposed LDS read, since tokens are contiguous in HBM and QK^T contracts over features;
//  * V (features x keys, keys contiguous) is already the A operand of O^T += V P^T: a lane's
//    fragment is 16 contiguous bytes, loaded from global memory straight into registers one
//    tile ahead (at d = 128 the K images fill the LDS, and V needs no transposition);
//  * scores are transposed, S^T = K Q^T, so a lane holds one query row's scores, the row
//    max / sum need one v_permlane32_swap, and P feeds the second product from registers
//    (the dense forward's key permutation, fa_fwd.hip);
//  * online softmax in log2 units with the lazy rescale; the true max travels separately;
//  * after the loop the 4 waves leave (m, m_used, l, O^T) in their own LDS regions, one
//    barrier, and the 256 threads merge them in wave order.  nsplit == 1 stores O, l, m;
//    otherwise an fp32 partial goes to the workspace and decode_combine merges the partials of
//    each row in split order.  No atomics, no hand-off: bitwise reproducible.
//
// VEC = false (Nk % 8 != 0, or K / V not 16-B aligned) is the same kernel with 2-byte loads
// staged through registers: slower, correct, and never a copy of the cache.
#include <type_traits>

#include "fa_common.h"
#include "fa_decode_params.h"
#include "fa_decode_plan.h"
#include "fa_internal.h"
#include "../../include/fa_hip.h"

namespace fa {

thread_local int g_decode_nsplit = 0;

// One 16-bit element at byte offset `off` of a slab, 0 where `ok` is false (VEC = false paths).
__device__ __forceinline__ unsigned load16(__amdgpu_buffer_rsrc_t rs, bool ok, int off) {
    return __builtin_amdgcn_raw_buffer_load_b16(rs, ok ? off : kDecOobOff, 0, 0);
}
// Keys key .. key + 7 of the row that starts at element `row`, as one 16-B fragment; 0 past Nk
// (the next row's elements otherwise) and where `ok` is false.
__device__ __forceinline__ u32x4 load8x16(__amdgpu_buffer_rsrc_t rs, bool ok, int row, int key, int Nk) {
    const auto pair = [&](int e) {
        return load16(rs, ok && key + e < Nk, (row + key + e) * 2) | load16(rs, ok && key + e + 1 < Nk, (row + key + e + 1) * 2) << 16;
    };
    return u32x4{pair(0), pair(2), pair(4), pair(6)};
}

// One K tile into a wave's LDS image: 16-B chunk `it * 64 + lane` (byte it * 1024 + lane * 16) is
// feature it * 8 + kf0, keys key0 .. key0 + 7.  VEC: D / 8 LDS-DMA instructions of 1 KiB (no
// VGPRs); else 2-byte loads packed in registers and one 16-B LDS write per chunk.
template <class T, int D, bool VEC>
__device__ __forceinline__ void decode_stage_k(__amdgpu_buffer_rsrc_t krs, char* buf, int key0, int kf0, int lane, int d,
                                               int Nk) {
#pragma unroll
    for (int it = 0; it < D / 8; ++it) {
        const int f = it * 8 + kf0;
        if constexpr (VEC) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (__attribute__((address_space(3))) void*)(buf + it * 1024), 16,
                                                     f < d ? (f * Nk + key0) * 2 : kDecOobOff, 0, 0, 0);
        } else {
            *(u32x4*)(buf + it * 1024 + lane * 16) = load8x16(krs, f < d, f * Nk, key0, Nk);
        }
    }
}

template <class T, int D, int DV, bool VEC>
__global__ __launch_bounds__(kDecodeThreads) void decode_fwd(DecodeParams p) {
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    constexpr int BN = kDecodeKeyTile;
    constexpr int KROW = BN * 2;             // K image: [D][64 keys], 128-B rows, 32-B chunk XOR swizzle
    constexpr int KBUF = D * KROW;           // one K tile
    constexpr int MSTAT = DV * 128;          // merge image: [DV][32 rows] floats, then m_true, m_used, l
    constexpr int MBYTES = MSTAT + 3 * 128;
    constexpr int WSTRIDE = 2 * KBUF > MBYTES ? 2 * KBUF : MBYTES;   // a wave's LDS: two K tiles, later its merge image
    __shared__ __attribute__((aligned(1024))) char smem[4 * WSTRIDE];

    const int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int b = lid / p.nsplit, sp = lid - b * p.nsplit;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int N = p.N, Nk = p.Nk, d = p.d, dv = p.dv, G = p.group, rows = N * G;

    // The slab's extents (two scalar loads) and its visible tiles [t0, t0 + nt): from the first
    // query's left edge to the last query's right edge, inside the nk keys.  This workgroup
    // takes the sp-th of nsplit equal shares of THAT range; an empty share stores the empty
    // state and leaves before any K / V load.
    const VarlenExt ve = varlen_extents(p.q_lens, p.k_lens, b, N, Nk, p.wleft, p.wright);
    const int klo = max(0, ve.off - ve.left), khi = min(ve.nk, ve.nq + ve.off + ve.right);
    int t0 = 0, nt = 0;
    if (ve.nq > 0 && khi > klo) {
        t0 = klo / BN;
        nt = (khi + BN - 1) / BN - t0;
    }
    const int tps = (nt + p.nsplit - 1) / p.nsplit;
    const int ts = t0 + sp * tps, te = min(t0 + nt, ts + tps);
    if (ts >= te) {
        decode_store_empty<T>(p, b, sp);
        return;
    }

    // lane (r, h): row r = g * N + i of the tile; dead rows (past G * N, or i >= nq) carry zeros
    const int g = r / N, i = r - g * N;
    const bool live_row = r < rows && i < ve.nq;
    const int lo_r = live_row ? i + ve.off - ve.left : 0x3FFFFFFF;      // the row's visible keys [lo_r, hi_r]
    const int hi_r = live_row ? min(i + ve.off + ve.right, ve.nk - 1) : -1;
    const int lo_max = ve.nq - 1 + ve.off - ve.left;                    // tiles inside [lo_max, hi_min] need no select
    const int hi_min = min(ve.nk - 1, ve.off + ve.right);

    // Q^T fragments (B operand of S^T = K Q^T): k-step s holds Q[row][features 16 s + 8 h ..+7]
    F8 qf[D / 16];
    {   // branch-free gathers through a descriptor over the group's G query slabs (<= 32 * d elements)
        const auto qrs = slab_rsrc((const T*)p.Q + (int64_t)b * G * d * N, (uint32_t)(rows * d * 2));
#pragma unroll
        for (int s = 0; s < D / 16; ++s)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int f = 16 * s + 8 * h + e;
                const unsigned short w =
                    __builtin_amdgcn_raw_buffer_load_b16(qrs, (live_row && f < d) ? ((g * d + f) * N + i) * 2 : kDecOobOff, 0, 0);
                qf[s][e] = __builtin_bit_cast(T, w);
            }
    }

    const auto krs = slab_rsrc((const T*)p.K + (int64_t)b * Nk * d, (uint32_t)(Nk * d * 2));
    const auto vrs = slab_rsrc((const T*)p.V + (int64_t)b * Nk * dv, (uint32_t)(Nk * dv * 2));

    // K staging: 16-B chunk `it * 64 + lane` of the image (byte it * 1024 + lane * 16) is feature
    // f = it * 8 + lane / 8, physical chunk pc = lane % 8, which holds the keys of logical 32-B
    // block (pc / 2) ^ swz(f), half pc % 2.  swz(f) = bit 1 of f, the same for every `it`.
    const int kf0 = lane >> 3, kpc = lane & 7;
    const int kkey = (((kpc >> 1) ^ (((kf0 >> 1) & 1) << 1)) * 16) + (kpc & 1) * 8;
    char* const kbuf0 = smem + wave * WSTRIDE;
    char* const kbuf1 = kbuf0 + KBUF;
    auto stage_k = [&](char* buf, int t) { decode_stage_k<T, D, VEC>(krs, buf, t * BN + kkey, kf0, lane, d, Nk); };
    // V fragments (A operand of O^T += V P^T): feature cb * 32 + r, keys kb * 32 + 16 s + 8 h ..+7
    constexpr int NV = DV / 32 * 4;
    auto load_v = [&](F8 (&v)[NV], int t) {
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = cb * 32 + r, key = t * BN + q * 16 + 8 * h;
                if constexpr (VEC) {
                    const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(vrs, f < dv ? (f * Nk + key) * 2 : kDecOobOff, 0, 0);
                    v[cb * 4 + q] = __builtin_bit_cast(F8, w);
                } else {
                    v[cb * 4 + q] = __builtin_bit_cast(F8, load8x16(vrs, f < dv, f * Nk, key, Nk));
                }
            }
    };

    // transposed K reads (fa_fwd.hip): lane r ends up with key pi(r) = r with bits 2 and 3 swapped
    const int kh = (lane >> 4) & 1, ii = lane & 15, qq = ii >> 2, pp = ii & 3;
    const int sig = (pp == 1) ? 2 : (pp == 2) ? 1 : pp;
    int koff[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
        koff[kb] = (8 * h + qq) * KROW + (((kb * 2 + kh) ^ (((qq >> 1) & 1) << 1)) * 32) + 8 * sig;

    f32x16 oacc[DV / 32];
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) oacc[cb][x] = 0.0f;
    float m_used = kNegInf, m_true = kNegInf, l_run = 0.0f;
    const float c = p.scale_log2;
    const float thr_raw = kRescaleLog2 / c;

    // One tile: S^T from the K image, then the next tile's K DMA into the other image (after this
    // tile's LDS reads, which would otherwise wait for it: the compiler orders every LDS read
    // behind every LDS-DMA in flight), softmax, O^T += V P^T.
    auto compute = [&](const char* kbuf, const F8 (&v)[NV], int t, char* knext) {
        f32x16 sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int x = 0; x < 16; ++x) sacc[kb][x] = 0.0f;
#pragma unroll
            for (int s = 0; s < D / 16; ++s) {
                const char* a = kbuf + koff[kb] + 16 * s * KROW;
                const F4 lo = __builtin_bit_cast(F4, ds_read_tr16(a));
                const F4 hi = __builtin_bit_cast(F4, ds_read_tr16(a + 4 * KROW));
                const F8 af = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                sacc[kb] = mfma32x32x16(af, qf[s], sacc[kb]);
            }
        }
        if (t + 4 < te) stage_k(knext, t + 4);
        // the mask is a select, on the tiles that straddle an edge of some live row's range
        // (lengths, window and the ragged last tile are one range per row); wave-uniform test
        const int key0 = t * BN;
        if (key0 < lo_max || key0 + BN - 1 > hi_min) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int kt = key0 + kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
                    if (kt < lo_r || kt > hi_r) sacc[kb][x] = kNegInf;
                }
        }
        // lazy rescale, row-local (dense_fwd_tiled's LOCAL body): m_used moves only for a row
        // that passed the threshold itself; a row with no visible key yet keeps -inf
        const float mt = lane_max<2>(sacc);
        m_true = vmax(m_true, mt);
        if (__builtin_amdgcn_ballot_w64(mt > m_used + thr_raw) != 0) {
            float m_new = fmaxf(m_used, swap_halves_max(mt));
            float alpha = exp2_fast((m_used - m_new) * c);
            if (!(m_new > m_used + thr_raw)) { m_new = m_used; alpha = 1.0f; }
            l_run *= alpha;
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int x = 0; x < 16; ++x) oacc[cb][x] *= alpha;
            m_used = m_new;
        }
        const float msub = m_used == kNegInf ? 0.0f : m_used;
        float ps[4];
        F8 pf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pv = exp2_fast((sacc[kb][x] - msub) * c);
                if (kb == 0 && x < 4) ps[x] = pv; else ps[x & 3] += pv;
                pf[kb][x >> 3][x & 7] = (T)pv;
            }
        l_run += (ps[0] + ps[1]) + (ps[2] + ps[3]);
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int s = 0; s < 2; ++s) oacc[cb] = mfma32x32x16(v[cb * 4 + kb * 2 + s], pf[kb][s], oacc[cb]);
    };

    // The wave's tiles: ts + wave, + 4, ...  Tile t + 4 is in flight (V into the other register
    // set, K by DMA into the other image) while tile t is computed; the wait at the top of each
    // step, vmcnt(0) with the other counters left alone, is for this wave's own loads.
    auto landed = [] {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("" ::: "memory");
    };
    F8 v0[NV], v1[NV];
    int t = ts + wave;
    if (t < te) {
        stage_k(kbuf0, t);
        load_v(v0, t);
    }
    while (t < te) {
        landed();
        if (t + 4 < te) load_v(v1, t + 4);
        compute(kbuf0, v0, t, kbuf1);
        t += 4;
        if (t >= te) break;
        landed();
        if (t + 4 < te) load_v(v0, t + 4);
        compute(kbuf1, v1, t, kbuf0);
        t += 4;
    }
    asm volatile("" ::: "memory");

    // ---- merge the 4 waves (one barrier), then store ----
    m_true = swap_halves_max(m_true);
    const float lw = swap_halves_sum(l_run);
    {
        float* const img = (float*)(smem + wave * WSTRIDE);
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) img[(cb * 32 + acc_row(x, h)) * 32 + r] = oacc[cb][x];
        if (h == 0) {
            img[MSTAT / 4 + r] = m_true;
            img[MSTAT / 4 + 32 + r] = m_used;
            img[MSTAT / 4 + 64 + r] = lw;
        }
    }
    __syncthreads();
    // thread (row r, feature group fg): DV / 8 features of one row, the waves in order
    const int fg = tid >> 5;
    float m = kNegInf, wgt[4], lsum = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) m = vmax(m, ((const float*)(smem + w * WSTRIDE))[MSTAT / 4 + r]);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float* const img = (const float*)(smem + w * WSTRIDE);
        const float mu = img[MSTAT / 4 + 32 + r];
        wgt[w] = mu == kNegInf ? 0.0f : exp2_fast((mu - m) * c);
        lsum += wgt[w] * img[MSTAT / 4 + 64 + r];
    }
    if (r >= rows) return;
    const bool live = live_row && lsum > 0.0f;   // else O = 0, l = 0, m = -inf, by select
    const int64_t R = (int64_t)b * rows + r;     // = (b * G + g) * N + i
    const float inv = 1.0f / lsum;
    float* const part = p.nsplit == 1 ? nullptr : p.part + ((int64_t)sp * p.batch * rows + R) * (dv + 2);
    T* const Orow = (T*)p.O + ((int64_t)b * G + g) * dv * N + i;
#pragma unroll
    for (int k = 0; k < DV / 8; ++k) {
        const int f = fg * (DV / 8) + k;
        float o = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) o += wgt[w] * ((const float*)(smem + w * WSTRIDE))[f * 32 + r];
        if (f < dv) {
            if (part) part[f] = live ? o : 0.0f;
            else Orow[(int64_t)f * N] = live ? (T)(o * inv) : (T)0.0f;
        }
    }
    if (fg == 0) {
        if (part) {
            part[dv] = live ? lsum : 0.0f;
            part[dv + 1] = live ? m : kNegInf;
        } else {
            p.l[R] = live ? lsum : 0.0f;
            p.m[R] = live ? m * p.scale : kNegInf;
        }
    }
}

// One thread per (row, feature): the row's nsplit partials in split order.  m = max m_s (exact,
// so the same bits for every split count), weights 2^((m_s - m) c), O = sum w O_s / sum w l_s.
template <class T>
__global__ __launch_bounds__(kDecodeThreads) void decode_combine(DecodeParams p, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * kDecodeThreads + threadIdx.x;
    if (idx >= total) return;
    const int dv = p.dv, N = p.N;
    const int64_t R = idx / dv;
    const int f = (int)(idx - R * dv);
    const int64_t stride = (int64_t)p.batch * p.group * N * (dv + 2);
    const float* const base = p.part + R * (dv + 2);
    float m = kNegInf;
    for (int s = 0; s < p.nsplit; ++s) m = vmax(m, base[s * stride + dv + 1]);
    float lsum = 0.0f, o = 0.0f;
    for (int s = 0; s < p.nsplit; ++s) {
        const float ms = base[s * stride + dv + 1];
        const float w = ms == kNegInf ? 0.0f : exp2_fast((ms - m) * p.scale_log2);
        lsum += w * base[s * stride + dv];
        o += w * base[s * stride + f];
    }
    const bool live = lsum > 0.0f;
    const int64_t bq = R / N;
    const int i = (int)(R - bq * N);
    ((T*)p.O)[(bq * dv + f) * N + i] = live ? (T)(o / lsum) : (T)0.0f;
    if (f == 0) {
        p.l[R] = live ? lsum : 0.0f;
        p.m[R] = live ? m * p.scale : kNegInf;
    }
}

void launch_decode_combine(int dtype, const DecodePlan& pl, const DecodeParams& p, hipStream_t s) {
    const int64_t total = (int64_t)p.batch * p.group * p.N * p.dv;
    const dim3 grid((unsigned)pl.combine_grid), blk(kDecodeThreads);
    if (dtype == FA_DTYPE_F16) hipLaunchKernelGGL(decode_combine<f16>, grid, blk, 0, s, p, total);
    else hipLaunchKernelGGL(decode_combine<bf16>, grid, blk, 0, s, p, total);
}

template <class T>
static hipError_t launch_decode(const DecodePlan& pl, const DecodeParams& p, int Dc, int DVc, hipStream_t s) {
    const dim3 grid((unsigned)pl.grid), blk(kDecodeThreads);
    by_dim_class(Dc, [&](auto Dk) {
        by_dim_class(DVc, [&](auto DVk) {
            constexpr int D = decltype(Dk)::value, DV = decltype(DVk)::value;
            if (pl.kernel == kDecodeVec) hipLaunchKernelGGL((decode_fwd<T, D, DV, true>), grid, blk, 0, s, p);
            else hipLaunchKernelGGL((decode_fwd<T, D, DV, false>), grid, blk, 0, s, p);
        });
    });
    if (pl.nsplit > 1) {
        const int64_t total = (int64_t)p.batch * p.group * p.N * p.dv;
        hipLaunchKernelGGL(decode_combine<T>, dim3((unsigned)pl.combine_grid), blk, 0, s, p, total);
    }
    return hipGetLastError();
}

int launch_decode_fwd(const DecodeArgs& a, hipStream_t s, const char** why) {
    const DecodePlan pl = decode_plan(a.dtype, a.N, a.Nk, a.d, a.dv, a.batch, a.group, g_decode_nsplit,
                                      aligned16(a.K) && aligned16(a.V));
    if (pl.kernel == kDecodeNone) {
        *why = "shape outside the decode kernels (api.cpp checks it first)";
        return FA_ERR_UNSUPPORTED;
    }
    if (pl.grid > INT32_MAX || pl.combine_grid > INT32_MAX) {
        *why = "grid too large";
        return FA_ERR_UNSUPPORTED;
    }
    if (pl.total > 0 && (!a.workspace || a.workspace_bytes < pl.total)) {
        *why = "workspace missing or smaller than fa_decode_fwd_workspace()";
        return FA_ERR_WORKSPACE;
    }
    const MaskInts mi = mask_ints(kMaskVarlen, a.left, a.right, a.N, a.Nk);
    DecodeParams p;
    p.Q = a.Q; p.K = a.K; p.V = a.V; p.O = a.O; p.l = a.l; p.m = a.m;
    p.q_lens = a.q_lens; p.k_lens = a.k_lens;
    p.part = pl.total ? (float*)al256(a.workspace) : nullptr;
    p.N = (int)a.N; p.Nk = (int)a.Nk; p.d = (int)a.d; p.dv = (int)a.dv;
    p.batch = (int)a.batch; p.group = (int)a.group;
    p.nsplit = pl.nsplit; p.total_wg = (int)pl.grid;
    p.wleft = mi.left; p.wright = mi.right;
    p.scale = a.scale; p.scale_log2 = a.scale * kLog2e;
    const int Dc = head_dim_class(a.d), DVc = head_dim_class(a.dv);
    const hipError_t e = a.dtype == FA_DTYPE_F16 ? launch_decode<f16>(pl, p, Dc, DVc, s) : launch_decode<bf16>(pl, p, Dc, DVc, s);
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    return FA_OK;
}

}  // namespace fa
