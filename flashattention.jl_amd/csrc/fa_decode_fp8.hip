// fa_decode_fp8.hip — decode attention over an fp8 (e4m3fn) KV cache for gfx950 (MI355X, CDNA4):
// fa_decode.hip's kernel with K and V stored as one byte per element plus one fp32 scale per KV
// slab (fa_decode_fp8_fwd).  Decode is bound by the bytes of the cache; this halves them.
//
// The work split is fa_decode.hip's: the G * N <= 32 query rows of a KV slab are one 32-row
// MFMA tile, a slab's visible tile range is cut into nsplit shares (one workgroup of 4 waves
// each, under xcd_remap), a wave takes alternate 64-key tiles with wave-private staging and no
// workgroup barrier in the key loop, V travels one tile ahead in registers, the softmax is the
// lazy-rescale online one in log2 units, the waves merge through LDS in wave order and
// decode8_combine merges the shares in split order.  The data path is new:
//
//  * the K image is [D][64 keys] of BYTES (64-B rows, D * 64 B per tile, half of the 16-bit
//    image).  VEC fills it by LDS-DMA, 16 B = 16 keys per lane, 16 feature rows per 1-KiB
//    instruction, D / 16 instructions per tile, no VGPRs.  The 16-B chunks of a row are XOR
//    swizzled with bits 1..2 of the row: physical chunk pc of row f holds keys
//    16 (pc ^ ((f >> 1) & 3)) .. + 15;
//  * it is read with ds_read_b64_tr_b8: in a 16-lane group lane 2 q + p supplies the 8 bytes of
//    row q, columns 8 p .. 8 p + 7 of an 8 x 16 block, and lane i receives column i, row q in
//    byte q.  Rows are features and columns keys, so lane (r, h) holds key kb * 32 + r (no key
//    permutation), features 16 s + 8 h .. + 7, and four v_cvt_scalef32_pk_{bf16,f16}_fp8 with
//    scale 1.0 make the A operand of S^T = K Q^T.  Every e4m3fn value is exact in bf16 and fp16;
//  * with keys in natural order, accumulator x of lane half h is key acc_row(x, h) of its
//    32-key block: the lane's P values are the 4-key chunks h, 2 + h, 4 + h, 6 + h.  V's A
//    operand must bring the same chunks: VEC loads 16 contiguous bytes per lane (keys
//    kb * 32 + 16 h .. + 15 of feature cb * 32 + r, one buffer_load_b128 per 32 keys) and two
//    v_permlane32_swap exchange dwords between the lane halves; the converts run right before
//    O^T += V P^T;
//  * the scales never touch an element: ks folds into the score scale (c = scale ks log2 e, per
//    slab), the stored m is m_raw scale ks, and vs multiplies O once where it is normalised
//    (the nsplit = 1 epilogue or the combine); partials stay unscaled.
//
// VEC = false (Nk % 16 != 0, or K8 / V8 not 16-B aligned) is the same kernel with single-byte
// buffer loads packed in registers: slower, correct, and never a copy of the cache.
#include <type_traits>

#include "fa_common.h"
#include "fa_decode8_params.h"
#include "fa_decode_plan.h"
#include "fa_internal.h"
#include "../../include/fa_hip.h"

namespace fa {

namespace {

// Four bytes from byte offset `off` of a slab, each 0 where `ok` is false or its key is past Nk
// (the next row's bytes otherwise): the VEC = false loads.
__device__ __forceinline__ unsigned load4x8(__amdgpu_buffer_rsrc_t rs, bool ok, int row, int key, int Nk) {
    unsigned w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        w |= (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs, ok && key + e < Nk ? row + key + e : kDec8OobOff, 0, 0) << (8 * e);
    return w;
}

// One K tile into a wave's LDS image: 16-B chunk `it * 64 + lane` (byte it * 1024 + lane * 16) is
// feature it * 16 + kf0, keys key0 .. key0 + 15.  VEC: D / 16 LDS-DMA instructions of 1 KiB (no
// VGPRs); else byte loads packed in registers and one 16-B LDS write per chunk.
template <int D, bool VEC>
__device__ __forceinline__ void decode8_stage_k(__amdgpu_buffer_rsrc_t krs, char* buf, int key0, int kf0, int lane, int d,
                                                int Nk) {
#pragma unroll
    for (int it = 0; it < D / 16; ++it) {
        const int f = it * 16 + kf0;
        if constexpr (VEC) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (__attribute__((address_space(3))) void*)(buf + it * 1024), 16,
                                                     f < d ? f * Nk + key0 : kDec8OobOff, 0, 0, 0);
        } else {
            u32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = load4x8(krs, f < d, f * Nk, key0 + 4 * j, Nk);
            *(u32x4*)(buf + it * 1024 + lane * 16) = w;
        }
    }
}

template <class T, int D, int DV, bool VEC>
__global__ __launch_bounds__(kDecodeThreads) void decode8_fwd(Decode8Params p) {
    typedef typename Frag8<T>::type F8;
    constexpr int BN = kDecodeKeyTile;
    constexpr int KROW = BN;                 // K image: [D][64 keys] bytes, 64-B rows, 16-B chunk XOR swizzle
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

    // The slab's extents and its visible tiles [t0, t0 + nt), and this workgroup's share of
    // them, exactly as fa_decode.hip: an empty share stores the empty state and leaves before
    // any K / V load.
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
        decode8_store_empty<T>(p, b, sp);
        return;
    }
    // the slab's scales (scalar loads): ks folds into the score scale, vs waits for the epilogue
    const float ks = p.k_scale ? p.k_scale[b] : 1.0f, vs = p.v_scale ? p.v_scale[b] : 1.0f;
    const float sk = p.scale * ks;

    // lane (r, h): row r = g * N + i of the tile; dead rows (past G * N, or i >= nq) carry zeros
    const int g = r / N, i = r - g * N;
    const bool live_row = r < rows && i < ve.nq;
    const int lo_r = live_row ? i + ve.off - ve.left : 0x3FFFFFFF;      // the row's visible keys [lo_r, hi_r]
    const int hi_r = live_row ? min(i + ve.off + ve.right, ve.nk - 1) : -1;
    const int lo_max = ve.nq - 1 + ve.off - ve.left;                    // tiles inside [lo_max, hi_min] need no select
    const int hi_min = min(ve.nk - 1, ve.off + ve.right);

    // Q^T fragments (B operand of S^T = K Q^T): k-step s holds Q[row][features 16 s + 8 h ..+7]
    F8 qf[D / 16];
    {
        const auto qrs = slab_rsrc((const T*)p.Q + (int64_t)b * G * d * N, (uint32_t)(rows * d * 2));
#pragma unroll
        for (int s = 0; s < D / 16; ++s)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int f = 16 * s + 8 * h + e;
                const unsigned short w =
                    __builtin_amdgcn_raw_buffer_load_b16(qrs, (live_row && f < d) ? ((g * d + f) * N + i) * 2 : kDec8OobOff, 0, 0);
                qf[s][e] = __builtin_bit_cast(T, w);
            }
    }

    const auto krs = slab_rsrc(p.K + (int64_t)b * Nk * d, (uint32_t)(Nk * d));
    const auto vrs = slab_rsrc(p.V + (int64_t)b * Nk * dv, (uint32_t)(Nk * dv));

    // K staging: 16-B chunk `it * 64 + lane` of the image is feature f = it * 16 + lane / 4,
    // physical chunk pc = lane % 4, which holds the 16 keys of logical chunk pc ^ swz(f),
    // swz(f) = bits 1..2 of f, the same for every `it`.
    const int kf0 = lane >> 2, kpc = lane & 3;
    const int kkey = (kpc ^ ((kf0 >> 1) & 3)) * 16;
    char* const kbuf0 = smem + wave * WSTRIDE;
    char* const kbuf1 = kbuf0 + KBUF;
    auto stage_k = [&](char* buf, int t) { decode8_stage_k<D, VEC>(krs, buf, t * BN + kkey, kf0, lane, d, Nk); };
    // V (A operand of O^T += V P^T), feature cb * 32 + r, per 32-key block kb one u32x4 whose
    // dword j is the 4-key chunk h + 4 (j & 1) + 2 (j >> 1) of the block: the chunks of this
    // lane half's P values, k-step s in dwords s and s + 2.  VEC loads the 16 contiguous bytes
    // of keys 16 h .. + 15 (chunks 4 h .. 4 h + 3) and v_swap (in compute, once they have
    // landed) brings them to that order; the narrow path loads each chunk where it belongs.
    constexpr int NV = DV / 32 * 2;
    auto load_v = [&](u32x4 (&v)[NV], int t) {
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int f = cb * 32 + r, key = t * BN + kb * 32;
                if constexpr (VEC) {
                    v[cb * 2 + kb] = __builtin_amdgcn_raw_buffer_load_b128(vrs, f < dv ? f * Nk + key + 16 * h : kDec8OobOff, 0, 0);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        v[cb * 2 + kb][j] = load4x8(vrs, f < dv, f * Nk, key + 4 * (h + 4 * (j & 1) + 2 * (j >> 1)), Nk);
                }
            }
    };
    // lane half 0 holds chunks (0, 1, 2, 3), half 1 (4, 5, 6, 7); v_permlane32_swap exchanges the
    // upper half of its first operand with the lower half of its second: dwords (0, 1) become
    // chunks (0, 4) | (1, 5) and dwords (2, 3) chunks (2, 6) | (3, 7).
    auto v_swap = [](u32x4 w) {
        const auto a = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);
        const auto c = __builtin_amdgcn_permlane32_swap(w[2], w[3], false, false);
        return u32x4{a[0], a[1], c[0], c[1]};
    };

    // transposed K reads: in its 16-lane group lane 2 q + p supplies feature row 8 h + q
    // (+ 16 s), the 8 keys p of logical chunk kb * 2 + kh; lane r receives key kb * 32 + r
    const int kh = (lane >> 4) & 1, qq = (lane & 15) >> 1, pp = lane & 1;
    int koff[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) koff[kb] = (8 * h + qq) * KROW + (((kb * 2 + kh) ^ ((qq >> 1) & 3)) * 16) + 8 * pp;

    f32x16 oacc[DV / 32];
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) oacc[cb][x] = 0.0f;
    float m_used = kNegInf, m_true = kNegInf, l_run = 0.0f;
    const float c = sk * kLog2e;
    const float thr_raw = kRescaleLog2 / c;

    // One tile: S^T from the K image, then the next tile's K DMA into the other image (after this
    // tile's LDS reads: the compiler orders every LDS read behind every LDS-DMA in flight),
    // softmax, O^T += V P^T.
    auto compute = [&](const char* kbuf, const u32x4 (&v)[NV], int t, char* knext) {
        f32x16 sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int x = 0; x < 16; ++x) sacc[kb][x] = 0.0f;
#pragma unroll
            for (int s = 0; s < D / 16; ++s) {
                const i32x2 k8 = ds_read_tr8(kbuf + koff[kb] + 16 * s * KROW);
                sacc[kb] = mfma32x32x16(cvt8<T>((unsigned)k8[0], (unsigned)k8[1]), qf[s], sacc[kb]);
            }
        }
        if (t + 4 < te) stage_k(knext, t + 4);
        // the mask is a select, on the tiles that straddle an edge of some live row's range;
        // accumulator x of lane half h is key acc_row(x, h) of its 32-key block
        const int key0 = t * BN;
        if (key0 < lo_max || key0 + BN - 1 > hi_min) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int kt = key0 + kb * 32 + acc_row(x, h);
                    if (kt < lo_r || kt > hi_r) sacc[kb][x] = kNegInf;
                }
        }
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
            for (int kb = 0; kb < 2; ++kb) {
                const u32x4 w = VEC ? v_swap(v[cb * 2 + kb]) : v[cb * 2 + kb];
#pragma unroll
                for (int s = 0; s < 2; ++s) oacc[cb] = mfma32x32x16(cvt8<T>(w[s], w[s + 2]), pf[kb][s], oacc[cb]);
            }
    };

    // The wave's tiles: ts + wave, + 4, ...  Tile t + 4 is in flight (V into the other register
    // set, K by DMA into the other image) while tile t is computed; the wait at the top of each
    // step, vmcnt(0) with the other counters left alone, is for this wave's own loads.
    auto landed = [] {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("" ::: "memory");
    };
    u32x4 v0[NV], v1[NV];
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
    const float inv = vs / lsum;                 // the V scale, once, where O is normalised
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
            p.m[R] = live ? m * sk : kNegInf;
        }
    }
}

// One thread per (row, feature): the row's nsplit partials in split order, with the scales of
// the row's KV slab.  m = max m_s (exact, so the same bits for every split count), weights
// 2^((m_s - m) c), O = vs sum w O_s / sum w l_s.
template <class T>
__global__ __launch_bounds__(kDecodeThreads) void decode8_combine(Decode8Params p, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * kDecodeThreads + threadIdx.x;
    if (idx >= total) return;
    const int dv = p.dv, N = p.N;
    const int64_t R = idx / dv;
    const int f = (int)(idx - R * dv);
    const int64_t bq = R / N;
    const int i = (int)(R - bq * N);
    const int b = (int)(bq / p.group);
    const float ks = p.k_scale ? p.k_scale[b] : 1.0f, vs = p.v_scale ? p.v_scale[b] : 1.0f;
    const float sk = p.scale * ks, c = sk * kLog2e;
    const int64_t stride = (int64_t)p.batch * p.group * N * (dv + 2);
    const float* const base = p.part + R * (dv + 2);
    float m = kNegInf;
    for (int s = 0; s < p.nsplit; ++s) m = vmax(m, base[s * stride + dv + 1]);
    float lsum = 0.0f, o = 0.0f;
    for (int s = 0; s < p.nsplit; ++s) {
        const float ms = base[s * stride + dv + 1];
        const float w = ms == kNegInf ? 0.0f : exp2_fast((ms - m) * c);
        lsum += w * base[s * stride + dv];
        o += w * base[s * stride + f];
    }
    const bool live = lsum > 0.0f;
    ((T*)p.O)[(bq * dv + f) * N + i] = live ? (T)(o * (vs / lsum)) : (T)0.0f;
    if (f == 0) {
        p.l[R] = live ? lsum : 0.0f;
        p.m[R] = live ? m * sk : kNegInf;
    }
}

template <class T>
hipError_t launch_decode8(const DecodePlan& pl, const Decode8Params& p, int Dc, int DVc, hipStream_t s) {
    const dim3 grid((unsigned)pl.grid), blk(kDecodeThreads);
    by_dim_class(Dc, [&](auto Dk) {
        by_dim_class(DVc, [&](auto DVk) {
            constexpr int D = decltype(Dk)::value, DV = decltype(DVk)::value;
            if (pl.kernel == kDecodeVec) hipLaunchKernelGGL((decode8_fwd<T, D, DV, true>), grid, blk, 0, s, p);
            else hipLaunchKernelGGL((decode8_fwd<T, D, DV, false>), grid, blk, 0, s, p);
        });
    });
    if (pl.nsplit > 1) {
        const int64_t total = (int64_t)p.batch * p.group * p.N * p.dv;
        hipLaunchKernelGGL(decode8_combine<T>, dim3((unsigned)pl.combine_grid), blk, 0, s, p, total);
    }
    return hipGetLastError();
}

}  // namespace

// decode8_combine for the kernels of another file (fa_decode_paged_fp8.hip)
void launch_decode8_combine(int dtype, const DecodePlan& pl, const Decode8Params& p, hipStream_t s) {
    const int64_t total = (int64_t)p.batch * p.group * p.N * p.dv;
    const dim3 grid((unsigned)pl.combine_grid), blk(kDecodeThreads);
    if (dtype == FA_DTYPE_F16) hipLaunchKernelGGL(decode8_combine<f16>, grid, blk, 0, s, p, total);
    else hipLaunchKernelGGL(decode8_combine<bf16>, grid, blk, 0, s, p, total);
}

int launch_decode_fp8_fwd(const DecodeFp8Args& a8, hipStream_t s, const char** why) {
    const DecodeArgs& a = a8.a;
    const DecodePlan pl = decode_fp8_plan(a.dtype, a.N, a.Nk, a.d, a.dv, a.batch, a.group, g_decode_nsplit,
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
        *why = "workspace missing or smaller than fa_decode_fp8_fwd_workspace()";
        return FA_ERR_WORKSPACE;
    }
    const MaskInts mi = mask_ints(kMaskVarlen, a.left, a.right, a.N, a.Nk);
    Decode8Params p;
    p.Q = a.Q; p.K = (const uint8_t*)a.K; p.V = (const uint8_t*)a.V; p.O = a.O; p.l = a.l; p.m = a.m;
    p.k_scale = a8.k_scale; p.v_scale = a8.v_scale;
    p.q_lens = a.q_lens; p.k_lens = a.k_lens;
    p.part = pl.total ? (float*)al256(a.workspace) : nullptr;
    p.N = (int)a.N; p.Nk = (int)a.Nk; p.d = (int)a.d; p.dv = (int)a.dv;
    p.batch = (int)a.batch; p.group = (int)a.group;
    p.nsplit = pl.nsplit; p.total_wg = (int)pl.grid;
    p.wleft = mi.left; p.wright = mi.right;
    p.scale = a.scale;
    const int Dc = head_dim_class(a.d), DVc = head_dim_class(a.dv);
    const hipError_t e = a.dtype == FA_DTYPE_F16 ? launch_decode8<f16>(pl, p, Dc, DVc, s) : launch_decode8<bf16>(pl, p, Dc, DVc, s);
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    return FA_OK;
}

}  // namespace fa
