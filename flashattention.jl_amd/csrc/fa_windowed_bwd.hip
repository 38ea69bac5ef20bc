// fa_windowed_bwd.hip — the windowed attention backward on gfx950 (fa_windowed.h has the
// geometry, the composed path and the plan).
//
// Kernels: win_bwd_rows (one or two windows per workgroup, and at 128 features),
// win_bwd_strip (persistent, the eight windows of a forward strip per workgroup) with its
// store helpers, and win_bwd_f32.
// Host: the composed backward, the backward launcher (launch_windowed_bwd), and the
// definition of g_win_bwd_grid.  Built without the register-pressure trackers the forward
// file gets (Makefile).
#include "fa_windowed.h"

namespace fa {

// --------------------------------------------------------------------------
// Fused windowed BACKWARD, one window per workgroup (bf16/f16, 2-D, stride >= ws,
// ws <= 7, d, dv <= 64): the exact chain rule of windowed_fa for non-overlapping
// windows, where every covered pixel belongs to exactly one window, so
// dyw = window(dy ./ count) is dy itself and the fold is a direct store.
// Replaces, for these shapes, the composed gather -> dense backward -> fold
// path (T = 49 tokens is not a multiple of 8, so that path runs the SIMT
// backward: 20 ms at B = 32).
//
//   staging  : q, k, v, dy rows by the row-shift loads of the forward kernel into
//              [feature][slot] images (128-B swizzled rows).  y is not read (round 5:
//              a fifth of the loads, on CUs that run two windows at B = 1).
//   phase 1  : wave (qb, kb) computes the 32x32 blocks S = Q Kᵀ and dP = dO Vᵀ
//              (queries on accumulator rows, keys on lanes) with −lse/τ as S's
//              initial accumulator, P = exp2(c·S'), and D = rowsum(P ∘ dP) (= rowsum
//              (dy ∘ y)): each wave's 32-key partial by DPP / permlane16 sums within
//              its lane halves, the two key halves' partials added through LDS; then
//              dS = P ∘ (dP − D), and P, dS (bf16) go into [key][query] images (144-B rows).
//   phase 2  : 12 blocks over the 4 waves: dVᵀ = dOᵀ P, dKᵀ = τ Qᵀ dS (row
//              reads), dQᵀ = τ Kᵀ dSᵀ (dSᵀ by transposed reads of the [key][query]
//              image); each lane stores one slot's features straight to its pixel.
// Padding slots (tx or ty >= ws): keys masked (P = dS = 0), queries have lse = +inf.
// --------------------------------------------------------------------------
template <class T, int D, int DV, int NWIN>
__global__ __launch_bounds__(256 * NWIN) void win_bwd_rows(const T* __restrict__ q, const T* __restrict__ k,
                                                    const T* __restrict__ v, const T* __restrict__ y,
                                                    const T* __restrict__ dy, const float* __restrict__ lw,
                                                    const float* __restrict__ mw, T* __restrict__ dq,
                                                    T* __restrict__ dk, T* __restrict__ dvo, WinDev g, int d,
                                                    int dv, int nwin_total, float scale, float scale_log2) {
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    constexpr int NTH = 256 * NWIN, KROW = 128, PROW = 144;
    constexpr int QIMG = D * KROW, VIMG = DV * KROW, PIMG = 64 * PROW;
    constexpr int OQ = 0, OK_ = QIMG, OV = 2 * QIMG, ODO = 2 * QIMG + VIMG, OP = 2 * QIMG + 2 * VIMG,
                  ODS = OP + PIMG, OLSE = ODS + PIMG, OD = OLSE + 256, REGION = OD + 4 * 256;
    constexpr int NIQ = D * 8 / 256, NIV = DV * 8 / 256;    // items per thread: window x feature x 8 slot rows
    static_assert(D * 8 % 256 == 0 && DV * 8 % 256 == 0, "item split");
    __shared__ __attribute__((aligned(16))) char smem[NWIN * REGION];
    auto kswz = [](int f) { return ((f >> 1) & 1) << 1; };

    FA_STAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W_ = g.S[0], H_ = g.S[1], P_ = g.P, ws = g.ws, st = g.stride;
    // NWIN horizontally adjacent windows (xcd_remap: contiguous runs per XCD), 4 waves each
    const int nperimg = g.O[0] * g.O[1];
    struct Win { int wx, wy, b, xs, y0, ax; bool ok; };
    auto win_of = [&](int wl) {
        Win w;
        const int id = xcd_remap(blockIdx.x, gridDim.x) * NWIN + wl;   // 32-bit: the host keeps L·B < 2^31
        w.ok = id < nwin_total;
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
    // staging item it -> (window it % NWIN, feature (it / NWIN) >> 3, slot row (it / NWIN) & 7): the
    // NWIN windows' loads of one (feature, row) sit on adjacent lanes, 2·ws bytes apart, and share
    // their cache lines; every item of a lane belongs to window tid % NWIN (NTH % NWIN == 0).
    // Descriptors span the images the workgroup's windows can span (NWIN, clamped to the
    // batch: a pair may straddle images), as in win_rows1s.
    const int b0 = win_of(0).b;
    const int nimg = min(NWIN, nwin_total / nperimg - b0);
    const int wl_me = NWIN == 1 ? 0 : (int)(tid % NWIN);
    const Win wme = win_of(wl_me);
    auto item_off = [&](int it, int C) {
        const int rest = NWIN == 1 ? it : it / NWIN, yy = rest & 7, f = rest >> 3, yr = wme.y0 + yy;
        const bool ok = wme.ok && yy < ws && yr >= 0 && yr < H_ && f < C;
        return ok ? (((wme.b - b0) * C + f) * P_ + yr * W_ + wme.ax) * 2 : 0x7FFFFFF0;
    };
    const auto qrs = slab_rsrc(q + (int64_t)b0 * d * P_, (uint32_t)(nimg * d * P_ * 2));
    const auto krs = slab_rsrc(k + (int64_t)b0 * d * P_, (uint32_t)(nimg * d * P_ * 2));
    const auto vrs = slab_rsrc(v + (int64_t)b0 * dv * P_, (uint32_t)(nimg * dv * P_ * 2));
    (void)y;
    const auto drs = slab_rsrc(dy + (int64_t)b0 * dv * P_, (uint32_t)(nimg * dv * P_ * 2));
    u32x4 rq[NIQ], rk[NIQ], rv[NIV], rd[NIV];
#pragma unroll
    for (int j = 0; j < NIQ; ++j) {
        const int o = item_off(tid + NTH * j, d);
        rq[j] = __builtin_amdgcn_raw_buffer_load_b128(qrs, o, 0, 0);
        rk[j] = __builtin_amdgcn_raw_buffer_load_b128(krs, o, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NIV; ++j) {
        const int o = item_off(tid + NTH * j, dv);
        rv[j] = __builtin_amdgcn_raw_buffer_load_b128(vrs, o, 0, 0);
        rd[j] = __builtin_amdgcn_raw_buffer_load_b128(drs, o, 0, 0);
    }
    // per-slot constant −lse/τ of window tid >> 6 (+inf lse outside the window)
    if (tid < 64 * NWIN) {
        const int wl = tid >> 6, tx = tid & 7, ty = (tid >> 3) & 7;
        const Win w = win_of(wl);
        float nl = kNegInf;
        if (w.ok && tx < ws && ty < ws) {
            const int64_t wid = (int64_t)(w.wx + g.O[0] * w.wy) + (int64_t)g.L * w.b;
            const int64_t li = ty * ws + tx + (int64_t)g.T * wid;
            nl = -(mw[li] + __logf(lw[li])) / scale;
        }
        ((float*)(smem + wl * REGION + OLSE))[tid & 63] = nl;
    }
    unsigned mask[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t0 = 2 * j, t1 = 2 * j + 1;
        const bool v0 = t0 < ws && wme.xs + t0 >= 0 && wme.xs + t0 < W_;
        const bool v1 = t1 < ws && wme.xs + t1 >= 0 && wme.xs + t1 < W_;
        mask[j] = (v0 ? 0x0000FFFFu : 0u) | (v1 ? 0xFFFF0000u : 0u);
    }
    const int sh_me = wme.xs - wme.ax;
    // NWIN > 1: lanes of a wave shift by different amounts; away from the image's left and
    // right edges every shift is 0 or 1 pixel (one v_alignbyte per dword), as in win_rows1s
    const bool near_shift = NWIN > 1 && __builtin_amdgcn_ballot_w64((sh_me >> 1) != 0) == 0;
    const unsigned ab_me = (sh_me & 1) ? 2u : 0u;
    char* const sme = smem + wl_me * REGION;
    auto koff = [&](int it) {
        const int rest = NWIN == 1 ? it : it / NWIN, yy = rest & 7, f = rest >> 3;
        return f * KROW + (((yy >> 1) ^ kswz(f)) * 32) + (yy & 1) * 16;
    };
    auto stage_all = [&](auto fast) {
        auto shifted = [&](const u32x4& val) {
            u32x4 o;
            if constexpr (NWIN == 1) {
                o = shift_row(val, sh_me, mask);
            } else if constexpr (decltype(fast)::value) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    o[j] = __builtin_amdgcn_alignbyte(j < 3 ? val[j + 1] : 0u, val[j], ab_me) & mask[j];
            } else {
                o = shift_row_lane(val, sh_me, mask);
            }
            return o;
        };
#pragma unroll
        for (int j = 0; j < NIQ; ++j) {
            const int o = koff(tid + NTH * j);
            *(u32x4*)(sme + OQ + o) = shifted(rq[j]);
            *(u32x4*)(sme + OK_ + o) = shifted(rk[j]);
        }
        FA_STAMP(1);
#pragma unroll
        for (int j = 0; j < NIV; ++j) {
            const int o = koff(tid + NTH * j);
            *(u32x4*)(sme + OV + o) = shifted(rv[j]);
            *(u32x4*)(sme + ODO + o) = shifted(rd[j]);
        }
    };
    if (near_shift) stage_all(std::true_type{});
    else stage_all(std::false_type{});
    __syncthreads();
    FA_STAMP(2);

    // ---- this wave's window ----
    const Win w = win_of(wave >> 2);
    char* const wsm = smem + (wave >> 2) * REGION;
    const int b = w.b, xs = w.xs, y0 = w.y0;
    float* const lse_s = (float*)(wsm + OLSE);   // −lse/τ per query slot (raw score units)
    float* const dsum = (float*)(wsm + OD);      // D per query slot: one partial per key half [2][64]

    // ---- phase 1: S and dP blocks (qb, kb) of this wave ----
    const int qb = wave & 1, kb = (wave >> 1) & 1;
    const int g4 = lane >> 4, kh = g4 & 1, qq = (lane & 15) >> 2, pp = lane & 3;
    // tr-read of a [feature][slot] image: 32 slots of block sb, features 16 s + 8 h .. + 7
    auto frag_tr = [&](int img, int sb, int s16) {
        const int orow = (16 * s16 + 8 * h + qq) * KROW;
        const char* a = wsm + img + orow + (((sb * 2 + kh) ^ kswz(qq)) * 32) + 8 * pp;
        return __builtin_shufflevector(__builtin_bit_cast(F4, ds_read_tr16(a)),
                                       __builtin_bit_cast(F4, ds_read_tr16(a + 4 * KROW)), 0, 1, 2, 3, 4, 5, 6, 7);
    };
    f32x16 sa, pa;
#pragma unroll
    for (int x4 = 0; x4 < 4; ++x4) {
        const f32x4 l4 = *(const f32x4*)(lse_s + qb * 32 + acc_row(4 * x4, h));
#pragma unroll
        for (int e = 0; e < 4; ++e) { sa[4 * x4 + e] = l4[e]; pa[4 * x4 + e] = 0.0f; }
    }
#pragma unroll
    for (int s16 = 0; s16 < D / 16; ++s16) sa = mfma32x32x16(frag_tr(OQ, qb, s16), frag_tr(OK_, kb, s16), sa);
#pragma unroll
    for (int s16 = 0; s16 < DV / 16; ++s16) pa = mfma32x32x16(frag_tr(ODO, qb, s16), frag_tr(OV, kb, s16), pa);
    const int kslot = kb * 32 + r;
    const bool kvalid = (kslot & 7) < ws && (kslot >> 3) < ws;
    // P (fp32 for dS, bf16 into the [key][query] image, 4 consecutive queries per 8-byte
    // write) and this wave's 32-key partial of D = rowsum(P ∘ dP) for each of its queries
    float pr[16];
#pragma unroll
    for (int x4 = 0; x4 < 4; ++x4) {
        typename Frag8<T>::half p4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            pr[4 * x4 + e] = kvalid ? exp2_fast(sa[4 * x4 + e] * scale_log2) : 0.0f;
            p4[e] = (T)pr[4 * x4 + e];
        }
        *(typename Frag8<T>::half*)(wsm + OP + kslot * PROW + (qb * 32 + acc_row(4 * x4, h)) * 2) = p4;
    }
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        float v = pr[x] * pa[x];   // keys on lanes: sum over the 32 lanes of this half (h)
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, false));
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));
        auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(r16[0]) + __uint_as_float(r16[1]);
        if (r == 0) dsum[kb * 64 + qb * 32 + acc_row(x, h)] = v;
    }
    lds_barrier();
    // dS = P ∘ (dP − D), D = the two key halves' partials
#pragma unroll
    for (int x4 = 0; x4 < 4; ++x4) {
        const int qrow = qb * 32 + acc_row(4 * x4, h);
        const f32x4 d4 = *(const f32x4*)(dsum + qrow) + *(const f32x4*)(dsum + 64 + qrow);
        typename Frag8<T>::half s4;
#pragma unroll
        for (int e = 0; e < 4; ++e) s4[e] = (T)(pr[4 * x4 + e] * (pa[4 * x4 + e] - d4[e]));
        *(typename Frag8<T>::half*)(wsm + ODS + kslot * PROW + qrow * 2) = s4;
    }
    lds_barrier();
    FA_STAMP(3);

    // ---- phase 2: dVᵀ, dKᵀ, dQᵀ blocks ----
    // row read: 8 consecutive slots 16 s + 8 h of feature row f of a [feature][slot] image
    auto frag_row = [&](int img, int f, int s16) {
        return *(const F8*)(wsm + img + f * KROW + ((s16 ^ kswz(f)) * 32) + 16 * h);
    };
    auto store_px = [&](T* out, int C, int slot, int fbase, const f32x16& acc, float mul) {
        const int tx = slot & 7, ty = slot >> 3, px = xs + tx, py = y0 + ty;
        if (w.ok && tx < ws && ty < ws && px >= 0 && px < W_ && py >= 0 && py < H_) {
            T* ob = out + (int64_t)b * C * P_ + (int64_t)py * W_ + px;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = fbase + acc_row(x, h);
                if (f < C) ob[(int64_t)f * P_] = (T)(acc[x] * mul);
            }
        }
    };
    constexpr int NDV = DV / 32 * 2, NDK = D / 32 * 2, NBLK = NDV + 2 * NDK;
#pragma unroll
    for (int i = 0; i < (NBLK + 3) / 4; ++i) {
        const int blk = (wave & 3) + 4 * i;
        if (blk >= NBLK) break;
        f32x16 acc;
#pragma unroll
        for (int x = 0; x < 16; ++x) acc[x] = 0.0f;
        if (blk < NDV) {                              // dVᵀ[cb, kb2] = dOᵀ P
            const int cb = blk >> 1, kb2 = blk & 1, f = cb * 32 + r;
#pragma unroll
            for (int s16 = 0; s16 < 4; ++s16)
                acc = mfma32x32x16(frag_row(ODO, f, s16),
                                   *(const F8*)(wsm + OP + (kb2 * 32 + r) * PROW + (16 * s16 + 8 * h) * 2), acc);
            store_px(dvo, dv, kb2 * 32 + r, cb * 32, acc, 1.0f);
        } else if (blk < NDV + NDK) {                 // dKᵀ[fb, kb2] = τ Qᵀ dS
            const int b2 = blk - NDV, fb = b2 >> 1, kb2 = b2 & 1, f = fb * 32 + r;
#pragma unroll
            for (int s16 = 0; s16 < 4; ++s16)
                acc = mfma32x32x16(frag_row(OQ, f, s16),
                                   *(const F8*)(wsm + ODS + (kb2 * 32 + r) * PROW + (16 * s16 + 8 * h) * 2), acc);
            store_px(dk, d, kb2 * 32 + r, fb * 32, acc, scale);
        } else {                                      // dQᵀ[fb, qb2] = τ Kᵀ dSᵀ
            const int b2 = blk - NDV - NDK, fb = b2 >> 1, qb2 = b2 & 1, f = fb * 32 + r;
#pragma unroll
            for (int s16 = 0; s16 < 4; ++s16) {
                const char* a = wsm + ODS + (16 * s16 + 8 * h + qq) * PROW + (qb2 * 32 + kh * 16 + 4 * pp) * 2;
                const F8 bt = __builtin_shufflevector(__builtin_bit_cast(F4, ds_read_tr16(a)),
                                                      __builtin_bit_cast(F4, ds_read_tr16(a + 4 * PROW)),
                                                      0, 1, 2, 3, 4, 5, 6, 7);
                acc = mfma32x32x16(frag_row(OK_, f, s16), bt, acc);
            }
            store_px(dq, d, qb2 * 32 + r, fb * 32, acc, scale);
        }
    }
    FA_STAMP(4);
    FA_STAMP(5);
}

// --------------------------------------------------------------------------
// Strip BACKWARD: the eight windows of a forward strip per workgroup, one per
// wave (bf16/f16, 2-D, stride == ws <= 7, d, dv <= 64, width % 8 == 0, 16-B
// aligned tensors; the default from kStripBwdMin strips on).  Same strip
// geometry, rotated slots and swizzled LDS-DMA images as win_strip; every
// gradient leaves as whole 16-B chunks of the strip's pixels.
//
//   phase A  (16-feature chunks, Sᵀ-style images): Sᵀ = K·Qᵀ, keys on accumulator
//            rows, queries on lanes, as in the forward; P = exp(τS − lse) from the
//            forward's (l, m) (read by a dword DMA) as bf16 B fragments (n = query)
//            while the dO / V chunks land; then dPᵀ = V·dOᵀ in the same
//            accumulators; D = rowsum(P ∘ dP) in-lane (= rowsum(dO ∘ y): y is
//            never read); τ dS = τ P ∘ (dP − D) as bf16 B fragments.  The phase-B
//            A operands of K and Q (lane = feature) are read from the same images
//            into registers, so the strip's data is loaded from HBM once.
//   phase B  (no loads): Pᵀ and dSᵀ with keys on lanes by an identity MFMA
//            (C = A·I with the fragments as A: exact, no LDS round trip);
//            dVᵀ = dOᵀ P (dO rows from the (dO, V) images, still in the ring),
//            dKᵀ = Qᵀ (τ dS), dQᵀ = Kᵀ (τ dS)ᵀ, 32 output features at a time, each
//            written as a 16-feature strip image [16 f][8 rows][64 px] (twice) and
//            stored as whole 16-B chunks.
//   loads    : a ring of four 32-KB buffers refilled as soon as a slot is read
//            (Q / K slots at once, dO / V slots after dV), continuing into the
//            next strip (persistent: one workgroup per CU over consecutive
//            strips); exact vmcnt counts (loads, DMAs and stores retire in order);
//            LDS-only barriers.
// Keys / queries outside the window (slot row >= ws, columns outside [c0, c1))
// are masked (K / V fragments zeroed, -inf exponent bias, selects on the query
// lanes), so a non-finite neighbour pixel never enters this window's sums.
// --------------------------------------------------------------------------
#define FA_VM_CASE(N) \
    case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
__device__ __forceinline__ void wait_vm(int n) {   // n: even, 0 .. 46 (anything else waits for all)
    switch (n) {
        FA_VM_CASE(0) FA_VM_CASE(2) FA_VM_CASE(4) FA_VM_CASE(6) FA_VM_CASE(8) FA_VM_CASE(10) FA_VM_CASE(12)
        FA_VM_CASE(14) FA_VM_CASE(16) FA_VM_CASE(18) FA_VM_CASE(20) FA_VM_CASE(22) FA_VM_CASE(24) FA_VM_CASE(26)
        FA_VM_CASE(28) FA_VM_CASE(30) FA_VM_CASE(32) FA_VM_CASE(34) FA_VM_CASE(36) FA_VM_CASE(38) FA_VM_CASE(40)
        FA_VM_CASE(42) FA_VM_CASE(44) FA_VM_CASE(46)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}
#undef FA_VM_CASE

// Per-lane store plan of a 16-feature strip image, fixed for the strip: unit
// u = it * 512 + tid (it = 0, 1) is (feature it * 8 + (tid >> 6), row (tid >> 3) & 7,
// 16-B chunk tid & 7); the two units differ by constants.
struct StripStore {
    int go0;          // byte offset of the unit's chunk in the slab, feature 0
    int roff;         // LDS byte offset of unit 0 in the image
    bool full;        // a whole in-image 16-B chunk
    bool part;        // straddles a strip end (2-B stores; only when the ends are unaligned)
    int e0, e1;       // the straddling chunk's pixels inside the strip: [e0, e1)
};
__device__ __forceinline__ StripStore strip_store_plan(int tid, int y0, int ws, int H_, int W_, int X0, int xlo, int xhi) {
    const int f = tid >> 6, row = (tid >> 3) & 7, j = tid & 7;
    const int y = y0 + row, x0 = X0 + 8 * j;
    const bool rok = row < ws && y >= 0 && y < H_ && x0 + 8 > xlo && x0 < xhi;
    StripStore p;
    p.full = rok && x0 >= xlo && x0 + 8 <= xhi;
    p.part = rok && !p.full;
    p.go0 = (y * W_ + x0) * 2;                       // + feature * P * 2 at the store
    p.roff = f * 1024 + row * 128 + ((j ^ simg_swz(f, row)) << 4);
    p.e0 = max(xlo - x0, 0);
    p.e1 = min(xhi - x0, 8);
    return p;
}

// A 16-feature strip image [16 f][8 rows][64 px] (simg_pos) of output features
// fbase .. fbase + 15 as 16-B chunk stores, 2 per lane (invalid lanes get an
// out-of-range offset: the store is dropped); chunks straddling a strip end as
// 2-B stores (PARTIAL only).
template <class T, bool PARTIAL>
__device__ __forceinline__ void strip_store16(const char* img, __amdgpu_buffer_rsrc_t ors, const StripStore& sp, int tid,
                                              int fbase, int C, int P_) {
    if (FA_WIN_ABL & 32) return;
    const int f = tid >> 6;
    u32x4 val[2];
    const uint32_t ra = lds_off(img) + sp.roff;      // unit 1: + 8 KB
    asm volatile("ds_read_b128 %0, %1" : "=v"(val[0]) : "v"(ra) : "memory");
    asm volatile("ds_read_b128 %0, %1 offset:8192" : "=v"(val[1]) : "v"(ra) : "memory");
    lds_wait();
    lds_fence(val[0]);
    lds_fence(val[1]);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int fg = fbase + it * 8 + f;
        const bool ok = fg < C && sp.full;
        __builtin_amdgcn_raw_buffer_store_b128(val[it], ors, ok ? sp.go0 + fg * P_ * 2 : 0x7FFFFFF0, 0, 0);
    }
    if (PARTIAL && sp.part) {                        // only when some strip end is not on a 16-B chunk
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int fg = fbase + it * 8 + f;
            if (fg >= C) continue;
            const int go = sp.go0 + fg * P_ * 2;
            for (int e = 0; e < 8; ++e)
                if (e >= sp.e0 && e < sp.e1)
                    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(val[it][e >> 1] >> (16 * (e & 1))), ors,
                                                          go + 2 * e, 0, 0);
        }
    }
}

// 8 accumulator values (registers X0 .. X0 + 7: features acc_row(x, h) - 16 (X0 / 8) of one
// slot) into a 16-feature strip image at base (= simg_pos(4h, row, px)): the feature offsets
// are immediates (the swizzle depends on feature bit 2 = h only); pairs share one conversion.
template <class T, int X0, int X = X0>
__device__ __forceinline__ void img_w8(uint32_t base, const f32x16& acc) {
    if constexpr (X < X0 + 8) {
        typedef T T2 __attribute__((ext_vector_type(2)));
        typedef float F2 __attribute__((ext_vector_type(2)));
        const T2 pr = __builtin_convertvector((F2){acc[X], acc[X + 1]}, T2);
        const unsigned u = __builtin_bit_cast(unsigned, pr);
        constexpr int f0 = (X & 3) + 8 * (X >> 2) - 2 * X0, f1 = ((X + 1) & 3) + 8 * ((X + 1) >> 2) - 2 * X0;
        asm volatile("ds_write_b16 %0, %1 offset:%2" : : "v"(base), "v"(u), "i"(f0 * 1024) : "memory");
        asm volatile("ds_write_b16_d16_hi %0, %1 offset:%2" : : "v"(base), "v"(u), "i"(f1 * 1024) : "memory");
        img_w8<T, X0, X + 2>(base, acc);
    }
}

struct StripPos {                                    // one strip: batch slab, window row, first window
    int b, wy, y0, wx0, nvalid;
};

template <class T, int D, int DV, bool PARTIAL>
__global__ __launch_bounds__(512, 1) void win_bwd_strip(const T* __restrict__ q, const T* __restrict__ k,
                                                        const T* __restrict__ v, const T* __restrict__ dy,
                                                        const float* __restrict__ lw, const float* __restrict__ mw,
                                                        T* __restrict__ dq, T* __restrict__ dk, T* __restrict__ dvo,
                                                        WinDev g, int d, int dv, int nsx, int k0, int nstrip,
                                                        unsigned* __restrict__ ctr, float scale, float scale_log2) {
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    static_assert(D % 32 == 0 && D <= 64 && DV % 32 == 0 && DV <= 64, "head dims");
    constexpr int NQK = D / 16, NOV = DV / 16, NA = NQK + NOV;   // loads: (Q, K), then (dO, V) 16-feature chunks
    constexpr int NC = D / 32, NCV = DV / 32;        // 32-feature output chunks of dQ / dK and of dV
    constexpr int R = 4, BUF = 32768, IMG = 16384;
    static_assert(NA >= R, "every ring slot is a load of the strip");
    __shared__ __attribute__((aligned(16))) char smem[R * BUF + IMG + 2 * 2 * 8 * 64 * 4 + 16];
    char* const img = smem + R * BUF;                // 16-feature gradient image
    float* const lms = (float*)(img + IMG);          // l, m of a strip's windows: [parity][l | m][window][64]
    unsigned* const nsid_lds = (unsigned*)(img + IMG + 2 * 2 * 8 * 64 * 4);   // the next strip, broadcast

    // lane-derived values are re-derived from an opaque copy of threadIdx.x in every strip
    // iteration: hoisted out of the loop, their many per-lane addresses would stay live and spill
    int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W_ = g.S[0], H_ = g.S[1], P_ = g.P, ws = g.ws, st = g.stride, nwx = g.O[0];
    auto pos_of = [&](int sid) __attribute__((always_inline)) {
        const int sxi = sid % nsx, t0 = sid / nsx;
        StripPos p;
        p.wy = t0 % g.O[1];
        p.b = t0 / g.O[1];
        p.wx0 = sxi == 0 ? 0 : k0 + (sxi - 1) * kStripW;
        p.y0 = p.wy * st - g.pad;
        p.nvalid = min(sxi == 0 ? k0 : kStripW, nwx - p.wx0);
        return p;
    };
    auto ax_of = [&](const StripPos& p, int w) __attribute__((always_inline)) {
        return min(max(((p.wx0 + w) * st - g.pad) & ~1, 0), W_ - 8);
    };
    // one DMA instruction = one feature row fl of an Sᵀ-style image: lane -> (slot row, window)
    auto dma_qk = [&](const StripPos& p, __amdgpu_buffer_rsrc_t rs, char* im, int fl, int fg, int C)
        __attribute__((always_inline)) {
        const int pc = lane >> 3, pw = lane & 7;
        const int w = pw ^ sqk_swz(fl, pc), y = p.y0 + pc;
        const bool ok = w < p.nvalid && pc < ws && y >= 0 && y < H_ && fg < C;
        const int off = ok ? (fg * P_ + y * W_ + ax_of(p, w)) * 2 : 0x7FFFFFF0;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(im + fl * 1024), 16,
                                                 off, 0, 0, 0);
    };
    // VMEM instructions this wave has issued (loads, DMAs, counted stores), and the count
    // right after each ring slot's load: the wait for a slot is vmcnt(issued - mark)
    // (loads, stores and DMA retire in issue order: MI355X_MICROARCH, vmcnt).  Slots are
    // runtime values (a strip's NA loads need not be a multiple of R), so the marks are
    // four scalars, not an array (which would go to scratch).
    int vm_issued = 0;
    int mark0 = 0, mark1 = 0, mark2 = 0, mark3 = 0;
    auto mark_of = [&](int slot) __attribute__((always_inline)) {
        return slot == 0 ? mark0 : slot == 1 ? mark1 : slot == 2 ? mark2 : mark3;
    };
    // load j of strip p into ring slot `slot`: 32 DMA instructions (one feature row each), 4 per
    // wave; a strip's l, m (2 DMA instructions per wave, into parity par) right after its load 0
    auto issue = [&](const StripPos& p, int j, int slot, int par) __attribute__((always_inline)) {
        char* buf = smem + slot * BUF;
        const int64_t bo = (int64_t)p.b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rr = i * 8 + wave;                 // 0..31
            if (j < NQK) {
                if (rr < 16) dma_qk(p, slab_rsrc(q + bo * d * P_, (uint32_t)(d * P_ * 2)), buf, rr, j * 16 + rr, d);
                else dma_qk(p, slab_rsrc(k + bo * d * P_, (uint32_t)(d * P_ * 2)), buf + 16384, rr - 16,
                            j * 16 + rr - 16, d);
            } else {
                if (rr < 16) dma_qk(p, slab_rsrc(dy + bo * dv * P_, (uint32_t)(dv * P_ * 2)), buf, rr,
                                    (j - NQK) * 16 + rr, dv);
                else dma_qk(p, slab_rsrc(v + bo * dv * P_, (uint32_t)(dv * P_ * 2)), buf + 16384, rr - 16,
                            (j - NQK) * 16 + rr - 16, dv);
            }
        }
        vm_issued += 4;
        mark0 = slot == 0 ? vm_issued : mark0;
        mark1 = slot == 1 ? vm_issued : mark1;
        mark2 = slot == 2 ? vm_issued : mark2;
        mark3 = slot == 3 ? vm_issued : mark3;
        if (j == 0) {
            const int64_t wrow = (int64_t)g.T * ((int64_t)nwx * p.wy + (int64_t)g.L * p.b);   // window (0, wy)
            const int off = (wave < p.nvalid && lane < g.T) ? (g.T * (p.wx0 + wave) + lane) * 4 : 0x7FFFFFF0;
            float* dst = lms + par * 1024 + wave * 64;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(slab_rsrc(lw + wrow, (uint32_t)(g.T * nwx * 4)),
                                                     (__attribute__((address_space(3))) void*)dst, 4, off, 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(slab_rsrc(mw + wrow, (uint32_t)(g.T * nwx * 4)),
                                                     (__attribute__((address_space(3))) void*)(dst + 512), 4, off, 0, 0,
                                                     0);
            vm_issued += 2;
        }
    };

    // Strips are dealt dynamically within XCD groups.  Workgroup b belongs to group
    // x = b mod 8 (the XCD the dispatcher deals it to), and group x owns the contiguous
    // strip range [lo, hi), sized in proportion to its M workgroups (>= M strips, as
    // nstrip >= G): its workgroup l takes strips lo + l and lo + l + M, then lo + 2M + c
    // for each c it draws from the group's counter (zeroed by the launcher, 64 B apart).
    // So neighbouring strips of a window row, which share the 128-B lines at their ends,
    // run at about the same time on one XCD and meet in its L2 (dealt chip-wide, each
    // shared line was fetched once per XCD that touched it: 2.0x the algorithmic bytes
    // in FETCH_SIZE, r03_win_strip_pmc.txt).  Workgroups start up to ~20 us apart and run
    // at different speeds; a static deal of 8 strips each left ~11 % of the CUs idle and
    // a ~20 us tail.  The draw for the strip after next is issued by lane 0 of wave 0
    // right after a strip's first wait and counted as a vector-memory op; its answer is
    // certain to have landed at the next strip's first wait (every DMA of that strip was
    // issued after it), where it is broadcast through LDS.
    const int G = (int)gridDim.x;
    const int NG = G < 8 ? G : 8, grp = (int)blockIdx.x % NG;
    const int M = G / NG + (grp < G % NG ? 1 : 0);   // workgroups of the group
    auto cum = [&](int x) { return x * (G / NG) + min(x, G % NG); };   // workgroups of groups < x
    const int lo = (int)((int64_t)nstrip * cum(grp) / G), hi = (int)((int64_t)nstrip * cum(grp + 1) / G);
    unsigned* const gctr = ctr + 16 * grp;
    int sid = lo + (int)blockIdx.x / NG;
    int nsid = sid + M;                              // the strip after cur
    unsigned drawn = 0u;                             // lane 0 of wave 0: the counter's last answer
    StripPos cur = pos_of(sid);
#pragma unroll
    for (int j = 0; j < R; ++j) issue(cur, j, j, 0);
    int gbase = 0;                                   // ring slot of the current strip's load 0

    int g4, kh, qq, pp, sig;
    const unsigned one = std::is_same<T, bf16>::value ? 0x3F80u : 0x3C00u;
    // one-hot B fragment: element e of lane (r, h) is 1 iff 16 s2 + 8 h + e == r
    auto ident = [&](int s2) __attribute__((always_inline)) {
        const int e = r - 16 * s2 - 8 * h;
        u32x4 u = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (e == 2 * i) u[i] = one;
            if (e == 2 * i + 1) u[i] = one << 16;
        }
        return __builtin_bit_cast(F8, u);
    };
    const F8 id0 = ident(0), id1 = ident(1);

    for (int it = 0; sid < hi; ++it) {
        [[maybe_unused]] const int fa_sid = sid;
        FA_BSTAMP(0);
        tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        lane = tid & 63; r = lane & 31; h = lane >> 5;
        g4 = lane >> 4; kh = g4 & 1; qq = (lane & 15) >> 2; pp = lane & 3;
        sig = (pp == 1) ? 2 : (pp == 2) ? 1 : pp;
        bool has_next = false;                       // set at the first wait (refills use it later)
        StripPos nxt = cur;
        const int par = it & 1;
        auto slot_of = [&](int j) __attribute__((always_inline)) { return (gbase + j) & (R - 1); };
        // load j landed in every wave: its own DMA (counted wait), then the LDS barrier
        auto step_wait = [&](int j) __attribute__((always_inline)) {
            __builtin_amdgcn_sched_barrier(0);          // keep each step's work in its step (register pressure)
            wait_vm(vm_issued - mark_of(slot_of(j)));
            if (j == 0 && it > 0 && wave == 0) {
                asm volatile("" : "+v"(drawn));          // landed with this wait (see the deal above)
                if (lane == 0) lds_w32u(nsid_lds, (unsigned)(lo + 2 * M) + drawn);
            }
            lds_barrier();
            if (j == 0) {
                if (it > 0) {
                    nsid = (int)__builtin_bit_cast(unsigned, lds_b32(nsid_lds));
                    lds_wait();
                    asm volatile("" : "+v"(nsid));
                    nsid = __builtin_amdgcn_readfirstlane(nsid);
                }
                has_next = nsid < hi;
                nxt = has_next ? pos_of(nsid) : cur;
                if (wave == 0) {                         // draw the strip after nsid
                    if (lane == 0) drawn = atomic_add_ret(gctr, 1u);
                    vm_issued += 1;
                }
            }
            FA_BSTAMP(1 + j);
        };
        // ring slot of load j is free: issue the load R later in the stream (this strip's, or the next's)
        auto refill = [&](int j) __attribute__((always_inline)) {
            if (j + R < NA) issue(cur, j + R, slot_of(j), par);
            else if (has_next) issue(nxt, j + R - NA, slot_of(j), par ^ 1);
        };

        // ---- this wave's window ----
        const int wl = wave;
        const bool wok = wl < cur.nvalid;
        const int y0 = cur.y0, b = cur.b;
        const int wx = cur.wx0 + wl, xs = wx * st - g.pad, ax = ax_of(cur, wl);
        const int c0 = xs - ax, c1 = c0 + ws;
        auto slot_ok = [&](int s) __attribute__((always_inline)) {   // slot s of this window: a real token of the image
            const int sx = s & 7, sy = s >> 3;
            return wok && sy < ws && sx >= c0 && sx < c1 && y0 + sy >= 0 && y0 + sy < H_;
        };
        // Masking.  Keys: the K / V fragments (A operands; lane = key) are zeroed per lane for
        // keys outside the window (slot row >= ws or column outside [c0, c1)), so Sᵀ and dPᵀ are
        // finite there whatever the neighbour pixels hold; P gets a -inf exponent bias for those
        // keys: per column (register x & 7, wave-uniform) and per slot row (lane half, kb, x >> 3).
        // Queries (lanes): P and dS are selected to 0 outside the window.  Rows outside the image
        // are zero-padding tokens, as in the forward (P > 0, K = V = 0: no contribution).
        bool qv[2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int qs = qb * 32 + r;
            qv[qb] = wok && (qs >> 3) < ws && (qs & 7) >= c0 && (qs & 7) < c1;
        }
        bool kfv[2];                                     // this lane's key (A row) of tr-read block blk: lane i of
        {                                                // a 16-lane group receives column i, i.e. chunk qq
            const int sq = (qq == 1) ? 2 : (qq == 2) ? 1 : qq;   // sig of the supplying lanes
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const int krow = 4 * blk + 2 * kh + (sq >> 1), kcol = 4 * (sq & 1) + (lane & 3);
                kfv[blk] = krow < ws && kcol >= c0 && kcol < c1;
            }
        }
        float colb[8], rowb[2][2];                       // 0 or -inf exponent bias
#pragma unroll
        for (int c = 0; c < 8; ++c) colb[c] = (c >= c0 && c < c1) ? 0.0f : kNegInf;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x2 = 0; x2 < 2; ++x2) rowb[kb][x2] = (kb * 4 + 2 * x2 + h < ws) ? 0.0f : kNegInf;

        f32x16 acc[2][2];                                // Sᵀ over the (Q, K) chunks, then dPᵀ: [key block][query block]
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int x = 0; x < 16; ++x) acc[kb][qb][x] = 0.0f;
        F8 pf[2][2][2], dsf[2][2][2];                    // P, τ dS: [query block][key block][16-key half]
        // phase-B A operands kept in registers (lane r = feature 32 c + r): K rows for dQ
        // (8 consecutive keys of a slot row), Q rows for dK (the transposed fragments'
        // query order 16 s' + 4h + {0..3, 8..11}); read from the phase-A images
        u32x4 kst[NC][2][2];
        u32x2 qlo[NC][2][2], qhi[NC][2][2];

        // ---- phase A ----
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            step_wait(j);
            const char* buf = smem + slot_of(j) * BUF;
            s16x4 rk[2][2], rq[2][2];                    // keys (K / V, permuted), queries (Q / dO)
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const char* a = buf + 16384 + sqk_pos(8 * h + qq, 4 * blk + 2 * kh + (sig >> 1), wl) + (sig & 1) * 8;
                rk[blk][0] = lds_tr16(a);
                rk[blk][1] = lds_tr16(buf + 16384 + sqk_pos(8 * h + qq + 4, 4 * blk + 2 * kh + (sig >> 1), wl) + (sig & 1) * 8);
                const char* aq = buf + sqk_pos(8 * h + qq, 4 * blk + 2 * kh + (pp >> 1), wl) + (pp & 1) * 8;
                rq[blk][0] = lds_tr16(aq);
                rq[blk][1] = lds_tr16(buf + sqk_pos(8 * h + qq + 4, 4 * blk + 2 * kh + (pp >> 1), wl) + (pp & 1) * 8);
            }
            if (j < NQK) {                               // this chunk's 16 features of the K / Q stashes
                const int c = j >> 1, fl = r & 15;
                if ((r >> 4) == (j & 1)) {
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int s2 = 0; s2 < 2; ++s2)
                            kst[c][kb][s2] = lds_b128(buf + 16384 + sqk_pos(fl, kb * 4 + s2 * 2 + h, wl));
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                        for (int s_ = 0; s_ < 2; ++s_) {
                            qlo[c][qb][s_] = lds_b64(buf + sqk_pos(fl, qb * 4 + 2 * s_, wl) + 8 * h);
                            qhi[c][qb][s_] = lds_b64(buf + sqk_pos(fl, qb * 4 + 2 * s_ + 1, wl) + 8 * h);
                        }
                }
            }
            lds_wait();
            if (j < NQK) {
                const int c = j >> 1;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) lds_fence(kst[c][kb][s2]);
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                    for (int s_ = 0; s_ < 2; ++s_) { lds_fence(qlo[c][qb][s_]); lds_fence(qhi[c][qb][s_]); }
            }
            F8 kf[2], qf[2];
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
                for (int i = 0; i < 2; ++i) { lds_fence(rk[blk][i]); lds_fence(rq[blk][i]); }
                u32x4 ku = __builtin_bit_cast(u32x4, __builtin_shufflevector(rk[blk][0], rk[blk][1], 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
                for (int i = 0; i < 4; ++i) ku[i] = kfv[blk] ? ku[i] : 0u;
                kf[blk] = __builtin_bit_cast(F8, ku);
                qf[blk] = __builtin_shufflevector(__builtin_bit_cast(F4, rq[blk][0]), __builtin_bit_cast(F4, rq[blk][1]),
                                                  0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) acc[kb][qb] = mfma32x32x16(kf[kb], qf[qb], acc[kb][qb]);
            if (j < NQK) {                               // a Q / K slot is free at once; dO / V stay for dV
                lds_barrier();
                refill(j);
            }
            if (j == NQK - 1) {                          // Sᵀ complete: P = exp(τS − lse) (bf16), while dO / V load
                const float* ls = lms + par * 1024 + wl * 64;
                float lq[2], mq[2];
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) {
                    const int qs = qb * 32 + r;
                    const int tq = qv[qb] ? (qs >> 3) * ws + (qs & 7) - c0 : 0;   // window token of the query slot
                    lq[qb] = lds_b32(ls + tq);
                    mq[qb] = lds_b32(ls + 512 + tq);
                }
                lds_wait();
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) {
                    lds_fence(lq[qb]);
                    lds_fence(mq[qb]);
                    const float nl = (mq[qb] + __logf(lq[qb])) * kLog2e;
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int x2 = 0; x2 < 2; ++x2) {
                            const float nlb = nl - rowb[kb][x2];           // +inf on slot rows >= ws
                            u32x4 pu;
#pragma unroll
                            for (int e = 0; e < 8; e += 2) {            // packed fp32: v_pk_fma / v_pk_add
                                const int x = 8 * x2 + e;
                                const f32x2 sv = {acc[kb][qb][x], acc[kb][qb][x + 1]};
                                const f32x2 arg = __builtin_elementwise_fma(sv, (f32x2){scale_log2, scale_log2},
                                                                            (f32x2){-nlb, -nlb}) +
                                                  (f32x2){colb[e], colb[e + 1]};
                                const f32x2 pr = {exp2_fast(arg[0]), exp2_fast(arg[1])};
                                pu[e >> 1] = qv[qb] ? pk2<T>(pr) : 0u;
                                acc[kb][qb][x] = acc[kb][qb][x + 1] = 0.0f;
                            }
                            pf[qb][kb][x2] = __builtin_bit_cast(F8, pu);
                        }
                }
                // pin P here, under the dO / V loads (the optimizer would sink it to its first use)
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int x2 = 0; x2 < 2; ++x2) asm volatile("" : "+v"(pf[qb][kb][x2]));
            }
        }

        // ---- D = rowsum(P ∘ dP), τ dS = τ P ∘ (dP − D) per query (lane) ----
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            f32x2 ds2 = {0.0f, 0.0f};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int x = 0; x < 16; x += 2)
                    ds2 = __builtin_elementwise_fma(unpk2<T>(__builtin_bit_cast(u32x4, pf[qb][kb][x >> 3])[(x & 7) >> 1]),
                                                    (f32x2){acc[kb][qb][x], acc[kb][qb][x + 1]}, ds2);
            const float Dq = swap_halves_sum(ds2[0] + ds2[1]);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int x2 = 0; x2 < 2; ++x2) {
                    u32x4 du;
#pragma unroll
                    for (int e = 0; e < 8; e += 2) {
                        const int x = 8 * x2 + e;
                        const f32x2 p2 = unpk2<T>(__builtin_bit_cast(u32x4, pf[qb][kb][x2])[e >> 1]);
                        const f32x2 t = (p2 * ((f32x2){acc[kb][qb][x], acc[kb][qb][x + 1]} - Dq)) * scale;
                        du[e >> 1] = qv[qb] ? pk2<T>(t) : 0u;   // (select: dPᵀ of a query outside the window may be inf)
                    }
                    dsf[qb][kb][x2] = __builtin_bit_cast(F8, du);
                }
        }

        // ---- phase B: dVᵀ = dOᵀ P, dKᵀ = Qᵀ (τ dS), dQᵀ = Kᵀ (τ dS)ᵀ, 32 output features at a time,
        //      each stored through the 16-feature image in two passes ----
        const int xs0 = cur.wx0 * st - g.pad, X0 = xs0 & ~7;   // strip start, its 16-B aligned base
        const int xlo = max(xs0, 0), xhi = min(xs0 + cur.nvalid * ws, W_);
        unsigned cm[4];                                  // slot-column mask of a 16-B row fragment
#pragma unroll
        for (int j = 0; j < 4; ++j)
            cm[j] = ((2 * j >= c0 && 2 * j < c1) ? 0x0000FFFFu : 0u) | ((2 * j + 1 >= c0 && 2 * j + 1 < c1) ? 0xFFFF0000u : 0u);
        const StripStore sp = strip_store_plan(tid, y0, ws, H_, W_, X0, xlo, xhi);
        // one 32 x 32 output block pair (features on accumulator rows, slot kb/qb * 32 + r on the
        // lane) through the image: features 0..15, then 16..31
        auto out_chunk = [&](const f32x16 (&oa)[2], T* base, int C, int fbase) __attribute__((always_inline)) {
            const auto ors = slab_rsrc(base + (int64_t)b * C * P_, (uint32_t)(C * P_ * 2));
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    const int s = blk * 32 + r;
                    if (slot_ok(s) && !(FA_WIN_ABL & 64)) {
                        const uint32_t a0 = lds_off(img) + simg_pos(4 * h, s >> 3, ax + (s & 7) - X0);
                        if (pass == 0) img_w8<T, 0>(a0, oa[blk]);
                        else img_w8<T, 8>(a0, oa[blk]);
                    }
                }
                lds_barrier();
                strip_store16<T, PARTIAL>(img, ors, sp, tid, fbase + 16 * pass, C, P_);
                if (!PARTIAL && !(FA_WIN_ABL & 32)) vm_issued += 2;
                lds_barrier();                           // the image is free again
            }
        };
        // transpose: block (kb, qb) of X (B fragments, queries on lanes) -> keys on lanes, then
        // B fragments [key block][query block][s'] whose query order is 16 s' + 4h + {0..3, 8..11}
        auto transpose = [&](const F8 (&xf)[2][2][2], F8 (&xt)[2][2][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) {
                    f32x16 c;
#pragma unroll
                    for (int x = 0; x < 16; ++x) c[x] = 0.0f;
                    c = mfma32x32x16(xf[qb][kb][0], id0, c);
                    c = mfma32x32x16(xf[qb][kb][1], id1, c);
#pragma unroll
                    for (int x = 0; x < 16; ++x) xt[kb][qb][x >> 3][x & 7] = (T)c[x];
                }
        };
        // keys on lanes: oa[kb] = Σ A(f, queries) · xt[kb]
        // this lane's two column masks (selects, not a lane-indexed array: that went to scratch)
        const unsigned cmh0 = h ? cm[2] : cm[0], cmh1 = h ? cm[3] : cm[1];
        auto keys_out = [&](const u32x2 (&lo)[2][2], const u32x2 (&hi)[2][2], const F8 (&xt)[2][2][2], f32x16 (&oa)[2])
            __attribute__((always_inline)) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int x = 0; x < 16; ++x) oa[kb][x] = 0.0f;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int s_ = 0; s_ < 2; ++s_) {
                    const u32x4 u = {lo[qb][s_][0] & cmh0, lo[qb][s_][1] & cmh1, hi[qb][s_][0] & cmh0, hi[qb][s_][1] & cmh1};
                    const F8 af = __builtin_bit_cast(F8, u);
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) oa[kb] = mfma32x32x16(af, xt[kb][qb][s_], oa[kb]);
                }
        };
        FA_BSTAMP(18);
        F8 xt[2][2][2];
        transpose(pf, xt);
        FA_BSTAMP(19);
        // dVᵀ: dO rows from the (dO, V) images still in the ring; each frees two ring slots
#pragma unroll
        for (int c = 0; c < NCV; ++c) {
            u32x2 lo[2][2], hi[2][2];
            {
                const int j = NQK + 2 * c + (r >> 4);    // this lane's feature's (dO, V) load
                const char* buf = smem + slot_of(j) * BUF;
                const int fl = r & 15;
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                    for (int s_ = 0; s_ < 2; ++s_) {
                        lo[qb][s_] = lds_b64(buf + sqk_pos(fl, qb * 4 + 2 * s_, wl) + 8 * h);
                        hi[qb][s_] = lds_b64(buf + sqk_pos(fl, qb * 4 + 2 * s_ + 1, wl) + 8 * h);
                    }
                lds_wait();
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                    for (int s_ = 0; s_ < 2; ++s_) { lds_fence(lo[qb][s_]); lds_fence(hi[qb][s_]); }
            }
            lds_barrier();                               // every wave has read both slots
            if (c == 0) FA_BSTAMP(20);
            f32x16 oa[2];
            keys_out(lo, hi, xt, oa);
            refill(NQK + 2 * c);
            refill(NQK + 2 * c + 1);
            if (c == 0) FA_BSTAMP(21);
            out_chunk(oa, dvo, dv, 32 * c);
            FA_BSTAMP(9 + c);
        }
        // dKᵀ (keys on lanes), from the Q stash
        transpose(dsf, xt);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            f32x16 oa[2];
            keys_out(qlo[c], qhi[c], xt, oa);
            out_chunk(oa, dk, d, 32 * c);
            FA_BSTAMP(11 + c);
        }
        // dQᵀ (queries on lanes), from the K stash
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            f32x16 oa[2];
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int x = 0; x < 16; ++x) oa[qb][x] = 0.0f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    u32x4 kr = kst[c][kb][s2];
#pragma unroll
                    for (int i = 0; i < 4; ++i) kr[i] &= cm[i];
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb)
                        oa[qb] = mfma32x32x16(__builtin_bit_cast(F8, kr), dsf[qb][kb][s2], oa[qb]);
                }
            out_chunk(oa, dq, d, 32 * c);
            FA_BSTAMP(13 + c);
        }
        FA_BSTAMP(15);
        cur = nxt;
        sid = nsid;
        gbase = (gbase + NA) & (R - 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last draw and stores retire before exit
}

// fp32 fused windowed BACKWARD (same shapes as win_rows_f32, stride >= ws so
// dyw = dy and the fold is a direct store).  Staging as win_rows_f32 for q, k, v,
// dy; y rows feed D = rowsum(dy ∘ y) by LDS float adds.  Phase 1, wave (qb, kb):
// S and dP blocks (queries on accumulator rows, keys on lanes) on exact-f32 MFMA,
// P = exp2(c (S − lse/τ)), dS = P (dP − D), both written to [query][65] LDS rows.
// Phase 2: 12 output blocks over the 4 waves with every operand read from LDS:
// dVᵀ = dOᵀ P, dKᵀ = τ Qᵀ dS (contraction over queries), dQᵀ = τ Kᵀ dSᵀ
// (contraction over keys); each lane stores one slot's features to its pixel.
template <int D, int DV>
__global__ __launch_bounds__(256) void win_bwd_f32(const float* __restrict__ q, const float* __restrict__ k,
                                                   const float* __restrict__ v, const float* __restrict__ y,
                                                   const float* __restrict__ dy, const float* __restrict__ lw,
                                                   const float* __restrict__ mw, float* __restrict__ dq,
                                                   float* __restrict__ dk, float* __restrict__ dvo, WinDev g, int d,
                                                   int dv, float scale, float scale_log2) {
    constexpr int NTH = 256, ROW = 65;
    constexpr int QI = 0, KI = D * ROW, VI = 2 * D * ROW, DOI = VI + DV * ROW, PI = DOI + DV * ROW,
                  DSI = PI + 64 * ROW, LSEI = DSI + 64 * ROW, DI = LSEI + 64, REGION = DI + 64;
    constexpr int NIQ = D * 8 / NTH, NIV = DV * 8 / NTH;
    static_assert(D * 8 % NTH == 0 && DV * 8 % NTH == 0, "item split");
    extern __shared__ float sm[];
    (void)REGION;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W_ = g.S[0], H_ = g.S[1], P_ = g.P, ws = g.ws, st = g.stride;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int wx = bid % g.O[0], wy = (bid / g.O[0]) % g.O[1], b = bid / (g.O[0] * g.O[1]);
    const int xs = wx * st - g.pad, y0 = wy * st - g.pad;
    const int ax = min(max(xs, 0), W_ - 8);
    const int sh = xs - ax;
    const int64_t wid = (int64_t)(wx + g.O[0] * wy) + (int64_t)g.L * b;
    auto item_off = [&](int it, int C) {
        const int yy = it & 7, f = it >> 3, yr = y0 + yy;
        const bool ok = yy < ws && yr >= 0 && yr < H_ && f < C;
        return ok ? (f * P_ + yr * W_ + ax) * 4 : 0x7FFFFFE0;
    };
    const auto qrs = slab_rsrc(q + (int64_t)b * d * P_, (uint32_t)(d * P_ * 4));
    const auto krs = slab_rsrc(k + (int64_t)b * d * P_, (uint32_t)(d * P_ * 4));
    const auto vrs = slab_rsrc(v + (int64_t)b * dv * P_, (uint32_t)(dv * P_ * 4));
    const auto yrs = slab_rsrc(y + (int64_t)b * dv * P_, (uint32_t)(dv * P_ * 4));
    const auto drs = slab_rsrc(dy + (int64_t)b * dv * P_, (uint32_t)(dv * P_ * 4));
    u32x4 rq[NIQ][2], rk[NIQ][2], rv[NIV][2], rd[NIV][2], ry[NIV][2];
#pragma unroll
    for (int j = 0; j < NIQ; ++j) {
        const int o = item_off(tid + NTH * j, d);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            rq[j][hh] = __builtin_amdgcn_raw_buffer_load_b128(qrs, o + 16 * hh, 0, 0);
            rk[j][hh] = __builtin_amdgcn_raw_buffer_load_b128(krs, o + 16 * hh, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < NIV; ++j) {
        const int o = item_off(tid + NTH * j, dv);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            rv[j][hh] = __builtin_amdgcn_raw_buffer_load_b128(vrs, o + 16 * hh, 0, 0);
            rd[j][hh] = __builtin_amdgcn_raw_buffer_load_b128(drs, o + 16 * hh, 0, 0);
            ry[j][hh] = __builtin_amdgcn_raw_buffer_load_b128(yrs, o + 16 * hh, 0, 0);
        }
    }
    if (tid < 64) {
        const int tx = tid & 7, ty = tid >> 3;
        float nl = kNegInf;
        if (tx < ws && ty < ws) {
            const int64_t li = ty * ws + tx + (int64_t)g.T * wid;
            nl = -(mw[li] + __logf(lw[li])) / scale;
        }
        sm[LSEI + tid] = nl;
        sm[DI + tid] = 0.0f;
    }
    bool valid[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) valid[t] = t < ws && xs + t >= 0 && xs + t < W_;
    auto pix = [&](const u32x4 (&raw)[2], int t) {
        const int src = t + sh;
        unsigned val = 0u;
#pragma unroll
        for (int e = 0; e < 8; ++e) val = src == e ? (e < 4 ? raw[0][e] : raw[1][e - 4]) : val;
        return valid[t] ? __uint_as_float(val) : 0.0f;
    };
    auto stage = [&](const u32x4 (&raw)[2], int it, int img) {
        const int yy = it & 7, f = it >> 3;
#pragma unroll
        for (int t = 0; t < 8; ++t) sm[img + f * ROW + yy * 8 + t] = pix(raw, t);
    };
#pragma unroll
    for (int j = 0; j < NIQ; ++j) {
        stage(rq[j], tid + NTH * j, QI);
        stage(rk[j], tid + NTH * j, KI);
    }
    __syncthreads();   // D zeroed before the adds
#pragma unroll
    for (int j = 0; j < NIV; ++j) {
        const int it = tid + NTH * j, yy = it & 7, f = it >> 3;
        stage(rv[j], it, VI);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float a = pix(rd[j], t), yv = pix(ry[j], t);
            sm[DOI + f * ROW + yy * 8 + t] = a;
            const float pr = a * yv;
            if (pr != 0.0f) atomicAdd(&sm[DI + yy * 8 + t], pr);
        }
    }
    __syncthreads();

    // ---- phase 1: S, dP blocks (qb, kb) of this wave ----
    const int qb = wave & 1, kb = wave >> 1;
    f32x16 sa, pa;
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        const int qs = qb * 32 + acc_row(x, h);
        sa[x] = sm[LSEI + qs];
        pa[x] = -sm[DI + qs];
    }
#pragma unroll
    for (int t = 0; t < D / 2; ++t)
        sa = mfma32x32x2(sm[QI + (2 * t + h) * ROW + qb * 32 + r], sm[KI + (2 * t + h) * ROW + kb * 32 + r], sa);
#pragma unroll
    for (int t = 0; t < DV / 2; ++t)
        pa = mfma32x32x2(sm[DOI + (2 * t + h) * ROW + qb * 32 + r], sm[VI + (2 * t + h) * ROW + kb * 32 + r], pa);
    const int kslot = kb * 32 + r;
    const bool kvalid = (kslot & 7) < ws && (kslot >> 3) < ws;
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        const int qs = qb * 32 + acc_row(x, h);
        const float pr = kvalid ? exp2_fast(sa[x] * scale_log2) : 0.0f;
        sm[PI + qs * ROW + kslot] = pr;
        sm[DSI + qs * ROW + kslot] = pr * pa[x];
    }
    __syncthreads();

    // ---- phase 2 ----
    auto store_px = [&](float* out, int C, int slot, int fbase, const f32x16& acc, float mul) {
        const int tx = slot & 7, ty = slot >> 3, px = xs + tx, py = y0 + ty;
        if (tx < ws && ty < ws && px >= 0 && px < W_ && py >= 0 && py < H_) {
            float* ob = out + (int64_t)b * C * P_ + (int64_t)py * W_ + px;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = fbase + acc_row(x, h);
                if (f < C) ob[(int64_t)f * P_] = acc[x] * mul;
            }
        }
    };
    constexpr int NDV = DV / 32 * 2, NDK = D / 32 * 2, NBLK = NDV + 2 * NDK;
#pragma unroll
    for (int i = 0; i < (NBLK + 3) / 4; ++i) {
        const int blk = wave + 4 * i;
        if (blk >= NBLK) break;
        f32x16 acc;
#pragma unroll
        for (int x = 0; x < 16; ++x) acc[x] = 0.0f;
        if (blk < NDV) {                              // dVᵀ[cb, kb2] = Σ_q dOᵀ P
            const int cb = blk >> 1, kb2 = blk & 1;
#pragma unroll 8
            for (int t = 0; t < 32; ++t)
                acc = mfma32x32x2(sm[DOI + (cb * 32 + r) * ROW + 2 * t + h], sm[PI + (2 * t + h) * ROW + kb2 * 32 + r], acc);
            store_px(dvo, dv, kb2 * 32 + r, cb * 32, acc, 1.0f);
        } else if (blk < NDV + NDK) {                 // dKᵀ[fb, kb2] = τ Σ_q Qᵀ dS
            const int b2 = blk - NDV, fb = b2 >> 1, kb2 = b2 & 1;
#pragma unroll 8
            for (int t = 0; t < 32; ++t)
                acc = mfma32x32x2(sm[QI + (fb * 32 + r) * ROW + 2 * t + h], sm[DSI + (2 * t + h) * ROW + kb2 * 32 + r], acc);
            store_px(dk, d, kb2 * 32 + r, fb * 32, acc, scale);
        } else {                                      // dQᵀ[fb, qb2] = τ Σ_key Kᵀ dSᵀ
            const int b2 = blk - NDV - NDK, fb = b2 >> 1, qb2 = b2 & 1;
#pragma unroll 8
            for (int t = 0; t < 32; ++t)
                acc = mfma32x32x2(sm[KI + (fb * 32 + r) * ROW + 2 * t + h], sm[DSI + (qb2 * 32 + r) * ROW + 2 * t + h], acc);
            store_px(dq, d, qb2 * 32 + r, fb * 32, acc, scale);
        }
    }
}

// --------------------------------------------------------------------------
// Host side.  win_bwd_plan (fa_windowed.h) names the kernel; the code below launches it.
// --------------------------------------------------------------------------
thread_local int g_win_bwd_grid = 0;   // benchmark knob: the strip backward's workgroups (0: one per CU)

// Before a kernel that stores only the covered pixels: pixels no window covers get zero gradient.
static int zero_uncovered_grads(const WindowedBwdArgs& a, hipStream_t s, const char** why) {
    if (fully_covered(a.g)) return FA_OK;
    const size_t esz = esize(a.dtype);
    hipError_t e;
    if ((e = hipMemsetAsync(a.dq, 0, (size_t)(a.g.P * a.d * a.batch) * esz, s)) != hipSuccess ||
        (e = hipMemsetAsync(a.dk, 0, (size_t)(a.g.P * a.d * a.batch) * esz, s)) != hipSuccess ||
        (e = hipMemsetAsync(a.dv_, 0, (size_t)(a.g.P * a.dv * a.batch) * esz, s)) != hipSuccess)
        return hip_status(e, why);
    return FA_OK;
}

template <class T, int NWIN, int D, int DV>
static void launch_bwd_rows(const WindowedBwdArgs& a, const WinDev& g, hipStream_t s) {
    const int64_t nw = a.g.L * a.batch;
    hipLaunchKernelGGL((win_bwd_rows<T, D, DV, NWIN>), dim3((unsigned)((nw + NWIN - 1) / NWIN)), dim3(256 * NWIN), 0, s,
                       (const T*)a.q, (const T*)a.k, (const T*)a.v, (const T*)a.y, (const T*)a.dy, a.l, a.m,
                       (T*)a.dq, (T*)a.dk, (T*)a.dv_, g, (int)a.d, (int)a.dv, (int)nw, a.scale, a.scale * kLog2e);
}

// bf16 / f16: the per-window and strip kernels
template <class T>
static int windowed_bwd_16bit(const WindowedBwdArgs& a, WinBwdKernel plan, int64_t cus, hipStream_t s,
                              const char** why) {
    const WinDev g = to_dev(a.g);
    if (const int rc = zero_uncovered_grads(a, s, why); rc != FA_OK) return rc;
    switch (plan) {
        case kWinBwdStrip:
        case kWinBwdStripPartial: {
            const int k0 = strip_first(a.g);
            const int64_t nsx = strip_count(a.g, k0), nstrip = nsx * a.g.O[1] * a.batch;
            // persistent: one workgroup per CU, strips dealt by 8 XCD-group counters in the workspace
            const int64_t gmax = g_win_bwd_grid > 0 ? (int64_t)g_win_bwd_grid : cus;
            const int64_t grid = nstrip < gmax ? nstrip : gmax;
            // the counters are atomic words: round their address up to 256 B as the dense
            // backward does (the header allows any workspace alignment; windowed_workspace
            // reserves the 256-B slack, and its buffers are far larger than the 512 B used)
            unsigned* const ctr = (unsigned*)(((uintptr_t)a.workspace + 255) & ~(uintptr_t)255);
            if (!a.workspace || a.workspace_bytes < (size_t)((char*)ctr - (char*)a.workspace) + 512) {
                *why = "workspace missing (the strip backward keeps its strip counters there)";
                return FA_ERR_WORKSPACE;
            }
            if (const int rc = hip_status(hipMemsetAsync(ctr, 0, 512, s), why); rc != FA_OK)   // 8 group counters, 64 B apart
                return rc;
            by_head_class(a.d, a.dv, [&](auto D, auto DV) {
                auto strip = [&](auto PARTIAL) {
                    hipLaunchKernelGGL((win_bwd_strip<T, D, DV, PARTIAL>), dim3((unsigned)grid), dim3(512), 0, s,
                                       (const T*)a.q, (const T*)a.k, (const T*)a.v, (const T*)a.dy, a.l, a.m, (T*)a.dq,
                                       (T*)a.dk, (T*)a.dv_, g, (int)a.d, (int)a.dv, (int)nsx, k0, (int)nstrip, ctr,
                                       a.scale, a.scale * kLog2e);
                };
                if (plan == kWinBwdStrip) strip(std::false_type{});
                else strip(std::true_type{});
            });
            break;
        }
        case kWinBwdRows128:
            launch_bwd_rows<T, 1, 128, 128>(a, g, s);
            break;
        case kWinBwdRows2:
        case kWinBwdRows1:
            by_head_class(a.d, a.dv, [&](auto D, auto DV) {
                if (plan == kWinBwdRows2) launch_bwd_rows<T, 2, D, DV>(a, g, s);
                else launch_bwd_rows<T, 1, D, DV>(a, g, s);
            });
            break;
        default:
            *why = "windowed backward: no 16-bit kernel for this plan";
            return FA_ERR_UNSUPPORTED;
    }
    return launch_status(why);
}

static int windowed_bwd_f32(const WindowedBwdArgs& a, hipStream_t s, const char** why) {
    const WinDev g = to_dev(a.g);
    if (const int rc = zero_uncovered_grads(a, s, why); rc != FA_OK) return rc;
    by_head_class(a.d, a.dv, [&](auto D, auto DV) {
        constexpr int Dc = D, DVc = DV;
        const size_t lds = (size_t)(2 * Dc * 65 + 2 * DVc * 65 + 2 * 64 * 65 + 128) * 4;
        (void)hipFuncSetAttribute((const void*)win_bwd_f32<Dc, DVc>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((win_bwd_f32<Dc, DVc>), dim3((unsigned)(a.g.L * a.batch)), dim3(256), lds, s, (const float*)a.q,
                           (const float*)a.k, (const float*)a.v, (const float*)a.y, (const float*)a.dy, a.l, a.m,
                           (float*)a.dq, (float*)a.dk, (float*)a.dv_, g, (int)a.d, (int)a.dv, a.scale, a.scale * kLog2e);
    });
    return launch_status(why);
}

// the composed path: gather, dense forward (for the per-window outputs) and backward, fold
template <class T>
static int windowed_bwd_composed(const WindowedBwdArgs& a, hipStream_t s, const char** why) {
    const WinDev g = to_dev(a.g);
    const int64_t tok = a.g.T * a.g.L * a.batch;
    const int64_t nb = a.g.L * a.batch;
    char* ws = (char*)(((uintptr_t)a.workspace + 255) & ~(uintptr_t)255);
    auto take = [&](size_t bytes) { void* p = ws; ws += align256(bytes); return p; };
    void* qw = take(tok * a.d * sizeof(T));
    void* kw = take(tok * a.d * sizeof(T));
    void* vw = take(tok * a.dv * sizeof(T));
    void* ow = take(tok * a.dv * sizeof(T));
    void* dyw = take(tok * a.dv * sizeof(T));
    void* dqw = take(tok * a.d * sizeof(T));
    void* dkw = take(tok * a.d * sizeof(T));
    void* dvw = take(tok * a.dv * sizeof(T));
    float* lw = (float*)take(tok * 4);
    float* mw = (float*)take(tok * 4);
    const size_t dws = dense_bwd_workspace(a.dtype, a.g.T, a.g.T, a.d, a.dv, nb);
    void* dwork = take(dws);
    const size_t fws = dense_fwd_workspace(a.dtype, a.g.T, a.g.T, a.d, a.dv, nb);
    void* fwork = take(fws);
    hipError_t e;
    if ((e = gather<T>(a.q, qw, (int)a.d, a.batch, g, false, s)) != hipSuccess ||
        (e = gather<T>(a.k, kw, (int)a.d, a.batch, g, false, s)) != hipSuccess ||
        (e = gather<T>(a.v, vw, (int)a.dv, a.batch, g, false, s)) != hipSuccess ||
        (e = gather<T>(a.dy, dyw, (int)a.dv, a.batch, g, true, s)) != hipSuccess)
        return hip_status(e, why);
    // per-window outputs O_w (the backward's D = rowsum(dO_w ∘ O_w) needs them)
    DenseArgs da{a.dtype, qw, kw, vw, ow, lw, mw, a.g.T, a.g.T, a.d, a.dv, nb, a.scale};
    da.scale64 = a.scale64;
    da.workspace = fwork;
    da.workspace_bytes = fws;
    int rc = launch_dense_fwd(da, s, why);
    if (rc != FA_OK) return rc;
    DenseBwdArgs ba{a.dtype, qw, kw, vw, ow, dyw, a.l, a.m, dqw, dkw, dvw, a.g.T, a.g.T, a.d, a.dv, nb,
                    a.scale, dwork, dws};
    ba.scale64 = a.scale64;
    rc = launch_dense_bwd(ba, s, why);
    if (rc != FA_OK) return rc;
    if ((e = fold<T>(dqw, a.dq, (int)a.d, a.batch, g, false, s)) != hipSuccess ||
        (e = fold<T>(dkw, a.dk, (int)a.d, a.batch, g, false, s)) != hipSuccess ||
        (e = fold<T>(dvw, a.dv_, (int)a.dv, a.batch, g, false, s)) != hipSuccess)
        return hip_status(e, why);
    return FA_OK;
}

int launch_windowed_bwd(const WindowedBwdArgs& a, hipStream_t s, const char** why) {
    if (const int rc = win_args_fit(a.g, a.d, a.dv, a.batch, why); rc != FA_OK) return rc;
    const int64_t cus = win_cus(device_cus(s));
    const WinBwdKernel plan =
        win_bwd_plan(a.dtype, a.g, a.d, a.dv, a.batch, g_win_force_composed,
                     aligned16(a.q) && aligned16(a.k) && aligned16(a.v) && aligned16(a.y) && aligned16(a.dy),
                     aligned16(a.dq) && aligned16(a.dk) && aligned16(a.dv_), cus);
    if (plan == kWinBwdF32) return windowed_bwd_f32(a, s, why);
    if (plan != kWinBwdComposed) {
        if (a.dtype == FA_DTYPE_BF16) return windowed_bwd_16bit<bf16>(a, plan, cus, s, why);
        return windowed_bwd_16bit<f16>(a, plan, cus, s, why);
    }
    switch (a.dtype) {
        case FA_DTYPE_BF16: return windowed_bwd_composed<bf16>(a, s, why);
        case FA_DTYPE_F16: return windowed_bwd_composed<f16>(a, s, why);
        case FA_DTYPE_F32: return windowed_bwd_composed<float>(a, s, why);
        case FA_DTYPE_F64: return windowed_bwd_composed<double>(a, s, why);
    }
    *why = "unknown dtype";
    return FA_ERR_INVALID_ARG;
}

}  // namespace fa
