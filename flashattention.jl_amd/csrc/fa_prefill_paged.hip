// fa_prefill_paged.hip — chunked PREFILL attention over a paged KV cache for gfx950 (MI355X,
// CDNA4): fa_decode_paged_fwd's arguments and semantics without its N * group <= 32 row limit
// (fa_prefill_paged_fwd).  A design of its own: where a decode wave walks its own key tiles, here
// many row tiles share each key tile.
//
//  * ROWS.  The N * G query rows of a KV slab are ordered position-major, R = i * G + g, and cut
//    into blocks of kPrefillRows = 128 consecutive R.  One workgroup of 4 waves takes one block,
//    each wave one 32-row MFMA tile of it.  Any G packs without dead rows (only the ragged end and
//    rows i >= nq are dead), and a block spans about 128 / G positions, so its mask edges touch
//    few key tiles.  Row -> (i, g) is one division per lane; the Q^T fragments are gathered once
//    by branch-free 2-byte buffer loads and stay in registers.
//  * K AND V ONCE PER WORKGROUP.  Each 64-key tile of K and of V is staged into LDS once by the
//    256 threads and read by all four waves: HBM and L2 see a tile once per 128 rows.  K is the
//    swizzled [D][64 keys] image that ds_read_tr16 reads (fa_decode.hip's), V a [DV][64 keys]
//    image whose 16-B chunk c of feature f lies at chunk c ^ ((f >> 1) & 7): a lane's ds_read_b128
//    is the A operand of O^T += V P^T, and 16 lanes on 16 features hit 16 different bank groups.
//    Two stages (64 KiB at D = DV = 128), ONE workgroup barrier per tile: at the top of step t a
//    thread waits for its own loads of tile t, the barrier publishes the stage and retires every
//    read of the other one, tile t + 1 is requested into that one, tile t is computed.
//  * ADDRESSING.  TILE (page_size % 64 == 0): a tile lies in one page; one wave-uniform table
//    entry per tile, clamped, makes the K and V buffer descriptors over the rest of that page, and
//    (D + DV) / 32 LDS-DMA instructions of 1 KiB per wave move the tile with no VGPR.  CHUNK
//    (every other multiple of 8): a thread looks up the page of its K chunk and of its V chunk
//    (8 keys, 16 B, always inside one page), loads (D + DV) / 32 chunks under a predicate (a
//    chunk at or past nk is neither looked up nor loaded and reads as zeros) and writes them with
//    ds_write_b128 when the tile's turn comes.  Either way the table entries of tile t + 2 are
//    requested when tile t + 1's loads are issued.
//  * KEY RANGE.  From the first tile of the block's smallest `lo` to the last tile of its largest
//    `hi`, cut into nsplit shares (prefill_paged_plan).  A workgroup with no visible tile stores
//    the empty state and leaves before any table, K or V read.  A wave skips the tiles outside its
//    own rows' range, and applies the select only on tiles that straddle an edge of a live row.
//  * SOFTMAX AND PRODUCTS are the decode kernels': transposed scores on mfma32x32x16, P kept in
//    registers as the B operand of the second product, log2 units with the lazy rescale, the true
//    max carried separately.  No merge across waves: each wave owns its rows.  nsplit > 1 writes
//    fp32 partials in decode_combine's layout and fa_decode.hip's decode_combine merges them: no
//    atomics, every output bitwise reproducible, m the same bits for every nsplit.
//
// The kernel reads table entry (j, b) only for j < ceil(nk_b / page_size) and clamps each to
// [0, num_pages) before it forms an address.
#include <type_traits>

#include "fa_common.h"
#include "fa_decode_params.h"
#include "fa_decode_plan.h"
#include "fa_internal.h"
#include "../../include/fa_hip.h"

namespace fa {

namespace {

struct PrefillPagedParams {
    DecodeParams p;          // K, V: the page pools; Nk: the logical capacity; total_wg: batch * nblk * nsplit
    const int32_t* table;    // (max_pages, batch)
    int page_size, num_pages, max_pages;
    int nblk;                // row blocks per KV slab: ceil(N * group / kPrefillRows)
};

// A thread's table look-ups of one tile between the request and the loads.  TILE: one entry for
// the wave, rem = the tile's first row in its page.  CHUNK: entry 0 for the thread's K chunk, 1
// for its V chunk, rem = the chunk's first row in its page, < 0 for a chunk at or past nk.
template <bool TILE>
struct PrefillPageRef {
    static constexpr int n = TILE ? 1 : 2;
    int raw[n], rem[n];
};

// 8 keys (16 B) at element `elem` of page `page` of a pool, zeros where `ok` is false.
__device__ __forceinline__ u32x4 prefill_chunk(const char* pool, int64_t page_bytes, int page, int elem, bool ok) {
    u32x4 w = {0u, 0u, 0u, 0u};
    if (ok) w = *(const u32x4*)(pool + (int64_t)page * page_bytes + (int64_t)elem * 2);
    return w;
}

// The descriptor over the rest of page `page` from its row `row0` on (both wave-uniform).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t prefill_page_rsrc(const char* pool, int64_t page_bytes, int page, int row0) {
    return slab_rsrc(pool + (int64_t)page * page_bytes + row0 * 2, (uint32_t)(page_bytes - row0 * 2));
}

// The empty state of the block's rows [R0, Rend): O = 0, l = 0, m = -inf (final, or as a partial).
template <class T>
__device__ __forceinline__ void prefill_store_empty(const DecodeParams& p, int b, int sp, int R0, int Rend) {
    const int N = p.N, dv = p.dv, G = p.group, nrow = Rend - R0;
    const int64_t rows = (int64_t)N * G;
    if (p.nsplit == 1) {
        T* const O = (T*)p.O;
        for (int idx = threadIdx.x; idx < nrow * dv; idx += kPrefillThreads) {
            const int f = idx / nrow, R = R0 + idx - f * nrow, i = R / G, g = R - i * G;
            O[(((int64_t)b * G + g) * dv + f) * N + i] = (T)0.0f;
        }
        for (int k = threadIdx.x; k < nrow; k += kPrefillThreads) {
            const int R = R0 + k, i = R / G, g = R - i * G;
            const int64_t Rl = ((int64_t)b * G + g) * N + i;
            p.l[Rl] = 0.0f;
            p.m[Rl] = kNegInf;
        }
    } else {
        for (int idx = threadIdx.x; idx < nrow * (dv + 2); idx += kPrefillThreads) {
            const int k = idx / (dv + 2), c = idx - k * (dv + 2), R = R0 + k, i = R / G, g = R - i * G;
            const int64_t Rl = ((int64_t)b * G + g) * N + i;
            p.part[((int64_t)sp * p.batch * rows + Rl) * (dv + 2) + c] = c == dv + 1 ? kNegInf : 0.0f;
        }
    }
}

// Two waves per SIMD: the register budget (256) that lets two workgroups share a CU wherever the
// LDS does (2 x 64 KiB at D = DV = 128), so one computes while the other waits at its barrier.
template <class T, int D, int DV, bool TILE>
__global__ __launch_bounds__(kPrefillThreads, 2) void prefill_paged_fwd(PrefillPagedParams pp) {
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    typedef PrefillPageRef<TILE> Pg;
    constexpr int BN = kDecodeKeyTile;
    constexpr int KROW = BN * 2;                   // both images: 128-B rows of 64 keys
    constexpr int KBUF = D * KROW, VBUF = DV * KROW;
    constexpr int STAGE = KBUF + VBUF;             // one tile of K and of V
    constexpr int NK = D / 32, NVC = DV / 32;      // 16-B chunks a thread stages per tile of K, of V
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

    const DecodeParams& p = pp.p;
    const int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int per_slab = pp.nblk * p.nsplit;
    const int b = lid / per_slab, in_slab = lid - b * per_slab;
    const int blk = in_slab / p.nsplit, sp = in_slab - blk * p.nsplit;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int N = p.N, d = p.d, dv = p.dv, G = p.group, rows = N * G;

    // The block's rows [R0, Rend), its live positions [ib0, ib1], the tiles [t0, t0 + nt) that some
    // live row of it sees, and this workgroup's share of them.  All workgroup-uniform.
    const VarlenExt ve = varlen_extents(p.q_lens, p.k_lens, b, N, p.Nk, p.wleft, p.wright);
    const int R0 = blk * kPrefillRows, Rend = min(R0 + kPrefillRows, rows);
    const int ib0 = R0 / G, ib1 = min((Rend - 1) / G, ve.nq - 1);
    int t0 = 0, nt = 0;
    if (ib0 <= ib1) {
        const int klo = max(0, ib0 + ve.off - ve.left), khi = min(ve.nk, ib1 + 1 + ve.off + ve.right);
        if (khi > klo) {
            t0 = klo / BN;
            nt = (khi + BN - 1) / BN - t0;
        }
    }
    const int tps = (nt + p.nsplit - 1) / p.nsplit;
    const int ts = t0 + sp * tps, te = min(t0 + nt, ts + tps);
    if (ts >= te) {
        prefill_store_empty<T>(p, b, sp, R0, Rend);
        return;
    }

    // lane (r, h): row R = i * G + g; dead rows (past N * G, or i >= nq) carry zeros
    const int R = R0 + wave * 32 + r;
    const int i = R / G, g = R - i * G;
    const bool in_range = R < rows;
    const bool live_row = in_range && i < ve.nq;
    const int lo_r = live_row ? i + ve.off - ve.left : 0x3FFFFFFF;      // the row's visible keys [lo_r, hi_r]
    const int hi_r = live_row ? min(i + ve.off + ve.right, ve.nk - 1) : -1;
    // the wave's live positions [iw0, iw1]: tiles outside [w_lo_min, w_hi_max] are skipped, tiles
    // inside [w_lo_max, w_hi_min] need no select
    const int Rw0 = R0 + wave * 32, Rw1 = min(Rw0 + 32, rows);
    const int iw0 = Rw0 / G, iw1 = min((Rw1 - 1) / G, ve.nq - 1);
    const bool wave_live = Rw0 < rows && iw0 <= iw1;
    const int w_lo_min = wave_live ? iw0 + ve.off - ve.left : 0x3FFFFFFF;
    const int w_hi_max = wave_live ? min(ve.nk - 1, iw1 + ve.off + ve.right) : -1;
    const int w_lo_max = iw1 + ve.off - ve.left, w_hi_min = min(ve.nk - 1, iw0 + ve.off + ve.right);

    // Q^T fragments (B operand of S^T = K Q^T): k-step s holds Q[row][features 16 s + 8 h ..+7]
    F8 qf[D / 16];
    {
        const auto qrs = slab_rsrc((const T*)p.Q + (int64_t)b * G * d * N, (uint32_t)((int64_t)rows * d * 2));
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

    // ---- the paged cache ----
    const int ps = pp.page_size, last_page = pp.num_pages - 1;
    const int64_t kpage = (int64_t)ps * d * 2, vpage = (int64_t)ps * dv * 2;   // bytes of one page
    const int32_t* const tab = pp.table + (int64_t)b * pp.max_pages;           // read below ceil(nk / ps) only
    const char* const kpool = (const char*)p.K;
    const char* const vpool = (const char*)p.V;
    const auto clamp_page = [&](int raw) { return min(max(raw, 0), last_page); };

    // Staging, shared by the 256 threads: 16-B chunk `it * 256 + tid` of an image (byte
    // (it * 256 + tid) * 16) is feature f = it * 32 + tid / 8, physical chunk spc = tid % 8.  In
    // the K image it holds the keys of logical 32-B block (spc / 2) ^ swz(f), half spc % 2, swz(f)
    // = bit 1 of f; in the V image logical chunk spc ^ ((f >> 1) & 7).  Both are the same for
    // every `it`.
    const int sf0 = tid >> 3, spc = tid & 7;
    const int kkey = (((spc >> 1) ^ (((sf0 >> 1) & 1) << 1)) * 16) + (spc & 1) * 8;
    const int vkey = (spc ^ ((sf0 >> 1) & 7)) * 8;

    // The table look-ups of tile t (t < te: the tile's first key is below nk, and so, per chunk,
    // is every key looked up: j < ceil(nk / ps)).
    const auto lookup = [&](int t) {
        Pg pg;
        if constexpr (TILE) {
            const int tpp = ps / BN, j = t / tpp;   // workgroup-uniform
            pg.raw[0] = tab[j];
            pg.rem[0] = (t - j * tpp) * BN;
        } else {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int key = t * BN + (c == 0 ? kkey : vkey);
                pg.raw[c] = 0;
                pg.rem[c] = -1;
                if (key < ve.nk) {
                    const int j = (int)((unsigned)key / (unsigned)ps);
                    pg.raw[c] = tab[j];
                    pg.rem[c] = key - j * ps;
                }
            }
        }
        return pg;
    };

    // One tile of K and V on its way.  TILE: (D + DV) / 32 LDS-DMA instructions of 1 KiB per wave
    // into stage `st`.  CHUNK: as many predicated 16-B loads into kreg / vreg, which stage_write
    // puts into the stage when the tile's turn comes.
    u32x4 kreg[TILE ? 1 : NK], vreg[TILE ? 1 : NVC];
    const auto stage_load = [&](const Pg& pg, char* st) {
        if constexpr (TILE) {
            const int page = clamp_page(__builtin_amdgcn_readfirstlane(pg.raw[0]));
            const int row0 = __builtin_amdgcn_readfirstlane(pg.rem[0]);
            const auto krs = prefill_page_rsrc(kpool, kpage, page, row0);
            const auto vrs = prefill_page_rsrc(vpool, vpage, page, row0);
            char* const kd = st + wave * 1024;
            char* const vd = st + KBUF + wave * 1024;
#pragma unroll
            for (int it = 0; it < NK; ++it) {
                const int f = it * 32 + sf0;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (__attribute__((address_space(3))) void*)(kd + it * 4096), 16,
                                                         f < d ? (f * ps + kkey) * 2 : kDecOobOff, 0, 0, 0);
            }
#pragma unroll
            for (int it = 0; it < NVC; ++it) {
                const int f = it * 32 + sf0;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (__attribute__((address_space(3))) void*)(vd + it * 4096), 16,
                                                         f < dv ? (f * ps + vkey) * 2 : kDecOobOff, 0, 0, 0);
            }
        } else {
            const int kp = clamp_page(pg.raw[0]), vp = clamp_page(pg.raw[1]);
#pragma unroll
            for (int it = 0; it < NK; ++it) {
                const int f = it * 32 + sf0;
                kreg[it] = prefill_chunk(kpool, kpage, kp, f * ps + pg.rem[0], pg.rem[0] >= 0 && f < d);
            }
#pragma unroll
            for (int it = 0; it < NVC; ++it) {
                const int f = it * 32 + sf0;
                vreg[it] = prefill_chunk(vpool, vpage, vp, f * ps + pg.rem[1], pg.rem[1] >= 0 && f < dv);
            }
        }
    };
    const auto stage_write = [&](char* st) {
        if constexpr (!TILE) {
#pragma unroll
            for (int it = 0; it < NK; ++it) *(u32x4*)(st + (it * 256 + tid) * 16) = kreg[it];
#pragma unroll
            for (int it = 0; it < NVC; ++it) *(u32x4*)(st + KBUF + (it * 256 + tid) * 16) = vreg[it];
        }
    };

    // transposed K reads (fa_fwd.hip): lane r ends up with key pi(r) = r with bits 2 and 3 swapped
    const int kh = (lane >> 4) & 1, ii = lane & 15, qq = ii >> 2, pp4 = ii & 3;
    const int sig = (pp4 == 1) ? 2 : (pp4 == 2) ? 1 : pp4;
    int koff[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
        koff[kb] = (8 * h + qq) * KROW + (((kb * 2 + kh) ^ (((qq >> 1) & 1) << 1)) * 32) + 8 * sig;
    // V reads (A operand of O^T += V P^T): feature cb * 32 + r, keys q * 16 + 8 h ..+7 of the tile
    int voff[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) voff[q] = KBUF + r * KROW + (((q * 2 + h) ^ ((r >> 1) & 7)) * 16);

    f32x16 oacc[DV / 32];
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) oacc[cb][x] = 0.0f;
    float m_used = kNegInf, m_true = kNegInf, l_run = 0.0f;
    const float c = p.scale_log2;
    const float thr_raw = kRescaleLog2 / c;

    // One tile from stage `st`: S^T from the K image, select, softmax, O^T += V P^T from the V image.
    const auto compute = [&](const char* st, int t) {
        f32x16 sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int x = 0; x < 16; ++x) sacc[kb][x] = 0.0f;
#pragma unroll
            for (int s = 0; s < D / 16; ++s) {
                const char* a = st + koff[kb] + 16 * s * KROW;
                const F4 lo = __builtin_bit_cast(F4, ds_read_tr16(a));
                const F4 hi = __builtin_bit_cast(F4, ds_read_tr16(a + 4 * KROW));
                const F8 af = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                sacc[kb] = mfma32x32x16(af, qf[s], sacc[kb]);
            }
        }
        const int key0 = t * BN;
        if (key0 < w_lo_max || key0 + BN - 1 > w_hi_min) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int kt = key0 + kb * 32 + (x & 3) + 4 * ((x >> 2) & 1) + 8 * h + 16 * (x >> 3);
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
        float ps4[4];
        F8 pf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pv = exp2_fast((sacc[kb][x] - msub) * c);
                if (kb == 0 && x < 4) ps4[x] = pv; else ps4[x & 3] += pv;
                pf[kb][x >> 3][x & 7] = (T)pv;
            }
        l_run += (ps4[0] + ps4[1]) + (ps4[2] + ps4[3]);
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const F8 vf = *(const F8*)(st + voff[kb * 2 + s] + cb * 32 * KROW);
                    oacc[cb] = mfma32x32x16(vf, pf[kb][s], oacc[cb]);
                }
    };

    // The workgroup's tiles ts .. te - 1, stage t & 1 ... alternating.  At the top of step t a
    // thread's own loads of tile t have landed (vmcnt(0), the other counters left alone; CHUNK:
    // and are written to the stage); the barrier publishes the stage and retires every wave's
    // reads of the other stage (tile t - 1), into which tile t + 1 is then requested, with the
    // table entries of tile t + 2.
    const auto landed = [] {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("" ::: "memory");
    };
    Pg pg = lookup(ts);
    stage_load(pg, smem);
    if (ts + 1 < te) pg = lookup(ts + 1);
    int cur = 0;
    for (int t = ts; t < te; ++t, cur ^= 1) {
        char* const st = smem + cur * STAGE;
        landed();
        stage_write(st);
        __syncthreads();
        if (t + 1 < te) stage_load(pg, smem + (cur ^ 1) * STAGE);
        if (t + 2 < te) pg = lookup(t + 2);
        const int key0 = t * BN;
        if (key0 <= w_hi_max && key0 + BN - 1 >= w_lo_min) compute(st, t);
    }

    // ---- store: each wave owns its rows ----
    if (!in_range) return;
    m_true = swap_halves_max(m_true);
    const float lw = swap_halves_sum(l_run);
    const float wgt = m_used == kNegInf ? 0.0f : exp2_fast((m_used - m_true) * c);   // l and O relative to the true max
    const float lsum = wgt * lw;
    const bool live = live_row && lsum > 0.0f;   // else O = 0, l = 0, m = -inf, by select
    const int64_t Rl = ((int64_t)b * G + g) * N + i;
    if (p.nsplit == 1) {
        const float inv = 1.0f / lsum;
        T* const Orow = (T*)p.O + ((int64_t)b * G + g) * dv * N + i;
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = cb * 32 + acc_row(x, h);
                if (f < dv) Orow[(int64_t)f * N] = live ? (T)(wgt * oacc[cb][x] * inv) : (T)0.0f;
            }
        if (h == 0) {
            p.l[Rl] = live ? lsum : 0.0f;
            p.m[Rl] = live ? m_true * p.scale : kNegInf;
        }
    } else {
        float* const part = p.part + ((int64_t)sp * p.batch * rows + Rl) * (dv + 2);
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int f = cb * 32 + acc_row(x, h);
                if (f < dv) part[f] = live ? wgt * oacc[cb][x] : 0.0f;
            }
        if (h == 0) {
            part[dv] = live ? lsum : 0.0f;
            part[dv + 1] = live ? m_true : kNegInf;
        }
    }
}

template <class T>
hipError_t launch_prefill_paged(const PrefillPlan& pl, const PrefillPagedParams& pp, int Dc, int DVc, hipStream_t s) {
    const dim3 grid((unsigned)pl.grid), blk(kPrefillThreads);
    by_dim_class(Dc, [&](auto Dk) {
        by_dim_class(DVc, [&](auto DVk) {
            constexpr int D = decltype(Dk)::value, DV = decltype(DVk)::value;
            if (pl.kernel == kPrefillTile) hipLaunchKernelGGL((prefill_paged_fwd<T, D, DV, true>), grid, blk, 0, s, pp);
            else hipLaunchKernelGGL((prefill_paged_fwd<T, D, DV, false>), grid, blk, 0, s, pp);
        });
    });
    if (pl.nsplit > 1) launch_decode_combine(std::is_same<T, f16>::value ? FA_DTYPE_F16 : FA_DTYPE_BF16, pl, pp.p, s);
    return hipGetLastError();
}

}  // namespace

int launch_prefill_paged_fwd(const DecodePagedArgs& ap, hipStream_t s, const char** why) {
    const DecodeArgs& a = ap.a;
    const PrefillPlan pl = prefill_paged_plan(a.dtype, a.N, a.d, a.dv, a.batch, a.group, ap.page_size, ap.max_pages, g_decode_nsplit);
    if (pl.kernel == kDecodeNone || !aligned16(a.K) || !aligned16(a.V)) {
        *why = "shape outside the paged prefill kernels (api.cpp checks it first)";
        return FA_ERR_UNSUPPORTED;
    }
    if (pl.grid > INT32_MAX || pl.combine_grid > INT32_MAX) {
        *why = "grid too large";
        return FA_ERR_UNSUPPORTED;
    }
    if (pl.total > 0 && (!a.workspace || a.workspace_bytes < pl.total)) {
        *why = "workspace missing or smaller than fa_prefill_paged_fwd_workspace()";
        return FA_ERR_WORKSPACE;
    }
    const MaskInts mi = mask_ints(kMaskVarlen, a.left, a.right, a.N, a.Nk);
    PrefillPagedParams pp;
    DecodeParams& p = pp.p;
    p.Q = a.Q; p.K = a.K; p.V = a.V; p.O = a.O; p.l = a.l; p.m = a.m;
    p.q_lens = a.q_lens; p.k_lens = a.k_lens;
    p.part = pl.total ? (float*)al256(a.workspace) : nullptr;
    p.N = (int)a.N; p.Nk = (int)a.Nk; p.d = (int)a.d; p.dv = (int)a.dv;
    p.batch = (int)a.batch; p.group = (int)a.group;
    p.nsplit = pl.nsplit; p.total_wg = (int)pl.grid;
    p.wleft = mi.left; p.wright = mi.right;
    p.scale = a.scale; p.scale_log2 = a.scale * kLog2e;
    pp.table = ap.block_table;
    pp.page_size = (int)ap.page_size;
    pp.num_pages = (int)std::min<int64_t>(ap.num_pages, INT32_MAX);   // an entry is an int32: ids past it cannot be named
    pp.max_pages = (int)ap.max_pages;
    pp.nblk = (int)pl.blocks;
    const int Dc = head_dim_class(a.d), DVc = head_dim_class(a.dv);
    const hipError_t e = a.dtype == FA_DTYPE_F16 ? launch_prefill_paged<f16>(pl, pp, Dc, DVc, s) : launch_prefill_paged<bf16>(pl, pp, Dc, DVc, s);
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    return FA_OK;
}

}  // namespace fa
