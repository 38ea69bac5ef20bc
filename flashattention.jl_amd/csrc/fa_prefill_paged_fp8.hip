// fa_prefill_paged_fp8.hip — chunked PREFILL attention over a paged fp8 (e4m3fn) KV cache for
// gfx950 (MI355X, CDNA4): fa_decode_paged_fp8_fwd's arguments and semantics without its
// N * group <= 32 row limit (fa_prefill_paged_fp8_fwd).  The row split, the key range, the ring
// and the softmax are prefill_paged_fwd's (fa_prefill_paged.hip); the bytes, the converts and the
// scales are decode_paged8_fwd's (fa_decode_paged_fp8.hip); what neither has is a V operand that
// comes out of a shared byte image in LDS.
//
//  * ROWS, KEY RANGE, SPLIT.  R = i * G + g in blocks of kPrefillRows = 128, one workgroup of 4
//    waves per block and one 32-row MFMA tile per wave, Q gathered once into registers; the block's
//    visible tiles are cut into nsplit shares (prefill_paged_fp8_plan); a wave skips the tiles
//    outside its own rows' range and applies the select only on straddling tiles; each wave stores
//    its own rows, fp32 partials in decode8_combine's layout when nsplit > 1.
//  * BYTE STAGES.  A stage is the K image [D][64 keys] and the V image [DV][64 keys] of BYTES, 64-B
//    rows, (D + DV) * 64 B (16 KiB at D = DV = 128); two stages and one workgroup barrier per tile,
//    as the parent.  In both images a row has four 16-B chunks of 16 keys; physical chunk pc of row
//    f holds logical chunk pc ^ swz(f), with swz_K(f) = (f >> 1) & 3 (fa_decode_fp8.hip's, for
//    ds_read_b64_tr_b8) and swz_V(f) = (f >> 2) & 3 (below).
//  * K is read by all four waves with ds_read_tr8 + cvt8: keys arrive in natural order, so
//    accumulator x of lane half h is key acc_row(x, h) of its 32-key block, in the mask select and
//    in the P fragments.
//  * V FROM LDS.  For k-step s of block kb, lane (r, h) needs feature cb * 32 + r and the 4-key
//    pieces h and 2 + h of 16-key chunk kb * 2 + s: two dwords 8 B apart in one 16-B chunk of a
//    byte row.  They are fetched as one two-address dword read (the pair of loads below becomes a
//    ds_read2_b32) and go straight into cvt8: no exchange between lane halves, no select, no
//    VALU instruction beside the four converts.  Banks: a 256-B bank period is four 64-B rows, so
//    a 16-B slot of it is (f mod 4, physical chunk).  The 32 feature rows of one address pass
//    read logical chunk c; with bits 2..3 of the row in the XOR the rows r, r + 4, r + 8, r + 12
//    (the same f mod 4) sit in four different chunks, so the 16 rows r = 0 .. 15 cover the 16
//    slots once, rows 16 .. 31 a second time.  Each slot is thus read by two rows, and by both
//    lane halves at dwords h: 2 lanes per bank on half of the banks, the floor for any fetch in
//    which a lane half reads 8 of a chunk's 16 bytes (the other 8 are the other half's).  A
//    16-B read per lane would be conflict-free and move twice the bytes: the same LDS time.
//  * STAGING.  The stage is (D + DV) / 16 units of 1 KiB (16 feature rows, K's first); unit
//    u = it * 4 + wave belongs to wave `wave`, so "is there a unit", "is it K or V" are
//    wave-uniform and every (D, DV) class stages with all 64 lanes of each instruction busy.
//    Lane l of a unit is row l / 4, physical chunk l % 4: its keys kkey (K units) and vkey
//    (V units) are the same for every unit it stages.
//  * ADDRESSING.  TILE (page_size % 64 == 0): one wave-uniform table entry per tile, clamped,
//    makes the K and V byte descriptors over the rest of that page (page8_rsrc's form), and the
//    workgroup moves a tile by (D + DV) / 16 LDS-DMA instructions of 1 KiB with no VGPR.  CHUNK
//    (every other multiple of 16): a thread looks up the page of its K chunk and of its V chunk
//    (16 keys, 16 B, always inside one page), loads its chunks under a predicate (a chunk at or
//    past nk is neither looked up nor loaded and reads as zeros) and writes them with
//    ds_write_b128 when the tile's turn comes.  Either way the table entries of tile t + 2 are
//    requested when tile t + 1's loads are issued.
//  * SCALES.  Two scalar loads per workgroup after the empty-share exit.  c = scale ks log2 e, the
//    stored m is m_raw scale ks, vs multiplies O once where it is normalised (here when
//    nsplit == 1, else in decode8_combine, whose row -> slab mapping R / N / group holds for any
//    N * group); partials stay unscaled and no element is multiplied by a scale.
//
// The kernel reads table entry (j, b) only for j < ceil(nk_b / page_size) and clamps each to
// [0, num_pages) before it forms an address.
#include <type_traits>

#include "fa_common.h"
#include "fa_decode8_params.h"
#include "fa_decode_plan.h"
#include "fa_internal.h"
#include "../../include/fa_hip.h"

namespace fa {

namespace {

struct PrefillPaged8Params {
    Decode8Params p;         // K, V: the byte page pools; Nk: the logical capacity; total_wg: batch * nblk * nsplit
    const int32_t* table;    // (max_pages, batch)
    int page_size, num_pages, max_pages;
    int nblk;                // row blocks per KV slab: ceil(N * group / kPrefillRows)
};

// A thread's table look-ups of one tile between the request and the loads.  TILE: one entry for
// the wave, rem = the tile's first row in its page.  CHUNK: entry 0 for the thread's K chunk, 1
// for its V chunk, rem = the chunk's first row in its page, < 0 for a chunk at or past nk (or of
// an image the thread's wave stages no unit of).
template <bool TILE>
struct Prefill8PageRef {
    static constexpr int n = TILE ? 1 : 2;
    int raw[n], rem[n];
};

// 16 keys (16 B) at byte `elem` of page `page` of a pool, zeros where `ok` is false.
__device__ __forceinline__ u32x4 prefill8_chunk(const uint8_t* pool, int64_t page_bytes, int page, int elem, bool ok) {
    u32x4 w = {0u, 0u, 0u, 0u};
    if (ok) w = *(const u32x4*)(pool + (int64_t)page * page_bytes + elem);
    return w;
}

// The descriptor over the rest of page `page` from its row `row0` on (both wave-uniform): a
// tile's lane offsets f * page_size + key in tile stay inside the page, kDec8OobOff reads 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t prefill8_page_rsrc(const uint8_t* pool, int64_t page_bytes, int page, int row0) {
    return slab_rsrc(pool + (int64_t)page * page_bytes + row0, (uint32_t)(page_bytes - row0));
}

// The empty state of the block's rows [R0, Rend): O = 0, l = 0, m = -inf (final, or as a partial).
template <class T>
__device__ __forceinline__ void prefill8_store_empty(const Decode8Params& p, int b, int sp, int R0, int Rend) {
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

// Two waves per SIMD, a budget of 256 VGPRs, as the parent; with byte stages the LDS (at most
// 32 KiB) no longer decides how many workgroups share a CU, the registers do.
template <class T, int D, int DV, bool TILE>
__global__ __launch_bounds__(kPrefillThreads, 2) void prefill_paged8_fwd(PrefillPaged8Params pp) {
    typedef typename Frag8<T>::type F8;
    typedef Prefill8PageRef<TILE> Pg;
    constexpr int BN = kDecodeKeyTile;
    constexpr int KROW = BN;                       // both images: 64-B rows of 64 keys
    constexpr int KBUF = D * KROW, VBUF = DV * KROW;
    constexpr int STAGE = KBUF + VBUF;             // one tile of K and of V
    constexpr int KU = D / 16, NU = (D + DV) / 16; // 1-KiB units of 16 rows: K's, then V's
    constexpr int NIT = (NU + 3) / 4;              // units a wave stages per tile, at most
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

    const Decode8Params& p = pp.p;
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
        prefill8_store_empty<T>(p, b, sp, R0, Rend);
        return;
    }
    // the slab's scales (scalar loads): ks folds into the score scale, vs waits for the epilogue
    const float ks = p.k_scale ? p.k_scale[b] : 1.0f, vs = p.v_scale ? p.v_scale[b] : 1.0f;
    const float sk = p.scale * ks;

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
                    __builtin_amdgcn_raw_buffer_load_b16(qrs, (live_row && f < d) ? ((g * d + f) * N + i) * 2 : kDec8OobOff, 0, 0);
                qf[s][e] = __builtin_bit_cast(T, w);
            }
    }

    // ---- the paged cache ----
    const int ps = pp.page_size, last_page = pp.num_pages - 1;
    const int64_t kpage = (int64_t)ps * d, vpage = (int64_t)ps * dv;     // bytes of one page
    const int32_t* const tab = pp.table + (int64_t)b * pp.max_pages;     // read below ceil(nk / ps) only
    const auto clamp_page = [&](int raw) { return min(max(raw, 0), last_page); };

    // Staging: unit u = it * 4 + wave (u < NU) is bytes [u * 1024, + 1024) of the stage, rows
    // 16 u .. + 15 of the K image for u < KU, rows 16 (u - KU) .. + 15 of the V image otherwise;
    // lane l is row sf0 = l / 4 of the unit, physical chunk spc = l % 4.  16 u does not reach the
    // bits of either swizzle, so a lane's K chunks hold keys kkey .. + 15 of the tile and its V
    // chunks vkey .. + 15, whatever the unit.  has_k / has_v: the wave stages a unit of that image.
    const int sf0 = lane >> 2, spc = lane & 3;
    const int kkey = (spc ^ ((sf0 >> 1) & 3)) * 16;
    const int vkey = (spc ^ ((sf0 >> 2) & 3)) * 16;
    bool has_k = false, has_v = false;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int u = it * 4 + wave;
        has_k |= u < KU;
        has_v |= u >= KU && u < NU;
    }

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
                if ((c == 0 ? has_k : has_v) && key < ve.nk) {
                    const int j = (int)((unsigned)key / (unsigned)ps);
                    pg.raw[c] = tab[j];
                    pg.rem[c] = key - j * ps;
                }
            }
        }
        return pg;
    };

    // One tile of K and V on its way.  TILE: the wave's units by LDS-DMA, 1 KiB each, into stage
    // `st`.  CHUNK: as many predicated 16-B loads into creg, which stage_write puts into the stage
    // when the tile's turn comes.
    u32x4 creg[TILE ? 1 : NIT];
    const auto stage_load = [&](const Pg& pg, char* st) {
        if constexpr (TILE) {
            const int page = clamp_page(__builtin_amdgcn_readfirstlane(pg.raw[0]));
            const int row0 = __builtin_amdgcn_readfirstlane(pg.rem[0]);
            const auto krs = prefill8_page_rsrc(p.K, kpage, page, row0);
            const auto vrs = prefill8_page_rsrc(p.V, vpage, page, row0);
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int u = it * 4 + wave;   // wave-uniform, and so are both branches
                if (u < KU) {
                    const int f = u * 16 + sf0;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (__attribute__((address_space(3))) void*)(st + u * 1024), 16,
                                                             f < d ? f * ps + kkey : kDec8OobOff, 0, 0, 0);
                } else if (u < NU) {
                    const int f = (u - KU) * 16 + sf0;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (__attribute__((address_space(3))) void*)(st + u * 1024), 16,
                                                             f < dv ? f * ps + vkey : kDec8OobOff, 0, 0, 0);
                }
            }
        } else {
            const int kp = clamp_page(pg.raw[0]), vp = clamp_page(pg.raw[1]);
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int u = it * 4 + wave;
                if (u < KU) {
                    const int f = u * 16 + sf0;
                    creg[it] = prefill8_chunk(p.K, kpage, kp, f * ps + pg.rem[0], pg.rem[0] >= 0 && f < d);
                } else if (u < NU) {
                    const int f = (u - KU) * 16 + sf0;
                    creg[it] = prefill8_chunk(p.V, vpage, vp, f * ps + pg.rem[1], pg.rem[1] >= 0 && f < dv);
                }
            }
        }
    };
    const auto stage_write = [&](char* st) {
        if constexpr (!TILE) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int u = it * 4 + wave;
                if (u < NU) *(u32x4*)(st + u * 1024 + lane * 16) = creg[it];
            }
        }
    };

    // transposed K reads (fa_decode_fp8.hip): in its 16-lane group lane 2 q + p supplies feature
    // row 8 h + q (+ 16 s), the 8 keys p of logical chunk kb * 2 + kh; lane r receives key kb * 32 + r
    const int kh = (lane >> 4) & 1, qq = (lane & 15) >> 1, pp2 = lane & 1;
    int koff[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) koff[kb] = (8 * h + qq) * KROW + (((kb * 2 + kh) ^ ((qq >> 1) & 3)) * 16) + 8 * pp2;
    // V reads (A operand of O^T += V P^T): feature cb * 32 + r, logical chunk c = kb * 2 + s, the
    // 4-key pieces h (this dword) and 2 + h (8 B on)
    int voff[4];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) voff[cc] = KBUF + r * KROW + ((cc ^ ((r >> 2) & 3)) * 16) + 4 * h;

    f32x16 oacc[DV / 32];
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) oacc[cb][x] = 0.0f;
    float m_used = kNegInf, m_true = kNegInf, l_run = 0.0f;
    const float c = sk * kLog2e;
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
                const i32x2 k8 = ds_read_tr8(st + koff[kb] + 16 * s * KROW);
                sacc[kb] = mfma32x32x16(cvt8<T>((unsigned)k8[0], (unsigned)k8[1]), qf[s], sacc[kb]);
            }
        }
        // accumulator x of lane half h is key acc_row(x, h) of its 32-key block
        const int key0 = t * BN;
        if (key0 < w_lo_max || key0 + BN - 1 > w_hi_min) {
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
                    const unsigned* const v8 = (const unsigned*)(st + voff[kb * 2 + s] + cb * 32 * KROW);
                    oacc[cb] = mfma32x32x16(cvt8<T>(v8[0], v8[2]), pf[kb][s], oacc[cb]);
                }
    };

    // The workgroup's tiles ts .. te - 1, the stages alternating.  At the top of step t a thread's
    // own loads of tile t have landed (vmcnt(0), the other counters left alone; CHUNK: and are
    // written to the stage); the barrier publishes the stage and retires every wave's reads of the
    // other stage (tile t - 1), into which tile t + 1 is then requested, with the table entries of
    // tile t + 2.
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
        const float inv = vs / lsum;             // the V scale, once, where O is normalised
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
            p.m[Rl] = live ? m_true * sk : kNegInf;
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
hipError_t launch_prefill_paged8(const PrefillPlan& pl, const PrefillPaged8Params& pp, int Dc, int DVc, hipStream_t s) {
    const dim3 grid((unsigned)pl.grid), blk(kPrefillThreads);
    by_dim_class(Dc, [&](auto Dk) {
        by_dim_class(DVc, [&](auto DVk) {
            constexpr int D = decltype(Dk)::value, DV = decltype(DVk)::value;
            if (pl.kernel == kPrefill8Tile) hipLaunchKernelGGL((prefill_paged8_fwd<T, D, DV, true>), grid, blk, 0, s, pp);
            else hipLaunchKernelGGL((prefill_paged8_fwd<T, D, DV, false>), grid, blk, 0, s, pp);
        });
    });
    if (pl.nsplit > 1) launch_decode8_combine(std::is_same<T, f16>::value ? FA_DTYPE_F16 : FA_DTYPE_BF16, pl, pp.p, s);
    return hipGetLastError();
}

}  // namespace

int launch_prefill_paged_fp8_fwd(const DecodePagedFp8Args& ap, hipStream_t s, const char** why) {
    const DecodeArgs& a = ap.a;
    const PrefillPlan pl = prefill_paged_fp8_plan(a.dtype, a.N, a.d, a.dv, a.batch, a.group, ap.page_size, ap.max_pages, g_decode_nsplit);
    if (pl.kernel == kDecodeNone || !aligned16(a.K) || !aligned16(a.V)) {
        *why = "shape outside the paged fp8 prefill kernels (api.cpp checks it first)";
        return FA_ERR_UNSUPPORTED;
    }
    if (pl.grid > INT32_MAX || pl.combine_grid > INT32_MAX) {
        *why = "grid too large";
        return FA_ERR_UNSUPPORTED;
    }
    if (pl.total > 0 && (!a.workspace || a.workspace_bytes < pl.total)) {
        *why = "workspace missing or smaller than fa_prefill_paged_fp8_fwd_workspace()";
        return FA_ERR_WORKSPACE;
    }
    const MaskInts mi = mask_ints(kMaskVarlen, a.left, a.right, a.N, a.Nk);
    PrefillPaged8Params pp;
    Decode8Params& p = pp.p;
    p.Q = a.Q; p.K = (const uint8_t*)a.K; p.V = (const uint8_t*)a.V; p.O = a.O; p.l = a.l; p.m = a.m;
    p.k_scale = ap.k_scale; p.v_scale = ap.v_scale;
    p.q_lens = a.q_lens; p.k_lens = a.k_lens;
    p.part = pl.total ? (float*)al256(a.workspace) : nullptr;
    p.N = (int)a.N; p.Nk = (int)a.Nk; p.d = (int)a.d; p.dv = (int)a.dv;
    p.batch = (int)a.batch; p.group = (int)a.group;
    p.nsplit = pl.nsplit; p.total_wg = (int)pl.grid;
    p.wleft = mi.left; p.wright = mi.right;
    p.scale = a.scale;
    pp.table = ap.block_table;
    pp.page_size = (int)ap.page_size;
    pp.num_pages = (int)std::min<int64_t>(ap.num_pages, INT32_MAX);   // an entry is an int32: ids past it cannot be named
    pp.max_pages = (int)ap.max_pages;
    pp.nblk = (int)pl.blocks;
    const int Dc = head_dim_class(a.d), DVc = head_dim_class(a.dv);
    const hipError_t e = a.dtype == FA_DTYPE_F16 ? launch_prefill_paged8<f16>(pl, pp, Dc, DVc, s) : launch_prefill_paged8<bf16>(pl, pp, Dc, DVc, s);
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    return FA_OK;
}

}  // namespace fa
