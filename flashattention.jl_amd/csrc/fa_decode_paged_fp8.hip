// fa_decode_paged_fp8.hip — decode attention over a PAGED fp8 (e4m3fn) KV cache for gfx950
// (MI355X, CDNA4): fa_decode_fp8.hip's arithmetic on fa_decode_paged.hip's cache layout
// (fa_decode_paged_fp8_fwd).
//
// K8_pages (page_size, d, num_pages) and V8_pages (page_size, dv, num_pages) are pools of BYTE
// pages, keys contiguous per feature; block_table (max_pages, batch) names, per KV slab, the page
// of each run of page_size logical keys; k_scale / v_scale hold one float per KV slab.  The cache
// is never gathered and never widened: the table is read on the device, ahead of the loads that
// need it, and the bytes are converted in registers right before the MFMAs.
//
// From decode8_fwd (fa_decode_fp8.hip), unchanged: the 32-row tile, batch x nsplit workgroups of
// 4 waves under xcd_remap, alternate 64-key tiles per wave, the wave-private double-buffered K
// image [D][64 keys] of bytes with the 16-B chunk XOR swizzle, ds_read_b64_tr_b8 and the packed
// fp8 converts, V as 16 B per lane per 32 keys with two v_permlane32_swap, V one tile ahead in
// registers, no workgroup barrier in the key loop, the lazy-rescale softmax, the merge in wave
// order, decode8_combine, and the scales (ks in the score scale, vs once where O is normalised).
// With one byte per element the page geometry is not fa_decode_paged.hip's:
//
//  * TILE (page_size % 64 == 0): a key tile lies in one page.  The wave reads ONE table entry per
//    tile (a uniform load, v_readfirstlane, clamp to [0, num_pages)) and builds the tile's K and V
//    buffer descriptors from it: base = pool + page * page_bytes + row0 (64-bit, byte units; row0
//    the tile's first row in its page), num_records = the rest of that page.  K goes into the
//    image by D / 16 LDS-DMA instructions of 1 KiB with the tile-invariant lane offsets
//    f * page_size + kkey, V by buffer_load_b128 at f * page_size + kb * 32 + 16 h; a feature
//    >= d or dv reads 0 through kDec8OobOff and no offset can leave the page;
//  * CHUNK (every other multiple of 16): a 64-key tile spans several pages, but each 16-B chunk
//    of 16 keys lies in one.  A lane's K chunk is the same 16 keys of the tile for every feature
//    row it stages (the swizzle depends on lane / 4 only, and the rows of one lane are 16 apart),
//    so it needs ONE look-up for K and two for V (the 32-key blocks kb = 0, 1): three per lane
//    and tile where the 16-bit kernel needs five.  A chunk whose first key is >= nk is neither
//    looked up nor loaded and reads as zeros.  A chunk is one predicated 16-B global load from a
//    64-bit address; the D / 16 K chunks wait in registers and go to the image by one
//    ds_write_b128 each at the top of their tile's step;
//  * either way the table entries of the wave's tile AFTER NEXT (t + 8) are requested when tile
//    t + 4's loads are issued: only the prologue waits on a table read.
//
// The kernel reads entry (j, b) only for j < ceil(nk_b / page_size); whatever an entry holds,
// the clamp keeps every access inside the pools.
#include <type_traits>

#include "fa_common.h"
#include "fa_decode8_params.h"
#include "fa_decode_plan.h"
#include "fa_internal.h"
#include "../../include/fa_hip.h"

namespace fa {

namespace {

struct DecodePaged8Params {
    Decode8Params p;         // K, V: the byte page pools; Nk: the logical capacity max_pages * page_size
    const int32_t* table;    // (max_pages, batch)
    int page_size, num_pages, max_pages;
};

// What a lane keeps of a tile's table look-ups between the request and the loads.  TILE: one
// entry for the wave, rem = the tile's first row in its page.  CHUNK: entry 0 for the lane's K
// chunk, 1..2 for its V chunks, rem = the chunk's first row in its page, < 0 for a chunk that
// starts at or past nk (not looked up, not loaded).  raw is the entry as loaded: the clamp is
// applied where it is used.
template <bool TILE>
struct PageRef8 {
    static constexpr int n = TILE ? 1 : 3;
    int raw[n], rem[n];
};

// 16 keys (16 B) at byte `elem` of page `page` of a pool, zeros where `ok` is false.
__device__ __forceinline__ u32x4 paged8_chunk(const uint8_t* pool, int64_t page_bytes, int page, int elem, bool ok) {
    u32x4 w = {0u, 0u, 0u, 0u};
    if (ok) w = *(const u32x4*)(pool + (int64_t)page * page_bytes + elem);
    return w;
}

// The descriptor over the rest of page `page` from its row `row0` on (both wave-uniform): a
// tile's lane offsets f * page_size + key in tile stay inside the page, kDec8OobOff reads 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t page8_rsrc(const uint8_t* pool, int64_t page_bytes, int page, int row0) {
    return slab_rsrc(pool + (int64_t)page * page_bytes + row0, (uint32_t)(page_bytes - row0));
}

// TILE: one K tile into a wave's LDS image by D / 16 LDS-DMA instructions of 1 KiB (no VGPRs):
// 16-B chunk `it * 64 + lane` is feature it * 16 + kf0, keys kkey .. kkey + 15 of the tile.
template <int D>
__device__ __forceinline__ void paged8_dma_k(__amdgpu_buffer_rsrc_t krs, char* buf, int kkey, int kf0, int d, int ps) {
#pragma unroll
    for (int it = 0; it < D / 16; ++it) {
        const int f = it * 16 + kf0;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (__attribute__((address_space(3))) void*)(buf + it * 1024), 16,
                                                 f < d ? f * ps + kkey : kDec8OobOff, 0, 0, 0);
    }
}

template <class T, int D, int DV, bool TILE>
__global__ __launch_bounds__(kDecodeThreads) void decode_paged8_fwd(DecodePaged8Params pp) {
    typedef typename Frag8<T>::type F8;
    typedef PageRef8<TILE> Pg;
    constexpr int BN = kDecodeKeyTile;
    constexpr int KROW = BN;                 // K image: [D][64 keys] bytes, 64-B rows, 16-B chunk XOR swizzle
    constexpr int KBUF = D * KROW;           // one K tile
    constexpr int MSTAT = DV * 128;          // merge image: [DV][32 rows] floats, then m_true, m_used, l
    constexpr int MBYTES = MSTAT + 3 * 128;
    constexpr int WSTRIDE = 2 * KBUF > MBYTES ? 2 * KBUF : MBYTES;   // a wave's LDS: two K tiles, later its merge image
    __shared__ __attribute__((aligned(1024))) char smem[4 * WSTRIDE];

    const Decode8Params& p = pp.p;
    const int lid = xcd_remap(blockIdx.x, p.total_wg);
    const int b = lid / p.nsplit, sp = lid - b * p.nsplit;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int N = p.N, d = p.d, dv = p.dv, G = p.group, rows = N * G;

    // The slab's extents against its logical capacity p.Nk, its visible tiles [t0, t0 + nt) and
    // this workgroup's share of them, exactly as fa_decode.hip: an empty share stores the empty
    // state and leaves before any table, K or V load.
    const VarlenExt ve = varlen_extents(p.q_lens, p.k_lens, b, N, p.Nk, p.wleft, p.wright);
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

    // ---- the paged cache ----
    const int ps = pp.page_size, last_page = pp.num_pages - 1;
    const int64_t kpage = (int64_t)ps * d, vpage = (int64_t)ps * dv;     // bytes of one page
    const int32_t* const tab = pp.table + (int64_t)b * pp.max_pages;     // read below ceil(nk / ps) only
    const auto clamp_page = [&](int raw) { return min(max(raw, 0), last_page); };

    // K staging: 16-B chunk `it * 64 + lane` of the image (byte it * 1024 + lane * 16) is feature
    // f = it * 16 + lane / 4, physical chunk pc = lane % 4, which holds the 16 keys of logical
    // chunk pc ^ swz(f), swz(f) = bits 1..2 of f: the same for every `it`, so a lane stages the
    // same 16 keys of a tile, kkey .. kkey + 15, for all its D / 16 feature rows.
    const int kf0 = lane >> 2, kpc = lane & 3;
    const int kkey = (kpc ^ ((kf0 >> 1) & 3)) * 16;
    char* const kbuf0 = smem + wave * WSTRIDE;
    char* const kbuf1 = kbuf0 + KBUF;

    // The table look-ups of tile t (t < te, so every key looked up is below nk rounded up to the
    // tile and, per chunk, below nk itself: j < ceil(nk / ps)).
    const auto lookup = [&](int t) {
        Pg pg;
        if constexpr (TILE) {
            const int tpp = ps / BN, j = t / tpp;   // wave-uniform
            pg.raw[0] = tab[j];
            pg.rem[0] = (t - j * tpp) * BN;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int key = t * BN + (c == 0 ? kkey : (c - 1) * 32 + 16 * h);
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
    // TILE: the wave's page, uniform and clamped, and the tile's first row in it
    const auto tile_page = [&](const Pg& pg) { return clamp_page(__builtin_amdgcn_readfirstlane(pg.raw[0])); };
    const auto tile_row0 = [&](const Pg& pg) { return __builtin_amdgcn_readfirstlane(pg.rem[0]); };

    // One K tile.  TILE: D / 16 LDS-DMA instructions of 1 KiB into the image `buf`.  CHUNK: D / 16
    // predicated 16-B loads into kreg, written to the image by write_k when the tile's turn comes.
    u32x4 kreg[TILE ? 1 : D / 16];
    const auto stage_k = [&](char* buf, const Pg& pg) {
        if constexpr (TILE) {
            paged8_dma_k<D>(page8_rsrc(p.K, kpage, tile_page(pg), tile_row0(pg)), buf, kkey, kf0, d, ps);
        } else {
            const int page = clamp_page(pg.raw[0]);
#pragma unroll
            for (int it = 0; it < D / 16; ++it) {
                const int f = it * 16 + kf0;
                kreg[it] = paged8_chunk(p.K, kpage, page, f * ps + pg.rem[0], pg.rem[0] >= 0 && f < d);
            }
        }
    };
    const auto write_k = [&](char* buf) {
        if constexpr (!TILE) {
#pragma unroll
            for (int it = 0; it < D / 16; ++it) *(u32x4*)(buf + it * 1024 + lane * 16) = kreg[it];
        }
    };
    // V (A operand of O^T += V P^T), feature cb * 32 + r, per 32-key block kb the 16 contiguous
    // bytes of keys kb * 32 + 16 h .. + 15: the 4-key chunks 4 h .. 4 h + 3 of the block, which
    // v_swap (in compute, once they have landed) brings to the order of this lane half's P values.
    constexpr int NV = DV / 32 * 2;
    const auto load_v = [&](u32x4 (&v)[NV], const Pg& pg) {
        if constexpr (TILE) {
            const auto vrs = page8_rsrc(p.V, vpage, tile_page(pg), tile_row0(pg));
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    const int f = cb * 32 + r;
                    v[cb * 2 + kb] = __builtin_amdgcn_raw_buffer_load_b128(vrs, f < dv ? f * ps + kb * 32 + 16 * h : kDec8OobOff, 0, 0);
                }
        } else {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int page = clamp_page(pg.raw[1 + kb]), rem = pg.rem[1 + kb];
#pragma unroll
                for (int cb = 0; cb < DV / 32; ++cb) {
                    const int f = cb * 32 + r;
                    v[cb * 2 + kb] = paged8_chunk(p.V, vpage, page, f * ps + rem, rem >= 0 && f < dv);
                }
            }
        }
    };
    // lane half 0 holds chunks (0, 1, 2, 3), half 1 (4, 5, 6, 7); v_permlane32_swap exchanges the
    // upper half of its first operand with the lower half of its second: dwords (0, 1) become
    // chunks (0, 4) | (1, 5) and dwords (2, 3) chunks (2, 6) | (3, 7).
    const auto v_swap = [](u32x4 w) {
        const auto a = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);
        const auto c = __builtin_amdgcn_permlane32_swap(w[2], w[3], false, false);
        return u32x4{a[0], a[1], c[0], c[1]};
    };

    // transposed K reads: in its 16-lane group lane 2 q + p supplies feature row 8 h + q
    // (+ 16 s), the 8 keys p of logical chunk kb * 2 + kh; lane r receives key kb * 32 + r
    const int kh = (lane >> 4) & 1, qq = (lane & 15) >> 1, pp2 = lane & 1;
    int koff[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) koff[kb] = (8 * h + qq) * KROW + (((kb * 2 + kh) ^ ((qq >> 1) & 3)) * 16) + 8 * pp2;

    f32x16 oacc[DV / 32];
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) oacc[cb][x] = 0.0f;
    float m_used = kNegInf, m_true = kNegInf, l_run = 0.0f;
    const float c = sk * kLog2e;
    const float thr_raw = kRescaleLog2 / c;

    // One tile, as decode8_fwd's: S^T from the K image, then (TILE) the next tile's K DMA into the
    // other image, after this tile's LDS reads, which would otherwise wait for it; softmax;
    // O^T += V P^T.  pg_next: the look-ups of tile t + 4.
    const auto compute = [&](const char* kbuf, const u32x4 (&v)[NV], int t, char* knext, const Pg& pg_next) {
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
        if constexpr (TILE) {
            if (t + 4 < te) stage_k(knext, pg_next);
        }
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
            for (int kb = 0; kb < 2; ++kb) {
                const u32x4 w = v_swap(v[cb * 2 + kb]);
#pragma unroll
                for (int s = 0; s < 2; ++s) oacc[cb] = mfma32x32x16(cvt8<T>(w[s], w[s + 2]), pf[kb][s], oacc[cb]);
            }
    };

    // The wave's tiles: ts + wave, + 4, ...  While tile t is computed, tile t + 4's K and V are
    // in flight and so are the table entries of tile t + 8, requested with them; the wait at the
    // top of a step, vmcnt(0) with the other counters left alone, is for this wave's own loads.
    const auto landed = [] {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("" ::: "memory");
    };
    u32x4 v0[NV], v1[NV];
    int t = ts + wave;
    Pg pg = {}, pg_after = {};   // the look-ups of tile t + 4, and those of t + 8 on their way
    const auto step = [&](char* kcur, const u32x4 (&vcur)[NV], u32x4 (&vnext)[NV], char* knext) {
        landed();
        write_k(kcur);
        const bool more = t + 4 < te;
        if (more) {
            if constexpr (!TILE) stage_k(knext, pg);
            load_v(vnext, pg);
        }
        if (t + 8 < te) pg_after = lookup(t + 8);
        compute(kcur, vcur, t, knext, pg);
        pg = pg_after;
        t += 4;
    };
    if (t < te) {
        pg = lookup(t);
        stage_k(kbuf0, pg);
        load_v(v0, pg);
        if (t + 4 < te) pg = lookup(t + 4);
    }
    while (t < te) {
        step(kbuf0, v0, v1, kbuf1);
        if (t >= te) break;
        step(kbuf1, v1, v0, kbuf0);
    }
    asm volatile("" ::: "memory");

    // ---- merge the 4 waves (one barrier), then store: decode8_fwd's epilogue ----
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

template <class T>
hipError_t launch_decode_paged8(const DecodePlan& pl, const DecodePaged8Params& pp, int Dc, int DVc, hipStream_t s) {
    const dim3 grid((unsigned)pl.grid), blk(kDecodeThreads);
    by_dim_class(Dc, [&](auto Dk) {
        by_dim_class(DVc, [&](auto DVk) {
            constexpr int D = decltype(Dk)::value, DV = decltype(DVk)::value;
            if (pl.kernel == kPaged8Tile) hipLaunchKernelGGL((decode_paged8_fwd<T, D, DV, true>), grid, blk, 0, s, pp);
            else hipLaunchKernelGGL((decode_paged8_fwd<T, D, DV, false>), grid, blk, 0, s, pp);
        });
    });
    if (pl.nsplit > 1) launch_decode8_combine(std::is_same<T, f16>::value ? FA_DTYPE_F16 : FA_DTYPE_BF16, pl, pp.p, s);
    return hipGetLastError();
}

}  // namespace

int launch_decode_paged_fp8_fwd(const DecodePagedFp8Args& ap, hipStream_t s, const char** why) {
    const DecodeArgs& a = ap.a;
    const DecodePlan pl = decode_paged_fp8_plan(a.dtype, a.N, a.d, a.dv, a.batch, a.group, ap.page_size, ap.max_pages, g_decode_nsplit);
    if (pl.kernel == kDecodeNone || !aligned16(a.K) || !aligned16(a.V)) {
        *why = "shape outside the paged fp8 decode kernels (api.cpp checks it first)";
        return FA_ERR_UNSUPPORTED;
    }
    if (pl.grid > INT32_MAX || pl.combine_grid > INT32_MAX) {
        *why = "grid too large";
        return FA_ERR_UNSUPPORTED;
    }
    if (pl.total > 0 && (!a.workspace || a.workspace_bytes < pl.total)) {
        *why = "workspace missing or smaller than fa_decode_paged_fp8_fwd_workspace()";
        return FA_ERR_WORKSPACE;
    }
    const MaskInts mi = mask_ints(kMaskVarlen, a.left, a.right, a.N, a.Nk);
    DecodePaged8Params pp;
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
    const int Dc = head_dim_class(a.d), DVc = head_dim_class(a.dv);
    const hipError_t e = a.dtype == FA_DTYPE_F16 ? launch_decode_paged8<f16>(pl, pp, Dc, DVc, s) : launch_decode_paged8<bf16>(pl, pp, Dc, DVc, s);
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return FA_ERR_HIP;
    }
    return FA_OK;
}

}  // namespace fa
