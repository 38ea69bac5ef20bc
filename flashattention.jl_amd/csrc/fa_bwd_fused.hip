// fa_bwd_fused.hip — dense backward, the single pass: bwd_fused, its protocol (below), the
// asm wrappers it counts its own waits with, and the diagnostic hooks of -DFA_BWD_ABL /
// -DFA_BWD_STAMP4 builds.  Exports launch_fused.
#include <type_traits>
#include <utility>

#include "fa_bwd_common.h"
#include "fa_bwd_params.h"
#include "fa_dense_plan.h"

namespace fa {

// --------------------------------------------------------------------------
// Single-pass backward: the five MFMA products of OneDFastBack
// (src_cpp/FlashAttention.cpp:221-251) — S, dP, dVᵀ += dOᵀP, dKᵀ += QᵀdS and
// dQᵀ += KᵀdSᵀ — in one sweep, instead of the dK/dV pass plus a dQ pass that
// recomputes S and dP (7 products).
//
// A workgroup = 8 waves = 256 keys of one slab (member j of the slab's K = Nk/256
// workgroups); wave w keeps dKᵀ, dVᵀ of its 32 keys in registers (the dK/dV pass's
// layout) and the workgroup sweeps the slab's 64-query slices.  Per slice, dS goes
// through LDS once as a [key][query] image, and wave w computes one 32 x 32 tile of
// dQᵀ over all 256 keys from it and the K image.  The slab's K workgroups sum each
// slice's dQ in a FIXED order (deterministic, no float atomics): member j sweeps the
// slices rotated by 3j (step i: slice (i − 3j) mod T), so the member that adds to a
// slice after member j does so three steps later.  Where that order wraps from member
// K−1 to member 0 it is cut: a slice's members form chain A (the ones that reach it
// first, w0 .. K−1) and chain B (0 .. w0−1), each summed upwards, and dQ = A + B — one
// add, commutative, so the same bits whoever makes it.  Every member therefore waits
// only on the member before it, j − 1, dispatched before it.  The running fp32 sum is
// handed over through the workspace with sc1 stores, a per-slice counter (one lane,
// sc1) that the next member polls (one lane) before a barrier, and sc1 loads
// (MI355X_MICROARCH § visibility, first row of the sc1 hand-off table; 1 WG per CU).
// Chain A's tail stores its total; chain B's tail adds it in when A has finished by
// then (always, solo: A runs ≥ 3 steps earlier) and writes dQ, else stores its own
// total and leaves the add to bwd_dq_fast, which runs after every single pass (the
// slice's fin word, an agent-scope counter both tails add to, reads 2 then).
// Step i of a member, in issue order: B1 (vmcnt(4): slice i's Q/dO DMA landed, step
// i-1's four sum stores may still fly) | phase A, u = 0 | vmcnt(0): step i-1's sums
// stored | u = 1 | lane 0 polls the count of step i+1's slice; the sum loads of step i
// | B2; lane 0 publishes step i-1's count | the row constants and Q/dO DMA of step
// i+1 | the dQ tile (asm LDS reads) | vmcnt(NDMA): the sums landed, added | the sum
// stores (or the tail's dQ stores).  So no barrier waits on a store, and the only
// vmcnt(0) of a step is the one in the middle of phase A.
// No member needs another to be resident: dispatch within an XCD is in launch order,
// so the lowest unfinished workgroup is always on a CU or next in line, and it waits on
// nothing unfinished.  A co-tenant (another stream or process) can slow the chains but
// not strand them.  A poll gives up only if the whole launch publishes nothing for
// 100 ms (see wait_count); it then sets the slab's trip word and the call's status
// word `err`, the slab's other polls stop at once, and the guarded bwd_dq_fast that
// follows recomputes dQ of the slabs that tripped (dK, dV do not depend on the
// hand-off).
// --------------------------------------------------------------------------
// 16-B swizzle of the dSᵀ image, which is written by ds_write_b128 (8 groups of 8
// contiguous lanes, banks mod 128 B) at rows sig32(r) and read only transposed.  A
// write group covers rows {0..3} + {0, 8} (+ 4, 16, 20): the swizzle is a bijection of
// row bits {0, 1, 3}, so its 8 slots differ; its bit 2 = row bit 1, so rows q and
// q ^ 2 of a transposed read sit in opposite 64-B halves of their bank row.  (swz16
// gives rows 0 and 4 the same slot: measured 6.7e7 conflict cycles at N = 8192.)
__device__ __forceinline__ int swzds(int f) { return ((f >> 3) & 1) | ((f & 1) << 1) | (((f >> 1) & 1) << 2); }

// [R rows][64 tokens] LDS image written by 8 waves (cf. dma_image).
template <int R>
__device__ __forceinline__ void dma_image8(__amdgpu_buffer_rsrc_t rs, char* img, int ntok, int t0, int wave, int lane) {
    constexpr int NB = R / 8;                          // 1-KiB blocks
#pragma unroll
    for (int it = 0; it < (NB + 7) / 8; ++it) {
        const int blk = it * 8 + wave;
        if (NB % 8 == 0 || blk < NB) {
            const ImgChunk ch = img_chunk(blk * 64 + lane);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rs, (__attribute__((address_space(3))) void*)(img + blk * 1024), 16,
                (ch.f * ntok + t0 + 8 * ch.c) * 2, 0, 0, 0);
        }
    }
}

__device__ __forceinline__ void arrive(gu32* p) {
    __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane waits until *f >= want (its predecessor in a chain has published).  Every
// such wait is on the previous member of the slab, of lower launch id, so it cannot
// strand (see bwd_fused).  The poll gives up — the slab's trip word *serr and the
// call's status word *herr are set, the slab's other polls stop — only when neither
// the launch's arrival count *garr nor any publish count of the slab's KM members
// (prog[], one plain store per member and step: a single launch-wide counter bumped
// per publish measured 5 % slower, its atomics queueing on one address) has moved for
// stall_ticks (100 ms): a safety net for a dispatcher that broke launch order, not a
// scheduling decision.  A co-tenant that holds CUs for longer than that costs a
// recompute of the slab's dQ, never a wrong result.
__device__ __forceinline__ void wait_count(gu32* f, unsigned want, gu32* serr, gu32* herr, gu32* garr, gu32* prog,
                                           int KM, uint64_t stall_ticks) {
    if (ld_agent(f) >= want) return;
    auto progress = [&]() {
        unsigned sum = ld_agent(garr);
        for (int k = 0; k < KM; ++k) sum += ld_agent(prog + k);
        return sum;
    };
    // the progress counts are first read after 20 us of waiting (not at entry: a
    // short wait — the common case — then costs no more than the polls themselves)
    uint64_t tw = __builtin_amdgcn_s_memrealtime(), tc = tw;
    unsigned seen = 0u;
    bool have = false;
    for (;;) {
        __builtin_amdgcn_s_sleep(1);
        if (ld_agent(f) >= want || ld_agent(serr) != 0u) return;
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (now - tc < 2000) continue;   // look at the progress counts every 20 us
        tc = now;
        const unsigned pg = progress();
        if (!have || pg != seen) {
            have = true;
            seen = pg;
            tw = now;
        } else if (now - tw > stall_ticks) {
            st_agent(serr, 1u);
            st_agent(herr, 1u);
            // hdr[2]: a count of give-ups the pre-pass never resets (callers read it
            // around a series of calls: fa_hip.backward_handoff_trips)
            __hip_atomic_fetch_add(herr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
}

// LDS reads hidden from the compiler, with an immediate offset.  hipcc makes every
// LDS access it can see after a `buffer_load ... lds` wait for ALL outstanding
// vector-memory operations (s_waitcnt vmcnt(0): it cannot tell which buffer a DMA
// writes), which in bwd_fused put the next slice's Q/dO DMA and the running-sum
// loads in front of the dQ phase.  A result is not ready until an lgkmcnt wait;
// pass it through reg_fence() after that wait, before any use.
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
template <int OFF>
__device__ __forceinline__ u32x4 lds_b128_at(uint32_t a) {
    u32x4 r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(a), "i"(OFF) : "memory");
    return r;
}
template <int OFF>
__device__ __forceinline__ s16x4 lds_tr16_at(uint32_t a) {
    s16x4 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(a), "i"(OFF) : "memory");
    return r;
}
__device__ __forceinline__ void lds_w32(void* p, float v) {
    asm volatile("ds_write_b32 %0, %1" : : "v"(lds_addr(p)), "v"(v) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait() { asm volatile("s_waitcnt lgkmcnt(%0)" : : "i"(N) : "memory"); }
template <class X>
__device__ __forceinline__ void reg_fence(X& x) { asm volatile("" : "+v"(x)); }
// A copy of x the compiler cannot see through: values derived from it inside a loop
// are not hoisted (hoisted per-lane addresses stay live across the loop and spill).
__device__ __forceinline__ int opaque(int x) { asm volatile("" : "+v"(x)); return x; }
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// Buffer descriptor as four SGPRs for inline asm (raw buffer, stride 0, the
// make_buffer_rsrc flags used everywhere here).
__device__ __forceinline__ u32x4 desc_of(const void* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)(uintptr_t)base;
    return u32x4{(unsigned)a, (unsigned)(a >> 32), bytes, 0x00020000u};
}
// Vector-memory operations hidden from the compiler's waitcnt model: the caller
// counts vmcnt for them (they retire in issue order) and fences the results.
__device__ __forceinline__ void dma16_asm(const u32x4& desc, uint32_t lds_base, int voff) {
    // s_nop 4: five wait states between a VALU write of the descriptor SGPRs (v_readlane
    // of a spilled SGPR, which the hazard recognizer cannot see past the asm) and the read
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" : : "v"(voff), "s"(desc), "{m0}"(lds_base) : "memory");
}
template <int OFF>
__device__ __forceinline__ u32x4 load16_sc1_asm(const u32x4& desc, int voff) {
    u32x4 r;
    // no s_nop here: no spill restore lands in front of these (tools/vmem_sgpr_hazards.py,
    // tests/test_code_hazards.py); one per load cost 2 % at configs[3]
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3 sc1" : "=v"(r) : "v"(voff), "s"(desc), "i"(OFF) : "memory");
    return r;
}
// dma_image8 through dma16_asm; returns nothing, issues (R/8 + 7)/8 ops or fewer per wave
template <int R>
__device__ __forceinline__ void dma_image8_asm(const u32x4& desc, char* img, int ntok, int t0, int wave, int lane) {
    constexpr int NB = R / 8;
#pragma unroll
    for (int it = 0; it < (NB + 7) / 8; ++it) {
        const int blk = it * 8 + wave;
        if (NB % 8 == 0 || blk < NB) {
            const ImgChunk ch = img_chunk(blk * 64 + lane);
            dma16_asm(desc, lds_addr(img + blk * 1024), (ch.f * ntok + t0 + 8 * ch.c) * 2);
        }
    }
}
__device__ __forceinline__ float load4_asm(const float* p) {
    float r;
    asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}
// vmcnt immediates (gfx9 encoding: vmcnt[3:0] + [15:14], expcnt[6:4] = 7, lgkmcnt[11:8] = 15)
template <int N>
__device__ __forceinline__ void vm_wait() {
    static_assert(N >= 0 && N < 16, "vmcnt");
    __builtin_amdgcn_s_waitcnt(0x0F70 | N);
}

// Diagnostic phase stamps (tools/exp/bwd4_stamp.py; empty in the product build):
// -DFA_BWD_STAMP4=w records s_memtime of workgroup w's first lane at phase points of
// its first 128 steps (0 after B1, 8 end of phase A, 9 after B2, 10 end of the dQ phase).
#ifdef FA_BWD_STAMP4
__device__ unsigned long long g_bwd_stamp[128 * 16];
#define BWD_STAMP(pt)                                                                          \
    do {                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                     \
        if (blockIdx.x == FA_BWD_STAMP4 && threadIdx.x == 0 && i < 128)                        \
            g_bwd_stamp[i * 16 + (pt)] = __builtin_amdgcn_s_memtime();                         \
        __builtin_amdgcn_sched_barrier(0);                                                     \
    } while (0)
#else
#define BWD_STAMP(pt)
#endif

template <class T, int D, int DV>
__global__ __launch_bounds__(512, 1) void bwd_fused(BwdParams p) {
    typedef typename Frag8<T>::type F8;
    typedef typename Frag8<T>::half F4;
    constexpr int KSUB = D * 128;                  // K image of 64 keys: [D][64]
    constexpr int QB = D * 128, OB = DV * 128;
    constexpr int STAGE = QB + OB + 512;           // Q, dO images + (−lse, −D) of one slice
    constexpr int DSB = 256 * 128;                 // dSᵀ image [256 keys][64 queries]
    constexpr int NTQ = D / 16;                    // 32 x 32 dQᵀ tiles per slice (<= 8 waves)
    __shared__ __attribute__((aligned(16))) char smem[4 * KSUB + STAGE + DSB];
    char* const kimg = smem;
    char* const qimg = smem + 4 * KSUB;
    char* const oimg = qimg + QB;
    float* const rowc = (float*)(oimg + OB);       // −lse[64] (raw units), −D[64]
    char* const dsimg = qimg + STAGE;

#ifdef FA_BWD_ABL
    const int abl = p.ablate;
#else
    constexpr int abl = 0;   // the timing-only ablations exist only in -DFA_BWD_ABL builds
#endif
    const int lid = p.xcd ? xcd_remap(blockIdx.x, p.total_wg) : (int)blockIdx.x;
    const int KM = p.nkb, NS = p.nqt, OFF = p.hoff;   // members per slab, slices
    const int b = lid / KM, j = lid - b * KM;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = p.N, Nk = p.Nk;
    const auto qrs = bslab<T>(p.Q, (int64_t)b * N * D, (int64_t)N * D);
    const auto ors = bslab<T>(p.dO, (int64_t)b * N * DV, (int64_t)N * DV);
    const auto krs = bslab<T>(p.K, (int64_t)b * Nk * D, (int64_t)Nk * D);
    const auto vrs = bslab<T>(p.V, (int64_t)b * Nk * DV, (int64_t)Nk * DV);
    const int key0 = j * 256;
    const int kj = key0 + 32 * wave + sig32(r);   // this lane's key (column of S, dP, dKᵀ, dVᵀ)
    const bool key_ok = kj < p.nkv;   // (the padded path's zero rows: P = 0, nothing stored)
    const float c = p.scale_log2;
    const float* nlse = p.nlse + (int64_t)b * N;
    const float* nDg = p.nD + (int64_t)b * N;
    const int64_t pslab = (int64_t)2 * NS * NTQ * 1024;   // floats of running sums per slab (two chains)
    const int pchain4 = NS * NTQ * 4096;                  // bytes of one chain's sums
    const auto prs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.part + b * pslab), (short)0, (int)(pslab * 4),
                                                       0x00020000);
    const u32x4 pdesc = desc_of(p.part + b * pslab, (uint32_t)(pslab * 4));
    const u32x4 qdesc = desc_of((const T*)p.Q + (int64_t)b * N * D, (uint32_t)(N * D * 2));
    const u32x4 odesc = desc_of((const T*)p.dO + (int64_t)b * N * DV, (uint32_t)(N * DV * 2));
    // this wave's loop DMA ops per slice (dma_image8_asm), >= for every wave: a lower bound
    constexpr int NDMA = (D / 8 >= 8 ? D / 64 : 0) + (DV / 8 >= 8 ? DV / 64 : 0);
    // The hand-off's bookkeeping (polls, publishes, the XCD words) is lane 0's alone, so
    // its pointers and state live in LDS, read where they are used through an address
    // the compiler cannot see through (hc(): never hoisted into registers).  Held in
    // SGPRs across the loop they spilled, and their v_readlane restores ran in every
    // step of every wave (35 more SGPR spills than round 4's single chain, 4 times the
    // restores in the loop, 6-13 % slower).
    struct HoffCtx {
        gu32* cnt[2];      // chains A, B: [NS] members of the chain that have published slice t
        gu32* fin;         // [NS] tails of a wrapped slice's two chains that stored their sums
        gu32* serr;        // this slab's trip word
        gu32* err;         // the call's status word (err[1]: the sticky give-up count)
        gu32* garr;        // the launch's arrival count
        gu32* prog;        // [KM] the slab's publish progress
        gu32* xccw;        // [KM] its members' XCDs + 1
        gu32* comb;        // a wrapped slice is left to bwd_dq_fast's combine
        uint64_t stall;    // no-progress bound of a poll
        unsigned next_known;   // j + 1's XCD seen (or not needed)
        unsigned pub;      // the last step's publish: kind | ch << 2 | pos << 3 | t << 12
                           // (pos < K <= CUs < 512; t < 2^20, fused_plan)
        unsigned nodirect; // tests: a chain-B tail never takes the direct add (p.nodirect)
    };
    __shared__ HoffCtx s_hc;
    typedef __attribute__((address_space(3))) HoffCtx LHoff;
    auto hc = [&]() {
        uint32_t a = lds_addr(&s_hc);
        asm volatile("" : "+v"(a));
        return (LHoff*)(uintptr_t)a;
    };
    auto my_xcc = []() { return (__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) & 7u) + 1u; };   // HW_REG_XCC_ID[3:0]
    if (tid == 0) {
        const FusedFlags ff = fused_flags(p.batch, NS, KM);
        s_hc.cnt[0] = (gu32*)(p.flags + ff.cnt + (int64_t)b * NS);
        s_hc.cnt[1] = (gu32*)(p.flags + ff.cnt + (int64_t)(p.batch + b) * NS);
        s_hc.fin = (gu32*)(p.flags + ff.fin + (int64_t)b * NS);
        s_hc.serr = (gu32*)(p.flags + ff.serr + b);
        s_hc.err = (gu32*)p.err;
        s_hc.garr = (gu32*)(p.flags + ff.garr);
        s_hc.prog = (gu32*)(p.flags + ff.prog + (int64_t)b * KM);
        s_hc.xccw = (gu32*)(p.flags + ff.xcc + (int64_t)b * KM);
        s_hc.comb = (gu32*)(p.hdr + 3);
        s_hc.stall = (uint64_t)p.stall_ticks;
        s_hc.next_known = (!p.l2local || j + 1 >= KM) ? 1u : 0u;
        s_hc.pub = 0u;
        s_hc.nodirect = p.nodirect ? 1u : 0u;
        st_agent(s_hc.xccw + j, my_xcc());
        arrive(s_hc.garr);
    }
    // lane 0: wait until chain ch's member pos - 1 has published slice t
    auto poll = [&](int ch, int t, int pos) {
        LHoff* const h = hc();
        wait_count(h->cnt[ch] + t, (unsigned)pos, h->serr, h->err, h->garr, h->prog, KM, h->stall);
    };

    // This lane's reads of the images.  The offsets of ImgReader (fa_bwd_common.h) are
    // written out here, and the reads go through lambdas: built from the struct, this
    // kernel's register allocation gains SGPR spills and, in two instantiations, 32 B of
    // scratch; this form compiles to the code it had before the struct existed.
    const int g = lane >> 4, kh = g & 1, qq = (lane & 15) >> 2, pp = lane & 3;
    const int sig = tr_sig(pp);
    int tro[2][2];
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
            const int sw = ((sp << 1) | h) | (((qq >> 1) & 1) << 2);
            tro[tb][sp] = (8 * h + qq) * 128 + (((tb * 4 + kh * 2 + (sig >> 1)) ^ sw) * 16) + (sig & 1) * 8;
        }
    const int rsw = swz16(r);
    auto trfrag = [&](const char* img, int tb, int s) -> F8 { return img_tr<T>(img, tro, tb, s); };
    auto rowfrag = [&](const char* img, int cb, int tb, int s2) -> F8 { return img_row<T>(img, r, h, rsw, cb, tb, s2); };
    auto slice_of = [&](int i) {
        int t = (i - OFF * j) % NS;
        return t < 0 ? t + NS : t;
    };
    // this member's link in slice t's chains: the members that reach t first (steps
    // (t + OFF·j') mod NS ascending) are j' >= w0 = ceil((NS − t)/OFF); when w0 < KM the
    // order wraps and is cut there into chain A = w0 .. KM−1 (ch 0) and B = 0 .. w0−1
    // (ch 1), else one chain 0 .. KM−1
    struct Link {
        int ch, pos, len;
        bool wrap;
    };
    // Walked without divisions (a runtime % NS and / OFF per use cost ~50 SALU
    // instructions each, in every wave): the step's slice t and w0 = ceil((NS − t)/OFF)
    // as w0 and r0 = NS − t − (w0 − 1)·OFF in [1, OFF], advanced by one slice per step.
    struct Walk {
        int t, w0, r0;
    };
    const int w0_at0 = (NS + OFF - 1) / OFF, r0_at0 = NS - (w0_at0 - 1) * OFF;   // slice 0
    auto walk_at = [&](int t) {
        Walk s;
        s.t = t;
        s.w0 = (NS - t + OFF - 1) / OFF;
        s.r0 = NS - t - (s.w0 - 1) * OFF;
        return s;
    };
    auto advance = [&](const Walk& s) {
        Walk n;
        if (s.t + 1 == NS) {
            n.t = 0;
            n.w0 = w0_at0;
            n.r0 = r0_at0;
        } else {
            n.t = s.t + 1;
            n.w0 = s.r0 == 1 ? s.w0 - 1 : s.w0;
            n.r0 = s.r0 == 1 ? OFF : s.r0 - 1;
        }
        return n;
    };
    auto link_of = [&](const Walk& s) {
        const int w0 = s.w0;
        Link L;
        L.wrap = w0 < KM;
        L.ch = L.wrap && j < w0 ? 1 : 0;
        L.pos = L.wrap && j >= w0 ? j - w0 : j;
        L.len = !L.wrap ? KM : L.ch ? w0 : KM - w0;
        return L;
    };
    // a publish after the step's sums left: the chain's count, or for the tail of a
    // wrapped slice's chain an add to the slice's fin word (no return value: a returning
    // atomic would make this wave wait for the step's running-sum loads).  fin == 2
    // after the launch means both tails stored their totals: chain B's tail found A
    // unfinished, stored instead of writing dQ, and flagged the launch (comb) so that
    // bwd_dq_fast adds them.  Every publish counts as progress of the slab: prog[j] takes
    // the number of steps done, which grows with every publish (lane 0, s_hc.pub).
    auto publish = [&](unsigned steps) {
        // every word read at once (one LDS round trip on wave 0 after B2, not a chain)
        LHoff* const h = hc();
        const unsigned pk = h->pub;
        gu32* const c0 = h->cnt[0];
        gu32* const c1 = h->cnt[1];
        gu32* const fn = h->fin;
        gu32* const cm = h->comb;
        gu32* const pg = h->prog;
        const int kind = pk & 3u, chp = (pk >> 2) & 1u, posp = (pk >> 3) & 511u, tp = pk >> 12;
        if (kind == 1) {
            st_agent((chp ? c1 : c0) + tp, (unsigned)(posp + 1));
        } else if (kind == 2) {
            __hip_atomic_fetch_add(fn + tp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (chp == 1) st_agent(cm, 1u);
        }
        if (kind != 0) st_agent(pg + j, steps);
    };
    auto load_rowc = [&](int t) {
        const int q = t * 64 + (tid & 63);
        float v = 0.0f;
        if (tid < 64) v = q < N ? nlse[q] : kNegInf;
        else if (tid < 128) v = q < N ? nDg[q] : 0.0f;
        return v;
    };

    // ---- prologue: K images (once), the first slice, V fragments of this lane's key ----
    Walk cur = walk_at(slice_of(0));
    int t = cur.t;
    {
        const float rc = load_rowc(t);
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) dma_image8<D>(krs, kimg + i4 * KSUB, Nk, key0 + 64 * i4, wave, lane);
        dma_image8<D>(qrs, qimg, N, t * 64, wave, lane);
        dma_image8<DV>(ors, oimg, N, t * 64, wave, lane);
        if (tid < 128) rowc[tid] = rc;
    }
    F8 vf[DV / 16];
#pragma unroll
    for (int s = 0; s < DV / 16; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const T x = __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b16(vrs, ((16 * s + 8 * h + e) * Nk + kj) * 2, 0, 0));
            vf[s][e] = key_ok ? x : (T)0.0f;
        }
    f32x16 dk[D / 32], dv[DV / 32];
#pragma unroll
    for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) dk[cb][x] = 0.0f;
#pragma unroll
    for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
        for (int x = 0; x < 16; ++x) dv[cb][x] = 0.0f;
    const char* const kmine = kimg + (wave >> 1) * KSUB;   // the 64-key image holding this wave's keys
    const int ktb = wave & 1;
    const int dsrow = 32 * wave + sig32(r);                  // this lane's dSᵀ row
    const int cbq = wave % (D / 32), uq = wave / (D / 32);   // this wave's dQᵀ tile (wave < NTQ)

    // the prologue's loads have landed: no LDS-DMA the compiler knows of is pending in
    // the loop (its DMA is asm), so it adds no vmcnt(0) before the loop's LDS reads
    vm_wait<0>();
    // L2-local hand-off: once the next member (j + 1, the reader of every running sum
    // this one hands on) is known to run on this member's XCD, the sums are stored
    // plainly and stay in that XCD's L2, where its sc1 loads (L1 bypass, L2-served) find
    // them; until then — nothing waits for it: lane 0 looks for its XCD word once per
    // step while it is missing — sc1 stores (L2 write-through, dropped) as everywhere
    // else.  A chain's tail stores sc1 always.
    __shared__ unsigned s_local;       // read after B2 of each step
    __shared__ unsigned s_direct[2];   // chain B's tail of step i's slice: A had finished (slot i & 1)
    auto look_next = [&]() {           // lane 0
        LHoff* const h = hc();
        if (h->next_known) return;
        const unsigned x = ld_agent(h->xccw + j + 1);
        if (x != 0u) {
            h->next_known = 1u;
            s_local = x == my_xcc() ? 1u : 0u;
        }
    };
    if (tid == 0) {
        s_local = 0u;
        look_next();
    }

    bool pub_prev = false;   // the last step left a publish for lane 0 (kind in s_hc.pub)
    for (int i = 0; i < NS; ++i) {
        t = cur.t;
        const Link lk = link_of(cur);
        const Walk nxt = advance(cur);
        const int pos = lk.pos;
        const int tq = opaque(tid), lq = tq & 63, rq = lq & 31, hq = lq >> 5;   // re-derived per step
        const bool tail = pos == lk.len - 1;
        const bool btail = lk.wrap && tail && lk.ch == 1;   // chain B's tail: makes A + B when A is done
        // B1: this slice's images landed; lane 0 has seen the predecessor's count for
        // slice t (polled at the end of the previous step's dQ phase, or here for the
        // first step; the barrier releases the other waves' sum loads).  The previous
        // step's running-sum stores (this wave's last >= 4 vector-memory ops) may still
        // be in flight: every wave drains them in the middle of phase A and their count
        // is published after B2.  (vmcnt retires in issue order; a poll load behind
        // those stores would wait for them, hence the poll's place.)
        const bool has_tile = NTQ >= 8 || wave < NTQ;
        if (has_tile && i > 0 && !(abl & 18)) __builtin_amdgcn_s_waitcnt(0x0F74);   // vmcnt(4)
        else __builtin_amdgcn_s_waitcnt(0x0F70);                                    // vmcnt(0)
        if (i == 0 && tid == 0 && !(abl & 1)) {
            if (pos > 0) poll(lk.ch, t, pos);
            if (btail) s_direct[0] = !hc()->nodirect && ld_agent(hc()->fin + t) >= 1u ? 1u : 0u;
        }
        __syncthreads();
        BWD_STAMP(0);

        // ---- S, dP, P, dS; dVᵀ, dKᵀ updates; dSᵀ into LDS ----
        const int pofs = lk.ch * pchain4 + (t * NTQ + wave) * 4096 + lq * 16;
        const bool ldpin = pos > 0 && has_tile && !(abl & 10);
        u32x4 pin[4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x16 sa, dp;
            const f32x4* Lq = (const f32x4*)(rowc + u * 32 + 8 * h);
            const f32x4* Dq = (const f32x4*)(rowc + 64 + u * 32 + 8 * h);
            const f32x4 l0 = Lq[0], l1 = Lq[1], l2 = Lq[4], l3 = Lq[5];
            const f32x4 d0 = Dq[0], d1 = Dq[1], d2 = Dq[4], d3 = Dq[5];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sa[e] = l0[e]; sa[4 + e] = l1[e]; sa[8 + e] = l2[e]; sa[12 + e] = l3[e];
                dp[e] = d0[e]; dp[4 + e] = d1[e]; dp[8 + e] = d2[e]; dp[12 + e] = d3[e];
            }
#pragma unroll
            for (int s = 0; s < D / 16; ++s) sa = mfma32x32x16(trfrag(qimg, u, s), trfrag(kmine, ktb, s), sa);
#pragma unroll
            for (int s = 0; s < DV / 16; ++s) dp = mfma32x32x16(trfrag(oimg, u, s), vf[s], dp);
            if (u == 1) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): last step's sums stored
            F8 pf[2], dsf[2];
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float pr = key_ok ? exp2_fast(sa[x] * c) : 0.0f;
                pf[x >> 3][x & 7] = (T)pr;
                dsf[x >> 3][x & 7] = (T)(pr * dp[x]);
            }
#pragma unroll
            for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) dv[cb] = mfma32x32x16(rowfrag(oimg, cb, u, s2), pf[s2], dv[cb]);
#pragma unroll
            for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) dk[cb] = mfma32x32x16(rowfrag(qimg, cb, u, s2), dsf[s2], dk[cb]);
            // dSᵀ row kj: queries 32u + 16 s2 + 8h + {0..7}
#pragma unroll
            for (int s2 = 0; s2 < 2 && !(abl & 32); ++s2)
                *(F8*)(dsimg + dsrow * 128 + (((4 * u + 2 * s2 + h) ^ swzds(dsrow)) * 16)) = dsf[s2];
        }

        BWD_STAMP(8);
        // running sum of the members before this one (sc1 loads, after B1).  Loaded
        // whether or not this member is the chain's head (which adds nothing), and the
        // DMA and row constants below are unconditional too: a straight-line step
        // lets the compiler count vmcnt for the sums past the DMA instead of vmcnt(0).
        // lane 0 polls for the NEXT step's slice here: every wave's queue is empty
        // (drained in the middle of this phase), so the poll pays only its own latency,
        // and barriers B2 and B1 order it before every wave's sum loads of that step
        if (wave == 0 && i + 1 < NS && !(abl & 1)) {
            const int tn = nxt.t;
            const Link ln = link_of(nxt);
            if (tq == 0) {
                look_next();
                // a chain-B tail reads chain A's fin word with its poll (one round
                // trip for both; read again if A was not done then)
                const bool bt = ln.wrap && ln.ch == 1 && ln.pos == ln.len - 1;
                gu32* const fw = hc()->fin + tn;
                const unsigned f0 = bt ? ld_agent(fw) : 0u;
                if (ln.pos > 0) poll(ln.ch, tn, ln.pos);
                if (bt) s_direct[(i + 1) & 1] = !hc()->nodirect && (f0 >= 1u || ld_agent(fw) >= 1u) ? 1u : 0u;
            }
        }
        if (has_tile && !(abl & 10)) {
            pin[0] = load16_sc1_asm<0>(pdesc, pofs);
            pin[1] = load16_sc1_asm<1024>(pdesc, pofs);
            pin[2] = load16_sc1_asm<2048>(pdesc, pofs);
            pin[3] = load16_sc1_asm<3072>(pdesc, pofs);
        }
        // a chain-B tail at d, dv <= 64 loads chain A's total here too, before it knows
        // (after B2) whether A had finished at its poll: used only if it had (then the
        // poll, earlier in program order, saw A's publish, which follows A's stores),
        // and counted with the running sum (vm_wait<NDMA>).  At 128 its 16 registers
        // would spill across the dQ phase: loaded after that phase instead.
        constexpr bool kPrefA = D <= 64 && DV <= 64;
        u32x4 pa[4];
        if (kPrefA && has_tile && btail && !(abl & 10)) {
            const int pofa = pofs - pchain4;
            pa[0] = load16_sc1_asm<0>(pdesc, pofa);
            pa[1] = load16_sc1_asm<1024>(pdesc, pofa);
            pa[2] = load16_sc1_asm<2048>(pdesc, pofa);
            pa[3] = load16_sc1_asm<3072>(pdesc, pofa);
        }
        __syncthreads();   // B2: dSᵀ complete, the slice's images free, last step's sums stored
        BWD_STAMP(9);
        // chain B's tail: whether A's total was there at the poll (lane 0's word, ordered
        // by B2).  Read and waited for here: the dQ phase below counts its own LDS reads
        // by hand (lgkm_wait), so no compiler-issued LDS read may land among them.
        const unsigned dword = btail ? s_direct[i & 1] : 0u;
        const unsigned lword = s_local;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const bool direct = btail && __builtin_amdgcn_readfirstlane(dword) != 0u;
        const bool local = __builtin_amdgcn_readfirstlane(lword) != 0u;
        if (pub_prev && tid == 0) publish((unsigned)i);

        // next slice's images and row constants (land before the next B1)
        // (the last step reloads its own slice: harmless, nothing reads it)
        float rc;
        bool rc_in;
        {
            const int tn = i + 1 < NS ? nxt.t : t;
            const int q = tn * 64 + lq;
            rc = load4_asm((tq < 64 ? nlse : nDg) + (q < N ? q : N - 1));   // asm: counted below
            rc_in = q < N;
            if (!(abl & 64)) {
                dma_image8_asm<D>(qdesc, qimg, N, tn * 64, wave, lq);
                dma_image8_asm<DV>(odesc, oimg, N, tn * 64, wave, lq);
            }
        }

        // ---- dQᵀ tile (features 32 cbq.., queries 32 uq..) over the 256 keys ----
        if (has_tile) {
            f32x16 acc;
#pragma unroll
            for (int x = 0; x < 16; ++x) acc[x] = 0.0f;
            // asm LDS reads (see lds_b128_at), one step ahead of the MFMA: the DMA
            // just issued and the running-sum loads stay in flight meanwhile
            uint32_t ka[4];
            const int rswq = swz16(rq);
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) ka[q4] = lds_addr(kimg + img_row_off(rq, hq, rswq, cbq, q4 >> 1, q4 & 1));
            const int qqq = (lq & 15) >> 2, khq = (lq >> 4) & 1, sgq = tr_sig(lq & 3);
            const uint32_t da = lds_addr(dsimg + (8 * hq + qqq) * 128 +
                                         (((uq * 4 + khq * 2 + (sgq >> 1)) ^ swzds(8 * hq + qqq)) * 16) + (sgq & 1) * 8);
            u32x4 fa[2];
            s16x4 flo[2], fhi[2];
            auto issue = [&](auto kc) {
                constexpr int kk = decltype(kc)::value;
                fa[kk & 1] = lds_b128_at<(kk >> 2) * KSUB>(ka[kk & 3]);
                flo[kk & 1] = lds_tr16_at<2048 * kk>(da);
                fhi[kk & 1] = lds_tr16_at<2048 * kk + 512>(da);
            };
            issue(std::integral_constant<int, 0>{});
            static_for<16>([&](auto kc) {
                constexpr int kk = decltype(kc)::value;
                if constexpr (kk + 1 < 16) {
                    issue(std::integral_constant<int, kk + 1>{});
                    lgkm_wait<3>();
                } else {
                    lgkm_wait<0>();
                }
                reg_fence(fa[kk & 1]);
                reg_fence(flo[kk & 1]);
                reg_fence(fhi[kk & 1]);
                const F4 lo = __builtin_bit_cast(F4, flo[kk & 1]);
                const F4 hi = __builtin_bit_cast(F4, fhi[kk & 1]);
                acc = mfma32x32x16(__builtin_bit_cast(F8, fa[kk & 1]), __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7),
                                   acc);
            });
            // the sums (asm loads): all but this wave's NDMA DMA ops retired
            if (!(abl & 64)) vm_wait<NDMA>(); else vm_wait<0>();
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) reg_fence(pin[c4]);
            reg_fence(rc);
            // the next slice's row constants (phase A's reads of rowc ended at B2)
            if (tq < 128) lds_w32(rowc + tq, rc_in ? rc : (tq < 64 ? kNegInf : 0.0f));
            if (ldpin) {
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * c4 + e] += __uint_as_float(pin[c4][e]);
            }
            // chain B's tail with A finished: A's total (its tail's sc1 stores, published
            // through fin before this step's poll) in, after this chain's own sum
            if (direct) {
                if constexpr (!kPrefA) {
                    const int pofa = pofs - pchain4;
                    pa[0] = load16_sc1_asm<0>(pdesc, pofa);
                    pa[1] = load16_sc1_asm<1024>(pdesc, pofa);
                    pa[2] = load16_sc1_asm<2048>(pdesc, pofa);
                    pa[3] = load16_sc1_asm<3072>(pdesc, pofa);
                    vm_wait<0>();
                }
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    reg_fence(pa[c4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * c4 + e] += __uint_as_float(pa[c4][e]);
                }
            }
            if ((tail && !lk.wrap) || direct) {
                // 32-bit lane offset + scalar row offset (no hoisted 64-bit addresses)
                const int q = t * 64 + 32 * uq + sig32(rq);
                const auto qo = bslab<T>(p.dQ, (int64_t)b * N * D, (int64_t)N * D);
                const int vo = q < N ? ((cbq * 32 + 4 * hq) * N + q) * 2 : N * D * 2;   // past N: dropped
#pragma unroll
                for (int x = 0; x < 16; ++x)
                    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (T)(acc[x] * p.scale)), qo, vo,
                                                          ((x & 3) + 8 * (x >> 2)) * N * 2, 0);
            } else if (!(abl & 18)) {
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const u32x4 v4 = {__float_as_uint(acc[4 * c4]), __float_as_uint(acc[4 * c4 + 1]),
                                      __float_as_uint(acc[4 * c4 + 2]), __float_as_uint(acc[4 * c4 + 3])};
                    if (local && !tail) __builtin_amdgcn_raw_buffer_store_b128(v4, prs, pofs + c4 * 1024, 0, 0);
                    else __builtin_amdgcn_raw_buffer_store_b128(v4, prs, pofs + c4 * 1024, 0, 16);   // sc1
                }
            }
        }
        BWD_STAMP(10);
        // publish kind: 0 none (dQ written), 1 chain count, 2 fin word (a wrapped chain's tail)
        const unsigned kind = (tail && !lk.wrap) || direct ? 0u : tail ? 2u : 1u;
        pub_prev = kind != 0u;
        if (tid == 0) hc()->pub = kind | (unsigned)lk.ch << 2 | (unsigned)pos << 3 | (unsigned)t << 12;
        cur = nxt;
    }
    if (pub_prev) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) publish((unsigned)NS);
    }
    if (key_ok) {
        const auto ko = bslab<T>(p.dK, (int64_t)b * Nk * D, (int64_t)Nk * D);
        const auto vo = bslab<T>(p.dV, (int64_t)b * Nk * DV, (int64_t)Nk * DV);
        const int lo = (4 * h * Nk + kj) * 2;
#pragma unroll
        for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x)
                __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (T)(dk[cb][x] * p.scale)), ko, lo,
                                                      (cb * 32 + (x & 3) + 8 * (x >> 2)) * Nk * 2, 0);
#pragma unroll
        for (int cb = 0; cb < DV / 32; ++cb)
#pragma unroll
            for (int x = 0; x < 16; ++x)
                __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (T)dv[cb][x]), vo, lo,
                                                      (cb * 32 + (x & 3) + 8 * (x >> 2)) * Nk * 2, 0);
    }
}

#ifdef FA_BWD_STAMP4
extern "C" int fa_debug_bwd_stamps(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bwd_stamp), (size_t)n * 8, 0, hipMemcpyDeviceToHost);
}
#endif

template <class T>
hipError_t launch_fused(const BwdParams& p, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    by_dim_class(p.d, [&](auto D) {
        by_dim_class(p.dv, [&](auto DV) {
            hipLaunchKernelGGL((bwd_fused<T, decltype(D)::value, decltype(DV)::value>), dim3((unsigned)p.total_wg),
                               dim3(512), 0, s, p);
            e = hipGetLastError();
        });
    });
    return e;
}
template hipError_t launch_fused<bf16>(const BwdParams&, hipStream_t);
template hipError_t launch_fused<f16>(const BwdParams&, hipStream_t);

}  // namespace fa
