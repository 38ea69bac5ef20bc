// fa_bwd_common.h — device pieces shared by the dense backward (fa_bwd*.hip) and the
// circulant backward (fa_circulant_bwd.hip): the swizzled 64-token LDS image of their
// MFMA kernels (the one statement of its layout: the writers' chunk map and the
// readers) and the vectorised pre-pass body; then what the dense MFMA kernel files
// share among themselves.
#pragma once

#include "fa_common.h"

namespace fa {

// --------------------------------------------------------------------------
// The [rows][64 tokens] LDS image (bf16 / fp16).  Rows are features, 128 B each, and
// the eight 16-B chunks of row f sit at positions c ^ g(f) with the XOR swizzle
// g(f) = ((f>>3)&3) | ((f>>1)&1)<<2, which makes BOTH access patterns
// conflict-free: the transposed reads ds_read_b64_tr_b16 (A operands of the
// score / dP products: 4 consecutive rows × 64 B per half-wave) and the
// ds_read_b128 row reads (A operands of the gradient products: 16 rows per
// lane group, one 16-B chunk each).
// --------------------------------------------------------------------------
__device__ __forceinline__ int swz16(int f) { return ((f >> 3) & 3) | (((f >> 1) & 1) << 2); }

// Writers fill the image linearly, 16 B at a time (LDS-DMA lane-linearly, or b128
// stores of chunks staged in registers), so the swizzle goes into the GLOBAL address:
// the image's P-th 16 B hold row f, tokens 8 c .. 8 c + 7 of the tile.
struct ImgChunk {
    int f, c;
};
__device__ __forceinline__ ImgChunk img_chunk(int P) {
    const int f = P >> 3;
    return {f, (P & 7) ^ swz16(f)};
}

// ds_read_b64_tr_b16 takes its four 4-token pieces from lanes 4q + pp in the order
// 0, 2, 1, 3: piece sig(pp) of the 16 tokens a 16-lane group reads.
__device__ __forceinline__ int tr_sig(int pp) { return (pp == 1) ? 2 : (pp == 2) ? 1 : pp; }

// Byte offset of the b128 row read of lane (r, h), rsw = swz16(r): row 32 cb + r,
// tokens 32 tb + 16 s2 + 8 h .. + 7.
__device__ __forceinline__ int img_row_off(int r, int h, int rsw, int cb, int tb, int s2) {
    return (cb * 32 + r) * 128 + (((tb * 4 + 2 * s2 + h) ^ rsw) * 16);
}

// Reads of MFMA A operands by lane = 32 h + r, given the lane's offsets (ImgReader).
// Transposed: element e = feature 16 s + 8 h + e of token 32 tb + r.
template <class T>
__device__ __forceinline__ typename Frag8<T>::type img_tr(const char* img, const int (&tro)[2][2], int tb, int s) {
    typedef typename Frag8<T>::half F4;
    const char* a = img + tro[tb][s & 1] + 16 * s * 128;
    const F4 lo = __builtin_bit_cast(F4, ds_read_tr16(a));
    const F4 hi = __builtin_bit_cast(F4, ds_read_tr16(a + 4 * 128));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// By rows: element e = token 32 tb + 16 s2 + 8 h + e of feature 32 cb + r.
template <class T>
__device__ __forceinline__ typename Frag8<T>::type img_row(const char* img, int r, int h, int rsw, int cb, int tb,
                                                           int s2) {
    return *(const typename Frag8<T>::type*)(img + img_row_off(r, h, rsw, cb, tb, s2));
}

// A lane's reader, built once per kernel from the thread's index in its workgroup.
// (bwd_fused, fa_bwd_fused.hip, is the one kernel that writes these offsets out itself and
// calls img_tr / img_row: see there.  A change to tro is made in both places.)
template <class T>
struct ImgReader {
    typedef typename Frag8<T>::type F8;
    int tro[2][2];   // [token block tb][s & 1] byte offset of the transposed read of feature step s
    int r, h, rsw;

    __device__ __forceinline__ explicit ImgReader(int tid) {
        const int lane = tid & 63;
        r = lane & 31;
        h = lane >> 5;
        // lane 4 qq + pp of 16-lane group g supplies row 8 h + qq, tokens 32 tb + 16 kh + 4 sig ..
        const int g = lane >> 4, kh = g & 1, qq = (lane & 15) >> 2, pp = lane & 3;
        const int sig = tr_sig(pp);
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const int sw = ((sp << 1) | h) | (((qq >> 1) & 1) << 2);   // swz16(16 s + 8 h + qq)
                tro[tb][sp] = (8 * h + qq) * 128 + (((tb * 4 + kh * 2 + (sig >> 1)) ^ sw) * 16) + (sig & 1) * 8;
            }
        rsw = swz16(r);
    }
    __device__ __forceinline__ F8 tr(const char* img, int tb, int s) const { return img_tr<T>(img, tro, tb, s); }
    __device__ __forceinline__ F8 row(const char* img, int cb, int tb, int s2) const {
        return img_row<T>(img, r, h, rsw, cb, tb, s2);
    }
};

// --------------------------------------------------------------------------
// Pre-pass body, 16-B variant (bf16 / fp16, N % 8 == 0, O and dO 16-B aligned): the
// thread owns the 8 consecutive queries idx .. idx + 7 of the [batch][N] rows, keeps
// 16 row loads in flight for the dO∘O row sums and writes −rowsum and −(m + ln l)/τ.
// --------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void prepass_rows8(const T* O, const T* dO, const float* l, const float* m, float* nD,
                                              float* nlse, int64_t idx, int N, int dv, float scale) {
    constexpr int U = 8;
    const int64_t b = idx / N, n = idx - b * N;
    O += b * (int64_t)N * dv + n;
    dO += b * (int64_t)N * dv + n;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
    auto fma8 = [&](const u32x4& a, const u32x4& c) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned wa = a[k], wc = c[k];
            acc[2 * k] = fmaf((float)__builtin_bit_cast(T, (unsigned short)(wa & 0xFFFFu)),
                              (float)__builtin_bit_cast(T, (unsigned short)(wc & 0xFFFFu)), acc[2 * k]);
            acc[2 * k + 1] = fmaf((float)__builtin_bit_cast(T, (unsigned short)(wa >> 16)),
                                  (float)__builtin_bit_cast(T, (unsigned short)(wc >> 16)), acc[2 * k + 1]);
        }
    };
    int c = 0;
    for (; c + U <= dv; c += U) {
        u32x4 ro[U], rd[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ro[u] = *(const u32x4*)(O + (int64_t)(c + u) * N);
            rd[u] = *(const u32x4*)(dO + (int64_t)(c + u) * N);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) fma8(rd[u], ro[u]);
    }
    for (; c < dv; ++c) fma8(*(const u32x4*)(dO + (int64_t)c * N), *(const u32x4*)(O + (int64_t)c * N));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        nD[idx + k] = -acc[k];
        nlse[idx + k] = -(m[idx + k] + logf(l[idx + k])) / scale;
    }
}

// --------------------------------------------------------------------------
// Dense MFMA backward (fa_bwd_dq.hip, fa_bwd_dkdv.hip, fa_bwd_fused.hip): a slab's buffer
// descriptor, the LDS-DMA of one image by 4 waves, the single pass's inter-workgroup words
// and its dQᵀ column order.
// --------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bslab(const void* base, int64_t off_elems, int64_t elems) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const T*)base + off_elems), (short)0,
                                             (int)(elems * (int64_t)sizeof(T)), 0x00020000);
}

// LDS-DMA one [R rows][64 tokens] image (R*128 bytes) from a [*][ntok] slab at
// token t0.  4 waves; each wave-instruction fills 1 KiB (8 rows) lane-linearly,
// so the swizzle is applied to the per-lane GLOBAL address (cdna guide rule 21).
template <int R>
__device__ __forceinline__ void dma_image(__amdgpu_buffer_rsrc_t rs, char* img, int ntok, int t0, int wave, int lane) {
#pragma unroll
    for (int it = 0; it < R / 32; ++it) {
        const int blk = it * 4 + wave;                    // 1-KiB block of the image
        const ImgChunk ch = img_chunk(blk * 64 + lane);   // row and chunk of the 16 B this lane fills
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs, (__attribute__((address_space(3))) void*)(img + blk * 1024), 16,
            (ch.f * ntok + t0 + 8 * ch.c) * 2, 0, 0, 0);
    }
}

// Inter-workgroup words of the single-pass kernel: global (never flat), agent
// scope, relaxed (global_load / global_store ... sc1).
typedef __attribute__((address_space(1))) unsigned gu32;
__device__ __forceinline__ unsigned ld_agent(gu32* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(gu32* p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int sig32(int r) { return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1); }

}  // namespace fa
