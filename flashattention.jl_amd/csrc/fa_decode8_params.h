// fa_decode8_params.h — what the fp8-cache decode kernels share on the device side: the
// parameter struct of decode8_fwd / decode8_combine (fa_decode_fp8.hip), which
// decode_paged8_fwd (fa_decode_paged_fp8.hip) extends with its page table, the out-of-range
// buffer offset, the exact e4m3fn -> 16-bit convert, the transposed byte read of the K image,
// the empty-state store, and the host function through which fa_decode_paged_fp8.hip launches
// fa_decode_fp8.hip's decode8_combine.
#pragma once

#include <type_traits>

#include "fa_common.h"
#include "fa_decode_plan.h"

namespace fa {

struct Decode8Params {
    const void* Q;
    const uint8_t *K, *V;
    const float *k_scale, *v_scale;   // `batch` floats each, or nullptr (1.0)
    void* O;
    float *l, *m;
    const int32_t *q_lens, *k_lens;
    float* part;     // nsplit > 1: [nsplit][batch * group][N][dv + 2] = O (unnormalised, unscaled), l, m (raw units)
    int N, Nk, d, dv, batch, group, nsplit, total_wg;
    int wleft, wright;   // mask_ints(kMaskVarlen)
    float scale;
};

typedef int i32x2 __attribute__((ext_vector_type(2)));

constexpr int kDec8OobOff = 0x7FFFFFF0;   // a buffer offset past every slab: reads as 0

// Eight e4m3fn bytes (lo: elements 0..3, hi: 4..7) as one 16-bit MFMA operand; exact.
template <class T>
__device__ __forceinline__ typename Frag8<T>::type cvt8(unsigned lo, unsigned hi) {
    if constexpr (std::is_same<T, bf16>::value) {
        typedef __bf16 x2 __attribute__((ext_vector_type(2)));
        const x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, 1.0f, false);
        const x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, 1.0f, true);
        const x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, 1.0f, false);
        const x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, 1.0f, true);
        return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    } else {
        typedef _Float16 x2 __attribute__((ext_vector_type(2)));
        const x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)lo, 1.0f, false);
        const x2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)lo, 1.0f, true);
        const x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)hi, 1.0f, false);
        const x2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)hi, 1.0f, true);
        return f16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    }
}

// ds_read_b64_tr_b8 (the lane mapping is in fa_decode_fp8.hip's header)
__device__ __forceinline__ i32x2 ds_read_tr8(const char* lds_ptr) {
    return __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2*)(lds_void*)lds_ptr);
}

// The empty state of the workgroup's rows: O = 0, l = 0, m = -inf (final, or as a partial).
template <class T>
__device__ __forceinline__ void decode8_store_empty(const Decode8Params& p, int b, int sp) {
    const int N = p.N, dv = p.dv, rows = N * p.group;
    const int64_t R0 = (int64_t)b * rows;
    if (p.nsplit == 1) {
        T* const O = (T*)p.O;
        for (int idx = threadIdx.x; idx < rows * dv; idx += kDecodeThreads) {
            const int f = idx / rows, row = idx - f * rows, g = row / N, i = row - g * N;
            O[(((int64_t)b * p.group + g) * dv + f) * N + i] = (T)0.0f;
        }
        for (int row = threadIdx.x; row < rows; row += kDecodeThreads) {
            p.l[R0 + row] = 0.0f;
            p.m[R0 + row] = kNegInf;
        }
    } else {
        float* const part = p.part + ((int64_t)sp * p.batch * rows + R0) * (dv + 2);
        for (int idx = threadIdx.x; idx < rows * (dv + 2); idx += kDecodeThreads)
            part[idx] = idx % (dv + 2) == dv + 1 ? kNegInf : 0.0f;
    }
}

// decode8_combine<f16 or bf16> on pl.combine_grid workgroups (fa_decode_fp8.hip; nsplit > 1 only).
void launch_decode8_combine(int dtype, const DecodePlan& pl, const Decode8Params& p, hipStream_t s);

}  // namespace fa
