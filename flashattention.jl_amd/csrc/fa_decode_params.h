// fa_decode_params.h — what the 16-bit decode kernels share on the device side: the parameter
// struct of decode_fwd / decode_combine (fa_decode.hip), which decode_paged_fwd
// (fa_decode_paged.hip) extends with its page table, the out-of-range buffer offset, the
// empty-state store, and the host function through which fa_decode_paged.hip launches
// fa_decode.hip's decode_combine.
#pragma once

#include "fa_common.h"
#include "fa_decode_plan.h"

namespace fa {

struct DecodeParams {
    const void *Q, *K, *V;
    void* O;
    float *l, *m;
    const int32_t *q_lens, *k_lens;
    float* part;     // nsplit > 1: [nsplit][batch * group][N][dv + 2] = O (unnormalised), l, m (raw units)
    int N, Nk, d, dv, batch, group, nsplit, total_wg;
    int wleft, wright;   // mask_ints(kMaskVarlen)
    float scale, scale_log2;
};

constexpr int kDecOobOff = 0x7FFFFFF0;   // a buffer offset past every slab: reads as 0

// The empty state of the workgroup's rows: O = 0, l = 0, m = -inf (final, or as a partial).
template <class T>
__device__ __forceinline__ void decode_store_empty(const DecodeParams& p, int b, int sp) {
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

// decode_combine<f16 or bf16> on pl.combine_grid workgroups (fa_decode.hip; nsplit > 1 only).
void launch_decode_combine(int dtype, const DecodePlan& pl, const DecodeParams& p, hipStream_t s);

}  // namespace fa
