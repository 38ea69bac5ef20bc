// Launch timeline of the dense forward (dense_fwd_tiled): the product source included
// with FA_FWD_STAMP defined.  Per workgroup, wave 0 lane 0 records s_memrealtime
// (100 MHz) at phase k (0 entry, 1 main loop start, 2 main loop end, 3 after the O
// stores; 4..9 split the prologue and the epilogue, see fwd_timeline.py) and the CU it
// runs on (HW_REG_HW_ID, HW_REG_XCC_ID, slot 15).  Diagnostic only, never shipped; the
// stamps go to a buffer of their own.  Run: tools/exp/fwd_timeline.py.
// -DFA_FWD_SRC='"file.hip"' stamps another copy of the source (an A/B of two trees).
#include <hip/hip_runtime.h>
__device__ unsigned long long g_tl[16 * 8192];
#define FA_FWD_STAMP(k)                                                                               \
    do {                                                                                              \
        if (threadIdx.x == 0) {                                                                       \
            ::g_tl[blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memrealtime();                          \
            if ((k) == 0)                                                                             \
                ::g_tl[blockIdx.x * 16 + 15] =                                                          \
                    ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) << 32) | \
                    __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));                      \
        }                                                                                             \
    } while (0)
#ifndef FA_FWD_SRC
#define FA_FWD_SRC "../../flashattention.jl_amd/csrc/fa_fwd.hip"
#endif
#include FA_FWD_SRC

extern "C" int fwd_tl_launch(const void* Q, const void* K, const void* V, void* O, float* l, float* m, int N,
                             int d, int batch, void* stream) {
    fa::DenseArgs a{FA_DTYPE_BF16, Q, K, V, O, l, m, N, N, d, d, batch, 1.0f / sqrtf((float)d)};
    const char* why = "";
    return fa::launch_dense_fwd(a, (hipStream_t)stream, &why);
}

extern "C" int fwd_tl_read(unsigned long long* host_out, int nwg) {
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    if (nwg > 8192) return 4;
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_tl), sizeof(unsigned long long) * 16 * nwg) == hipSuccess ? 0 : 3;
}
