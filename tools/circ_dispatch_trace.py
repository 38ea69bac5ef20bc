"""Which kernels the circulant launchers start, on which grids: one pass over the shapes of
tests/test_circulant_plan_host.py's table (forward and backward, every dtype, the knob, the
alignment facts; B shrunk to 2 where the rule does not look at it), each launched once.  Left
out: the refused rows, and the rows at the 32-bit extent limits and the W = 1 grid cap, whose
tensors run to gigabytes.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/circ_dispatch_trace.py
    python tools/circ_dispatch_trace.py --list OUT/.../*_kernel_trace.csv > kernels.txt

The second form prints the library's kernels in launch order as `name grid block`.  Two builds
dispatch alike when their lists are equal (FA_HIP_LIB selects the library): the check a change
to csrc/fa_circulant_plan.h or the circulant launchers runs against its parent."""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flashattention.jl_amd"), os.path.join(ROOT, "tools")]

from dense_dispatch_trace import listing  # noqa: E402


def main():
    import torch

    import fa_hip

    L = fa_hip.lib()
    BF, HF, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64

    def mk(shape, dtype, seed, misaligned=False):
        g = torch.Generator(device="cuda").manual_seed(seed)
        n = shape[0] * shape[1] * shape[2]
        buf = torch.empty(n + 8, dtype=dtype, device="cuda")
        off = 1 if misaligned else 0   # one element: off a 16-B boundary at every element size
        t = buf[off:off + n].as_strided(shape, fa_hip.jl_strides(shape))
        t.copy_(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32))
        return t

    def shifted(t):
        out = mk(tuple(t.shape), t.dtype, 0, True)
        out.copy_(t)
        return out

    def fwd(N, d, dv, B, W, dtype=BF, knob=0, mis_kv=False, mis_q=False):
        q = mk((N, d, B), dtype, 1, mis_q)
        k = mk((N, d, B), dtype, 2, mis_kv)
        v = mk((N, dv, B), dtype, 3, mis_kv)
        old = L.fa_debug_set_circ_generic(knob)
        try:
            O, l, m = fa_hip.circulant_fa(q, k, v, W)
        finally:
            L.fa_debug_set_circ_generic(old)
        torch.cuda.synchronize()
        return q, k, v, O, l, m

    def bwd(N, d, dv, B, W, dtype=BF, knob=0, mis_q=False, mis_o=False, mis_do=False):
        q, k, v, O, l, m = fwd(N, d, dv, B, W, dtype, mis_q=mis_q)
        dO = mk((N, dv, B), dtype, 4, mis_do)
        if mis_o:
            O = shifted(O)
        old = L.fa_debug_set_circ_generic(knob)
        try:
            fa_hip.circulant_fa_backward(q, k, v, O, dO, l, m, W)
        finally:
            L.fa_debug_set_circ_generic(old)
        torch.cuda.synchronize()

    # ---- forward -----------------------------------------------------------
    fwd(4096, 64, 64, 2, 129)                          # tiled
    fwd(4096, 64, 64, 2, 129, dtype=HF)
    fwd(256, 32, 32, 1, 9)                             # a small grid stays tiled
    fwd(4096, 33, 32, 2, 129)                          # classes (64, 32)
    fwd(4096, 128, 65, 2, 129)                         # (128, 128)
    fwd(4088, 64, 64, 2, 129)
    fwd(4095, 64, 64, 8, 129)                          # 128 blocks: SIMT
    fwd(4095, 64, 64, 7, 129)                          # 112: one wave per query
    fwd(4096, 64, 64, 8, 129, mis_kv=True)             # misaligned K / V: SIMT
    fwd(4096, 64, 64, 7, 129, mis_kv=True)
    fwd(4092, 64, 64, 8, 129)                          # N % 8 != 0
    fwd(4096, 64, 64, 8, 129, knob=1)
    fwd(4096, 64, 64, 8, 129, knob=2)
    fwd(4095, 64, 64, 7, 129, knob=2)
    fwd(4095, 64, 64, 8, 129, knob=1)
    fwd(256, 32, 32, 1, 9, knob=1)
    fwd(256, 32, 32, 1, 9, knob=2)
    fwd(4096, 64, 64, 8, 129, dtype=F32)
    fwd(4096, 64, 64, 7, 129, dtype=F32)
    fwd(4096, 64, 64, 8, 129, dtype=F32, knob=1)
    for knob in (0, 1, 2):
        fwd(64, 32, 32, 2, 9, dtype=F64, knob=knob)
    fwd(4095, 64, 64, 8, 129, dtype=F64, mis_kv=True)
    for d, dv in ((32, 32), (33, 32), (32, 33), (65, 32), (32, 65)):   # the SIMT classes
        fwd(4095, d, dv, 8, 129)
    fwd(4095, 128, 128, 8, 129, dtype=HF)

    # ---- backward ----------------------------------------------------------
    bwd(4096, 64, 64, 2, 129)                          # 16-B pre-pass, MFMA
    bwd(4096, 64, 64, 2, 129, dtype=HF)
    bwd(4096, 33, 32, 2, 129)
    bwd(256, 32, 32, 1, 9)
    bwd(4096, 64, 64, 2, 129, mis_q=True)              # 16-B pre-pass, SIMT
    bwd(4096, 64, 64, 2, 129, mis_o=True)              # scalar pre-pass, MFMA
    bwd(4096, 64, 64, 2, 129, mis_do=True)             # scalar pre-pass, SIMT
    bwd(4095, 64, 64, 2, 129)
    bwd(4092, 64, 64, 2, 129)
    bwd(4096, 64, 64, 2, 129, knob=1)
    bwd(4096, 64, 64, 2, 129, knob=2)
    bwd(4096, 64, 64, 2, 129, dtype=F32)
    bwd(4096, 64, 64, 2, 129, dtype=F64)
    bwd(4096, 64, 64, 2, 129, dtype=F64, knob=2)
    bwd(4096, 64, 64, 2, 1)                            # W = 1: one kernel
    bwd(4096, 64, 64, 2, 1, dtype=F32)
    bwd(4096, 64, 64, 2, 1, dtype=F64)
    bwd(4096, 32, 64, 2, 1)
    bwd(4095, 64, 64, 2, 1, mis_q=True)
    bwd(4096, 64, 64, 2, 2)
    bwd(4095, 128, 128, 2, 129)                        # > 64 KiB of LDS
    bwd(4096, 128, 128, 2, 129, dtype=F64)
    bwd(4095, 32, 48, 2, 129)
    bwd(1000, 32, 32, 3, 9)
    bwd(1000, 32, 32, 3, 9, dtype=F64)
    print("circ_dispatch_trace: done")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--list":
        listing(sys.argv[2:])
    else:
        main()
