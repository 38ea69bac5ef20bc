"""Which kernels the dense and causal launchers start, on which grids: one pass over the shapes
of tests/test_dense_plan_host.py's table (forward and backward, dense and causal, the forced
variants and modes; B shrunk where the rule allows), each launched once.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/dense_dispatch_trace.py
    python tools/dense_dispatch_trace.py --list OUT/.../*_kernel_trace.csv > kernels.txt

The second form prints the library's kernels in launch order as `name grid block`.  Two builds
dispatch alike when their lists are equal (FA_HIP_LIB selects the library): the check a change
to csrc/fa_dense_plan.h or the dense launchers runs against its parent."""
from __future__ import annotations

import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flashattention.jl_amd")]


def listing(paths):
    rows = []
    for p in paths:
        with open(p, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                if "fa::" not in name and not name.startswith("_ZN2fa"):   # (bf16 / fp16 names stay mangled)
                    continue
                name = re.sub(r"\s*\[clone .*\]$", "", name)
                grid = r.get("Grid_Size_X") or r["Grid_Size"]
                block = r.get("Workgroup_Size_X") or r["Workgroup_Size"]
                rows.append((int(r["Start_Timestamp"]), name, grid, block))
    for _, name, grid, block in sorted(rows):
        print(name, grid, block)


def main():
    import torch

    import fa_hip

    L = fa_hip.lib()
    BF, HF, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64

    def mk(shape, dtype, seed, misaligned=False):
        g = torch.Generator(device="cuda").manual_seed(seed)
        n = shape[0] * shape[1] * shape[2]
        buf = torch.empty(n + 8, dtype=dtype, device="cuda")
        off = 1 if misaligned else 0   # one element: 2 B off a 16-B boundary at 16 bits
        t = buf[off:off + n].as_strided(shape, fa_hip.jl_strides(shape))
        t.copy_(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32))
        return t

    def knobs(**kw):
        """Set debug knobs, return a function that restores them."""
        old = [(name, getattr(L, "fa_debug_set_" + name)(v)) for name, v in kw.items()]
        return lambda: [getattr(L, "fa_debug_set_" + name)(v) for name, v in reversed(old)]

    def fwd(N, Nk, d, dv, B, dtype=BF, causal=False, mis_k=False, mis_q=False, no_ws=False, **kw):
        q = mk((N, d, B), dtype, 1, mis_q)
        k = mk((Nk, d, B), dtype, 2, mis_k)
        v = mk((Nk, dv, B), dtype, 3)
        restore = knobs(**kw)
        try:
            if no_ws:   # the entry without a workspace: ragged or misaligned K / V run the generic kernel
                O = fa_hip.jl_empty((N, dv, B), dtype)
                l, m = fa_hip.jl_empty((N, 1, B)), fa_hip.jl_empty((N, 1, B))
                fa_hip._check(L.fa_dense_fwd(fa_hip.DTYPES[dtype], q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(),
                                             l.data_ptr(), m.data_ptr(), N, Nk, d, dv, B, 0.0, None))
            else:
                O, l, m = (fa_hip.causal_fa if causal else fa_hip.dense_fa)(q, k, v)
        finally:
            restore()
        torch.cuda.synchronize()
        return q, k, v, O, l, m

    def bwd(N, Nk, d, dv, B, dtype=BF, causal=False, mis_q=False, **kw):
        q, k, v, O, l, m = fwd(N, Nk, d, dv, B, dtype, causal, mis_q=mis_q)
        dO = mk((N, dv, B), dtype, 4)
        restore = knobs(**kw)
        try:
            (fa_hip.causal_fa_backward if causal else fa_hip.dense_fa_backward)(q, k, v, O, dO, l, m)
        finally:
            restore()
        torch.cuda.synchronize()

    # ---- forward -----------------------------------------------------------
    fwd(4096, 4096, 64, 64, 32)                       # w8q2 wide, no split
    fwd(8192, 8192, 128, 128, 8)                      # p4
    fwd(256, 8192, 128, 128, 4)                       # w8b64 split, 64 x 2 tiles
    fwd(256, 1024, 128, 128, 512)                     # too few key tiles for p4: w8b64 wide
    fwd(2048, 2048, 96, 96, 32)                       # d below its class: w8b64 wide
    fwd(1024, 1001, 64, 64, 16)                       # padded K / V, ldk 1008
    fwd(1024, 1001, 64, 64, 16, no_ws=True)           # no workspace: generic
    fwd(1024, 1000, 64, 64, 16, mis_k=True)           # misaligned K: padded
    fwd(1004, 1024, 64, 64, 16)                       # N % 8 != 0: narrow
    fwd(4096, 4096, 64, 64, 32, mis_q=True)           # misaligned Q: narrow
    fwd(512, 512, 64, 64, 4, dtype=F32)
    fwd(256, 256, 64, 64, 2, dtype=F64)
    fwd(4096, 4096, 32, 64, 32, dtype=HF)
    fwd(512, 4096, 64, 64, 8)                         # w8q2 split
    fwd(4096, 4096, 64, 64, 16, causal=True)          # XCD order
    fwd(4096, 4096, 64, 64, 3, causal=True)           # slab order
    fwd(4096, 4096, 64, 64, 16, causal=True, causal_order=0)
    fwd(2048, 4096, 128, 128, 8, causal=True)         # never p4, never split
    fwd(1000, 1001, 48, 64, 4, causal=True)           # padded, narrow
    fwd(512, 512, 64, 64, 4, dtype=F32, causal=True)
    for variant in (5, 7, 20, 30):
        fwd(4096, 4096, 64, 64, 32, fwd_variant=variant)
        fwd(2048, 2048, 128, 128, 32, fwd_variant=variant)
    fwd(256, 1024, 128, 128, 512, fwd_variant=30)     # p4 refuses, the split stays off
    fwd(256, 8192, 64, 64, 4, fwd_variant=5)          # forced geometry: no split

    # ---- backward ----------------------------------------------------------
    bwd(8192, 8192, 128, 128, 8)                      # single pass, one XCD per slab
    bwd(1024, 1024, 64, 64, 64)                       # single pass
    bwd(1024, 1024, 64, 64, 63)                       # 252 workgroups: two passes
    bwd(1024, 1024, 64, 64, 63, bwd_mode=2)           # single pass, xcd 0
    bwd(1024, 1024, 64, 64, 64, bwd_mode=1)
    bwd(512, 1024, 64, 64, 64, bwd_mode=2)            # 3 K > T: two passes
    bwd(512, 1024, 64, 64, 64, bwd_mode=2, bwd_hoff=2)   # 2 K <= T: single pass
    bwd(768, 1024, 64, 64, 64, bwd_mode=2)            # 3 K <= T
    bwd(768, 1024, 64, 64, 64, bwd_mode=2, bwd_hoff=4)   # 4 K > T
    bwd(1024, 1024, 64, 64, 64, bwd_xcd=0)
    bwd(100, 77, 32, 48, 2)                           # padded
    bwd(1020, 1020, 64, 64, 64, dtype=HF)             # padded to 1024, single pass
    bwd(1024, 1024, 64, 64, 64, mis_q=True)           # misaligned Q: generic
    bwd(1024, 1024, 64, 64, 8, bwd_generic=1)
    bwd(100, 77, 32, 48, 2, bwd_generic=1)
    bwd(512, 512, 64, 64, 4, dtype=F32)
    bwd(256, 384, 96, 32, 2, dtype=F32)
    bwd(512, 512, 64, 64, 4, dtype=F32, bwd_generic=1)
    bwd(128, 128, 32, 32, 2, dtype=F64)
    bwd(1024, 1024, 64, 64, 64, causal=True)
    bwd(1024, 1024, 64, 64, 64, causal=True, bwd_mode=2)
    bwd(100, 177, 32, 48, 2, causal=True)
    bwd(256, 256, 64, 64, 2, dtype=F32, causal=True)
    bwd(128, 128, 32, 32, 2, dtype=F64, causal=True)
    print("dense_dispatch_trace: done")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--list":
        listing(sys.argv[2:])
    else:
        main()
