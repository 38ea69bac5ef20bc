"""Circulant forward and backward device time, one process, one run.

    python tools/circ_bwd_time.py [--window-s 0.1] [--windows 7]

Per shape: warm-up, then `windows` event-timed windows of back-to-back calls (as many as
fill `window-s` seconds, at least 20) of fa_circulant_fwd and of fa_circulant_bwd
(pre-pass included) through the C ABI, with preallocated outputs and workspace, so
nothing but the library's launches is in a window.  Prints the median and the spread per
call, the backward / forward ratio and the HBM rate of the array passes each needs
(forward 4: Q K V O; backward 13: O dO | Q dO K V dQ | K V Q dO dK dV).
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flashattention.jl_amd")]
import torch  # noqa: E402

import fa_hip  # noqa: E402

SHAPES = [  # (B·H, N, d, W, dtype)
    (64, 16384, 64, 129, torch.bfloat16),
    (1, 4096, 32, 16, torch.bfloat16),
    (1, 4096, 32, 256, torch.bfloat16),
]


def timed(fn, window_s, windows):
    """Median / min / max seconds per call over `windows` windows of `window_s` seconds."""
    out = []
    reps = 20
    for w in range(windows + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1) * 1e-3 / reps
        if w == 0:   # calibration window, not reported
            reps = max(20, min(20000, int(window_s / t) + 1))
        else:
            out.append(t)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=0.1)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    L = fa_hip.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    print(f"device: {torch.cuda.get_device_name(0)}; {a.windows} windows of {a.window_s} s", flush=True)
    for (B, N, d, W, dt) in SHAPES:
        mk = lambda: fa_hip.jl_tensor(torch.randn((N, d, B), generator=g, device="cuda"), dt)
        Q, K, V, dO = mk(), mk(), mk(), mk()
        O, dQ, dK, dV = (fa_hip.jl_empty((N, d, B), dt) for _ in range(4))
        l, m = fa_hip.jl_empty((N, 1, B)), fa_hip.jl_empty((N, 1, B))
        code = fa_hip.DTYPES[dt]
        nws = L.fa_circulant_bwd_workspace(code, N, d, d, B, W)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def fwd():
            rc = L.fa_circulant_fwd(code, P(Q), P(K), P(V), P(O), P(l), P(m), N, d, d, B, W, 0.0, st)
            assert rc == 0, L.fa_last_error()

        def bwd():
            rc = L.fa_circulant_bwd(code, P(Q), P(K), P(V), P(O), P(dO), P(l), P(m), P(dQ), P(dK), P(dV),
                                    N, d, d, B, W, 0.0, P(ws), nws, st)
            assert rc == 0, L.fa_last_error()

        for _ in range(10):
            fwd()
            bwd()
        torch.cuda.synchronize()
        assert L.fa_debug_last_circ_bwd_kernel() == 1, "not the MFMA path"
        esz = Q.element_size()
        arr = B * N * d * esz
        tf = timed(fwd, a.window_s, a.windows)
        tb = timed(bwd, a.window_s, a.windows)
        name = f"B {B} N {N} d {d} W {W} {str(dt)[6:]}"
        print(f"{name}: fwd {tf[0]*1e6:8.1f} us [{tf[1]*1e6:.1f}, {tf[2]*1e6:.1f}]  {4*arr/tf[0]/1e9:6.0f} GB/s | "
              f"bwd {tb[0]*1e6:8.1f} us [{tb[1]*1e6:.1f}, {tb[2]*1e6:.1f}]  {13*arr/tb[0]/1e9:6.0f} GB/s | "
              f"bwd/fwd {tb[0]/tf[0]:.2f}", flush=True)


if __name__ == "__main__":
    main()
