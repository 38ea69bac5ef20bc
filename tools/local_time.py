"""Local (sliding-window) against causal and dense attention, forward and backward device
time, one process, one run.

    python tools/local_time.py [--window-s 0.1] [--windows 7]

Per shape (N = Nk, d = dv, bf16): warm-up, then `windows` rounds; a round times one
event-timed window of back-to-back calls (as many as fill `window-s` seconds, at least 10) of
each of: fa_local_fwd / fa_local_bwd at the windows (1023, 0) and (511, 512), fa_causal_fwd /
fa_causal_bwd, fa_dense_fwd_ws and fa_dense_bwd in its two-pass form
(fa_debug_set_bwd_mode(1), like for like) — interleaved, so that clock and co-tenant drift hit
all of them alike.  Everything goes through the C ABI with preallocated outputs and
workspaces.

Prints the median and the spread per call, each local call's ratio to the causal call of the
same direction, and next to it the fraction of (wave, 64-token tile) bodies the local kernels
execute relative to the causal ones, counted from the kernels' own loop bounds (bodies below
restates them).  At (1023, 0) that fraction is under a third at both shapes, so each local
call must be faster than the causal call it is interleaved with: asserted at the end.
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

SHAPES = [  # (B·H, N, d)
    (16, 16384, 64),
    (64, 8192, 128),
]
WINDOWS = [(1023, 0), (511, 512)]


def bodies(N, Nk, d, left, right):
    """(wave, 64-token tile) bodies the three MFMA kernels execute under the window (left,
    right), a side of Nk or more meaning no bound (so (Nk, 0) counts the causal kernels and
    (Nk, Nk) the dense ones): forward, tiles the forward loads (workgroup-uniform), dQ pass,
    dK/dV pass.  The loop bounds and wave tests of dense_fwd_tiled, bwd_dq_fast, bwd_dkdv_fast."""
    off, NT, NQT = Nk - N, -(-Nk // 64), -(-N // 64)
    left, right = min(left, Nk), min(right, Nk)
    rows_wave = 64 if d <= 64 else 32           # forward: w8q2 (2 x 32 rows per wave) / w8b64
    BM = 8 * rows_wave
    fwd = fwd_ld = 0
    for q0 in range(0, N, BM):
        jt0 = max(0, q0 + off - left) // 64
        jt1 = min(NT, (min(q0 + BM - 1, N - 1) + off + right) // 64 + 1)
        fwd_ld += 8 * (jt1 - jt0)
        for w in range(8):
            wlo, whi = q0 + w * rows_wave + off - left, q0 + (w + 1) * rows_wave - 1 + off + right
            fwd += sum(1 for j in range(jt0, jt1) if j * 64 <= whi and j * 64 + 63 >= wlo)
    dq = 0
    for q0 in range(0, N, 128):                 # bwd_dq_fast: 4 waves x 32 queries
        t0 = max(0, q0 + off - left) // 64
        nt = min(NT, (min(q0 + 127, N - 1) + off + right) // 64 + 1)
        for w in range(4):
            wl = q0 + w * 32 + off
            dq += sum(1 for t in range(t0, nt) if t * 64 <= wl + 31 + right and t * 64 + 63 >= wl - left)
    kv = 0
    for k0 in range(0, Nk, 128):                # bwd_dkdv_fast: 4 waves x 32 keys
        qhi = k0 + 127 - off + left
        t0 = max(0, k0 - off - right) // 64
        t1 = 0 if qhi < 0 else min(NQT, qhi // 64 + 1)
        for w in range(4):
            wk = k0 + w * 32 - off
            kv += sum(1 for t in range(t0, t1) if t * 64 + 63 >= wk - right and t * 64 <= wk + 31 + left)
    return fwd, fwd_ld, dq, kv


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=0.1)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    L = fa_hip.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    dt = torch.bfloat16
    code = fa_hip.DTYPES[dt]
    print(f"device: {torch.cuda.get_device_name(0)}; {a.windows} interleaved windows of {a.window_s} s", flush=True)
    slower = []
    for (B, N, d) in SHAPES:
        mk = lambda: fa_hip.jl_tensor(torch.randn((N, d, B), generator=g, device="cuda"), dt)
        Q, K, V, dO = mk(), mk(), mk(), mk()
        O, dQ, dK, dV = (fa_hip.jl_empty((N, d, B), dt) for _ in range(4))
        l, m = fa_hip.jl_empty((N, 1, B)), fa_hip.jl_empty((N, 1, B))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        old_mode = L.fa_debug_set_bwd_mode(1)
        shape = (code, N, N, d, d, B)
        nws = max(L.fa_local_fwd_workspace(*shape), L.fa_local_bwd_workspace(*shape), L.fa_causal_fwd_workspace(*shape),
                  L.fa_dense_fwd_workspace(*shape), L.fa_causal_bwd_workspace(*shape), L.fa_dense_bwd_workspace(*shape), 1)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

        def lfwd(w):
            def f():
                rc = L.fa_local_fwd(code, P(Q), P(K), P(V), P(O), P(l), P(m), N, N, d, d, B, w[0], w[1], 0.0, P(ws), nws, st)
                assert rc == 0, L.fa_last_error()
            return f

        def lbwd(w):
            def f():
                rc = L.fa_local_bwd(code, P(Q), P(K), P(V), P(O), P(dO), P(l), P(m), P(dQ), P(dK), P(dV),
                                    N, N, d, d, B, w[0], w[1], 0.0, P(ws), nws, st)
                assert rc == 0, L.fa_last_error()
            return f

        def cfwd():
            rc = L.fa_causal_fwd(code, P(Q), P(K), P(V), P(O), P(l), P(m), N, N, d, d, B, 0.0, P(ws), nws, st)
            assert rc == 0, L.fa_last_error()

        def dfwd():
            rc = L.fa_dense_fwd_ws(code, P(Q), P(K), P(V), P(O), P(l), P(m), N, N, d, d, B, 0.0, P(ws), nws, st)
            assert rc == 0, L.fa_last_error()

        def cbwd():
            rc = L.fa_causal_bwd(code, P(Q), P(K), P(V), P(O), P(dO), P(l), P(m), P(dQ), P(dK), P(dV),
                                 N, N, d, d, B, 0.0, P(ws), nws, st)
            assert rc == 0, L.fa_last_error()

        def dbwd():
            rc = L.fa_dense_bwd(code, P(Q), P(K), P(V), P(O), P(dO), P(l), P(m), P(dQ), P(dK), P(dV),
                                N, N, d, d, B, 0.0, P(ws), nws, st)
            assert rc == 0, L.fa_last_error()

        # the backward of each form runs on its own forward's O, l, m: refresh them per window
        runs = []
        for w in WINDOWS:
            runs += [(f"local fwd {w}", lfwd(w), None), (f"local bwd {w}", lbwd(w), lfwd(w))]
        runs += [("causal fwd", cfwd, None), ("causal bwd", cbwd, cfwd), ("dense fwd", dfwd, None),
                 ("dense bwd 2-pass", dbwd, dfwd)]
        reps = {}
        for name, fn, pre in runs:
            if pre:
                pre()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps[name] = max(10, min(20000, int(a.window_s / window(fn, 10)) + 1))
        times = {name: [] for name, _, _ in runs}
        for _ in range(a.windows):
            for name, fn, pre in runs:
                if pre:
                    pre()
                times[name].append(window(fn, reps[name]))
        L.fa_debug_set_bwd_mode(old_mode)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"B {B} N {N} d {d} bf16", flush=True)
        for name, _, _ in runs:
            v = times[name]
            print(f"  {name:24s} {med[name]*1e6:9.1f} us [{min(v)*1e6:.1f}, {max(v)*1e6:.1f}]", flush=True)
        cf, cl, cq, ck = bodies(N, N, d, N, 0)
        df, dl, dq_, dk_ = bodies(N, N, d, N, N)
        print(f"  causal / dense: fwd {med['causal fwd'] / med['dense fwd']:.3f} (bodies {cf / df:.3f}), "
              f"bwd {med['causal bwd'] / med['dense bwd 2-pass']:.3f} (bodies dQ {cq / dq_:.3f}, dK/dV {ck / dk_:.3f})", flush=True)
        for w in WINDOWS:
            f, ld, q, k = bodies(N, N, d, *w)
            rf, rb = med[f"local fwd {w}"] / med["causal fwd"], med[f"local bwd {w}"] / med["causal bwd"]
            print(f"  local {w}: fwd / causal {rf:.3f} (bodies {f / cf:.3f}, tiles loaded {ld / cl:.3f} of causal); "
                  f"bwd / causal {rb:.3f} (bodies dQ pass {q / cq:.3f}, dK/dV pass {k / ck:.3f}, both {(q + k) / (cq + ck):.3f})",
                  flush=True)
            if w == (1023, 0):
                assert f / cf < 1 / 3 and (q + k) / (cq + ck) < 1 / 3
                slower += [f"B {B} N {N} d {d} {nm}" for nm, r in (("forward", rf), ("backward", rb)) if not r < 1.0]
    assert not slower, f"local (1023, 0) is not faster than causal: {slower}"


if __name__ == "__main__":
    main()
