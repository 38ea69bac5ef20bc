"""Varlen against local attention, and varlen at shorter lengths against varlen at full
lengths: forward and backward device time, one process, one run (tools/local_time.py's method).

    python tools/varlen_time.py [--window-s 0.1] [--windows 7]

Per shape (N = Nk, d = dv, bf16, the causal window (-1, 0)): warm-up, then `windows` rounds; a
round times one event-timed window of back-to-back calls (as many as fill `window-s` seconds, at
least 10) of each of: fa_local_fwd / fa_local_bwd, and fa_varlen_fwd / fa_varlen_bwd at full
lengths, at all lengths N/2, and at a fixed-seed uniform draw on [N/8, N] (q_lens = k_lens) —
interleaved, so that clock and co-tenant drift hit all of them alike.  Everything goes through
the C ABI with preallocated outputs, lengths and workspaces.

Prints the median and the spread per call; varlen-full's ratio to the local call of the same
interleaved run; and each shorter call's ratio to varlen-full, with the fraction of
(wave, 64-token tile) bodies it executes beside it, counted from the kernels' own loop bounds
(bodies below restates them per slab).  Asserts only that the N/2 calls are faster than the
full-length calls: under a causal window they execute about a quarter of the bodies.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import random
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


def bodies(N, Nk, d, nq, nk, left, right):
    """(wave, 64-token tile) bodies the three MFMA kernels execute on one slab of lengths
    (nq, nk) under the window (left, right), a negative side meaning no bound: forward, dQ pass,
    dK/dV pass.  The loop bounds and wave tests of dense_fwd_tiled, bwd_dq_fast and
    bwd_dkdv_fast under kMaskVarlen."""
    off = nk - nq
    left = nk if left < 0 else min(left, nk)
    right = nq if right < 0 else min(right, nq)
    NT, NQT = -(-nk // 64), -(-nq // 64)
    rows_wave = 64 if d <= 64 else 32
    BM = 8 * rows_wave
    fwd = 0
    for q0 in range(0, N, BM):
        hi = min(q0 + BM - 1, nq - 1) + off + right
        jt0, jt1 = max(0, q0 + off - left) // 64, (0 if hi < 0 else min(NT, hi // 64 + 1))
        if q0 >= nq or jt0 >= jt1:
            continue
        for w in range(8):
            if q0 + w * rows_wave >= nq:
                continue
            wlo, whi = q0 + w * rows_wave + off - left, q0 + (w + 1) * rows_wave - 1 + off + right
            fwd += sum(1 for j in range(jt0, jt1) if j * 64 <= whi and j * 64 + 63 >= wlo)
    dq = 0
    for q0 in range(0, N, 128):
        hi = min(q0 + 127, nq - 1) + off + right
        t0, nt = max(0, q0 + off - left) // 64, (0 if hi < 0 else min(NT, hi // 64 + 1))
        if q0 >= nq or t0 >= nt:
            continue
        for w in range(4):
            wl = q0 + w * 32 + off
            dq += sum(1 for t in range(t0, nt) if t * 64 <= wl + 31 + right and t * 64 + 63 >= wl - left)
    kv = 0
    for k0 in range(0, Nk, 128):
        qhi = k0 + 127 - off + left
        t0 = max(0, k0 - off - right) // 64
        t1 = 0 if qhi < 0 or k0 >= nk else min(NQT, qhi // 64 + 1)
        for w in range(4):
            wk = k0 + w * 32 - off
            kv += sum(1 for t in range(t0, t1) if t * 64 + 63 >= wk - right and t * 64 <= wk + 31 + left)
    return fwd, dq, kv


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
    left, right = -1, 0
    print(f"device: {torch.cuda.get_device_name(0)}; {a.windows} interleaved windows of {a.window_s} s; window ({left}, {right})",
          flush=True)
    slower = []
    for (B, N, d) in SHAPES:
        mk = lambda: fa_hip.jl_tensor(torch.randn((N, d, B), generator=g, device="cuda"), dt)
        Q, K, V, dO = mk(), mk(), mk(), mk()
        O, dQ, dK, dV = (fa_hip.jl_empty((N, d, B), dt) for _ in range(4))
        l, m = fa_hip.jl_empty((N, 1, B)), fa_hip.jl_empty((N, 1, B))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        shape = (code, N, N, d, d, B)
        nws = max(L.fa_local_fwd_workspace(*shape), L.fa_local_bwd_workspace(*shape), L.fa_varlen_fwd_workspace(*shape),
                  L.fa_varlen_bwd_workspace(*shape), 1)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        rnd = random.Random(7)
        draws = {"full": [N] * B, "half": [N // 2] * B, "uniform": [rnd.randint(N // 8, N) for _ in range(B)]}
        lens = {k: torch.tensor(v, dtype=torch.int32, device="cuda") for k, v in draws.items()}

        def lfwd():
            rc = L.fa_local_fwd(code, P(Q), P(K), P(V), P(O), P(l), P(m), N, N, d, d, B, left, right, 0.0, P(ws), nws, st)
            assert rc == 0, L.fa_last_error()

        def lbwd():
            rc = L.fa_local_bwd(code, P(Q), P(K), P(V), P(O), P(dO), P(l), P(m), P(dQ), P(dK), P(dV),
                                N, N, d, d, B, left, right, 0.0, P(ws), nws, st)
            assert rc == 0, L.fa_last_error()

        def vfwd(t):
            def f():
                rc = L.fa_varlen_fwd(code, P(Q), P(K), P(V), P(O), P(l), P(m), N, N, d, d, B, P(t), P(t), left, right, 0.0,
                                     P(ws), nws, st)
                assert rc == 0, L.fa_last_error()
            return f

        def vbwd(t):
            def f():
                rc = L.fa_varlen_bwd(code, P(Q), P(K), P(V), P(O), P(dO), P(l), P(m), P(dQ), P(dK), P(dV),
                                     N, N, d, d, B, P(t), P(t), left, right, 0.0, P(ws), nws, st)
                assert rc == 0, L.fa_last_error()
            return f

        # the backward of each form runs on its own forward's O, l, m: refresh them per window
        runs = [("local fwd", lfwd, None), ("local bwd", lbwd, lfwd)]
        for k, t in lens.items():
            runs += [(f"varlen fwd {k}", vfwd(t), None), (f"varlen bwd {k}", vbwd(t), vfwd(t))]
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
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"B {B} N {N} d {d} bf16", flush=True)
        for name, _, _ in runs:
            v = times[name]
            print(f"  {name:24s} {med[name]*1e6:9.1f} us [{min(v)*1e6:.1f}, {max(v)*1e6:.1f}]", flush=True)
        print(f"  varlen full / local: fwd {med['varlen fwd full'] / med['local fwd']:.3f}, "
              f"bwd {med['varlen bwd full'] / med['local bwd']:.3f}", flush=True)
        tot = {k: [sum(x) for x in zip(*(bodies(N, N, d, n, n, left, right) for n in v))] for k, v in draws.items()}
        for k in ("half", "uniform"):
            rf, rb = med[f"varlen fwd {k}"] / med["varlen fwd full"], med[f"varlen bwd {k}"] / med["varlen bwd full"]
            f, q, kv = (tot[k][i] / tot["full"][i] for i in range(3))
            both = (tot[k][1] + tot[k][2]) / (tot["full"][1] + tot["full"][2])
            print(f"  varlen {k} / full: fwd {rf:.3f} (bodies {f:.3f}); bwd {rb:.3f} (bodies dQ pass {q:.3f}, "
                  f"dK/dV pass {kv:.3f}, both {both:.3f})", flush=True)
            if k == "half":
                slower += [f"B {B} N {N} d {d} {nm}" for nm, r in (("forward", rf), ("backward", rb)) if not r < 1.0]
    assert not slower, f"varlen at N/2 is not faster than varlen at full lengths: {slower}"


if __name__ == "__main__":
    main()
