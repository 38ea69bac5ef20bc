"""Causal against dense attention, forward and backward device time, one process, one run.

    python tools/causal_time.py [--window-s 0.1] [--windows 7]

Per shape (N = Nk, d = dv, bf16): warm-up, then `windows` rounds; a round times one
event-timed window of back-to-back calls (as many as fill `window-s` seconds, at least 10) of
each of: fa_causal_fwd in its default launch order (block-major across an XCD's slabs,
heaviest blocks first), the same with the query blocks in order and slab by slab with a slab's
heaviest block first (fa_debug_set_causal_order(0), (1)), fa_dense_fwd_ws, fa_causal_bwd and fa_dense_bwd
in its two-pass form (fa_debug_set_bwd_mode(1), like for like) — interleaved, so that clock
and co-tenant drift hit all of them alike.  Everything goes through the C ABI with
preallocated outputs and workspaces.

Prints the median and the spread per call, the causal / dense ratio next to the fraction of
(wave, 64-token tile) bodies each causal kernel executes, counted from the kernels' own loop
bounds (tile_fractions below restates them), and the effective TFLOP/s at half the dense
FLOPs (forward 4 N^2 d B / 2, backward 10 N^2 d B / 2: the five products of the textbook
backward; the two-pass form executes seven).
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
    (64, 4096, 64),      # configs[1]
    (64, 8192, 128),     # configs[3]
    (16, 16384, 64),
]


def tile_fractions(N, Nk, d):
    """Executed / dense (wave, tile) bodies of the three causal MFMA kernels, and the
    forward's loaded-tile fraction (loads are workgroup-uniform), from their loop bounds."""
    off, NT, NQT = Nk - N, -(-Nk // 64), -(-N // 64)
    rows_wave = 64 if d <= 64 else 32           # forward: w8q2 (2 x 32 rows per wave) / w8b64
    BM = 8 * rows_wave
    fwd = fwd_ld = fwd_n = 0
    for q0 in range(0, N, BM):
        jt1 = min(NT, (min(q0 + BM - 1, N - 1) + off) // 64 + 1)
        for w in range(8):
            wlast = q0 + (w + 1) * rows_wave - 1 + off
            fwd += sum(1 for j in range(jt1) if j * 64 <= wlast)
            fwd_ld += jt1
            fwd_n += NT
    dq = dq_n = 0
    for q0 in range(0, N, 128):                 # bwd_dq_fast: 4 waves x 32 queries
        nt = min(NT, (min(q0 + 127, N - 1) + off) // 64 + 1)
        for w in range(4):
            dq += sum(1 for t in range(nt) if t * 64 <= q0 + w * 32 + off + 31)
            dq_n += NT
    kv = kv_n = 0
    for k0 in range(0, Nk, 128):                # bwd_dkdv_fast: 4 waves x 32 keys
        t0 = min(max(0, k0 - off) // 64, NQT - 1)
        for w in range(4):
            kv += sum(1 for t in range(t0, NQT) if t * 64 + 63 >= k0 + w * 32 - off)
            kv_n += NQT
    return fwd / fwd_n, fwd_ld / fwd_n, dq / dq_n, kv / kv_n


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
    for (B, N, d) in SHAPES:
        mk = lambda: fa_hip.jl_tensor(torch.randn((N, d, B), generator=g, device="cuda"), dt)
        Q, K, V, dO = mk(), mk(), mk(), mk()
        O, dQ, dK, dV = (fa_hip.jl_empty((N, d, B), dt) for _ in range(4))
        l, m = fa_hip.jl_empty((N, 1, B)), fa_hip.jl_empty((N, 1, B))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        old_mode = L.fa_debug_set_bwd_mode(1)
        nws = max(L.fa_causal_fwd_workspace(code, N, N, d, d, B), L.fa_dense_fwd_workspace(code, N, N, d, d, B),
                  L.fa_causal_bwd_workspace(code, N, N, d, d, B), L.fa_dense_bwd_workspace(code, N, N, d, d, B), 1)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

        def cfwd():
            rc = L.fa_causal_fwd(code, P(Q), P(K), P(V), P(O), P(l), P(m), N, N, d, d, B, 0.0, P(ws), nws, st)
            assert rc == 0, L.fa_last_error()

        def cfwd_inorder():
            old = L.fa_debug_set_causal_order(0)
            cfwd()
            L.fa_debug_set_causal_order(old)

        def cfwd_slabmajor():
            old = L.fa_debug_set_causal_order(1)
            cfwd()
            L.fa_debug_set_causal_order(old)

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
        runs = [("causal fwd", cfwd, None), ("causal fwd in order", cfwd_inorder, None),
                ("causal fwd slab-major", cfwd_slabmajor, None), ("dense fwd", dfwd, None),
                ("causal bwd", cbwd, cfwd), ("dense bwd 2-pass", dbwd, dfwd)]
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
        ff, fl, fq, fk = tile_fractions(N, N, d)
        print(f"B {B} N {N} d {d} bf16", flush=True)
        for name, _, _ in runs:
            v = times[name]
            print(f"  {name:22s} {med[name]*1e6:9.1f} us [{min(v)*1e6:.1f}, {max(v)*1e6:.1f}]", flush=True)
        fl_f, fl_b = 4.0 * N * N * d * B / 2, 10.0 * N * N * d * B / 2
        print(f"  forward : causal / dense {med['causal fwd'] / med['dense fwd']:.3f} (in order {med['causal fwd in order'] / med['dense fwd']:.3f}, "
              f"slab-major heaviest first {med['causal fwd slab-major'] / med['dense fwd']:.3f}); "
              f"tile bodies executed {ff:.3f}, tiles loaded {fl:.3f} of dense; "
              f"{fl_f / med['causal fwd'] / 1e12:.0f} TFLOP/s effective (dense {2 * fl_f / med['dense fwd'] / 1e12:.0f})")
        print(f"  backward: causal / dense 2-pass {med['causal bwd'] / med['dense bwd 2-pass']:.3f}; "
              f"tile bodies executed dQ pass {fq:.3f}, dK/dV pass {fk:.3f} of dense; "
              f"{fl_b / med['causal bwd'] / 1e12:.0f} TFLOP/s effective (dense {2 * fl_b / med['dense bwd 2-pass'] / 1e12:.0f})",
              flush=True)
        assert med["causal fwd"] < med["dense fwd"], "the causal forward is not faster than the dense one"
        assert med["causal bwd"] < med["dense bwd 2-pass"], "the causal backward is not faster than the dense two-pass one"


if __name__ == "__main__":
    main()
