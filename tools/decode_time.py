"""Decode attention against varlen attention on decode shapes: forward device time, one process,
one run (tools/varlen_time.py's method).

    python tools/decode_time.py [--window-s 0.05] [--windows 5] [--fp8 | --paged | --paged-fp8 | --prefill | --prefill-fp8]

Per shape (bf16, d = dv = 128, the causal window (-1, 0), nq queries per slab, B KV slabs, G query
heads per KV slab, a cache of Nk keys) and per draw of the cache lengths (all full; a fixed-seed
uniform draw on [Nk/8, Nk]): warm-up, then `windows` rounds; a round times one event-timed window
of back-to-back calls (as many as fill `window-s` seconds, at least 3) of fa_decode_fwd and of
fa_varlen_fwd with the same mask, interleaved, so that clock and co-tenant drift hit both alike.
Everything goes through the C ABI with preallocated outputs, lengths and workspaces.

The baseline for G > 1 runs on a cache REPEATED G times (B * G slabs), the only way fa_varlen_fwd
serves grouped heads; the repeat is made once, outside the timed region.

Prints the median and the spread of each, their ratio, and the decode time as a multiple of the
byte floor (sum_b nk_b) * (d + dv) * 2 B / 8 TB/s.  Asserts that decode_fa is faster than its
baseline by more than the larger of the two spreads (max - min of the windows).

--fp8 times the fp8 cache instead: fa_decode_fp8_fwd on quantize_kv_fp8's e4m3fn cache against
fa_decode_fwd on the 16-bit dequantised copy of that same cache (k8 * k_scale rounded to bf16),
same shapes, draws and method, outputs cross-checked.  Prints the ratio 16-bit / fp8 and the fp8
time over its own floor (sum_b nk_b) * (d + dv) * 1 B / 8 TB/s, and says for each row whether fp8
is faster by more than the larger spread; it asserts the cross-check only.

--paged times the paged cache: fa_decode_paged_fwd at page sizes 16, 64 and 256 on pools the same
cache was scattered into through shuffled page tables, against fa_decode_fwd on the contiguous
cache and against gather-then-fa_decode_fwd (paged_kv_gather of the 64-key pool, then
fa_decode_fwd: what a caller with a pool had to do), all in the same interleaved windows, same
shapes and draws, without the nq = 4 row.  The paged outputs are cross-checked against the
contiguous ones; nothing about the times is asserted.

--paged-fp8 times the paged fp8 cache: fa_decode_paged_fp8_fwd at page sizes 16, 64 and 256 on byte
pools quantize_kv_fp8's cache was scattered into through shuffled page tables, against
fa_decode_fp8_fwd on that contiguous fp8 cache (the cost of paging) and against fa_decode_paged_fwd
on 16-bit pools of the dequantised cache scattered through the same tables (the gain from fp8), in
the same interleaved windows, with --paged's shapes and draws.  The paged fp8 outputs are
cross-checked against the contiguous fp8 ones (bitwise equality is reported) and the 16-bit ones
to bf16 rounding; per page size it says whether fp8 is faster or slower than 16-bit by more than
the larger of the two spreads, or a tie; nothing about the times is asserted.

--prefill times chunked prefill over the paged cache: fa_prefill_paged_fwd with G = 8 on N in
{8, 512, 2048} new tokens after a context of 8192 and 32768 keys (k_len = context + N), B in
{1, 8}, page sizes 16 and 64, shuffled tables, against two yardsticks in the same interleaved
windows: "today", what a caller with a pool has without it (paged_kv_gather, a G-fold repeat and
fa_varlen_fwd, all timed), and "varlen alone", fa_varlen_fwd on a cache gathered and repeated
outside the timed region.  Outputs are cross-checked.  Per row: median [min, max] of each, the
two ratios, the achieved TFLOP/s of the new kernel and of varlen alone over the visible-pair
FLOPs 2 (d + dv) B G (N context + N (N + 1) / 2), and whether the new path beats "today" by more
than the sum of the two spreads (max - min); nothing about the times is asserted.

--prefill-fp8 times chunked prefill over the paged fp8 cache: fa_prefill_paged_fp8_fwd on byte pools
(e4m3fn of normal draws, scales of 1.0 passed as device arrays) on --prefill's grid, against
"today", widening the byte pools to 16-bit pools in torch (one pass, exact) and fa_prefill_paged_fwd,
all timed, and against "16-bit alone", fa_prefill_paged_fwd on pools widened beforehand.  Outputs
are cross-checked against 16-bit alone; the same columns and verdict as --prefill.
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

D = 128
SHAPES = [(1, B, G, Nk) for B in (8, 128) for G in (1, 8) for Nk in (8192, 32768)] + [(4, 8, 8, 32768)]   # (nq, B, G, Nk)
HBM_BYTES_PER_S = 8e12


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def fp8_leg(a, L, g, code, left, right):
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    dt = torch.bfloat16
    print("fp8: fa_decode_fp8_fwd on the e4m3fn cache against fa_decode_fwd on its 16-bit dequantised copy", flush=True)
    for (N, B, G, Nk) in SHAPES:
        mk = lambda n, b: fa_hip.jl_tensor(torch.randn((n, D, b), generator=g, device="cuda"), dt)
        Q, K, V = mk(N, B * G), mk(Nk, B), mk(Nk, B)
        K8, V8, KS, VS = fa_hip.quantize_kv_fp8(K, V)
        K.copy_(K8.float() * KS)   # the 16-bit leg's cache: the dequantised values, rounded to bf16
        V.copy_(V8.float() * VS)
        O, O8 = fa_hip.jl_empty((N, D, B * G), dt), fa_hip.jl_empty((N, D, B * G), dt)
        l, m = fa_hip.jl_empty((N, 1, B * G)), fa_hip.jl_empty((N, 1, B * G))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nw = max(L.fa_decode_fwd_workspace(code, N, Nk, D, D, B, G), 1)
        assert L.fa_decode_fp8_fwd_workspace(code, N, Nk, D, D, B, G) in (0, nw)
        ws = torch.empty(nw, dtype=torch.uint8, device="cuda")
        rnd = random.Random(7)
        for name, kl in {"full": [Nk] * B, "uniform": [rnd.randint(Nk // 8, Nk) for _ in range(B)]}.items():
            KL = torch.tensor(kl, dtype=torch.int32, device="cuda")

            def dec():
                rc = L.fa_decode_fwd(code, P(Q), P(K), P(V), P(O), P(l), P(m), N, Nk, D, D, B, G, None, P(KL), left, right,
                                     0.0, P(ws), nw, st)
                assert rc == 0, L.fa_last_error()

            def dec8():
                rc = L.fa_decode_fp8_fwd(code, P(Q), P(K8), P(V8), P(KS), P(VS), P(O8), P(l), P(m), N, Nk, D, D, B, G, None,
                                         P(KL), left, right, 0.0, P(ws), nw, st)
                assert rc == 0, L.fa_last_error()

            runs = [("fp8", dec8), ("16-bit", dec)]
            reps = {}
            for nm, fn in runs:
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                reps[nm] = max(3, min(20000, int(a.window_s / window(fn, 3)) + 1))
            # the 16-bit cache is the fp8 one rounded once more (2^-9 relative): outputs agree to bf16 rounding
            diff, top = float((O8.float() - O.float()).abs().max()), float(O.float().abs().max())
            assert diff <= top / 64, f"fp8 and 16-bit outputs disagree: {diff} against max |O| {top}"
            times = {nm: [] for nm, _ in runs}
            for _ in range(a.windows):
                for nm, fn in runs:
                    times[nm].append(window(fn, reps[nm]))
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = max(max(v) - min(v) for v in times.values())
            floor = sum(kl) * 2 * D / HBM_BYTES_PER_S
            print(f"nq {N} B {B:3d} G {G} Nk {Nk:5d} {name:7s}: fp8 {med['fp8']*1e6:9.1f} us "
                  f"[{min(times['fp8'])*1e6:.1f}, {max(times['fp8'])*1e6:.1f}]  16-bit {med['16-bit']*1e6:9.1f} us "
                  f"[{min(times['16-bit'])*1e6:.1f}, {max(times['16-bit'])*1e6:.1f}]  16-bit / fp8 {med['16-bit']/med['fp8']:5.2f}  "
                  f"fp8 / its byte floor {med['fp8']/floor:6.2f}  max |dO| {diff:.2e}  "
                  f"{'faster' if med['16-bit'] - med['fp8'] > spread else 'NOT FASTER than the spread'}", flush=True)
        del Q, K, V, K8, V8


PAGE_SIZES = (16, 64, 256)


def scatter(K, ps, g):
    """A contiguous (Nk, d, B) cache as a pool (ps, d, Nk / ps * B) of pages in shuffled order and
    its (Nk / ps, B) table."""
    Nk, d, B = K.shape
    mp = Nk // ps
    pages = K.reshape(mp, ps, d, B).permute(1, 2, 0, 3).reshape(ps, d, mp * B)      # page j of slab b at j * B + b
    perm = torch.randperm(mp * B, generator=g, device="cuda")
    pool = fa_hip.jl_empty((ps, d, mp * B), K.dtype)
    pool[:, :, perm] = pages
    return pool, fa_hip.jl_tensor(perm.reshape(mp, B).to(torch.int32), torch.int32)


def paged_leg(a, L, g, code, left, right):
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    dt = torch.bfloat16
    print("paged: fa_decode_paged_fwd at page sizes 16, 64, 256 (shuffled tables) against fa_decode_fwd on the contiguous "
          "cache and against paged_kv_gather + fa_decode_fwd", flush=True)
    for (N, B, G, Nk) in SHAPES:
        if N != 1:
            continue
        mk = lambda n, b: fa_hip.jl_tensor(torch.randn((n, D, b), generator=g, device="cuda"), dt)
        Q, K, V = mk(N, B * G), mk(Nk, B), mk(Nk, B)
        pools = {}
        for ps in PAGE_SIZES:
            gp = torch.Generator(device="cuda").manual_seed(ps)
            (KP, T), (VP, _) = scatter(K, ps, gp), scatter(V, ps, gp.manual_seed(ps))
            pools[ps] = (KP, VP, T)
        O = fa_hip.jl_empty((N, D, B * G), dt)
        OP = {ps: fa_hip.jl_empty((N, D, B * G), dt) for ps in PAGE_SIZES}
        OG = fa_hip.jl_empty((N, D, B * G), dt)
        l, m = fa_hip.jl_empty((N, 1, B * G)), fa_hip.jl_empty((N, 1, B * G))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nw = max(L.fa_decode_fwd_workspace(code, N, Nk, D, D, B, G), 1)
        for ps in PAGE_SIZES:
            assert L.fa_decode_paged_fwd_workspace(code, N, D, D, B, G, ps, Nk // ps) in (0, nw)
        ws = torch.empty(nw, dtype=torch.uint8, device="cuda")
        rnd = random.Random(7)
        for name, kl in {"full": [Nk] * B, "uniform": [rnd.randint(Nk // 8, Nk) for _ in range(B)]}.items():
            KL = torch.tensor(kl, dtype=torch.int32, device="cuda")

            def dec(Kc=K, Vc=V, Oc=O):
                rc = L.fa_decode_fwd(code, P(Q), P(Kc), P(Vc), P(Oc), P(l), P(m), N, Nk, D, D, B, G, None, P(KL), left, right,
                                     0.0, P(ws), nw, st)
                assert rc == 0, L.fa_last_error()

            def paged(ps):
                KP, VP, T = pools[ps]
                rc = L.fa_decode_paged_fwd(code, P(Q), P(KP), P(VP), P(T), P(OP[ps]), P(l), P(m), N, D, D, B, G, ps,
                                           KP.shape[2], Nk // ps, None, P(KL), left, right, 0.0, P(ws), nw, st)
                assert rc == 0, L.fa_last_error()

            def gather():
                Kg, Vg = fa_hip.paged_kv_gather(*pools[64])
                dec(Kg, Vg, OG)

            runs = [("contiguous", dec)] + [(f"page {ps}", (lambda ps=ps: paged(ps))) for ps in PAGE_SIZES] + [("gather", gather)]
            reps = {}
            for nm, fn in runs:
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                reps[nm] = max(3, min(20000, int(a.window_s / window(fn, 3)) + 1))
            top = float(O.float().abs().max())
            same = []
            for ps in PAGE_SIZES + ("gather",):
                o = OG if ps == "gather" else OP[ps]
                diff = float((o.float() - O.float()).abs().max())
                assert diff <= top / 64, f"page {ps} and contiguous outputs disagree: {diff} against max |O| {top}"
                same.append(bool(torch.equal(o, O)))
            times = {nm: [] for nm, _ in runs}
            for _ in range(a.windows):
                for nm, fn in runs:
                    times[nm].append(window(fn, reps[nm]))
            med = {k: statistics.median(v) for k, v in times.items()}
            cell = lambda nm: f"{nm} {med[nm]*1e6:8.1f} us [{min(times[nm])*1e6:.1f}, {max(times[nm])*1e6:.1f}]"
            print(f"nq {N} B {B:3d} G {G} Nk {Nk:5d} {name:7s}: " + "  ".join(cell(nm) for nm, _ in runs) + "  paged / contiguous " +
                  " ".join(f"{med[f'page {ps}']/med['contiguous']:5.2f}" for ps in PAGE_SIZES) +
                  f"  gather / page 64 {med['gather']/med['page 64']:6.2f}  bitwise equal to contiguous {same}", flush=True)
        del Q, K, V, pools


def paged_fp8_leg(a, L, g, code, left, right):
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    dt = torch.bfloat16
    print("paged fp8: fa_decode_paged_fp8_fwd at page sizes 16, 64, 256 (shuffled tables) against fa_decode_fp8_fwd on the "
          "contiguous fp8 cache and against fa_decode_paged_fwd on the 16-bit pools of the same logical cache", flush=True)
    for (N, B, G, Nk) in SHAPES:
        if N != 1:
            continue
        mk = lambda n, b: fa_hip.jl_tensor(torch.randn((n, D, b), generator=g, device="cuda"), dt)
        Q, K, V = mk(N, B * G), mk(Nk, B), mk(Nk, B)
        K8, V8, KS, VS = fa_hip.quantize_kv_fp8(K, V)
        K.copy_(K8.float() * KS)   # the 16-bit pools' cache: the dequantised values, rounded to bf16
        V.copy_(V8.float() * VS)
        pools8, pools16 = {}, {}
        for ps in PAGE_SIZES:
            for pools, (Kc, Vc) in ((pools8, (K8.view(torch.uint8), V8.view(torch.uint8))), (pools16, (K, V))):
                gp = torch.Generator(device="cuda").manual_seed(ps)
                (KP, T), (VP, _) = scatter(Kc, ps, gp), scatter(Vc, ps, gp.manual_seed(ps))
                pools[ps] = (KP, VP, T)
        mko = lambda: fa_hip.jl_empty((N, D, B * G), dt)
        O8, OP8, OP16 = mko(), {ps: mko() for ps in PAGE_SIZES}, {ps: mko() for ps in PAGE_SIZES}
        l, m = fa_hip.jl_empty((N, 1, B * G)), fa_hip.jl_empty((N, 1, B * G))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nw = max(L.fa_decode_fwd_workspace(code, N, Nk, D, D, B, G), 1)
        for ps in PAGE_SIZES:
            assert L.fa_decode_paged_fp8_fwd_workspace(code, N, D, D, B, G, ps, Nk // ps) in (0, nw)
        ws = torch.empty(nw, dtype=torch.uint8, device="cuda")
        rnd = random.Random(7)
        for name, kl in {"full": [Nk] * B, "uniform": [rnd.randint(Nk // 8, Nk) for _ in range(B)]}.items():
            KL = torch.tensor(kl, dtype=torch.int32, device="cuda")

            def dec8():
                rc = L.fa_decode_fp8_fwd(code, P(Q), P(K8), P(V8), P(KS), P(VS), P(O8), P(l), P(m), N, Nk, D, D, B, G, None,
                                         P(KL), left, right, 0.0, P(ws), nw, st)
                assert rc == 0, L.fa_last_error()

            def paged8(ps):
                KP, VP, T = pools8[ps]
                rc = L.fa_decode_paged_fp8_fwd(code, P(Q), P(KP), P(VP), P(KS), P(VS), P(T), P(OP8[ps]), P(l), P(m), N, D, D, B,
                                               G, ps, KP.shape[2], Nk // ps, None, P(KL), left, right, 0.0, P(ws), nw, st)
                assert rc == 0, L.fa_last_error()

            def paged16(ps):
                KP, VP, T = pools16[ps]
                rc = L.fa_decode_paged_fwd(code, P(Q), P(KP), P(VP), P(T), P(OP16[ps]), P(l), P(m), N, D, D, B, G, ps,
                                           KP.shape[2], Nk // ps, None, P(KL), left, right, 0.0, P(ws), nw, st)
                assert rc == 0, L.fa_last_error()

            runs = ([("fp8 contiguous", dec8)] + [(f"fp8 page {ps}", (lambda ps=ps: paged8(ps))) for ps in PAGE_SIZES] +
                    [(f"16-bit page {ps}", (lambda ps=ps: paged16(ps))) for ps in PAGE_SIZES])
            reps = {}
            for nm, fn in runs:
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                reps[nm] = max(3, min(20000, int(a.window_s / window(fn, 3)) + 1))
            # paged fp8 is the contiguous fp8 arithmetic on other addresses; the 16-bit cache is the fp8 one
            # rounded once more (2^-9 relative)
            top = float(O8.float().abs().max())
            same = [bool(torch.equal(OP8[ps], O8)) for ps in PAGE_SIZES]
            for ps in PAGE_SIZES:
                for what, o in (("fp8", OP8[ps]), ("16-bit", OP16[ps])):
                    diff = float((o.float() - O8.float()).abs().max())
                    assert diff <= top / 64, f"{what} page {ps} and contiguous fp8 outputs disagree: {diff} against max |O| {top}"
            times = {nm: [] for nm, _ in runs}
            for _ in range(a.windows):
                for nm, fn in runs:
                    times[nm].append(window(fn, reps[nm]))
            med = {k: statistics.median(v) for k, v in times.items()}
            sp = {k: max(v) - min(v) for k, v in times.items()}
            cell = lambda nm: f"{nm} {med[nm]*1e6:8.1f} us [{min(times[nm])*1e6:.1f}, {max(times[nm])*1e6:.1f}]"

            def verdict(ps):   # fp8 against 16-bit at one page size: beyond the larger of the two spreads, or a tie
                x, y = f"fp8 page {ps}", f"16-bit page {ps}"
                gap = med[y] - med[x]
                return "faster" if gap > max(sp[x], sp[y]) else "SLOWER" if -gap > max(sp[x], sp[y]) else "TIE"

            print(f"nq {N} B {B:3d} G {G} Nk {Nk:5d} {name:7s}: " + "  ".join(cell(nm) for nm, _ in runs) +
                  "  paged fp8 / contiguous fp8 " + " ".join(f"{med[f'fp8 page {ps}']/med['fp8 contiguous']:5.2f}" for ps in PAGE_SIZES) +
                  "  paged 16-bit / paged fp8 " + " ".join(f"{med[f'16-bit page {ps}']/med[f'fp8 page {ps}']:5.2f}" for ps in PAGE_SIZES) +
                  f"  fp8 against 16-bit {[verdict(ps) for ps in PAGE_SIZES]}  bitwise equal to contiguous fp8 {same}", flush=True)
        del Q, K, V, K8, V8, pools8, pools16


def prefill_leg(a, L, g, code, left, right):
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    dt = torch.bfloat16
    G = 8
    print("prefill: fa_prefill_paged_fwd (G = 8, shuffled tables) against today = paged_kv_gather + G-fold repeat + fa_varlen_fwd "
          "(all timed) and against fa_varlen_fwd alone on a cache gathered and repeated beforehand", flush=True)
    for B in (1, 8):
        for N in (8, 512, 2048):
            for ctx in (8192, 32768):
                for ps in (16, 64):
                    nk = ctx + N
                    mp = -(-nk // ps)
                    cap = mp * ps
                    mk = lambda n, b: fa_hip.jl_tensor(torch.randn((n, D, b), generator=g, device="cuda"), dt)
                    Q, K, V = mk(N, B * G), mk(cap, B), mk(cap, B)
                    gp = torch.Generator(device="cuda").manual_seed(ps)
                    (KP, T), (VP, _) = scatter(K, ps, gp), scatter(V, ps, gp.manual_seed(ps))
                    rep = lambda t: fa_hip.jl_tensor(t.repeat_interleave(G, dim=2), dt)
                    KR, VR = rep(K), rep(V)
                    mko = lambda: fa_hip.jl_empty((N, D, B * G), dt)
                    O, OT, OV = mko(), mko(), mko()
                    l, m = fa_hip.jl_empty((N, 1, B * G)), fa_hip.jl_empty((N, 1, B * G))
                    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                    nwp = max(L.fa_prefill_paged_fwd_workspace(code, N, D, D, B, G, ps, mp), 1)
                    nwv = max(L.fa_varlen_fwd_workspace(code, N, cap, D, D, B * G), 1)
                    wsp, wsv = torch.empty(nwp, dtype=torch.uint8, device="cuda"), torch.empty(nwv, dtype=torch.uint8, device="cuda")
                    KL = torch.full((B,), nk, dtype=torch.int32, device="cuda")
                    KLR = KL.repeat_interleave(G)

                    def new():
                        rc = L.fa_prefill_paged_fwd(code, P(Q), P(KP), P(VP), P(T), P(O), P(l), P(m), N, D, D, B, G, ps,
                                                    KP.shape[2], mp, None, P(KL), left, right, 0.0, P(wsp), nwp, st)
                        assert rc == 0, L.fa_last_error()

                    def var(Kc=KR, Vc=VR, Oc=OV):
                        rc = L.fa_varlen_fwd(code, P(Q), P(Kc), P(Vc), P(Oc), P(l), P(m), N, cap, D, D, B * G, None, P(KLR), left,
                                             right, 0.0, P(wsv), nwv, st)
                        assert rc == 0, L.fa_last_error()

                    def today():
                        Kg, Vg = fa_hip.paged_kv_gather(KP, VP, T)
                        var(rep(Kg), rep(Vg), OT)

                    runs = [("new", new), ("today", today), ("varlen alone", var)]
                    reps = {}
                    for nm, fn in runs:
                        for _ in range(2):
                            fn()
                        torch.cuda.synchronize()
                        reps[nm] = max(3, min(20000, int(a.window_s / window(fn, 3)) + 1))
                    top = float(OV.float().abs().max())
                    for what, o in (("new", O), ("today", OT)):
                        diff = float((o.float() - OV.float()).abs().max())
                        assert diff <= top / 64, f"{what} and varlen outputs disagree: {diff} against max |O| {top}"
                    times = {nm: [] for nm, _ in runs}
                    for _ in range(a.windows):
                        for nm, fn in runs:
                            times[nm].append(window(fn, reps[nm]))
                    med = {k: statistics.median(v) for k, v in times.items()}
                    sp = {k: max(v) - min(v) for k, v in times.items()}
                    flops = 2.0 * (D + D) * B * G * (N * ctx + N * (N + 1) / 2)
                    cell = lambda nm: f"{nm} {med[nm]*1e6:9.1f} us [{min(times[nm])*1e6:.1f}, {max(times[nm])*1e6:.1f}]"
                    beats = med["today"] - med["new"] > sp["today"] + sp["new"]
                    print(f"B {B} N {N:4d} context {ctx:5d} page {ps:2d}: " + "  ".join(cell(nm) for nm, _ in runs) +
                          f"  today / new {med['today']/med['new']:7.2f}  varlen alone / new {med['varlen alone']/med['new']:5.2f}  "
                          f"TFLOP/s new {flops/med['new']*1e-12:6.1f} varlen alone {flops/med['varlen alone']*1e-12:6.1f}  "
                          f"{'beats today by more than the spreads' if beats else 'DOES NOT BEAT today by more than the spreads'}",
                          flush=True)
                    del Q, K, V, KP, VP, KR, VR


def prefill_fp8_leg(a, L, g, code, left, right):
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    dt = torch.bfloat16
    G = 8
    print("prefill fp8: fa_prefill_paged_fp8_fwd on byte pools (G = 8, shuffled tables) against today = widening the byte pools to "
          "16-bit pools in torch + fa_prefill_paged_fwd (all timed) and against fa_prefill_paged_fwd alone on pools widened "
          "beforehand", flush=True)
    for B in (1, 8):
        for N in (8, 512, 2048):
            for ctx in (8192, 32768):
                for ps in (16, 64):
                    nk = ctx + N
                    mp = -(-nk // ps)
                    cap = mp * ps
                    mk = lambda n, b: torch.randn((n, D, b), generator=g, device="cuda")
                    Q = fa_hip.jl_tensor(mk(N, B * G), dt)
                    K8, V8 = (fa_hip.jl_tensor(mk(cap, B).to(torch.float8_e4m3fn).view(torch.uint8), torch.uint8) for _ in range(2))
                    gp = torch.Generator(device="cuda").manual_seed(ps)
                    (KP8, T), (VP8, _) = scatter(K8, ps, gp), scatter(V8, ps, gp.manual_seed(ps))
                    # one pass: read the bytes, write twice as many (exact; the scales are 1.0)
                    widen = lambda t: fa_hip.jl_empty(tuple(t.shape), dt).copy_(t.view(torch.float8_e4m3fn))
                    KP, VP = widen(KP8), widen(VP8)
                    ONE = torch.ones(B, dtype=torch.float32, device="cuda")
                    mko = lambda: fa_hip.jl_empty((N, D, B * G), dt)
                    O, OT, OV = mko(), mko(), mko()
                    l, m = fa_hip.jl_empty((N, 1, B * G)), fa_hip.jl_empty((N, 1, B * G))
                    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                    nw = max(L.fa_prefill_paged_fwd_workspace(code, N, D, D, B, G, ps, mp), 1)
                    assert L.fa_prefill_paged_fp8_fwd_workspace(code, N, D, D, B, G, ps, mp) in (0, nw)
                    ws = torch.empty(nw, dtype=torch.uint8, device="cuda")
                    KL = torch.full((B,), nk, dtype=torch.int32, device="cuda")

                    def new():
                        rc = L.fa_prefill_paged_fp8_fwd(code, P(Q), P(KP8), P(VP8), P(ONE), P(ONE), P(T), P(O), P(l), P(m), N, D, D,
                                                        B, G, ps, KP8.shape[2], mp, None, P(KL), left, right, 0.0, P(ws), nw, st)
                        assert rc == 0, L.fa_last_error()

                    def wide(Kc=KP, Vc=VP, Oc=OV):
                        rc = L.fa_prefill_paged_fwd(code, P(Q), P(Kc), P(Vc), P(T), P(Oc), P(l), P(m), N, D, D, B, G, ps,
                                                    Kc.shape[2], mp, None, P(KL), left, right, 0.0, P(ws), nw, st)
                        assert rc == 0, L.fa_last_error()

                    def today():
                        wide(widen(KP8), widen(VP8), OT)

                    runs = [("new", new), ("today", today), ("16-bit alone", wide)]
                    reps = {}
                    for nm, fn in runs:
                        for _ in range(2):
                            fn()
                        torch.cuda.synchronize()
                        reps[nm] = max(3, min(20000, int(a.window_s / window(fn, 3)) + 1))
                    top = float(OV.float().abs().max())
                    for what, o in (("new", O), ("today", OT)):
                        diff = float((o.float() - OV.float()).abs().max())
                        assert diff <= top / 64, f"{what} and 16-bit outputs disagree: {diff} against max |O| {top}"
                    times = {nm: [] for nm, _ in runs}
                    for _ in range(a.windows):
                        for nm, fn in runs:
                            times[nm].append(window(fn, reps[nm]))
                    med = {k: statistics.median(v) for k, v in times.items()}
                    sp = {k: max(v) - min(v) for k, v in times.items()}
                    flops = 2.0 * (D + D) * B * G * (N * ctx + N * (N + 1) / 2)
                    cell = lambda nm: f"{nm} {med[nm]*1e6:9.1f} us [{min(times[nm])*1e6:.1f}, {max(times[nm])*1e6:.1f}]"
                    beats = med["today"] - med["new"] > sp["today"] + sp["new"]
                    print(f"B {B} N {N:4d} context {ctx:5d} page {ps:2d}: " + "  ".join(cell(nm) for nm, _ in runs) +
                          f"  today / new {med['today']/med['new']:7.2f}  16-bit alone / new {med['16-bit alone']/med['new']:5.2f}  "
                          f"TFLOP/s new {flops/med['new']*1e-12:6.1f} 16-bit alone {flops/med['16-bit alone']*1e-12:6.1f}  "
                          f"{'beats today by more than the spreads' if beats else 'DOES NOT BEAT today by more than the spreads'}",
                          flush=True)
                    del Q, K8, V8, KP8, VP8, KP, VP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=0.05)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--paged", action="store_true")
    ap.add_argument("--paged-fp8", action="store_true")
    ap.add_argument("--prefill", action="store_true")
    ap.add_argument("--prefill-fp8", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    L = fa_hip.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    dt = torch.bfloat16
    code = fa_hip.DTYPES[dt]
    left, right = -1, 0
    print(f"device: {torch.cuda.get_device_name(0)}; {a.windows} interleaved windows of {a.window_s} s; bf16, d = dv = {D}, "
          f"window ({left}, {right})" + ("" if a.fp8 or a.paged or a.paged_fp8 or a.prefill or a.prefill_fp8 else
          "; the varlen baseline of G > 1 runs on a cache repeated G times outside the timed region"), flush=True)
    if a.fp8:
        return fp8_leg(a, L, g, code, left, right)
    if a.paged:
        return paged_leg(a, L, g, code, left, right)
    if a.paged_fp8:
        return paged_fp8_leg(a, L, g, code, left, right)
    if a.prefill:
        return prefill_leg(a, L, g, code, left, right)
    if a.prefill_fp8:
        return prefill_fp8_leg(a, L, g, code, left, right)
    missed = []
    for (N, B, G, Nk) in SHAPES:
        mk = lambda n, b: fa_hip.jl_tensor(torch.randn((n, D, b), generator=g, device="cuda"), dt)
        Q, K, V = mk(N, B * G), mk(Nk, B), mk(Nk, B)
        # (Nk, D, B) column-major is [B][D][Nk] in memory: repeating slab b G times in place
        rep = lambda t: t if G == 1 else fa_hip.jl_tensor(t.repeat_interleave(G, dim=2), dt)
        KR, VR = rep(K), rep(V)
        O, O2 = fa_hip.jl_empty((N, D, B * G), dt), fa_hip.jl_empty((N, D, B * G), dt)
        l, m = fa_hip.jl_empty((N, 1, B * G)), fa_hip.jl_empty((N, 1, B * G))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nwd = max(L.fa_decode_fwd_workspace(code, N, Nk, D, D, B, G), 1)
        nwv = max(L.fa_varlen_fwd_workspace(code, N, Nk, D, D, B * G), 1)
        wsd, wsv = torch.empty(nwd, dtype=torch.uint8, device="cuda"), torch.empty(nwv, dtype=torch.uint8, device="cuda")
        rnd = random.Random(7)
        draws = {"full": [Nk] * B, "uniform": [rnd.randint(Nk // 8, Nk) for _ in range(B)]}
        for name, kl in draws.items():
            KL = torch.tensor(kl, dtype=torch.int32, device="cuda")
            KLR = KL.repeat_interleave(G)

            def dec():
                rc = L.fa_decode_fwd(code, P(Q), P(K), P(V), P(O), P(l), P(m), N, Nk, D, D, B, G, None, P(KL), left, right,
                                     0.0, P(wsd), nwd, st)
                assert rc == 0, L.fa_last_error()

            def var():
                rc = L.fa_varlen_fwd(code, P(Q), P(KR), P(VR), P(O2), P(l), P(m), N, Nk, D, D, B * G, None, P(KLR), left, right,
                                     0.0, P(wsv), nwv, st)
                assert rc == 0, L.fa_last_error()

            runs = [("decode", dec), ("varlen", var)]
            reps = {}
            for nm, fn in runs:
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                reps[nm] = max(3, min(20000, int(a.window_s / window(fn, 3)) + 1))
            times = {nm: [] for nm, _ in runs}
            for _ in range(a.windows):
                for nm, fn in runs:
                    times[nm].append(window(fn, reps[nm]))
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = max(max(v) - min(v) for v in times.values())
            floor = sum(kl) * 2 * D * 2 / HBM_BYTES_PER_S
            ok = med["varlen"] - med["decode"] > spread
            print(f"nq {N} B {B:3d} G {G} Nk {Nk:5d} {name:7s}: decode {med['decode']*1e6:9.1f} us "
                  f"[{min(times['decode'])*1e6:.1f}, {max(times['decode'])*1e6:.1f}]  varlen {med['varlen']*1e6:10.1f} us "
                  f"[{min(times['varlen'])*1e6:.1f}, {max(times['varlen'])*1e6:.1f}]  varlen / decode {med['varlen']/med['decode']:7.2f}  "
                  f"decode / byte floor {med['decode']/floor:6.2f}  {'ok' if ok else 'MISSED'}", flush=True)
            if not ok:
                missed.append(f"nq {N} B {B} G {G} Nk {Nk} {name}")
        del Q, K, V, KR, VR
    assert not missed, f"decode_fa is not faster than its varlen_fa baseline by more than the spread: {missed}"


if __name__ == "__main__":
    main()
