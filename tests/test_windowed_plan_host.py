"""CPU test of the windowed dispatch plans (csrc/fa_windowed.h: win_fwd_plan, win_bwd_plan):
which kernel a shape gets.  The GPU parity tests pass whichever kernel runs; this table pins
the choice.  It was written by hand from the dispatch rules (the thresholds kRows4Min 1024,
kStripMin / kStripBwdMin 256, kRows3Min 600 / kRows3Max 1000, kBwdPairMaxPerCu 1.5, 256 CUs
when the device cannot be asked, two / three images' bytes below 2^31 for two / three windows
per row-shift workgroup), never by calling the plan.  No device is touched."""
from __future__ import annotations

import ctypes

import pytest

import fa_hip

F32, BF16, F16, F64 = 0, 1, 2, 3

# fa::WinFwdKernel
(F_COMPOSED, F_FUSED, F_FUSED_WS, F_ROWS, F_ROWS1, F_SHIFT1, F_SHIFT2, F_SHIFT3, F_SHIFT128, F_STRIP,
 F_F32) = range(11)
# fa::WinBwdKernel
B_COMPOSED, B_ROWS1, B_ROWS2, B_ROWS128, B_STRIP, B_STRIP_PARTIAL, B_F32 = range(7)

# geometries: (spatial, ws, stride, pad)
G7 = ((128, 128), 7, 7, 3)       # configs[2]: 19 x 19 = 361 windows, first strip 5 windows, 3 strips per row: 57
G7_56 = ((56, 112), 7, 7, 3)     # 8 x 16 windows, 2 strips per row (32 per image); right end x = 53: partial chunk
G7_32 = ((128, 32), 7, 7, 3)     # 19 x 5 windows, 15 strips per image
WS8 = ((24, 16), 8, 8, 3)        # 3 x 2 = 6 windows of 64 tokens
ONE8 = ((8, 8), 8, 8, 0)         # one window of 64 tokens per image
ONE7 = ((8, 7), 7, 8, 0)         # one window of 49 tokens per image, stride != ws (never strip)
S8 = ((48, 17), 7, 8, 1)         # 6 x 2 = 12 windows, stride != ws
ODDW = ((20, 16), 7, 7, 3)       # width % 8 != 0
OVER = ((16, 16), 7, 4, 3)       # stride < ws: overlapping windows
D1_64 = ((256,), 64, 64, 0)      # 1-D, 64 tokens
D1_128 = ((256,), 128, 128, 0)   # 1-D, 128 tokens
D3 = ((8, 8, 8), 4, 4, 0)        # 3-D, 64 tokens
NARROW = ((4, 16), 8, 8, 3)      # S[0] < 8
# the 8- and 16-pixel-wide strip shapes of tests/test_gpu_windowed_batch_edges.py: one strip per image
ONE7S = ((8, 7), 7, 7, 0)        # one window per image, first strip k0 = 8; the covered right end x = 7 is in a chunk
EDGE7 = ((8, 7), 7, 7, 3)        # two windows per image, k0 = 5 aligns the strip ends; right end past the image
TRI7S = ((16, 7), 7, 7, 3)       # three windows per image, aligned
# three images of P pixels at 64 features: 3 * P * 64 * 2 bytes on either side of 2^31 (win_rows1s x3's offsets)
BIG3_IN = ((2360, 2360), 7, 7, 3)    # 2 138 726 400 B
BIG3_OUT = ((2400, 2400), 7, 7, 3)   # 2 211 840 000 B; two images (1 474 560 000 B) still fit


def fwd(geom, B, want, dtype=BF16, d=64, dv=64, mode=0, qkv=1, y=1):
    return (dtype, geom, d, dv, B, mode, qkv, y, want)


FWD = [
    # configs[2] shape, auto
    fwd(G7, 1, F_SHIFT2),                       # 361 windows, 57 strips
    fwd(G7, 1, F_SHIFT2, dtype=F16),
    fwd(G7, 1, F_SHIFT2, d=32, dv=64),
    fwd(G7, 2, F_SHIFT3),                       # 722 windows
    fwd(G7, 4, F_SHIFT2),                       # 228 strips, 1444 windows
    fwd(G7, 5, F_STRIP),                        # 285 strips
    fwd(G7, 5, F_SHIFT2, y=0),                  # y misaligned: no strip
    fwd(G7, 5, F_FUSED, qkv=0),                 # q, k, v misaligned: register gather
    # kStripMin, both sides
    fwd(G7_32, 17, F_SHIFT2),                   # 3 * 5 * 17 = 255 strips
    fwd(G7_56, 8, F_STRIP),                     # 2 * 16 * 8 = 256 strips
    fwd(ONE7S, 255, F_SHIFT2),                  # one strip per image: 255 strips, 255 windows
    fwd(ONE7S, 256, F_STRIP),
    fwd(EDGE7, 255, F_SHIFT2),                  # 255 strips, 510 windows
    fwd(EDGE7, 256, F_STRIP),
    fwd(TRI7S, 255, F_SHIFT3),                  # 255 strips; 765 windows: three per workgroup
    fwd(TRI7S, 256, F_STRIP),
    # kRows3Min / kRows3Max, both sides (one window per image, stride != ws)
    fwd(ONE7, 599, F_SHIFT2),
    fwd(ONE7, 600, F_SHIFT3),
    fwd(ONE7, 999, F_SHIFT3),
    fwd(ONE7, 1000, F_SHIFT2),
    fwd(S8, 2, F_SHIFT2),                       # stride != ws: never strip
    fwd(S8, 50, F_SHIFT3),                      # 600 windows
    # ws = 8: row scatter; kRows4Min, both sides
    fwd(WS8, 2, F_ROWS1),
    fwd(WS8, 170, F_ROWS1),                     # 1020 windows
    fwd(WS8, 171, F_ROWS),                      # 1026
    fwd(ONE8, 1023, F_ROWS1),
    fwd(ONE8, 1024, F_ROWS),
    # shapes outside the row-staged kernels
    fwd(ODDW, 2, F_FUSED),
    fwd(OVER, 2, F_FUSED_WS),
    fwd(D1_64, 2, F_FUSED),
    fwd(D1_128, 2, F_COMPOSED),
    fwd(D3, 2, F_FUSED),
    # d or dv in (64, 128]
    fwd(G7, 1, F_SHIFT128, d=96, dv=96),
    fwd(G7, 5, F_SHIFT128, d=96, dv=32),
    fwd(G7, 1, F_SHIFT128, d=64, dv=128),
    fwd(G7, 1, F_COMPOSED, d=96, dv=96, qkv=0),
    fwd(WS8, 2, F_COMPOSED, d=96, dv=96),       # the 128-wide kernel is ws <= 7
    fwd(ODDW, 2, F_COMPOSED, d=96, dv=96),
    # fp32, Float64
    fwd(WS8, 2, F_F32, dtype=F32),
    fwd(G7, 1, F_F32, dtype=F32, qkv=0, y=0),   # the fp32 kernel does not ask for alignment
    fwd(NARROW, 2, F_COMPOSED, dtype=F32),
    fwd(WS8, 2, F_COMPOSED, dtype=F32, d=96, dv=96),
    fwd(OVER, 2, F_COMPOSED, dtype=F32),
    fwd(G7, 1, F_COMPOSED, dtype=F64),
    fwd(WS8, 2, F_COMPOSED, dtype=F64),
    # mode 1: composed everywhere
    fwd(G7, 1, F_COMPOSED, mode=1),
    fwd(G7, 5, F_COMPOSED, mode=1),
    fwd(G7, 1, F_COMPOSED, mode=1, d=96, dv=96),
    fwd(WS8, 2, F_COMPOSED, mode=1),
    fwd(WS8, 2, F_COMPOSED, mode=1, dtype=F32),
    fwd(OVER, 2, F_COMPOSED, mode=1),
    fwd(D1_64, 2, F_COMPOSED, mode=1),
    # mode 2: register gather; not at d > 64
    fwd(G7, 1, F_FUSED, mode=2),
    fwd(G7, 1, F_COMPOSED, mode=2, d=96, dv=96),
    # mode 3: one window per workgroup; not where the row-staged kernels do not apply
    fwd(G7, 1, F_SHIFT1, mode=3),
    fwd(G7, 5, F_SHIFT1, mode=3),
    fwd(WS8, 171, F_ROWS1, mode=3),
    fwd(ODDW, 2, F_FUSED, mode=3),
    # mode 4: four-window row scatter
    fwd(WS8, 2, F_ROWS, mode=4),
    fwd(G7, 1, F_ROWS, mode=4),
    fwd(G7, 1, F_FUSED, mode=4, qkv=0),
    # mode 5: one-window row scatter
    fwd(G7, 1, F_ROWS1, mode=5),
    fwd(OVER, 2, F_FUSED_WS, mode=5),
    # mode 6: two windows per workgroup
    fwd(G7, 2, F_SHIFT2, mode=6),
    fwd(G7, 5, F_SHIFT2, mode=6),
    fwd(WS8, 171, F_ROWS1, mode=6),             # ws 8 has no row-shift kernel
    # mode 10: strip below kStripMin too
    fwd(G7, 1, F_STRIP, mode=10),
    fwd(G7, 1, F_SHIFT2, mode=10, y=0),
    fwd(S8, 2, F_SHIFT2, mode=10),              # stride != ws
    fwd(ONE7S, 1, F_STRIP, mode=10),            # a single strip of one window
    fwd(EDGE7, 7, F_STRIP, mode=10),
    fwd(TRI7S, 2, F_STRIP, mode=10),
    # mode 12: three windows per workgroup, while three images' bytes fit 32-bit offsets
    fwd(G7, 1, F_SHIFT3, mode=12),
    fwd(G7, 5, F_SHIFT3, mode=12),
    fwd(WS8, 2, F_ROWS1, mode=12),
    fwd(ONE7, 7, F_SHIFT3, mode=12),            # one window per image: a workgroup spans three images
    fwd(BIG3_IN, 1, F_SHIFT3, mode=12),
    fwd(BIG3_OUT, 1, F_SHIFT2, mode=12),
    # mode 13 is the backward's; the forward takes two windows per workgroup
    fwd(G7, 2, F_SHIFT2, mode=13),
    fwd(G7, 5, F_SHIFT2, mode=13),
]


def bwd(geom, B, want, dtype=BF16, d=64, dv=64, mode=0, ins=1, grads=1, cus=256):
    return (dtype, geom, d, dv, B, mode, ins, grads, cus, want)


BWD = [
    # configs[2] shape, auto
    bwd(G7, 1, B_ROWS2),                        # 361 windows <= 1.5 * 256
    bwd(G7, 1, B_ROWS1, cus=128),               # 361 > 192
    bwd(G7, 1, B_ROWS2, dtype=F16),
    bwd(G7, 2, B_ROWS1),
    bwd(G7, 4, B_ROWS1),                        # 228 strips
    bwd(G7, 5, B_STRIP),                        # 285 strips, right end past the image
    bwd(G7, 5, B_ROWS1, grads=0),               # a gradient misaligned: no strip
    bwd(G7, 5, B_COMPOSED, ins=0),              # an input misaligned: no fused kernel
    # kStripBwdMin, both sides
    bwd(G7_32, 17, B_ROWS1),                    # 255 strips
    bwd(G7_56, 8, B_STRIP_PARTIAL),             # 256 strips; the covered right end x = 53 is in a chunk
    bwd(ONE7S, 255, B_ROWS2),                   # 255 strips; 255 windows <= 384
    bwd(ONE7S, 256, B_STRIP_PARTIAL),           # the covered right end x = 7 is in a chunk
    bwd(ONE7S, 257, B_STRIP_PARTIAL),
    bwd(EDGE7, 255, B_ROWS1),                   # 255 strips; 510 windows > 384
    bwd(EDGE7, 256, B_STRIP),                   # k0 = 5 aligns the ends, the right end is past the image
    bwd(TRI7S, 256, B_STRIP),
    # kBwdPairMaxPerCu, both sides; 256 CUs when the device cannot be asked
    bwd(ONE7, 384, B_ROWS2),
    bwd(ONE7, 385, B_ROWS1),
    bwd(ONE7, 192, B_ROWS2, cus=128),
    bwd(ONE7, 193, B_ROWS1, cus=128),
    bwd(ONE7, 384, B_ROWS2, cus=0),
    bwd(ONE7, 385, B_ROWS1, cus=0),
    bwd(S8, 2, B_ROWS2),
    # shapes outside the fused kernels
    bwd(WS8, 2, B_COMPOSED),                    # ws 8
    bwd(ODDW, 2, B_COMPOSED),
    bwd(OVER, 2, B_COMPOSED),
    bwd(D1_64, 2, B_COMPOSED),
    bwd(D3, 2, B_COMPOSED),
    # d or dv in (64, 128]
    bwd(G7, 1, B_ROWS128, d=96, dv=96),
    bwd(G7, 5, B_ROWS128, d=32, dv=96),
    bwd(G7, 1, B_COMPOSED, d=96, dv=96, ins=0),
    # fp32, Float64
    bwd(WS8, 2, B_F32, dtype=F32),
    bwd(G7, 1, B_F32, dtype=F32, ins=0, grads=0),
    bwd(NARROW, 2, B_COMPOSED, dtype=F32),
    bwd(WS8, 2, B_COMPOSED, dtype=F32, d=96, dv=96),
    bwd(G7, 1, B_COMPOSED, dtype=F64),
    # mode 1: composed everywhere
    bwd(G7, 1, B_COMPOSED, mode=1),
    bwd(G7, 5, B_COMPOSED, mode=1),
    bwd(G7, 1, B_COMPOSED, mode=1, d=96, dv=96),
    bwd(WS8, 2, B_COMPOSED, mode=1, dtype=F32),
    # mode 10: strip below kStripBwdMin too
    bwd(G7, 1, B_STRIP, mode=10),
    bwd(S8, 2, B_ROWS1, mode=10),               # stride != ws; a forced mode never pairs
    bwd(G7, 1, B_ROWS1, mode=10, grads=0),
    bwd(ONE7S, 1, B_STRIP_PARTIAL, mode=10),
    bwd(EDGE7, 7, B_STRIP, mode=10),
    bwd(TRI7S, 2, B_STRIP, mode=10),
    # mode 13: two windows per workgroup at any size
    bwd(G7, 2, B_ROWS2, mode=13),
    bwd(G7, 5, B_ROWS2, mode=13),
    bwd(G7, 1, B_ROWS128, mode=13, d=96, dv=96),
    # the forward's modes: one window per workgroup, never the strip kernel
    *[bwd(G7, 1, B_ROWS1, mode=m) for m in (2, 3, 4, 5, 6, 12)],
    bwd(G7, 5, B_ROWS1, mode=6),
    bwd(WS8, 2, B_F32, mode=3, dtype=F32),
]


@pytest.fixture(scope="module")
def L():
    lib = fa_hip.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    geom = [ci, ci, ctypes.POINTER(i64), i64, i64, i64, i64, i64, i64]
    lib.fa_debug_win_fwd_plan.restype = ci
    lib.fa_debug_win_fwd_plan.argtypes = geom + [ci, ci, ci]
    lib.fa_debug_win_bwd_plan.restype = ci
    lib.fa_debug_win_bwd_plan.argtypes = geom + [ci, ci, ci, ci]
    lib.fa_debug_set_win_composed.restype = ci
    lib.fa_debug_set_win_composed.argtypes = [ci]
    return lib


def _geom_args(dtype, geom, d, dv, B):
    S, ws, stride, pad = geom
    return (dtype, len(S), (ctypes.c_int64 * len(S))(*S), d, dv, B, ws, stride, pad)


def test_tables_name_every_kernel_and_mode():
    assert {r[-1] for r in FWD} == set(range(11))
    assert {r[-1] for r in BWD} == set(range(7))
    modes = {0, 1, 2, 3, 4, 5, 6, 10, 12, 13}
    assert {r[5] for r in FWD} == modes and {r[5] for r in BWD} == modes


def test_forward_plan(L):
    got = [L.fa_debug_win_fwd_plan(*_geom_args(dt, g, d, dv, B), mode, qkv, y)
           for dt, g, d, dv, B, mode, qkv, y, _ in FWD]
    wrong = [(row, k) for row, k in zip(FWD, got) if k != row[-1]]
    assert not wrong, wrong


def test_backward_plan(L):
    got = [L.fa_debug_win_bwd_plan(*_geom_args(dt, g, d, dv, B), mode, ins, grads, cus)
           for dt, g, d, dv, B, mode, ins, grads, cus, _ in BWD]
    wrong = [(row, k) for row, k in zip(BWD, got) if k != row[-1]]
    assert not wrong, wrong


def test_plans_do_not_read_the_thread_knob(L):
    args = _geom_args(BF16, G7, 64, 64, 1)
    old = L.fa_debug_set_win_composed(1)
    try:
        assert L.fa_debug_win_fwd_plan(*args, 0, 1, 1) == F_SHIFT2
        assert L.fa_debug_win_bwd_plan(*args, 0, 1, 1, 256) == B_ROWS2
    finally:
        L.fa_debug_set_win_composed(old)


def test_plan_entries_reject_bad_arguments(L):
    assert L.fa_debug_win_fwd_plan(*_geom_args(9, G7, 64, 64, 1), 0, 1, 1) == -1
    assert L.fa_debug_win_fwd_plan(*_geom_args(BF16, G7, 0, 64, 1), 0, 1, 1) == -1
    assert L.fa_debug_win_bwd_plan(*_geom_args(BF16, ((4, 4), 7, 7, 0), 64, 64, 1), 0, 1, 1, 256) == -1


def _align256(x):
    return (x + 255) & ~255


def test_forward_workspace_follows_the_plan(L):
    """fa_windowed_fwd_workspace (which cannot see the pointers): 0 exactly when the plan is a
    kernel that stores y directly within win_fused's limits, the window outputs when win_fused
    goes through the workspace, the composed path's size otherwise (the 128-wide and fp32
    kernels' plans included)."""
    direct = {F_FUSED, F_ROWS, F_ROWS1, F_SHIFT1, F_SHIFT2, F_SHIFT3, F_STRIP}
    esize = {F32: 4, BF16: 2, F16: 2, F64: 8}
    for dt, g, d, dv, B, mode, _, _, plan in FWD:
        S, ws, stride, pad = g
        T, nwin = ws ** len(S), B
        for s in S:
            nwin *= (s + 2 * pad - ws) // stride + 1
        tok, e = T * nwin, esize[dt]
        if plan in direct:
            want = 0
        elif plan == F_FUSED_WS:
            want = _align256(tok * dv * e) + 256
        else:
            want = (2 * _align256(tok * d * e) + 2 * _align256(tok * dv * e) +
                    _align256(L.fa_dense_fwd_workspace(dt, T, T, d, dv, nwin)) + 256)
        old = L.fa_debug_set_win_composed(mode)
        try:
            got = L.fa_windowed_fwd_workspace(*_geom_args(dt, g, d, dv, B))
        finally:
            L.fa_debug_set_win_composed(old)
        assert got == want, (dt, g, d, dv, B, mode, plan, got, want)
