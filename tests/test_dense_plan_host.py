"""CPU test of the dense dispatch plans (csrc/fa_dense_plan.h: dense_fwd_plan, dense_bwd_plan):
which kernel a dense or causal call gets, on what grid, and where its workspace regions lie.
The GPU parity tests pass whichever kernel runs; this table pins the choice.  It was written by
hand from the dispatch rules, never by calling the plan:

forward   fast = Nk % 8 == 0 and K, V aligned (else padded copies if the workspace holds them,
          else generic); wide = N % 8 == 0 and Q, O aligned; 512 rows per workgroup at
          d, dv <= 64, 256 above; split-KV when the grid is below 256 workgroups and there are
          >= 4 key tiles: nsplit = min(ceil(512 / wgs), tiles / 2), then evened out; p4 at
          d = dv = 128 (or variant 30) when its 256-row blocks number >= CUs, Q / O are wide,
          d = dv is exactly 64 or 128, Nk % 64 == 0 and Nk / 64 >= d / 8 + 1.
backward  fast = d, dv in {32, 64, 128}, N, Nk % 8 == 0, aligned; other 16-bit shapes pad;
          single pass with K = ceil(Nk / 256), T = ceil(N / 64) when CUs >= 8, hoff K <= T,
          K <= CUs; xcd = K <= CUs / 8 and B % 8 == 0; in auto also B K >= CUs and K divides
          CUs / 8 (xcd) or CUs.

Unless a row says otherwise: bf16, aligned, 256 CUs, auto knobs, ample workspace.  Shapes are
(N, Nk, d, dv, B).  No kernel is launched.

(16384, 16384, 64, 64, 1) under mode 2 is pinned as the SINGLE pass (K = 64 members, T = 256
slices: 3 K <= T and K <= CUs hold; the fill and K-divides rules are auto-only), which is what
the launcher did before the plans existed; the issue that asked for this table listed it as two
passes, which is the auto answer (64 workgroups < 256 CUs).  Both rows are below."""
from __future__ import annotations

import ctypes

import pytest

import fa_hip

F32, BF16, F16, F64 = 0, 1, 2, 3
AMPLE = 2 ** 64 - 1

# fa::DenseFwdKernel
(F_GENERIC, F_GENERIC_F32, F_F64, F_W8B64, F_W8B64_WIDE, F_W8Q2, F_W8Q2_WIDE, F_W8B64_SPLIT, F_W8Q2_SPLIT,
 F_P4) = range(10)
# fa::DenseBwdKernel
B_F64, B_GENERIC, B_F32_MFMA, B_TWO_PASS, B_SINGLE = range(5)

FWD_FIELDS = ("causal_bits", "pad", "ldk", "nsplit", "tps", "rows", "nqb", "total_wg", "grid", "block", "wide",
              "off_k", "off_v", "off_opart", "off_lpart", "off_mpart", "total")
BWD_FIELDS = ("padded", "N", "Nk", "d", "dv", "slabs_fit", "nkb", "nqt", "xcd", "off_nD", "off_nlse",
              "off_Q", "off_dQ", "off_K", "off_dK", "off_V", "off_dV", "off_O", "off_dO", "off_l", "off_m",
              "off_flags", "off_part", "flag_bytes", "total")


def fwd(shape, want, dtype=BF16, causal=0, variant=0, order=2, kv=1, qo=1, ws=AMPLE, cus=256, **fields):
    return (dtype, *shape, causal, variant, order, kv, qo, ws, cus), want, fields


def bwd(shape, want, dtype=BF16, causal=0, force=0, mode=0, hoff=3, xcd_knob=-1, al=1, ws=AMPLE, cus=256, **fields):
    return (dtype, *shape, causal, force, mode, hoff, xcd_knob, al, ws, cus), want, fields


CFG1 = (4096, 4096, 64, 64, 64)
CFG3 = (8192, 8192, 128, 128, 64)
SMALLQ = (256, 8192, 128, 128, 4)      # 4 workgroups, 128 key tiles
FEWKEYS = (256, 1024, 128, 128, 512)   # 16 key tiles < 128 / 8 + 1
RAGGED = (1024, 1001, 64, 64, 128)     # 2 x 128 = 256 workgroups: no split
RAGGED64 = (1024, 1001, 64, 64, 64)    # 128 workgroups, 16 key tiles: 4 splits of 4 tiles
D128 = (2048, 2048, 128, 128, 32)      # 8 x 32 = 256 blocks of 256 rows
# RAGGED64's workspace: K and V slabs of 1008 x 64 x 64 x 2 B, then opart 4 x 64 x 1024 x 64 x 4 B and
# lpart, mpart 4 x 64 x 1024 x 4 B, each region's 256 B of slack
R64_SLAB, R64_O, R64_LM = 8257536, 67108864, 1048576
R64_TOTAL = 2 * R64_SLAB + 256 + R64_O + 2 * R64_LM + 256

FWD = [
    fwd(CFG1, F_W8Q2_WIDE, nsplit=1, rows=512, nqb=8, total_wg=512, grid=512, block=512, ldk=4096, causal_bits=0, pad=0,
        total=0),
    fwd(CFG1, F_W8Q2_WIDE, dtype=F16),
    fwd((4096, 4096, 32, 64, 64), F_W8Q2_WIDE),
    fwd((4096, 4096, 64, 128, 64), F_W8B64_WIDE, rows=256, grid=1024),   # a 128 class on either side: 256 rows, no p4
    # p4 and its thresholds
    fwd(CFG3, F_P4, rows=256, nqb=32, total_wg=2048, grid=256, block=256, nsplit=1),
    fwd(CFG3, F_P4, cus=304, grid=304),
    fwd((8192, 8192, 128, 128, 8), F_P4, total_wg=256),                  # 256 blocks on 256 CUs
    fwd((8192, 8192, 128, 128, 8), F_W8B64_WIDE, cus=304, nsplit=1),      # fewer blocks than CUs; 256 workgroups: no split
    fwd((8192, 8192, 128, 128, 7), F_W8B64_SPLIT, nsplit=3, tps=43, grid=672),   # 224 blocks: min(ceil(512/224), 64) = 3
    fwd(CFG3, F_W8B64_WIDE, cus=0, nsplit=1, grid=2048),                  # CU count unknown: no p4 (and no split)
    fwd(FEWKEYS, F_W8B64_WIDE, grid=512, nsplit=1),
    fwd((256, 1088, 128, 128, 512), F_P4, grid=256),                      # 17 key tiles
    fwd((256, 1056, 128, 128, 512), F_W8B64_WIDE),                        # Nk % 64 != 0
    fwd((8192, 8192, 96, 96, 64), F_W8B64_WIDE, rows=256, grid=2048),     # p4 needs d equal to its class
    # misaligned K / V are padded; whole key tiles keep ldk = Nk, so p4 takes the copies (2 x 8192 x 128 x 64 x 2 B)
    fwd(CFG3, F_P4, kv=0, pad=1, ldk=8192, total=2 * 134217728 + 256),
    # split-KV and its thresholds
    fwd(SMALLQ, F_W8B64_SPLIT, nsplit=64, tps=2, rows=256, nqb=1, grid=256, off_opart=0, off_lpart=33554432,
        off_mpart=33816576, total=34078976),
    fwd(SMALLQ, F_W8B64_WIDE, ws=34078975, nsplit=1, grid=4),             # one byte short: no split
    fwd(SMALLQ, F_W8B64_WIDE, ws=0, nsplit=1),
    fwd((512, 1024, 64, 64, 255), F_W8Q2_SPLIT, nsplit=3, tps=6, grid=765),
    fwd((512, 1024, 64, 64, 256), F_W8Q2_WIDE, nsplit=1, total=0),
    fwd((512, 192, 64, 64, 4), F_W8Q2_WIDE, nsplit=1),                    # 3 key tiles
    fwd((512, 256, 64, 64, 4), F_W8Q2_SPLIT, nsplit=2, tps=2, grid=8),    # 4 key tiles
    fwd((512, 8192, 48, 64, 200), F_W8Q2_SPLIT, nsplit=3, tps=43),
    # ragged or misaligned K / V
    fwd(RAGGED, F_W8Q2_WIDE, pad=1, ldk=1008, off_k=0, off_v=16515072, total=33030400),
    fwd(RAGGED, F_GENERIC, ws=0, pad=0, ldk=1001, rows=128, nqb=8, grid=1024, block=256, total=33030400),
    fwd(RAGGED, F_GENERIC, ws=33030399, pad=0),
    fwd(RAGGED64, F_W8Q2_SPLIT, pad=1, ldk=1008, nsplit=4, tps=4, off_v=R64_SLAB, off_opart=2 * R64_SLAB,
        off_lpart=2 * R64_SLAB + R64_O, off_mpart=2 * R64_SLAB + R64_O + R64_LM, total=R64_TOTAL),
    fwd(RAGGED64, F_W8Q2_WIDE, ws=R64_TOTAL - 1, pad=1, nsplit=1),
    fwd((1024, 1000, 64, 64, 128), F_W8Q2_WIDE, kv=0, pad=1, ldk=1000, total=2 * 16384000 + 256),
    fwd((1024, 1000, 64, 64, 128), F_GENERIC, kv=0, ws=0, pad=0, total=0),
    fwd((1024, 1000, 64, 64, 128), F_W8Q2_WIDE, pad=0, total=0),
    # narrow forms
    fwd((4092, 4096, 64, 64, 64), F_W8Q2, nqb=8, wide=0),
    fwd(CFG1, F_W8Q2, qo=0),
    fwd((2044, 2048, 128, 128, 32), F_W8B64, nsplit=1),                   # p4 asked, its blocks fill the chip, not wide
    fwd(D128, F_W8B64, qo=0),
    # fp32, Float64, head dims above 128
    fwd((512, 512, 64, 64, 4), F_GENERIC_F32, dtype=F32, rows=128, grid=16, block=256, total=0),
    fwd((512, 1001, 64, 64, 4), F_GENERIC_F32, dtype=F32, total=0),
    fwd(CFG1, F_F64, dtype=F64, total=0),
    fwd((512, 512, 129, 64, 4), -1),
    # causal: the class's geometry, never split, never p4, no variant
    fwd((4096, 4096, 64, 64, 16), F_W8Q2_WIDE, causal=1, rows=512, grid=128, causal_bits=5),
    fwd((4096, 4096, 64, 64, 3), F_W8Q2_WIDE, causal=1, causal_bits=3),    # 24 / 8 = 3 workgroups per XCD, 8 per slab
    fwd((4096, 4096, 64, 64, 16), F_W8Q2_WIDE, causal=1, order=1, causal_bits=3),
    fwd((4096, 4096, 64, 64, 16), F_W8Q2_WIDE, causal=1, order=0, causal_bits=1),
    fwd((4092, 4096, 64, 64, 16), F_W8Q2, causal=1),
    fwd(SMALLQ, F_W8B64_WIDE, causal=1, nsplit=1, grid=4, total=0),
    fwd(CFG3, F_W8B64_WIDE, causal=1, grid=2048, causal_bits=5),
    fwd(D128, F_W8B64_WIDE, causal=1, variant=7),
    fwd(CFG1, F_W8Q2_WIDE, causal=1, variant=5),
    fwd((1000, 1001, 64, 64, 4), F_W8Q2_WIDE, causal=1, pad=1, ldk=1008),
    fwd((1000, 1001, 64, 64, 4), F_GENERIC, causal=1, ws=0, causal_bits=3),
    fwd((512, 512, 64, 64, 4), F_GENERIC_F32, dtype=F32, causal=1, causal_bits=3),
    # forced variants
    fwd(CFG1, F_W8B64_WIDE, variant=5, rows=256, grid=1024),
    fwd(CFG1, F_W8Q2_WIDE, variant=7),
    fwd(CFG1, F_W8Q2, variant=20),
    fwd(CFG1, F_P4, variant=30, grid=256, total_wg=1024),
    fwd(D128, F_W8B64_WIDE, variant=5),
    fwd(D128, F_W8Q2_WIDE, variant=7, rows=512, nqb=4, grid=128),          # the d = 128 form of w8q2
    fwd(D128, F_W8B64, variant=20),                                        # not p4: only 0 and 30 ask for it
    fwd(D128, F_P4, variant=30),
    fwd(SMALLQ, F_W8B64_WIDE, variant=5, nsplit=1),                        # forced geometries never split
    fwd((512, 1024, 64, 64, 255), F_W8Q2_WIDE, variant=7, nsplit=1),
    fwd((512, 1024, 64, 64, 255), F_W8Q2, variant=20, nsplit=1),
    fwd(SMALLQ, F_W8B64_SPLIT, variant=30, nsplit=64),                     # 4 blocks do not fill the chip: as auto
    fwd(FEWKEYS, F_W8B64_WIDE, variant=30, nsplit=1),
    # variant 30 where p4's blocks fill the chip but p4 refuses (d = 48): the split stays off
    fwd((512, 8192, 48, 64, 200), F_W8Q2_WIDE, variant=30, nsplit=1, grid=200),
    fwd((512, 32, 32, 32, 512), F_W8Q2_WIDE, variant=30),                  # no p4 at the 32 class
]

# (100, 77, 32, 48, 2) pads to (104, 80, 32, 64): row statistics 2 x 104 x 2 x 4 = 1664 B (1792 aligned),
# slabs Q 13312, K 10240, V 20480, O 26624, l 832 -> 1024 B
PADDED = (100, 77, 32, 48, 2)
PADDED_TOTAL = 256 + 1664 + 256 + 2 * (13312 + 10240 + 20480 + 26624 + 1024) + 256
# (1024, 1024, 64, 64, 64): row statistics 524288 B; hand-off words 3 x 64 x 16 + 64 + 2 x 64 x 4 + 1 = 3649
# (14848 B aligned); running sums 2 x 64 x 16 x 4 x 4096 B
SQ = (1024, 1024, 64, 64, 64)
SQ_END, SQ_FLAGS, SQ_SUMS = 256 + 524288, 14848, 33554432

BWD = [
    bwd(CFG3, B_SINGLE, nkb=32, nqt=128, xcd=1, padded=0),
    bwd(SQ, B_SINGLE, nkb=4, nqt=16, xcd=1, off_nD=256, off_nlse=256 + 262144, off_flags=SQ_END,
        off_part=SQ_END + SQ_FLAGS, flag_bytes=SQ_FLAGS, total=SQ_END + 256 + SQ_FLAGS + SQ_SUMS + 256),
    bwd(SQ, B_SINGLE, dtype=F16, nkb=4),
    bwd((1024, 1024, 64, 64, 63), B_TWO_PASS, nkb=0, nqt=0),           # 252 workgroups < 256 CUs
    bwd((1024, 1024, 64, 64, 63), B_SINGLE, mode=2, xcd=0),            # 63 % 8 != 0
    bwd((1024, 1024, 64, 64, 63), B_SINGLE, mode=3, xcd=0),
    bwd(SQ, B_TWO_PASS, mode=1, total=SQ_END + 256),
    # the xcd knob at 0: never one XCD per slab; K then has to divide the whole chip
    bwd(SQ, B_SINGLE, xcd_knob=0, xcd=0, nkb=4),
    bwd((1024, 768, 64, 64, 88), B_TWO_PASS, xcd_knob=0),              # K = 3: 256 % 3
    bwd((1024, 768, 64, 64, 88), B_SINGLE, xcd_knob=0, mode=2, xcd=0, nkb=3),
    # hoff K <= T
    bwd((512, 1024, 64, 64, 64), B_TWO_PASS, mode=2),                  # 3 x 4 > 8
    bwd((512, 1024, 64, 64, 64), B_SINGLE, mode=2, hoff=2, nkb=4, nqt=8),
    bwd((768, 1024, 64, 64, 64), B_SINGLE, mode=2, nqt=12),            # 3 x 4 <= 12
    bwd((768, 1024, 64, 64, 64), B_SINGLE, nqt=12),                    # ... and in auto
    bwd((768, 1024, 64, 64, 64), B_TWO_PASS, mode=2, hoff=4),          # 4 x 4 > 12
    bwd((704, 1024, 64, 64, 64), B_TWO_PASS, mode=2),                  # T = 11
    # K divides the CUs its members are dealt over (auto only)
    bwd((1024, 768, 64, 64, 88), B_TWO_PASS),                          # K = 3, one XCD per slab: 32 % 3
    bwd((1024, 768, 64, 64, 88), B_SINGLE, mode=2, nkb=3),
    bwd((16384, 16384, 64, 64, 1), B_TWO_PASS),                        # 64 workgroups
    bwd((16384, 16384, 64, 64, 1), B_SINGLE, mode=2, nkb=64, nqt=256), # K = 64 > 256 / 8: dealt over the chip
    # CU count
    bwd(SQ, B_TWO_PASS, cus=0),
    bwd(SQ, B_TWO_PASS, cus=0, mode=2),
    bwd(SQ, B_TWO_PASS, cus=7, mode=2),
    bwd(SQ, B_SINGLE, cus=8, nkb=4),                                   # K = 4 > 8 / 8: over the chip, 8 % 4 == 0
    bwd(SQ, B_TWO_PASS, cus=304),                                      # 256 workgroups < 304 CUs
    bwd(SQ, B_SINGLE, cus=304, mode=2, xcd=1),
    bwd((16384, 1024, 64, 64, 8), B_TWO_PASS, cus=3),
    # workspace
    bwd(SQ, B_SINGLE, ws=SQ_END + SQ_FLAGS + SQ_SUMS + 256),
    bwd(SQ, B_TWO_PASS, ws=SQ_END + SQ_FLAGS + SQ_SUMS + 255, total=SQ_END + 256),   # one byte short: silently
    # padded shapes
    bwd(PADDED, B_TWO_PASS, padded=1, N=104, Nk=80, d=32, dv=64, slabs_fit=1, off_nlse=256 + 832, off_Q=2048,
        off_dQ=15360, off_K=28672, off_dK=38912, off_V=49152, off_dV=69632, off_O=90112, off_dO=116736,
        off_l=143360, off_m=144384, total=PADDED_TOTAL),
    bwd(PADDED, B_TWO_PASS, ws=145408, slabs_fit=1),
    bwd(PADDED, B_TWO_PASS, ws=145407, slabs_fit=0),
    bwd(PADDED, B_TWO_PASS, al=0, padded=1),                           # copies are aligned whatever the tensors are
    bwd(PADDED, B_GENERIC, force=1, padded=0, N=100, off_nlse=256 + 800, total=PADDED_TOTAL),
    bwd((1020, 1020, 64, 64, 64), B_SINGLE, padded=1, N=1024, Nk=1024, nkb=4, nqt=16, xcd=1),
    bwd((1024, 1024, 48, 64, 64), B_SINGLE, padded=1, d=64),
    bwd((1020, 1020, 64, 64, 64), B_TWO_PASS, causal=1, padded=1),
    # not the MFMA kernels
    bwd(SQ, B_GENERIC, al=0, padded=0, total=SQ_END + 256),
    bwd(SQ, B_GENERIC, force=1),
    bwd(SQ, B_GENERIC, force=1, mode=2),
    bwd((512, 512, 64, 64, 4), B_F32_MFMA, dtype=F32, padded=0, total=256 + 16384 + 256),
    bwd((100, 77, 32, 48, 2), B_F32_MFMA, dtype=F32, al=0, padded=0),
    bwd((512, 512, 64, 64, 4), B_GENERIC, dtype=F32, force=1),
    bwd(((1 << 20) - 1, 64, 32, 32, 1024), B_F32_MFMA, dtype=F32),     # N B = 2^30 - 1024
    bwd((1 << 20, 64, 32, 32, 1024), B_GENERIC, dtype=F32),            # N B = 2^30
    bwd((64, 1 << 20, 32, 32, 1024), B_GENERIC, dtype=F32),
    bwd((128, 128, 32, 32, 2), B_F64, dtype=F64, off_nlse=256 + 2048, total=256 + 4096 + 256),
    bwd((128, 128, 32, 32, 2), B_F64, dtype=F64, causal=1, force=1, total=256 + 4096 + 256),
    # causal: never the single pass, whatever the mode
    *[bwd(SQ, B_TWO_PASS, causal=1, mode=m, nkb=0, total=SQ_END + 256) for m in (0, 1, 2, 3)],
    bwd(CFG3, B_TWO_PASS, causal=1),
    bwd(SQ, B_GENERIC, causal=1, al=0),
    bwd((512, 512, 64, 64, 4), B_F32_MFMA, dtype=F32, causal=1),
]


@pytest.fixture(scope="module")
def L():
    lib = fa_hip.lib()
    i64, ci, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    lib.fa_debug_dense_fwd_plan.restype = ci
    lib.fa_debug_dense_fwd_plan.argtypes = [ci] + [i64] * 5 + [ci] * 5 + [sz, ci, ctypes.POINTER(i64)]
    lib.fa_debug_dense_bwd_plan.restype = ci
    lib.fa_debug_dense_bwd_plan.argtypes = [ci] + [i64] * 5 + [ci] * 6 + [sz, ci, ctypes.POINTER(i64)]
    for name in ("fa_dense_fwd_workspace", "fa_causal_fwd_workspace", "fa_dense_bwd_workspace", "fa_causal_bwd_workspace"):
        getattr(lib, name).restype = sz
        getattr(lib, name).argtypes = [ci] + [i64] * 5
    for name in ("fwd_variant", "causal_order", "bwd_generic", "bwd_mode", "bwd_hoff", "bwd_xcd"):
        getattr(lib, "fa_debug_set_" + name).restype = ci
        getattr(lib, "fa_debug_set_" + name).argtypes = [ci]
    return lib


def _plan(entry, names, args):
    out = (ctypes.c_int64 * len(names))()
    return entry(*args, out), dict(zip(names, out))


def _check(entry, names, table):
    wrong = []
    for args, want, fields in table:
        got, out = _plan(entry, names, args)
        bad = {k: (out[k], v) for k, v in fields.items() if out[k] != v}
        if got != want or bad:
            wrong.append((args, "kernel", got, "want", want, bad))
    assert not wrong, wrong


def test_tables_name_every_kernel_and_knob_value():
    assert {w for _, w, _ in FWD} == set(range(10)) | {-1}
    assert {w for _, w, _ in BWD} == set(range(5))
    assert {a[7] for a, _, _ in FWD} == {0, 5, 7, 20, 30} and {a[8] for a, _, _ in FWD} == {0, 1, 2}
    assert {a[8] for a, _, _ in BWD} == {0, 1, 2, 3} and {a[9] for a, _, _ in BWD} == {2, 3, 4}
    assert {a[10] for a, _, _ in BWD} == {-1, 0}


def test_forward_plan(L):
    _check(L.fa_debug_dense_fwd_plan, FWD_FIELDS, FWD)


def test_backward_plan(L):
    _check(L.fa_debug_dense_bwd_plan, BWD_FIELDS, BWD)


def test_plans_do_not_read_the_thread_knobs(L):
    old = [L.fa_debug_set_fwd_variant(5), L.fa_debug_set_causal_order(0), L.fa_debug_set_bwd_generic(1),
           L.fa_debug_set_bwd_mode(1), L.fa_debug_set_bwd_hoff(4), L.fa_debug_set_bwd_xcd(0)]
    try:
        _check(L.fa_debug_dense_fwd_plan, FWD_FIELDS, FWD[:1] + [r for r in FWD if r[0][6]][:1])
        _check(L.fa_debug_dense_bwd_plan, BWD_FIELDS, BWD[:2])
    finally:
        for name, v in zip(("fwd_variant", "causal_order", "bwd_generic", "bwd_mode", "bwd_hoff", "bwd_xcd"), old):
            getattr(L, "fa_debug_set_" + name)(v)


def test_plan_entries_reject_bad_arguments(L):
    f, b = L.fa_debug_dense_fwd_plan, L.fa_debug_dense_bwd_plan
    assert f(9, *CFG1, 0, 0, 2, 1, 1, AMPLE, 256, None) == -1
    assert f(BF16, 0, 64, 64, 64, 1, 0, 0, 2, 1, 1, AMPLE, 256, None) == -1
    assert f(BF16, 128, 64, 64, 64, 1, 1, 0, 2, 1, 1, AMPLE, 256, None) == -1      # causal needs Nk >= N
    assert f(BF16, *CFG1, 0, 0, 2, 1, 1, AMPLE, 256, None) == F_W8Q2_WIDE           # (out may be null)
    assert b(9, *SQ, 0, 0, 0, 3, -1, 1, AMPLE, 256, None) == -1
    assert b(BF16, 1024, 1024, 64, 0, 64, 0, 0, 0, 3, -1, 1, AMPLE, 256, None) == -1
    assert b(BF16, 1024, 1024, 129, 64, 64, 0, 0, 0, 3, -1, 1, AMPLE, 256, None) == -1
    assert b(BF16, 128, 64, 64, 64, 1, 1, 0, 0, 3, -1, 1, AMPLE, 256, None) == -1


def _device_cus():
    """What fa_dense_bwd_workspace learns from the current device (0 without one)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 0


def test_workspace_entry_points_return_the_plans_total(L):
    """The four queries are the plan's total for the shape alone: aligned tensors, ample room; the
    forward at the auto variant (no CU count: it does not change the total), the backward under
    the thread's knobs and the current device's CU count."""
    for args, _, _ in FWD:
        dt, shape, causal = args[0], args[1:6], args[6]
        if shape[2] > 128 or shape[3] > 128:
            continue
        query = L.fa_causal_fwd_workspace if causal else L.fa_dense_fwd_workspace
        for cus in (0, 256):
            _, out = _plan(L.fa_debug_dense_fwd_plan, FWD_FIELDS, (dt, *shape, causal, 0, 2, 1, 1, AMPLE, cus))
            assert query(dt, *shape) == out["total"], (args, cus)
    cus = _device_cus()
    names = ("bwd_generic", "bwd_mode", "bwd_hoff", "bwd_xcd")
    for args, _, _ in BWD:
        dt, shape, causal, knobs = args[0], args[1:6], args[6], args[7:11]
        old = [getattr(L, "fa_debug_set_" + n)(v) for n, v in zip(names, knobs)]
        try:
            got = (L.fa_causal_bwd_workspace if causal else L.fa_dense_bwd_workspace)(dt, *shape)
        finally:
            for n, v in zip(names, old):
                getattr(L, "fa_debug_set_" + n)(v)
        _, out = _plan(L.fa_debug_dense_bwd_plan, BWD_FIELDS, (dt, *shape, causal, *knobs, 1, AMPLE, cus))
        assert got == out["total"], (args, got, out["total"])
