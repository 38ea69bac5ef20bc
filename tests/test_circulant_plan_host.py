"""CPU test of the circulant dispatch plans (csrc/fa_circulant_plan.h: circ_fwd_plan,
circ_bwd_plan): which kernel a circulant call gets, on what grid, with how much dynamic LDS,
and where the backward's workspace regions lie.  The GPU parity tests pass whichever kernel
runs; this table pins the choice.  It was written by hand from the dispatch rules, never by
calling the plan:

both      refused (-1, FA_ERR_UNSUPPORTED): d or dv above 128; N d esz or N dv esz >= 2^31 - 1 bytes,
          W > (2^31 - 1) / 2, N B > 2 (2^31 - 1).
forward   tiled MFMA (1) when 16-bit, N % 8 == 0, K and V aligned, knob 0: ceil(N / 128) B
          workgroups of 256 threads at the classes of d and dv; else one wave per query (2) under
          knob 1, or when knob is not 2 and ceil(N / 256) B < 128: ceil(N B / 4) workgroups,
          total_wg = B; else the LDS-tiled SIMT kernel (3) on ceil(N / 256) B workgroups at the
          larger class of d, dv, 32 keys per tile (8 at the 128 class).  Float64 (4): ceil(N B / 4).
backward  W = 1: circ_bwd_w1 alone on min(ceil(N B max(d, dv) / 256), 2^20) workgroups, family 2
          (3 for Float64).  Else a pre-pass, 8 queries per thread when 16-bit, N % 8 == 0 and
          O, dO aligned; then MFMA (1) when 16-bit, N % 8 == 0, Q, K, V, dO aligned, knob 0, on
          ceil(N / 128) B workgroups; else SIMT (2; Float64 3) on ceil(N / 32) B workgroups with
          asz (32 (2 (d + 1) + 2 (dv + 1)) + 32 x 33) B of LDS for dQ and
          asz (32 (2 (d + 1) + 2 (dv + 1)) + 2 x 32 x 33 + 64) for dK / dV.
          Workspace: nD at 0, nlse at al256(N B asz), total 256 + 2 al256(N B asz); asz 4, 8 for Float64.

Unless a row says otherwise: bf16, aligned, knob 0.  Shapes are (N, d, dv, B, W).  No kernel is
launched."""
from __future__ import annotations

import ctypes

import pytest

import fa_hip

F32, BF16, F16, F64 = 0, 1, 2, 3
TILED, WAVE, SIMT, FWD_F64 = 1, 2, 3, 4          # fa::CircFwdKernel
MFMA, BSIMT, BWD_F64 = 1, 2, 3                   # fa::CircBwdFamily
UNSUPPORTED = fa_hip.FA_ERR_UNSUPPORTED

FWD_FIELDS = ("Dc", "DVc", "simt_class", "simt_kt", "nqb", "total_wg", "grid", "block", "status")
BWD_FIELDS = ("w1", "w1_grid", "prepass_vec", "prepass_grid", "Dc", "DVc", "nblk", "total_wg", "grid", "lds_dq",
              "lds_dkdv", "off_nD", "off_nlse", "total", "status")


def fwd(shape, want, dtype=BF16, knob=0, kv=1, **fields):
    return (dtype, *shape, knob, kv), want, fields


def bwd(shape, want, dtype=BF16, knob=0, qkv=1, o=1, do=1, **fields):
    return (dtype, *shape, knob, qkv, o, do), want, fields


BIG = (4096, 64, 64, 8, 129)       # 256 blocks of 128, 128 of 256
RAG128 = (4095, 64, 64, 8, 129)    # ragged: 16 x 8 = 128 blocks of 256
RAG112 = (4095, 64, 64, 7, 129)    # 16 x 7 = 112
I31 = 2 ** 31 - 1

FWD = [
    fwd(BIG, TILED, Dc=64, DVc=64, nqb=32, total_wg=256, grid=256, block=256, simt_class=0, simt_kt=0, status=0),
    fwd(BIG, TILED, dtype=F16, nqb=32, grid=256),
    fwd((256, 32, 32, 1, 9), TILED, Dc=32, DVc=32, nqb=2, total_wg=2, grid=2),   # a small grid does not leave the MFMA kernel
    fwd((4096, 33, 32, 8, 129), TILED, Dc=64, DVc=32),
    fwd((4096, 128, 65, 8, 129), TILED, Dc=128, DVc=128),
    fwd((4088, 64, 64, 8, 129), TILED, nqb=32, grid=256),                          # N % 8 == 0 is enough
    # the wave / SIMT cut-over at 128 blocks of 256 queries
    fwd(RAG128, SIMT, simt_class=64, simt_kt=32, nqb=0, total_wg=128, grid=128, block=256, Dc=0, DVc=0),
    fwd(RAG112, WAVE, total_wg=7, grid=7167, block=256, nqb=0, simt_class=0),       # ceil(4095 x 7 / 4)
    fwd(BIG, SIMT, kv=0, total_wg=128, grid=128),
    fwd((4096, 64, 64, 7, 129), WAVE, kv=0, total_wg=7, grid=7168),
    fwd((4092, 64, 64, 8, 129), SIMT, total_wg=128),                               # N % 8 != 0
    # the knob
    fwd(BIG, WAVE, knob=1, total_wg=8, grid=8192),
    fwd(BIG, SIMT, knob=2, total_wg=128, grid=128),
    fwd(RAG112, SIMT, knob=2, total_wg=112, grid=112),
    fwd(RAG128, WAVE, knob=1, total_wg=8, grid=8190),
    fwd((256, 32, 32, 1, 9), WAVE, knob=1, grid=64),
    fwd((256, 32, 32, 1, 9), SIMT, knob=2, simt_class=32, simt_kt=32, total_wg=1, grid=1),
    # fp32: never tiled
    fwd(BIG, SIMT, dtype=F32, total_wg=128),
    fwd((4096, 64, 64, 7, 129), WAVE, dtype=F32, total_wg=7),
    fwd(BIG, WAVE, dtype=F32, knob=1),
    # Float64, under any knob
    *[fwd((64, 32, 32, 2, 9), FWD_F64, dtype=F64, knob=k, grid=32, block=256, nqb=0, total_wg=0) for k in (0, 1, 2)],
    fwd((4095, 64, 64, 8, 129), FWD_F64, dtype=F64, kv=0, grid=8190),
    # the SIMT classes: the larger class of d and dv on both sides
    fwd((4095, 32, 32, 8, 129), SIMT, simt_class=32, simt_kt=32),
    fwd((4095, 33, 32, 8, 129), SIMT, simt_class=64, simt_kt=32),
    fwd((4095, 32, 33, 8, 129), SIMT, simt_class=64, simt_kt=32),
    fwd((4095, 65, 32, 8, 129), SIMT, simt_class=128, simt_kt=8),
    fwd((4095, 32, 65, 8, 129), SIMT, simt_class=128, simt_kt=8),
    fwd((4095, 128, 128, 8, 129), SIMT, dtype=F16, simt_class=128, simt_kt=8),
    # refusals, and the last shape each check lets through
    fwd((4096, 129, 64, 8, 129), -1, status=UNSUPPORTED),
    fwd((4096, 64, 129, 8, 129), -1, status=UNSUPPORTED),
    fwd((4096, 129, 64, 8, 129), -1, dtype=F64, status=UNSUPPORTED),
    fwd((2 ** 24, 64, 32, 1, 9), -1, status=UNSUPPORTED),                          # Q, K slab of 2^31 B
    fwd((2 ** 24, 32, 64, 1, 9), -1, status=UNSUPPORTED),                          # V slab
    fwd((2 ** 24 - 8, 64, 64, 1, 9), TILED, status=0, nqb=131072),                 # 2^31 - 1024 B
    fwd((2 ** 23, 64, 64, 1, 9), -1, dtype=F32, status=UNSUPPORTED),
    fwd((2 ** 22, 64, 64, 1, 9), -1, dtype=F64, status=UNSUPPORTED),
    fwd((2 ** 23, 64, 64, 1, 9), TILED),
    fwd(BIG[:4] + (I31 // 2 + 1,), -1, status=UNSUPPORTED),
    fwd(BIG[:4] + (I31 // 2,), TILED, status=0),
    fwd((65536, 32, 32, 65536, 9), -1, status=UNSUPPORTED),                        # N B = 2^32
    fwd((65536, 32, 32, 65535, 9), TILED, total_wg=512 * 65535),
]

BIG_PART = 131072                   # 4096 x 8 x 4 B
BIG_TOTAL = 256 + 2 * BIG_PART
LDS64 = (4 * (32 * 4 * 65 + 1056), 4 * (32 * 4 * 65 + 2112 + 64))    # d = dv = 64: 37,504 and 41,984 B

BWD = [
    bwd(BIG, MFMA, w1=0, prepass_vec=1, prepass_grid=16, Dc=64, DVc=64, nblk=32, total_wg=256, grid=256, lds_dq=0,
        lds_dkdv=0, off_nD=0, off_nlse=BIG_PART, total=BIG_TOTAL, status=0),
    bwd(BIG, MFMA, dtype=F16, prepass_vec=1, nblk=32),
    bwd((4096, 33, 32, 8, 129), MFMA, Dc=64, DVc=32),
    bwd((256, 32, 32, 1, 9), MFMA, nblk=2, grid=2, prepass_grid=1, total=256 + 2 * 1024),
    # alignment: the pre-pass asks for O and dO, the MFMA kernels for Q, K, V and dO
    bwd(BIG, BSIMT, qkv=0, prepass_vec=1, prepass_grid=16, nblk=0, total_wg=0, grid=1024, lds_dq=LDS64[0],
        lds_dkdv=LDS64[1], Dc=0, DVc=0),
    bwd(BIG, MFMA, o=0, prepass_vec=0, prepass_grid=128, grid=256),
    bwd(BIG, BSIMT, do=0, prepass_vec=0, prepass_grid=128, grid=1024),
    bwd(RAG128, BSIMT, prepass_vec=0, prepass_grid=128, grid=128 * 8, off_nlse=131072, total=256 + 2 * 131072),
    bwd((4092, 64, 64, 8, 129), BSIMT, prepass_vec=0),
    # the knob: either value leaves the MFMA kernels, not the 16-B pre-pass
    bwd(BIG, BSIMT, knob=1, prepass_vec=1, grid=1024),
    bwd(BIG, BSIMT, knob=2, prepass_vec=1, grid=1024),
    bwd(BIG, BSIMT, dtype=F32, prepass_vec=0, prepass_grid=128, grid=1024, lds_dq=LDS64[0], total=BIG_TOTAL),
    bwd(BIG, BWD_F64, dtype=F64, prepass_vec=0, prepass_grid=128, grid=1024, lds_dq=2 * LDS64[0], lds_dkdv=2 * LDS64[1],
        off_nlse=2 * BIG_PART, total=256 + 4 * BIG_PART),
    bwd(BIG, BWD_F64, dtype=F64, knob=2),
    # W = 1: one kernel, no pre-pass
    bwd(BIG[:4] + (1,), BSIMT, w1=1, w1_grid=8192, prepass_vec=0, prepass_grid=0, grid=0, nblk=0, lds_dq=0,
        total=BIG_TOTAL),
    bwd(BIG[:4] + (1,), BSIMT, dtype=F32, w1=1, w1_grid=8192),
    bwd(BIG[:4] + (1,), BWD_F64, dtype=F64, w1=1, w1_grid=8192, total=256 + 4 * BIG_PART),
    bwd((4096, 32, 64, 8, 1), BSIMT, w1=1, w1_grid=8192),                          # the larger of d and dv
    bwd((4095, 64, 64, 8, 1), BSIMT, w1=1, qkv=0, w1_grid=8190),
    bwd((65536, 128, 128, 256, 1), BSIMT, w1=1, w1_grid=2 ** 20),                  # 2^23 blocks: capped
    bwd(BIG[:4] + (2,), MFMA, w1=0),
    # the SIMT kernels' LDS at d = dv = 128: above 64 KiB
    bwd((4095, 128, 128, 8, 129), BSIMT, lds_dq=70272, lds_dkdv=74752),
    bwd((4096, 128, 128, 8, 129), BWD_F64, dtype=F64, lds_dq=140544, lds_dkdv=149504),
    bwd((4095, 32, 48, 8, 129), BSIMT, lds_dq=4 * (32 * (66 + 98) + 1056), lds_dkdv=4 * (32 * (66 + 98) + 2112 + 64)),
    # a ragged element count: 1000 x 3 x 4 = 12,000 B -> 12,032
    bwd((1000, 32, 32, 3, 9), MFMA, prepass_vec=1, prepass_grid=2, nblk=8, grid=24, off_nlse=12032, total=256 + 2 * 12032),
    bwd((1000, 32, 32, 3, 9), BWD_F64, dtype=F64, off_nlse=24064, total=256 + 2 * 24064),
    # refusals: the workspace layout is the shape's all the same
    bwd((4096, 129, 64, 8, 129), -1, status=UNSUPPORTED, total=BIG_TOTAL),
    bwd((4096, 64, 129, 8, 129), -1, status=UNSUPPORTED),
    bwd((4096, 64, 129, 8, 1), -1, status=UNSUPPORTED, w1=0),
    bwd((2 ** 24, 64, 32, 1, 9), -1, status=UNSUPPORTED),
    bwd((2 ** 24 - 8, 64, 64, 1, 9), MFMA, status=0),
    bwd(BIG[:4] + (I31 // 2 + 1,), -1, status=UNSUPPORTED),
    bwd(BIG[:4] + (I31 // 2,), MFMA),
    bwd((65536, 32, 32, 65536, 9), -1, status=UNSUPPORTED),
    bwd((65536, 32, 32, 65535, 9), MFMA),
]


@pytest.fixture(scope="module")
def L():
    lib = fa_hip.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    lib.fa_debug_circ_fwd_plan.restype = ci
    lib.fa_debug_circ_fwd_plan.argtypes = [ci] + [i64] * 5 + [ci] * 2 + [ctypes.POINTER(i64)]
    lib.fa_debug_circ_bwd_plan.restype = ci
    lib.fa_debug_circ_bwd_plan.argtypes = [ci] + [i64] * 5 + [ci] * 4 + [ctypes.POINTER(i64)]
    lib.fa_debug_set_circ_generic.restype = ci
    lib.fa_debug_set_circ_generic.argtypes = [ci]
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


def test_tables_name_every_kernel_dtype_and_knob_value():
    assert {w for _, w, _ in FWD} == {TILED, WAVE, SIMT, FWD_F64, -1}
    assert {w for _, w, _ in BWD} == {MFMA, BSIMT, BWD_F64, -1}
    for table in (FWD, BWD):
        assert {a[0] for a, _, _ in table} == {F32, BF16, F16, F64} and {a[6] for a, _, _ in table} == {0, 1, 2}
    assert {(f["simt_class"], f["simt_kt"]) for _, w, f in FWD if w == SIMT and "simt_kt" in f} == {(32, 32), (64, 32), (128, 8)}


def test_forward_plan(L):
    _check(L.fa_debug_circ_fwd_plan, FWD_FIELDS, FWD)


def test_backward_plan(L):
    _check(L.fa_debug_circ_bwd_plan, BWD_FIELDS, BWD)


def test_plans_do_not_read_the_thread_knob(L):
    for knob in (1, 2):
        old = L.fa_debug_set_circ_generic(knob)
        try:
            _check(L.fa_debug_circ_fwd_plan, FWD_FIELDS, FWD)
            _check(L.fa_debug_circ_bwd_plan, BWD_FIELDS, BWD)
        finally:
            L.fa_debug_set_circ_generic(old)


def test_plan_entries_reject_bad_arguments(L):
    f, b = L.fa_debug_circ_fwd_plan, L.fa_debug_circ_bwd_plan
    assert f(9, *BIG, 0, 1, None) == -1 and b(9, *BIG, 0, 1, 1, 1, None) == -1
    for i in range(5):                                   # N, d, dv, B, W below 1
        shape = list(BIG)
        shape[i] = 0
        assert f(BF16, *shape, 0, 1, None) == -1 and b(BF16, *shape, 0, 1, 1, 1, None) == -1
    assert f(BF16, *BIG, 0, 1, None) == TILED and b(BF16, *BIG, 0, 1, 1, 1, None) == MFMA   # (out may be null)


def test_workspace_query_returns_the_plans_total(L):
    """For every shape of the table, refused ones included, whatever the knob and the alignment."""
    for args, _, fields in BWD:
        _, out = _plan(L.fa_debug_circ_bwd_plan, BWD_FIELDS, args)
        N, d, dv, B = args[1:5]
        asz = 8 if args[0] == F64 else 4
        assert out["total"] == L.fa_circulant_bwd_workspace(*args[:6]) == 256 + 2 * ((N * B * asz + 255) // 256 * 256), args
        assert out["off_nD"] == 0 and out["total"] == 256 + 2 * out["off_nlse"]


def test_refusals_are_the_entry_points(L):
    """A shape the plans refuse is a shape fa_circulant_fwd / fa_circulant_bwd answer with
    FA_ERR_UNSUPPORTED and the plan's reason, before any launch; a backward shape the plan
    accepts gets as far as the workspace check.  (An accepted forward would launch.)"""
    P = ctypes.c_void_p(16)   # never dereferenced
    for args, want, _ in BWD:
        rc = L.fa_circulant_bwd(args[0], *[P] * 10, *args[1:6], 0.0, None, 0, None)
        assert rc == (UNSUPPORTED if want == -1 else fa_hip.FA_ERR_WORKSPACE), args
        if want == -1:
            assert (b"head dimension" if max(args[2:4]) > 128 else b"32-bit") in L.fa_last_error()
    for args, want, _ in FWD:
        same_bwd, _ = _plan(L.fa_debug_circ_bwd_plan, BWD_FIELDS, (*args[:7], 1, 1, 1))
        assert (want == -1) == (same_bwd == -1), args        # one refusal rule for both directions
        if want == -1:
            rc = L.fa_circulant_fwd(args[0], *[P] * 6, *args[1:6], 0.0, None)
            assert rc == UNSUPPORTED, args
            assert (b"head dimension" if max(args[2:4]) > 128 else b"32-bit") in L.fa_last_error()
