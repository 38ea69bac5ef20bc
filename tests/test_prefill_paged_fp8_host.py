"""CPU tests of chunked prefill over a paged fp8 cache: the C ABI's checks before any launch
(fa_prefill_paged_fp8_fwd and its workspace query), the plan hook, and the Python mirror's shape
checks.  No device is touched."""
from __future__ import annotations

import ctypes

import pytest
import torch

import fa_hip
from fa_hip import DimensionMismatch

F32, BF16, F16, F64 = 0, 1, 2, 3
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
P = ctypes.c_void_p(256)   # a non-null, 16-B aligned pointer that no refused call dereferences
ODD = ctypes.c_void_p(264)
TILE, CHUNK = 8, 9


def call(dtype=BF16, Q=P, K=P, V=P, ks=None, vs=None, table=P, N=512, d=128, dv=128, batch=1, group=8, page_size=64,
         num_pages=1024, max_pages=64, ws=None, ws_bytes=0):
    L = fa_hip.lib()
    rc = L.fa_prefill_paged_fp8_fwd(dtype, Q, K, V, ks, vs, table, P, P, P, N, d, dv, batch, group, page_size, num_pages,
                                    max_pages, None, None, -1, 0, 0.0, ws, ws_bytes, None)
    return rc, L.fa_last_error().decode()


def plan(N, d, dv, batch, group, page_size, max_pages, force=0, dtype=BF16):
    out = (ctypes.c_int64 * 5)()
    k = fa_hip.lib().fa_debug_prefill_paged_fp8_plan(dtype, N, d, dv, batch, group, page_size, max_pages, force, out)
    assert k == out[0]
    return dict(kernel=out[0], nsplit=out[1], grid=out[2], total=out[3], blocks=out[4])


@pytest.mark.parametrize("kw,status,words", [
    (dict(Q=None), INVALID, "null pointer"),
    (dict(V=None), INVALID, "null pointer"),
    (dict(table=None), INVALID, "null pointer"),
    (dict(group=0), INVALID, "DimensionMismatch"),
    (dict(page_size=0), INVALID, "DimensionMismatch"),
    (dict(num_pages=0), INVALID, "DimensionMismatch"),
    (dict(max_pages=0), INVALID, "DimensionMismatch"),
    (dict(table=None, page_size=0), INVALID, "null pointer"),       # documented order: pointers, then dimensions
    (dict(page_size=0, d=129), INVALID, "DimensionMismatch"),       # dimensions before anything unsupported
    (dict(d=129), UNSUPPORTED, "head dimension exceeds the compiled maximum (128)"),
    (dict(N=17, group=1, page_size=16, max_pages=1), UNSUPPORTED, "max_pages * page_size >= N"),
    (dict(dtype=F32), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(dtype=F64), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(page_size=8), UNSUPPORTED, "page_size % 16 == 0"),
    (dict(page_size=24), UNSUPPORTED, "page_size % 16 == 0"),
    (dict(page_size=40), UNSUPPORTED, "page_size % 16 == 0"),
    (dict(K=ODD), UNSUPPORTED, "16-B aligned"),
    (dict(V=ODD), UNSUPPORTED, "16-B aligned"),
    (dict(d=129, dtype=F32, page_size=24), UNSUPPORTED, "head dimension"),         # head dims, dtype, page size, alignment
    (dict(dtype=F32, page_size=24, K=ODD), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(page_size=24, K=ODD), UNSUPPORTED, "page_size % 16 == 0"),
    (dict(page_size=1 << 24, max_pages=1), UNSUPPORTED, "32-bit addressing"),      # one page of 2^31 bytes
    (dict(page_size=1 << 10, max_pages=1 << 21), UNSUPPORTED, "32-bit addressing"),  # cap = 2^31
    (dict(N=1 << 20, group=8, page_size=1 << 10, max_pages=1 << 10), UNSUPPORTED, "32-bit addressing"),  # a slab's rows * d = 2^30
    (dict(page_size=24, max_pages=1 << 40), UNSUPPORTED, "page_size % 16 == 0"),   # unsupported before the extents
    (dict(), WORKSPACE, "fa_prefill_paged_fp8_fwd_workspace()"),                   # the scales may be NULL
    (dict(ks=P, vs=P, ws=P, ws_bytes=1024), WORKSPACE, "fa_prefill_paged_fp8_fwd_workspace()"),
])
def test_refusals_before_any_launch(kw, status, words):
    rc, msg = call(**kw)
    assert rc == status and words in msg and msg.startswith("fa_prefill_paged_fp8_fwd: ")


@pytest.mark.parametrize("N,batch", [(0, 2), (1, 0)])
def test_no_op_inputs_dereference_nothing(N, batch):
    rc = fa_hip.lib().fa_prefill_paged_fp8_fwd(BF16, None, None, None, None, None, None, None, None, None, N, 64, 64, batch,
                                               2, 64, 16, 4, None, None, -1, 0, 0.0, None, 0, None)
    assert rc == OK


@pytest.mark.parametrize("page_size,kernel", [(16, CHUNK), (48, CHUNK), (80, CHUNK), (64, TILE), (128, TILE), (192, TILE),
                                              (8, -1), (24, -1), (40, -1), (0, -1)])
def test_kernel_choice_by_page_size_alone(page_size, kernel):
    for N, G, B in ((1, 1, 1), (8, 8, 8), (2048, 8, 1)):
        assert plan(N, 128, 128, B, G, page_size, 4096)["kernel"] == kernel


@pytest.mark.parametrize("N,d,dv,B,G,ps,mp,force", [
    (40, 64, 64, 3, 4, 64, 8, 0), (2, 64, 64, 2, 8, 64, 3, 0), (512, 128, 128, 1, 8, 64, 136, 0), (2048, 128, 128, 8, 8, 16, 2176, 0),
    (8, 128, 128, 1, 8, 16, 513, 0), (33, 64, 64, 2, 1, 16, 13, 3), (130, 32, 128, 2, 1, 256, 1, 2), (1, 16, 8, 1, 1, 16, 1, 7)])
def test_plan_grid_and_workspace(N, d, dv, B, G, ps, mp, force):
    """The 16-bit prefill plan's numbers under the fp8 kernels' names; the workspace query is the plan's."""
    L = fa_hip.lib()
    pl = plan(N, d, dv, B, G, ps, mp, force)
    blocks = -(-N * G // 128)
    tiles = -(-ps * mp // 64)
    out = (ctypes.c_int64 * 5)()
    L.fa_debug_prefill_paged_plan(BF16, N, d, dv, B, G, ps, mp, force, out)
    assert pl["kernel"] == out[0] + 2 and [pl[k] for k in ("nsplit", "grid", "total", "blocks")] == list(out[1:])
    assert pl["blocks"] == blocks and pl["grid"] == B * blocks * pl["nsplit"]
    assert 1 <= pl["nsplit"] <= tiles and (force == 0 or pl["nsplit"] == min(force, tiles))
    assert pl["total"] == (0 if pl["nsplit"] == 1 else pl["nsplit"] * B * G * N * (dv + 2) * 4 + 256)
    old = L.fa_debug_set_decode_nsplit(force)
    try:
        assert L.fa_prefill_paged_fp8_fwd_workspace(BF16, N, d, dv, B, G, ps, mp) == pl["total"]
    finally:
        L.fa_debug_set_decode_nsplit(old)


def test_small_grids_split_and_refused_shapes_need_nothing():
    L = fa_hip.lib()
    assert plan(8, 128, 128, 1, 8, 64, 129)["nsplit"] > 1 and plan(2048, 128, 128, 8, 8, 64, 160)["nsplit"] == 1
    assert L.fa_prefill_paged_fp8_fwd_workspace(F32, 512, 128, 128, 1, 8, 64, 64) == 0
    assert L.fa_prefill_paged_fp8_fwd_workspace(BF16, 512, 128, 128, 1, 8, 24, 64) == 0
    assert plan(512, 128, 128, 1, 8, 64, 4)["kernel"] == -1                         # cap < N


def test_python_mirror():
    for name in ("paged_prefill_fp8_fa", "paged_prefill_fp8_fa_"):
        assert name in fa_hip.__all__
    q = torch.zeros(40, 64, 8, dtype=torch.bfloat16)
    kp, vp = torch.zeros(16, 64, 5, dtype=torch.uint8), torch.zeros(16, 64, 5, dtype=torch.float8_e4m3fn)
    table = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(TypeError):
        fa_hip.paged_prefill_fp8_fa(q, kp.to(torch.bfloat16), vp, table, group=4)      # a 16-bit pool
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_prefill_fp8_fa(q, kp, vp, table, group=3)                         # 8 query slabs, group 3
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_prefill_fp8_fa(q, kp, vp, table, group=2)                         # 4 KV slabs, a table for 2
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_prefill_fp8_fa(q, kp, vp[:8], table, group=4)                     # pools disagree in page_size
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_prefill_fp8_fa(q, kp, vp, table.long(), group=4)
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_prefill_fp8_fa(q, kp, vp, table, [0.5, 0.7, 0.9], torch.ones(1), group=4)  # 2 KV slabs, 3 and 1 scales
