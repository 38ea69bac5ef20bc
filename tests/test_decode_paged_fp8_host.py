"""CPU tests of decode attention over a paged fp8 cache: the C ABI's checks before any launch
(fa_decode_paged_fp8_fwd and its workspace query), the plan hook, and the Python mirror's type and
shape checks.  No device is touched."""
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
TILE, CHUNK, NONE = 4, 5, -1


def call(dtype=BF16, Q=P, K=P, V=P, ks=P, vs=P, table=P, N=1, d=128, dv=128, batch=8, group=8, page_size=64,
         num_pages=1024, max_pages=64, ws=None, ws_bytes=0):
    L = fa_hip.lib()
    rc = L.fa_decode_paged_fp8_fwd(dtype, Q, K, V, ks, vs, table, P, P, P, N, d, dv, batch, group, page_size, num_pages,
                                   max_pages, None, None, -1, 0, 0.0, ws, ws_bytes, None)
    return rc, L.fa_last_error().decode()


def plan(N, d, dv, batch, group, page_size, max_pages, force=0, dtype=BF16):
    out = (ctypes.c_int64 * 4)()
    k = fa_hip.lib().fa_debug_decode_paged_fp8_plan(dtype, N, d, dv, batch, group, page_size, max_pages, force, out)
    assert k == out[0]
    return dict(kernel=out[0], nsplit=out[1], grid=out[2], total=out[3])


@pytest.mark.parametrize("kw,status,words", [
    (dict(Q=None), INVALID, "null pointer"),
    (dict(table=None), INVALID, "null pointer"),
    (dict(group=0), INVALID, "DimensionMismatch"),
    (dict(page_size=0), INVALID, "DimensionMismatch"),
    (dict(num_pages=0), INVALID, "DimensionMismatch"),
    (dict(max_pages=0), INVALID, "DimensionMismatch"),
    (dict(table=None, page_size=0), INVALID, "null pointer"),       # documented order: pointers, then dimensions
    (dict(page_size=0, d=129), INVALID, "DimensionMismatch"),       # dimensions before anything unsupported
    (dict(d=129), UNSUPPORTED, "head dimension exceeds the compiled maximum (128)"),
    (dict(N=17, group=1, page_size=16, max_pages=1), UNSUPPORTED, "max_pages * page_size >= N"),
    (dict(N=3, group=11), UNSUPPORTED, "fa_varlen_fwd"),
    (dict(dtype=F32), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(page_size=8), UNSUPPORTED, "page_size % 16 == 0"),
    (dict(page_size=24), UNSUPPORTED, "page_size % 16 == 0"),
    (dict(K=ODD), UNSUPPORTED, "16-B aligned"),
    (dict(V=ODD), UNSUPPORTED, "16-B aligned"),
    (dict(d=129, N=3, group=11, page_size=24), UNSUPPORTED, "head dimension"),     # head dims before rows
    (dict(N=3, group=11, dtype=F32, page_size=24), UNSUPPORTED, "fa_varlen_fwd"),  # rows, dtype, page size, alignment
    (dict(dtype=F32, page_size=24, K=ODD), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(page_size=24, K=ODD), UNSUPPORTED, "page_size % 16 == 0"),
    (dict(page_size=1 << 24, max_pages=1), UNSUPPORTED, "32-bit addressing"),      # one page of 2^31 bytes
    (dict(page_size=1 << 23, max_pages=1), WORKSPACE, "workspace"),                # half of that: a 16-bit page's limit, not ours
    (dict(page_size=1 << 10, max_pages=1 << 21), UNSUPPORTED, "32-bit addressing"),  # cap = 2^31
    (dict(page_size=24, max_pages=1 << 40), UNSUPPORTED, "page_size % 16 == 0"),   # unsupported before the extents
    (dict(), WORKSPACE, "fa_decode_paged_fp8_fwd_workspace()"),
    (dict(ks=None, vs=None), WORKSPACE, "fa_decode_paged_fp8_fwd_workspace()"),    # NULL scales are accepted
    (dict(ws=P, ws_bytes=1024), WORKSPACE, "fa_decode_paged_fp8_fwd_workspace()"),
])
def test_refusals_before_any_launch(kw, status, words):
    rc, msg = call(**kw)
    assert rc == status and words in msg and msg.startswith("fa_decode_paged_fp8_fwd: ")


@pytest.mark.parametrize("N,batch", [(0, 2), (1, 0)])
def test_no_op_inputs_dereference_nothing(N, batch):
    rc = fa_hip.lib().fa_decode_paged_fp8_fwd(BF16, None, None, None, None, None, None, None, None, None, N, 64, 64, batch, 2,
                                              64, 16, 4, None, None, -1, 0, 0.0, None, 0, None)
    assert rc == OK


@pytest.mark.parametrize("page_size,kernel", [(16, CHUNK), (32, CHUNK), (48, CHUNK), (64, TILE), (128, TILE), (192, TILE),
                                              (8, NONE), (24, NONE), (0, NONE)])
def test_kernel_choice_by_page_size(page_size, kernel):
    assert plan(1, 128, 128, 8, 8, page_size, 64)["kernel"] == kernel


def test_plan_and_workspace_are_decode_plans_at_the_logical_capacity():
    L = fa_hip.lib()
    out = (ctypes.c_int64 * 4)()
    for (N, d, dv, B, G, ps, mp) in ((1, 128, 128, 8, 8, 64, 512), (4, 64, 64, 128, 8, 16, 512), (2, 48, 40, 2, 5, 48, 7),
                                      (1, 64, 64, 8, 1, 192, 1)):
        pl = plan(N, d, dv, B, G, ps, mp)
        L.fa_debug_decode_plan(BF16, N, ps * mp, d, dv, B, G, 0, 1, out)
        assert (pl["nsplit"], pl["grid"], pl["total"]) == (out[1], out[2], out[3])
        assert L.fa_decode_paged_fp8_fwd_workspace(BF16, N, d, dv, B, G, ps, mp) == L.fa_decode_fwd_workspace(BF16, N, ps * mp, d, dv, B, G)
    assert plan(1, 128, 128, 8, 8, 64, 512)["total"] > 0                               # a split shape: the partials only
    assert plan(1, 64, 64, 6, 1, 16, 12, force=7)["nsplit"] == 3                       # cap = 192: 3 key tiles
    assert L.fa_decode_paged_fp8_fwd_workspace(F32, 1, 128, 128, 8, 8, 64, 512) == 0   # refused shapes need nothing
    assert L.fa_decode_paged_fp8_fwd_workspace(BF16, 1, 128, 128, 8, 8, 24, 512) == 0


def test_python_mirror():
    for name in ("paged_decode_fp8_fa", "paged_decode_fp8_fa_"):
        assert name in fa_hip.__all__
    q = torch.zeros(1, 64, 8, dtype=torch.bfloat16)
    kp, vp = torch.zeros(16, 64, 5, dtype=torch.uint8), torch.zeros(16, 64, 5, dtype=torch.float8_e4m3fn)
    table = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(TypeError):
        fa_hip.paged_decode_fp8_fa(q, kp.to(torch.bfloat16), vp, table, group=4)       # a 16-bit pool
    with pytest.raises(TypeError):
        fa_hip.paged_decode_fp8_fa(q, kp, vp.view(torch.int8), table, group=4)
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_decode_fp8_fa(q, kp, vp, table, group=3)                          # 8 query slabs, group 3
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_decode_fp8_fa(q, kp, vp, table, group=2)                          # 4 KV slabs, a table for 2
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_decode_fp8_fa(q, kp, vp[:8], table, group=4)                      # pools disagree in page_size
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_decode_fp8_fa(q, kp, vp, table.long(), group=4)
    # the gather indexes fp8 and uint8 pools as bytes: logical key j * page_size + t of slab b is row t of page table[j, b]
    by = torch.arange(3 * 2 * 5, dtype=torch.uint8).reshape(5, 2, 3).permute(2, 1, 0)   # (page_size 3, d 2, 5 pages)
    tb = torch.tensor([[4, 0], [1, 9]], dtype=torch.int32)                             # 9 clamps to page 4
    K, V = fa_hip.paged_kv_gather(by, by.view(torch.float8_e4m3fn), tb)
    assert K.dtype == torch.uint8 and V.dtype == torch.float8_e4m3fn and torch.equal(K, V.view(torch.uint8))
    assert torch.equal(K[:3, :, 0], by[:, :, 4]) and torch.equal(K[3:, :, 0], by[:, :, 1])
    assert torch.equal(K[:3, :, 1], by[:, :, 0]) and torch.equal(K[3:, :, 1], by[:, :, 4])
