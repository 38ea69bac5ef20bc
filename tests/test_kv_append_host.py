"""CPU tests of the cache writers: the C ABI's checks before any launch (fa_kv_append_paged,
fa_kv_append_paged_fp8, fa_kv_quantize_fp8 and its workspace query), the plan hook, and the Python
mirror's shape checks.  No device is touched."""
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
BIG = dict(page_size=1 << 20, max_pages=1 << 20)   # unsupported comes before the extents


def append(fp8, dtype=BF16, Kn=P, Vn=P, K=P, V=P, table=P, N=40, d=128, dv=128, batch=2, page_size=64, num_pages=64,
           max_pages=4):
    L = fa_hip.lib()
    tail = (table, N, d, dv, batch, page_size, num_pages, max_pages, None, None, None)
    rc = L.fa_kv_append_paged_fp8(dtype, Kn, Vn, K, V, None, None, *tail) if fp8 else L.fa_kv_append_paged(dtype, Kn, Vn, K, V, *tail)
    return rc, L.fa_last_error().decode()


def quantize(dtype=BF16, K=P, s=P, Nk=64, d=64, dv=64, batch=2, ws=None, ws_bytes=0):
    L = fa_hip.lib()
    return L.fa_kv_quantize_fp8(dtype, K, P, P, P, s, P, Nk, d, dv, batch, ws, ws_bytes, None), L.fa_last_error().decode()


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kw,status,words", [
    (dict(Kn=None), INVALID, "null pointer"),
    (dict(V=None), INVALID, "null pointer"),
    (dict(table=None, page_size=0), INVALID, "null pointer"),       # documented order: pointers, then dimensions
    (dict(N=-1), INVALID, "DimensionMismatch"),
    (dict(num_pages=0), INVALID, "DimensionMismatch"),
    (dict(max_pages=0, d=129), INVALID, "DimensionMismatch"),       # dimensions before anything unsupported
    (dict(d=129, N=999, dtype=F32), UNSUPPORTED, "head dimension exceeds the compiled maximum (128)"),
    (dict(N=257, dtype=F32), UNSUPPORTED, "max_pages * page_size >= N"),
    (dict(dtype=F32, page_size=20, K=ODD), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(dtype=F64), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(page_size=20, K=ODD), UNSUPPORTED, "page_size % "),
    (dict(V=ODD, **BIG), UNSUPPORTED, "16-B aligned"),
    (dict(page_size=1 << 24, max_pages=1), UNSUPPORTED, "32-bit addressing"),      # one 16-bit page of 2^32 bytes
    (dict(page_size=1 << 10, max_pages=1 << 21), UNSUPPORTED, "32-bit addressing"),  # cap = 2^31
    (dict(N=1 << 23, page_size=1 << 10, max_pages=1 << 20), UNSUPPORTED, "32-bit addressing"),  # a source slab of 2^31 bytes
])
def test_append_refusals_before_any_launch(fp8, kw, status, words):
    fn = "fa_kv_append_paged_fp8" if fp8 else "fa_kv_append_paged"
    rc, msg = append(fp8, **kw)
    assert rc == status and words in msg and msg.startswith(fn + ": ")


def test_page_size_8_is_a_16_bit_page_size_only():
    """Past every check the call would launch, so the accepted side is shown by the next refusal."""
    for ps in (8, 24, 40):
        assert "16-B aligned" in append(False, N=8, page_size=ps, K=ODD)[1]
        assert "page_size % 16 == 0" in append(True, N=8, page_size=ps, K=ODD)[1]
    assert "16-B aligned" in append(True, N=8, page_size=48, K=ODD)[1]


@pytest.mark.parametrize("kw,status,words", [
    (dict(K=None), INVALID, "null pointer"),
    (dict(s=None, d=0), INVALID, "null pointer"),
    (dict(d=0, dtype=F32), INVALID, "DimensionMismatch"),
    (dict(Nk=-1), INVALID, "DimensionMismatch"),
    (dict(dtype=F32), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(Nk=1 << 24, d=64), UNSUPPORTED, "32-bit addressing"),     # a slab of 2^31 bytes
    (dict(), WORKSPACE, "fa_kv_quantize_fp8_workspace()"),
    (dict(ws=P, ws_bytes=8), WORKSPACE, "fa_kv_quantize_fp8_workspace()"),
])
def test_quantize_refusals_before_any_launch(kw, status, words):
    rc, msg = quantize(**kw)
    assert rc == status and words in msg and msg.startswith("fa_kv_quantize_fp8: ")


@pytest.mark.parametrize("N,batch", [(0, 2), (1, 0)])
def test_no_op_inputs_dereference_nothing(N, batch):
    L = fa_hip.lib()
    tail = (None, N, 64, 64, batch, 64, 16, 4, None, None, None)
    assert L.fa_kv_append_paged(BF16, None, None, None, None, *tail) == OK
    assert L.fa_kv_append_paged_fp8(F16, None, None, None, None, None, None, *tail) == OK
    assert L.fa_kv_quantize_fp8(BF16, None, None, None, None, None, None, N, 64, 64, batch, None, 0, None) == OK


def test_quantize_workspace_is_monotone_and_zero_where_refused():
    ws = fa_hip.lib().fa_kv_quantize_fp8_workspace
    small, large = ws(BF16, 64, 64, 64, 2), ws(BF16, 4096, 128, 128, 2)
    assert 256 < small <= large and large == 2 * 2 * 32 * 4 + 256        # 4096 * 128 elements in spans of 16384
    assert ws(BF16, 4096, 128, 128, 8) == 2 * 8 * 32 * 4 + 256 and ws(BF16, 4096, 64, 128, 2) == large
    assert ws(BF16, 1 << 22, 128, 128, 1) == 2 * 256 * 4 + 256           # at most 256 spans per slab
    assert ws(F32, 64, 64, 64, 2) == 0 and ws(BF16, 0, 64, 64, 2) == 0 and ws(BF16, 1 << 24, 64, 64, 1) == 0


@pytest.mark.parametrize("fp8", [0, 1])
def test_plan_splits_by_destination(fp8):
    def plan(N, d, dv, B, ps, mp):
        out = (ctypes.c_int64 * 6)()
        fa_hip.lib().fa_debug_kv_append_plan(fp8, N, d, dv, B, ps, mp, out)
        return dict(zip(("decode", "pages", "nseg", "feats", "nfsplit", "grid"), out))
    assert plan(1, 128, 128, 1024, 16, 64) == dict(decode=1, pages=0, nseg=0, feats=0, nfsplit=0, grid=1024)   # never a workgroup per feature
    assert plan(1, 32, 32, 1024, 64, 64)["grid"] == 256                                  # four slabs per workgroup
    chunk = 16 if fp8 else 8
    for N, ps, mp in ((2, 16, 8), (37, 16, 8), (2048, 64, 64), (2048, 4096, 2), (100, 16, 3)):
        pl = plan(N, 128, 72, 8, ps, mp)
        assert pl["decode"] == 0 and pl["pages"] == min(mp, (N - 2) // ps + 2)            # the most pages N rows touch
        assert pl["nseg"] == -(-ps // 1024) and pl["feats"] * (min(ps, 1024) // chunk) <= 512
        assert pl["nfsplit"] == -(-200 // pl["feats"]) and pl["grid"] == 8 * pl["pages"] * pl["nseg"] * pl["nfsplit"]


def test_python_mirror():
    for name in ("paged_kv_append_", "paged_kv_append_fp8_", "quantize_kv_fp8_hip"):
        assert name in fa_hip.__all__
    kn, vn = torch.zeros(5, 64, 2, dtype=torch.bfloat16), torch.zeros(5, 32, 2, dtype=torch.bfloat16)
    kp, vp = torch.zeros(16, 64, 5, dtype=torch.bfloat16), torch.zeros(16, 32, 5, dtype=torch.bfloat16)
    k8, v8 = kp.to(torch.uint8), vp.to(torch.float8_e4m3fn)
    table = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(TypeError):
        fa_hip.paged_kv_append_fp8_(kp, v8, table, kn, vn)                      # a 16-bit pool
    for f, a, b in ((fa_hip.paged_kv_append_, kp, vp), (fa_hip.paged_kv_append_fp8_, k8, v8)):
        with pytest.raises(DimensionMismatch):
            f(a, b, table, kn, vn[:4])                                          # K_new and V_new disagree in N
        with pytest.raises(DimensionMismatch):
            f(a, b[:8], table, kn, vn)                                          # pools disagree in page_size
        with pytest.raises(DimensionMismatch):
            f(a, b, table[:, :1], kn, vn)                                       # a table for one slab
        with pytest.raises(DimensionMismatch):
            f(a, b, table.long(), kn, vn)
        with pytest.raises(TypeError, match="no CPU fallback"):
            f(a, b, table, kn, vn)
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_kv_append_(kp, vp, table, kn.half(), vn.half())            # mixed element types
    with pytest.raises(DimensionMismatch):
        fa_hip.paged_kv_append_fp8_(k8, v8, table, kn, vn, [0.5, 0.7, 0.9])     # 2 slabs, 3 scales
    with pytest.raises(DimensionMismatch):
        fa_hip.quantize_kv_fp8_hip(kn, vn[:4])
    with pytest.raises(TypeError, match="no CPU fallback"):
        fa_hip.quantize_kv_fp8_hip(kn, vn)
