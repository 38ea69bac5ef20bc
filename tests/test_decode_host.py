"""CPU tests of decode attention: the C ABI's checks before any launch (fa_decode_fwd and its
workspace query), the plan hook, and the Python mirror's shape check.  No device is touched."""
from __future__ import annotations

import ctypes

import pytest
import torch

import fa_hip
from fa_hip import DimensionMismatch

F32, BF16, F16, F64 = 0, 1, 2, 3
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
P = ctypes.c_void_p(256)   # a non-null pointer that no refused call dereferences


def call(dtype=BF16, Q=P, N=1, Nk=4096, d=128, dv=128, batch=8, group=8, ws=None, ws_bytes=0):
    L = fa_hip.lib()
    rc = L.fa_decode_fwd(dtype, Q, P, P, P, P, P, N, Nk, d, dv, batch, group, None, None, -1, 0, 0.0, ws, ws_bytes, None)
    return rc, L.fa_last_error().decode()


def plan(N, Nk, d, dv, batch, group, force=0, aligned=1, dtype=BF16):
    out = (ctypes.c_int64 * 4)()
    k = fa_hip.lib().fa_debug_decode_plan(dtype, N, Nk, d, dv, batch, group, force, aligned, out)
    assert k == out[0]
    return dict(kernel=out[0], nsplit=out[1], grid=out[2], total=out[3])


def test_status_constants_are_the_headers():
    assert (fa_hip.FA_OK, fa_hip.FA_ERR_INVALID_ARG, fa_hip.FA_ERR_UNSUPPORTED, fa_hip.FA_ERR_WORKSPACE) == (
        OK, INVALID, UNSUPPORTED, WORKSPACE)


@pytest.mark.parametrize("kw,status,words", [
    (dict(Q=None), INVALID, "null pointer"),
    (dict(group=0), INVALID, "DimensionMismatch"),
    (dict(Q=None, group=0), INVALID, "null pointer"),           # documented order: pointers, then dimensions
    (dict(d=129), UNSUPPORTED, "head dimension exceeds the compiled maximum (128)"),
    (dict(N=4, Nk=3), UNSUPPORTED, "needs Nk >= N"),
    (dict(N=3, group=11), UNSUPPORTED, "fa_varlen_fwd"),
    (dict(dtype=F32), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(dtype=F64), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(d=129, N=3, group=11), UNSUPPORTED, "head dimension"),  # documented order: head dims before rows
    (dict(Nk=1 << 24), UNSUPPORTED, "32-bit addressing"),
    (dict(), WORKSPACE, "fa_decode_fwd_workspace()"),
    (dict(ws=P, ws_bytes=1024), WORKSPACE, "fa_decode_fwd_workspace()"),
])
def test_refusals_before_any_launch(kw, status, words):
    rc, msg = call(**kw)
    assert rc == status and words in msg and msg.startswith("fa_decode_fwd: ")


@pytest.mark.parametrize("kw", [dict(N=0), dict(batch=0)])
def test_no_op_inputs_dereference_nothing(kw):
    L = fa_hip.lib()
    args = dict(N=1, Nk=64, d=64, dv=64, batch=2, group=2)
    args.update(kw)
    rc = L.fa_decode_fwd(BF16, None, None, None, None, None, None, args["N"], args["Nk"], args["d"], args["dv"],
                         args["batch"], args["group"], None, None, -1, 0, 0.0, None, 0, None)
    assert rc == OK


def test_plan_splits_small_batches_of_long_caches_only():
    assert plan(1, 32768, 128, 128, 256, 8)["nsplit"] == 1       # batch >= kFwdSplitBelow
    assert plan(1, 192, 128, 128, 8, 8)["nsplit"] == 1           # fewer than 4 key tiles
    p = plan(1, 32768, 128, 128, 8, 8)
    assert p["nsplit"] >= 2 and p["grid"] == 8 * p["nsplit"] and 384 <= p["grid"] <= 512
    assert p["total"] == p["nsplit"] * 8 * 8 * 1 * (128 + 2) * 4 + 256


def test_workspace_answer_is_the_plans_total():
    L = fa_hip.lib()
    for shape in ((1, 32768, 128, 128, 8, 8), (4, 8192, 64, 64, 128, 8), (2, 333, 48, 40, 2, 5)):
        assert L.fa_decode_fwd_workspace(BF16, *shape) == plan(*shape)["total"]
    assert plan(1, 192, 64, 64, 8, 1)["total"] == 0 and L.fa_decode_fwd_workspace(BF16, 1, 192, 64, 64, 8, 1) == 0
    assert L.fa_decode_fwd_workspace(F32, 1, 32768, 128, 128, 8, 8) == 0      # refused shapes need nothing


def test_forced_range_count_is_clamped_to_the_tile_count():
    assert plan(1, 520, 64, 64, 6, 1, force=7)["nsplit"] == 7
    assert plan(1, 192, 64, 64, 6, 1, force=7)["nsplit"] == 3
    L = fa_hip.lib()
    old = L.fa_debug_set_decode_nsplit(3)
    try:
        assert L.fa_decode_fwd_workspace(BF16, 1, 520, 64, 64, 6, 1) == plan(1, 520, 64, 64, 6, 1, force=3)["total"] > 0
    finally:
        assert L.fa_debug_set_decode_nsplit(old) == 3


def test_narrow_loads_for_ragged_or_misaligned_caches_and_no_slabs():
    vec, narrow = plan(1, 4096, 128, 128, 8, 8), plan(1, 4093, 128, 128, 8, 8)
    assert (vec["kernel"], narrow["kernel"]) == (0, 1)
    assert plan(1, 4096, 128, 128, 8, 8, aligned=0)["kernel"] == 1
    # the workspace holds the partials only: the same bytes per range whatever the loads
    assert narrow["total"] - 256 == narrow["nsplit"] * 8 * 8 * 130 * 4
    assert plan(1, 4096, 128, 128, 8, 5, dtype=F32)["kernel"] == -1 and plan(3, 4096, 128, 128, 8, 11)["kernel"] == -1


def test_python_mirror():
    assert "decode_fa" in fa_hip.__all__ and "decode_fa_" in fa_hip.__all__
    q, k, v = torch.zeros(1, 64, 7), torch.zeros(128, 64, 2), torch.zeros(128, 64, 2)
    with pytest.raises(DimensionMismatch):
        fa_hip.decode_fa(q, k, v, group=4)
    with pytest.raises(DimensionMismatch):
        fa_hip.decode_fa(torch.zeros(1, 64, 8), k, v, group=0)
