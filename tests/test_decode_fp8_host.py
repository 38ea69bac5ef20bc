"""CPU tests of decode attention over an fp8 cache: the plan hook against decode_plan's, the C
ABI's checks before any launch (fa_decode_fp8_fwd), and the Python mirror (names, the cache
dtype, quantize_kv_fp8).  No device is touched."""
from __future__ import annotations

import ctypes

import pytest
import torch

import fa_hip

F32, BF16, F16, F64 = 0, 1, 2, 3
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
P = ctypes.c_void_p(256)   # a non-null pointer that no refused call dereferences


def call(dtype=BF16, Q=P, K8=P, N=1, Nk=4096, d=128, dv=128, batch=8, group=8, ws=None, ws_bytes=0):
    L = fa_hip.lib()
    rc = L.fa_decode_fp8_fwd(dtype, Q, K8, P, None, None, P, P, P, N, Nk, d, dv, batch, group, None, None, -1, 0, 0.0,
                             ws, ws_bytes, None)
    return rc, L.fa_last_error().decode()


def plan(hook, N, Nk, d, dv, batch, group, force=0, aligned=1, dtype=BF16):
    out = (ctypes.c_int64 * 4)()
    k = getattr(fa_hip.lib(), hook)(dtype, N, Nk, d, dv, batch, group, force, aligned, out)
    assert k == out[0]
    return dict(kernel=out[0], nsplit=out[1], grid=out[2], total=out[3])


@pytest.mark.parametrize("Nk", (4096, 4104, 4093, 528, 264))
@pytest.mark.parametrize("aligned", (1, 0))
def test_wide_loads_need_sixteen_keys_and_alignment(Nk, aligned):
    p8 = plan("fa_debug_decode_fp8_plan", 1, Nk, 128, 128, 8, 8, aligned=aligned)
    assert p8["kernel"] == (0 if Nk % 16 == 0 and aligned else 1)


@pytest.mark.parametrize("shape", [(1, 32768, 128, 128, 8, 8), (4, 8192, 64, 64, 128, 8), (2, 333, 48, 40, 2, 5),
                                   (1, 192, 64, 64, 8, 1)])
@pytest.mark.parametrize("force", (0, 3, 7))
def test_split_and_workspace_are_decode_plans(shape, force):
    p8, p16 = (plan(h, *shape, force=force) for h in ("fa_debug_decode_fp8_plan", "fa_debug_decode_plan"))
    assert {k: p8[k] for k in ("nsplit", "grid", "total")} == {k: p16[k] for k in ("nsplit", "grid", "total")}
    L = fa_hip.lib()
    old = L.fa_debug_set_decode_nsplit(force)
    try:
        assert L.fa_decode_fp8_fwd_workspace(BF16, *shape) == p8["total"]
    finally:
        L.fa_debug_set_decode_nsplit(old)


def test_refused_shapes_have_no_plan():
    assert plan("fa_debug_decode_fp8_plan", 1, 4096, 128, 128, 8, 5, dtype=F32)["kernel"] == -1
    assert plan("fa_debug_decode_fp8_plan", 3, 4096, 128, 128, 8, 11)["kernel"] == -1


@pytest.mark.parametrize("kw,status,words", [
    (dict(Q=None), INVALID, "null pointer"),
    (dict(K8=None), INVALID, "null pointer"),
    (dict(group=0), INVALID, "DimensionMismatch"),
    (dict(Q=None, group=0), INVALID, "null pointer"),           # documented order: pointers, then dimensions
    (dict(d=129), UNSUPPORTED, "head dimension exceeds the compiled maximum (128)"),
    (dict(N=4, Nk=3), UNSUPPORTED, "needs Nk >= N"),
    (dict(N=3, group=11), UNSUPPORTED, "fa_varlen_fwd"),
    (dict(dtype=F32), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(dtype=F64), UNSUPPORTED, "bf16 / fp16 only"),
    (dict(d=129, N=3, group=11), UNSUPPORTED, "head dimension"),  # documented order: head dims before rows
    (dict(Nk=1 << 24), UNSUPPORTED, "32-bit addressing"),         # a slab of 2^31 bytes
    (dict(), WORKSPACE, "fa_decode_fp8_fwd_workspace()"),
    (dict(ws=P, ws_bytes=1024), WORKSPACE, "fa_decode_fp8_fwd_workspace()"),
])
def test_refusals_before_any_launch(kw, status, words):
    rc, msg = call(**kw)
    assert rc == status and words in msg and msg.startswith("fa_decode_fp8_fwd: ")


@pytest.mark.parametrize("kw", [dict(N=0), dict(batch=0)])
def test_no_op_inputs_dereference_nothing(kw):
    args = dict(N=1, Nk=64, d=64, dv=64, batch=2, group=2)
    args.update(kw)
    rc = fa_hip.lib().fa_decode_fp8_fwd(BF16, None, None, None, None, None, None, None, None, args["N"], args["Nk"],
                                        args["d"], args["dv"], args["batch"], args["group"], None, None, -1, 0, 0.0,
                                        None, 0, None)
    assert rc == OK


def test_python_mirror():
    assert {"decode_fp8_fa", "decode_fp8_fa_", "quantize_kv_fp8"} <= set(fa_hip.__all__)
    q, k8 = torch.zeros(1, 64, 2, dtype=torch.bfloat16), torch.zeros(128, 64, 2, dtype=torch.uint8)
    for bad in (torch.bfloat16, torch.float8_e5m2, torch.int8):
        with pytest.raises(TypeError):
            fa_hip.decode_fp8_fa(q, k8, torch.zeros(128, 64, 2).to(bad))
    with pytest.raises(fa_hip.DimensionMismatch):
        fa_hip.decode_fp8_fa(torch.zeros(1, 64, 7, dtype=torch.bfloat16), k8, k8, group=4)


def test_quantize_kv_fp8_round_trips_within_half_an_ulp():
    g = torch.Generator().manual_seed(3)
    k, v = torch.randn(40, 24, 3, generator=g), 5.0 * torch.randn(40, 8, 3, generator=g)
    v[:, :, 1] = 0.0                                     # an all-zero slab: scale 1.0
    k8, v8, ks, vs = fa_hip.quantize_kv_fp8(k, v)
    assert k8.dtype == v8.dtype == torch.float8_e4m3fn and fa_hip.is_jl_contiguous(k8) and fa_hip.is_jl_contiguous(v8)
    assert ks.dtype == torch.float32 and ks.shape == vs.shape == (3,) and float(vs[1]) == 1.0
    for t, t8, s in ((k, k8, ks), (v, v8, vs)):
        amax = t.abs().amax(dim=(0, 1))
        assert torch.equal(s, torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)))
        x = (t / s).double()                             # the amax-scaled values, |x| <= 448
        # e4m3fn: 3 mantissa bits, so an ulp is 2^(floor(log2 |x|) - 3), 2^-9 below 2^-6
        ulp = torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -6))) - 3)
        assert bool(((t8.double() - x).abs() <= 0.5 * ulp * (1 + 1e-6)).all())
