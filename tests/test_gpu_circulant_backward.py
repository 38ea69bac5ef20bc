"""GPU tests of the circulant backward (fa_circulant_bwd through fa_hip.circulant_fa_backward)
against the float64 restatement tests/circ_bwd_ref.py, evaluated on the device's own O
with l, m from fa.circulant_fa, on bf16-representable inputs.

Tolerances are the project's existing ones, restated here:
  * fp32 / bf16 / fp16: assert_grad_close of test_gpu_backward.py, max|x−y| / max|y| and
    ‖x−y‖ / ‖y‖ (each floored at 1e-2) within GTOL = 2e-5 / 2e-2 / 5e-3;
  * Float64: 1e-12 relative to max(|y|, 1) (test_gpu_float64.py); that path recomputes the
    row statistics in double, so its reference does too (l = m = None).
Shapes are the smallest that reach each way the kernels can go wrong (see CASES)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from circ_bwd_ref import circulant_bwd_ref
from oracle import fa_oracle as O

pytestmark = pytest.mark.gpu
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16, "float64": torch.float64}
GTOL = {"float32": 2e-5, "bfloat16": 2e-2, "float16": 5e-3}
ELEM64 = 1e-12
MFMA, SIMT, F64 = 1, 2, 3   # fa_debug_last_circ_bwd_kernel()

BF, F16, F32, F64T = "bfloat16", "float16", "float32", "float64"
# (N, d, dv, W, B), dtypes, what it reaches
CASES = [
    ((256, 64, 64, 129, 2), (BF, F16, F32, F64T)),   # two workgroups per slab, wrap at both ends, several slabs
    ((384, 64, 64, 75, 1), (BF, F16)),               # p = 37: union start not on an 8-key chunk (off != 0)
    ((96, 64, 32, 200, 1), (BF, F32)),               # W > N, repeated keys, N < one workgroup, dv != d
    ((640, 64, 64, 2, 1), (BF,)),                    # even tiny W, most tiles fully masked
    ((1024, 128, 128, 511, 1), (BF, F16)),           # d = 128 budget, band wider than several tiles
    ((512, 32, 32, 64, 2), (BF,)),                   # d = 32 class
    ((136, 48, 40, 33, 1), (BF,)),                   # head dims inside a class (zero fill, masked stores)
    ((1001, 32, 16, 33, 2), (BF, F32, F64T)),        # ragged N: SIMT path
    ((30, 12, 6, 7, 1), (BF, F32, F64T)),
    ((5, 8, 8, 12, 1), (BF, F32, F64T)),             # N < W
]
PARAMS = [pytest.param(*shape, dt, id="-".join(map(str, shape)) + "-" + dt) for shape, dts in CASES for dt in dts]


@pytest.fixture(scope="module")
def fa():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    fa_hip.lib()
    return fa_hip


def _np(t):
    return t.detach().double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def inputs(N, d, dv, B):
    """bf16-representable q, k, v, do (float64 arrays; shared, never modified)."""
    rng = np.random.default_rng(N * 131 + d * 7 + dv)
    bf = lambda a: torch.tensor(a).to(torch.bfloat16).double().numpy()
    return tuple(bf(rng.standard_normal(s)) for s in ((N, d, B), (N, d, B), (N, dv, B), (N, dv, B)))


def assert_grad_close(x, y, dtype, what, floor=1e-2):
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape and np.all(np.isfinite(x)), what
    if dtype == "float64":
        err = np.abs(x - y).max() / max(np.abs(y).max(), 1.0)
        print(f"{what}: err / max(|y|, 1) {err:.3e}")
        assert err <= ELEM64, f"{what}: elementwise err {err:.3e}"
        return
    scale = max(np.abs(y).max(), floor)
    err = np.abs(x - y).max() / scale
    rel = np.linalg.norm(x - y) / max(np.linalg.norm(y), floor * np.sqrt(y.size))
    print(f"{what}: max err/max|y| {err:.2e}, norm rel {rel:.2e}")
    assert err <= GTOL[dtype] and rel <= GTOL[dtype], f"{what}: max err/max|y| {err:.2e}, norm rel {rel:.2e}"


def device_run(fa, N, d, dv, W, B, dtype, scale=0.0, wrap=None):
    """Forward + backward on the device; returns the tensors and the launched kernel family."""
    q, k, v, do = inputs(N, d, dv, B)
    Q, K, V, dO = (fa.jl_tensor(a, DT[dtype]) for a in (q, k, v, do))
    if wrap is not None:
        K, V = wrap(K), wrap(V)
    Oo, l, m = fa.circulant_fa(Q, K, V, W, scale)
    dQ, dK, dV = fa.circulant_fa_backward(Q, K, V, Oo, dO, l, m, W, scale)
    kind = fa.lib().fa_debug_last_circ_bwd_kernel()
    torch.cuda.synchronize()
    return dict(Q=Q, K=K, V=V, dO=dO, O=Oo, l=l, m=m, dQ=dQ, dK=dK, dV=dV, kind=kind)


def check_vs_ref(r, N, d, dv, W, B, dtype, scale=0.0):
    q, k, v, do = inputs(N, d, dv, B)
    f64 = dtype == "float64"
    ref = circulant_bwd_ref(q, k, v, _np(r["O"]), do, None if f64 else _np(r["l"]), None if f64 else _np(r["m"]),
                            W, scale)
    for nm, y in zip(("dQ", "dK", "dV"), ref):
        assert_grad_close(_np(r[nm]), y, dtype, nm)


def expected_kind(N, dtype):
    if dtype == "float64":
        return F64
    return MFMA if dtype in (BF, F16) and N % 8 == 0 else SIMT


@pytest.mark.parametrize("N,d,dv,W,B,dtype", PARAMS)
def test_backward_vs_reference(fa, N, d, dv, W, B, dtype):
    r = device_run(fa, N, d, dv, W, B, dtype)
    assert r["kind"] == expected_kind(N, dtype)
    check_vs_ref(r, N, d, dv, W, B, dtype)


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("W", [64, 128])
def test_full_band_equals_dense_backward(fa, W, dtype):
    """W = N, 2N: the band holds every key once / twice, P is the dense P."""
    N, d, dv, B = 64, 64, 64, 1
    q, k, v, do = inputs(N, d, dv, B)
    r = device_run(fa, N, d, dv, W, B, dtype)
    _, l, m = O.dense_fa3(q, k, v)
    ref = O.dense_fa_backward(q, k, v, _np(r["O"]), do, l, m)
    for nm, y in zip(("dQ", "dK", "dV"), ref):
        assert_grad_close(_np(r[nm]), y, dtype, nm)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_band_of_one_key(fa, dtype):
    """W = 1: P = 1, so dQ = dK = 0 exactly and dV = dO bitwise."""
    r = device_run(fa, 200, 32, 16, 1, 2, dtype)
    assert int(torch.count_nonzero(r["dQ"])) == 0 and int(torch.count_nonzero(r["dK"])) == 0
    assert torch.equal(r["dV"], r["dO"])


def test_kernel_family_proof(fa):
    """Which kernels ran: MFMA on the aligned bf16 shape, SIMT when forced or ragged, the
    double kernels for Float64; forced SIMT and MFMA agree within the bf16 tolerance."""
    L = fa.lib()
    shape = (256, 64, 64, 129, 2)
    tiled = device_run(fa, *shape, BF)
    assert tiled["kind"] == MFMA
    old = L.fa_debug_set_circ_generic(2)
    try:
        simt = device_run(fa, *shape, BF)
    finally:
        L.fa_debug_set_circ_generic(old)
    assert simt["kind"] == SIMT
    for nm in ("dQ", "dK", "dV"):
        assert_grad_close(_np(simt[nm]), _np(tiled[nm]), BF, nm + " SIMT vs MFMA")
    check_vs_ref(simt, *shape, BF)
    assert device_run(fa, 1001, 32, 16, 33, 2, BF)["kind"] == SIMT
    assert device_run(fa, 30, 12, 6, 7, 1, F64T)["kind"] == F64
    assert device_run(fa, *shape, BF)["kind"] == MFMA   # the knob was restored


def test_plan_is_what_ran(fa):
    """The family the launcher reports is circ_bwd_plan's answer (fa_debug_circ_bwd_plan) for the
    shape, the knob in force and the tensors' actual 16-B alignment, on the smallest shapes that
    reach every branch: MFMA, SIMT by ragged N, by the knob and by fp32, Float64, and W = 1."""
    L = fa.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    L.fa_debug_circ_bwd_plan.restype = ci
    L.fa_debug_circ_bwd_plan.argtypes = [ci] + [i64] * 5 + [ci] * 4 + [ctypes.POINTER(i64)]
    d, dv, B = 32, 32, 2
    ran = []
    for dtype, N, W, knob in ((BF, 256, 9, 0), (BF, 250, 9, 0), (BF, 256, 9, 2), (F32, 256, 9, 0), (F64T, 64, 9, 0),
                              (BF, 256, 1, 0), (F64T, 64, 1, 0)):
        old = L.fa_debug_set_circ_generic(knob)
        try:
            r = device_run(fa, N, d, dv, W, B, dtype)
        finally:
            L.fa_debug_set_circ_generic(old)
        al = lambda *names: int(all(r[n].data_ptr() % 16 == 0 for n in names))
        out = (i64 * 15)()
        want = L.fa_debug_circ_bwd_plan(fa.DTYPES[DT[dtype]], N, d, dv, B, W, knob, al("Q", "K", "V"), al("O"), al("dO"), out)
        assert r["kind"] == want and out[0] == (W == 1), (dtype, N, W, knob, r["kind"], want)
        ran.append(want)
    assert ran == [MFMA, SIMT, SIMT, SIMT, F64, SIMT, F64]


def test_unaligned_kv_views_fall_back(fa):
    """K / V views at an odd element offset (N % 8 == 0): not the 16-B path, same result."""
    def shifted(t):
        raw = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        view = raw[1:].as_strided(tuple(t.shape), fa.jl_strides(t.shape))
        view.copy_(t)
        assert view.data_ptr() % 16 != 0
        return view
    shape = (256, 64, 64, 129, 2)
    r = device_run(fa, *shape, BF, wrap=shifted)
    assert r["kind"] == SIMT
    check_vs_ref(r, *shape, BF)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_explicit_scale(fa, dtype):
    shape = (256, 64, 64, 129, 2)
    r = device_run(fa, *shape, dtype, scale=0.05)
    check_vs_ref(r, *shape, dtype, scale=0.05)


@pytest.mark.parametrize("N,d,dv,W,B,dtype", [(256, 64, 64, 129, 2, BF), (1001, 32, 16, 33, 2, F32)])
def test_outputs_fully_written_and_workspace_at_an_odd_address(fa, N, d, dv, W, B, dtype):
    """Sentinel-filled outputs are overwritten everywhere (bitwise the mirror's result), with
    the workspace starting at an odd address (the entry aligns inside the 256 B of slack)."""
    r = device_run(fa, N, d, dv, W, B, dtype)
    L = fa.lib()
    code = fa.DTYPES[DT[dtype]]
    outs = [fa.jl_empty(r[nm].shape, DT[dtype]).fill_(777.0) for nm in ("dQ", "dK", "dV")]
    nws = L.fa_circulant_bwd_workspace(code, N, d, dv, B, W)
    raw = torch.empty(nws + 1, dtype=torch.uint8, device="cuda")
    ws = raw[1:]
    assert ws.data_ptr() % 2 == 1
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.fa_circulant_bwd(code, P(r["Q"]), P(r["K"]), P(r["V"]), P(r["O"]), P(r["dO"]), P(r["l"]), P(r["m"]),
                            P(outs[0]), P(outs[1]), P(outs[2]), N, d, dv, B, W, 0.0, P(ws), nws,
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.fa_last_error()
    torch.cuda.synchronize()
    for nm, t in zip(("dQ", "dK", "dV"), outs):
        assert torch.equal(t, r[nm]), nm


@pytest.mark.parametrize("N,d,dv,W,B,dtype", [(2048, 64, 64, 129, 2, BF), (1001, 32, 16, 33, 2, F32)])
def test_bitwise_deterministic(fa, N, d, dv, W, B, dtype):
    a = device_run(fa, N, d, dv, W, B, dtype)
    b = device_run(fa, N, d, dv, W, B, dtype)
    for nm in ("dQ", "dK", "dV"):
        assert torch.equal(a[nm], b[nm]), nm


def test_medium_size_properties(fa):
    """(4096, 64, 64, 129, 2) bf16: every query's weights sum to one, so Σ_keys dV = Σ_q dO
    (the bound of test_backward_config4_properties); everything finite."""
    N, d, dv, W, B = 4096, 64, 64, 129, 2
    g = torch.Generator(device="cuda").manual_seed(5)
    mk = lambda c: fa.jl_tensor(torch.randn((N, c, B), generator=g, device="cuda"), torch.bfloat16)
    Q, K, V, dO = mk(d), mk(d), mk(dv), mk(dv)
    Oo, l, m = fa.circulant_fa(Q, K, V, W)
    dQ, dK, dV = fa.circulant_fa_backward(Q, K, V, Oo, dO, l, m, W)
    assert fa.lib().fa_debug_last_circ_bwd_kernel() == MFMA
    torch.cuda.synchronize()
    for t in (dQ, dK, dV):
        assert bool(torch.isfinite(t).all())
    assert torch.allclose(dV.float().sum(0), dO.float().sum(0), rtol=2e-2, atol=0.5)
