"""GPU tests of causal attention (fa_causal_fwd / fa_causal_bwd through fa_hip.causal_fa,
causal_fa_backward, causal_dpa) against the float64 yardstick tests/causal_ref.py on
bf16-representable inputs seeded per shape.

Tolerances are the project's existing ones, restated here:
  * forward: conftest.assert_close and its l, m rule (1e-5 fp32 / 1e-4 16-bit); Float64
    1e-12 relative to max(|y|, 1) (test_gpu_float64.py);
  * backward: assert_grad_close of test_gpu_backward.py, max|x-y| / max|y| and
    ||x-y|| / ||y|| (each floored at 1e-2) within GTOL = 2e-5 / 2e-2 / 5e-3 for fp32 / bf16 /
    fp16, and 1e-12 for Float64, whose device path recomputes the row statistics in double,
    so its reference does too (l = m = None).
The backward reference is evaluated on the device's own O, l, m.  Shapes are the smallest that
reach each way the kernels can go wrong (see CASES)."""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from causal_ref import causal_bwd_ref, causal_fwd_ref
from conftest import assert_close, assert_lm_close

pytestmark = pytest.mark.gpu
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16, "float64": torch.float64}
GTOL = {"float32": 2e-5, "bfloat16": 2e-2, "float16": 5e-3}
ELEM64 = 1e-12

BF, F16, F32, F64T = "bfloat16", "float16", "float32", "float64"
# (N, Nk, d, dv, B), dtypes, what it reaches
CASES = [
    ((1024, 1024, 64, 64, 2), (BF, F16, F32, F64T)),  # two 512-row workgroups per slab, jt1 = 8 and 16, diagonal in every wave; t0 0..14
    ((512, 576, 64, 64, 1), (BF, F16)),                # off = 64: odd jt1 (9), the unrolled loop's tail
    ((256, 296, 64, 64, 2), (BF,)),                    # off = 40, no multiple of 32: diagonal mid-fragment, t0 rounding
    ((520, 520, 64, 64, 1), (BF, F16)),                # _wide with a ragged last tile: both masks in one tile
    ((500, 500, 64, 64, 1), (BF, F32)),                # Nk % 8 != 0: padded K / V forward, padded backward, off from real extents
    ((200, 333, 48, 40, 2), (BF, F32, F64T)),          # head dims inside a class, ragged both ways, off = 133
    ((512, 512, 128, 128, 1), (BF, F16)),              # d = 128 class (w8b64, 256-row workgroups), backward register budget
    ((384, 384, 32, 32, 2), (BF,)),                    # d = 32 class
    ((8, 1000, 64, 64, 2), (BF, F32)),                 # decode-like: few queries, off = 992, one partial query block
    ((64, 64, 64, 64, 1), (BF,)),                      # jt1 = 1: the loop runs once
    ((1, 1, 16, 8, 3), (BF, F32, F64T)),               # degenerate
    ((5, 5, 8, 8, 1), (BF, F32, F64T)),
    ((2048, 2048, 64, 64, 1), (BF,)),                  # a grid the dense forward splits over keys: causal must not, and must be right
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
def inputs(N, Nk, d, dv, B):
    """bf16-representable q, k, v, do (float64 arrays; shared, never modified)."""
    rng = np.random.default_rng(N * 131 + Nk * 17 + d * 7 + dv)
    bf = lambda a: torch.tensor(a).to(torch.bfloat16).double().numpy()
    return tuple(bf(rng.standard_normal(s)) for s in ((N, d, B), (Nk, d, B), (Nk, dv, B), (N, dv, B)))


@functools.lru_cache(maxsize=None)
def fwd_ref(N, Nk, d, dv, B, scale=0.0):
    q, k, v, _ = inputs(N, Nk, d, dv, B)
    return causal_fwd_ref(q, k, v, scale)


def assert_fwd_close(r, ref, dtype, what=""):
    o, l, m = ref
    if dtype == "float64":
        for nm, x, y in (("O", r["O"], o), ("l", r["l"], l), ("m", r["m"], m)):
            tol = ELEM64 if nm == "O" else 1e-6      # l, m leave the Float64 kernel as float32
            err = np.abs(_np(x) - y).max() / max(np.abs(y).max(), 1.0)
            print(f"{what}{nm}: err / max(|y|, 1) {err:.3e}")
            assert err <= tol, f"{what}{nm}: {err:.3e}"
        return
    assert_close(_np(r["O"]), o, dtype, what + "O")
    assert_lm_close(_np(r["l"]), l, dtype, what + "l")
    assert_lm_close(_np(r["m"]), m, dtype, what + "m")


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


def device_run(fa, N, Nk, d, dv, B, dtype, scale=0.0, kv=None, backward=True):
    """Forward (+ backward) on the device.  kv: replaces the (k, v) float64 inputs."""
    q, k, v, do = inputs(N, Nk, d, dv, B)
    if kv is not None:
        k, v = kv
    Q, K, V, dO = (fa.jl_tensor(a, DT[dtype]) for a in (q, k, v, do))
    Oo, l, m = fa.causal_fa(Q, K, V, scale)
    r = dict(Q=Q, K=K, V=V, dO=dO, O=Oo, l=l, m=m)
    if backward:
        r["dQ"], r["dK"], r["dV"] = fa.causal_fa_backward(Q, K, V, Oo, dO, l, m, scale)
    torch.cuda.synchronize()
    return r


def check_bwd_vs_ref(r, N, Nk, d, dv, B, dtype, scale=0.0):
    q, k, v, do = inputs(N, Nk, d, dv, B)
    f64 = dtype == "float64"
    ref = causal_bwd_ref(q, k, v, _np(r["O"]), do, None if f64 else _np(r["l"]), None if f64 else _np(r["m"]), scale)
    for nm, y in zip(("dQ", "dK", "dV"), ref):
        assert_grad_close(_np(r[nm]), y, dtype, nm)


@pytest.mark.parametrize("N,Nk,d,dv,B,dtype", PARAMS)
def test_forward_and_backward_vs_reference(fa, N, Nk, d, dv, B, dtype):
    r = device_run(fa, N, Nk, d, dv, B, dtype)
    assert fa.lib().fa_debug_fwd_last_path() != 30
    assert_fwd_close(r, fwd_ref(N, Nk, d, dv, B), dtype)
    check_bwd_vs_ref(r, N, Nk, d, dv, B, dtype)


@pytest.mark.parametrize("dtype", [BF, F16, F32, F64T])
def test_row_0_sees_key_0_only(fa, dtype):
    """N == Nk: O[0] = V[0] bitwise, l[0] = 1, m[0] = tau q0.k0."""
    N, d, dv, B = 256, 64, 64, 2
    q, k, v, _ = inputs(N, N, d, dv, B)
    r = device_run(fa, N, N, d, dv, B, dtype, backward=False)
    assert torch.equal(r["O"][0], r["V"][0])
    assert bool((r["l"][0] == 1.0).all())
    m0 = (q[0] * k[0]).sum(axis=0) / math.sqrt(d)
    assert_lm_close(_np(r["m"][0, 0]), m0, F32 if dtype == F64T else dtype, "m[0]")


LEAK = [((1024, 1024, 64, 64, 2), 650), ((256, 296, 64, 64, 2), 139), ((512, 512, 128, 128, 1), 301)]


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("shape,j0", LEAK, ids=["-".join(map(str, s)) for s, _ in LEAK])
def test_no_leak_from_the_future(fa, shape, j0, dtype):
    """K and V at keys j >= j0 (inside a tile, off a 32 boundary) overwritten with +-3e4:
    the rows that cannot see them are bitwise unchanged, forward and dQ; dK, dV of the
    earlier keys still depend on later queries' P, so they are compared, within GTOL, with
    the perturbed problem's own yardstick, not with the unperturbed run: measured against
    that run they move by 0.08 to 66 times max|y| on these shapes (fp32 and bf16 alike),
    as the mathematics says they must."""
    N, Nk, d, dv, B = shape
    off = Nk - N
    q, k, v, do = inputs(*shape)
    base = device_run(fa, *shape, dtype)
    k2, v2 = k.copy(), v.copy()
    sign = np.where(np.arange(Nk - j0) % 2 == 0, 1.0, -1.0)[:, None, None]
    k2[j0:] = 3e4 * sign
    v2[j0:] = -3e4 * sign
    pert = device_run(fa, *shape, dtype, kv=(k2, v2))
    n_safe = j0 - off                      # rows i < n_safe have i + off < j0
    assert 0 < n_safe < N
    for nm in ("O", "l", "m", "dQ"):
        assert torch.equal(pert[nm][:n_safe], base[nm][:n_safe]), nm
    for nm in ("O", "l", "m", "dQ", "dK", "dV"):
        assert bool(torch.isfinite(pert[nm]).all()), nm
    # dK, dV of the keys < j0 are NOT those of the unperturbed run: the later queries, which
    # see the huge keys, put all their weight there, so their share of these sums (about
    # (N - n_safe) / N of dV[0]) is gone.  What must hold is that they are right for the
    # perturbed problem: compare with its own yardstick (on the perturbed run's O, l, m),
    # within GTOL; the distance to the unperturbed run is printed, not asserted.
    ref = causal_bwd_ref(q, k2, v2, _np(pert["O"]), do, _np(pert["l"]), _np(pert["m"]))
    for nm, y in zip(("dK", "dV"), ref[1:]):
        x, x0 = _np(pert[nm])[:j0], _np(base[nm])[:j0]
        print(f"{nm}[:j0] perturbed vs unperturbed run: max|diff| / max|y| {np.abs(x - x0).max() / np.abs(x0).max():.2e}")
        assert_grad_close(x, y[:j0], dtype, nm + "[:j0]")


@pytest.mark.parametrize("shape,dtype", [((520, 520, 64, 64, 1), BF), ((200, 333, 48, 40, 2), F32),
                                         ((512, 512, 128, 128, 1), F16)])
def test_last_row_equals_dense_last_row(fa, shape, dtype):
    """The last query sees every key."""
    N, Nk, d, dv, B = shape
    r = device_run(fa, *shape, dtype, backward=False)
    yd, ld, md = fa.dense_fa(r["Q"], r["K"], r["V"])
    torch.cuda.synchronize()
    assert_close(_np(r["O"][N - 1:]), _np(yd[N - 1:]), dtype, "O[last]")
    assert_lm_close(_np(r["l"][N - 1:]), _np(ld[N - 1:]), dtype, "l[last]")
    assert_lm_close(_np(r["m"][N - 1:]), _np(md[N - 1:]), dtype, "m[last]")


def test_kernel_choice_forward(fa):
    """(4096, 4096, 128, 128, 16) bf16: 256 blocks, where dense takes fa_fwd_p4; causal does not."""
    N, d, B = 4096, 128, 16
    g = torch.Generator(device="cuda").manual_seed(11)
    mk = lambda: fa.jl_tensor(torch.randn((N, d, B), generator=g, device="cuda"), torch.bfloat16)
    Q, K, V = mk(), mk(), mk()
    Oo, l, m = fa.causal_fa(Q, K, V)
    assert fa.lib().fa_debug_fwd_last_path() != 30
    torch.cuda.synchronize()
    sl = lambda t: _np(t[:, :, :1])
    o, lr, mr = causal_fwd_ref(sl(Q), sl(K), sl(V))
    assert_close(sl(Oo), o, BF, "O slab 0")
    assert_lm_close(sl(l), lr, BF, "l slab 0")
    assert_lm_close(sl(m), mr, BF, "m slab 0")


def test_kernel_choice_backward(fa):
    """(1024, 1024, 64, 64, 64) bf16 is single-pass-eligible: causal still runs the two passes
    (hand-off status -1) with a workspace smaller than the dense single pass's; the forced
    SIMT backward agrees with the MFMA one."""
    N, d, B = 1024, 64, 64
    L = fa.lib()
    g = torch.Generator(device="cuda").manual_seed(12)
    mk = lambda: fa.jl_tensor(torch.randn((N, d, B), generator=g, device="cuda"), torch.bfloat16)
    Q, K, V, dO = mk(), mk(), mk(), mk()
    Oo, l, m = fa.causal_fa(Q, K, V)
    dQ, dK, dV = fa.causal_fa_backward(Q, K, V, Oo, dO, l, m)
    assert fa.backward_handoff_status() == -1
    s5 = lambda t: _np(t[:, :, 5:6])
    ref = causal_bwd_ref(s5(Q), s5(K), s5(V), s5(Oo), s5(dO), s5(l), s5(m))
    for nm, x, y in zip(("dQ", "dK", "dV"), (dQ, dK, dV), ref):
        assert_grad_close(s5(x), y, BF, nm + " slab 5")
    old = L.fa_debug_set_bwd_mode(2)
    try:
        assert L.fa_causal_bwd_workspace(1, N, N, d, d, B) < L.fa_dense_bwd_workspace(1, N, N, d, d, B)
    finally:
        L.fa_debug_set_bwd_mode(old)
    shape = (1024, 1024, 64, 64, 2)
    mfma = device_run(fa, *shape, BF)
    old = L.fa_debug_set_bwd_generic(1)
    try:
        simt = device_run(fa, *shape, BF)
    finally:
        L.fa_debug_set_bwd_generic(old)
    for nm in ("dQ", "dK", "dV"):
        assert_grad_close(_np(simt[nm]), _np(mfma[nm]), BF, nm + " SIMT vs MFMA")
    check_bwd_vs_ref(simt, *shape, BF)


@pytest.mark.parametrize("shape,dtype", [((1024, 1024, 64, 64, 2), BF), ((200, 333, 48, 40, 2), F32)])
def test_bitwise_deterministic(fa, shape, dtype):
    a = device_run(fa, *shape, dtype)
    b = device_run(fa, *shape, dtype)
    for nm in ("O", "l", "m", "dQ", "dK", "dV"):
        assert torch.equal(a[nm], b[nm]), nm


def test_launch_order_knob_changes_no_bit(fa):
    """Every launch order of the query blocks (in order, a slab's heaviest first, block-major
    inside an XCD's share: 16 slabs of 2 blocks) computes the same bits."""
    L = fa.lib()
    shape = (1024, 1024, 64, 64, 16)
    a = device_run(fa, *shape, BF, backward=False)
    for order in (0, 1, 2):
        old = L.fa_debug_set_causal_order(order)
        try:
            b = device_run(fa, *shape, BF, backward=False)
        finally:
            L.fa_debug_set_causal_order(old)
        for nm in ("O", "l", "m"):
            assert torch.equal(a[nm], b[nm]), (order, nm)
    q, k, v, _ = inputs(*shape)
    assert_close(_np(a["O"][:, :, 9:10]), causal_fwd_ref(q[:, :, 9:10], k[:, :, 9:10], v[:, :, 9:10])[0], BF, "O slab 9")


@pytest.mark.parametrize("shape,dtype", [((520, 520, 64, 64, 1), BF), ((200, 333, 48, 40, 2), BF),
                                         ((200, 333, 48, 40, 2), F32)])
def test_raw_abi_outputs_fully_written_workspaces_at_an_odd_address(fa, shape, dtype):
    """Sentinel-filled outputs are overwritten everywhere, bitwise the mirror's result, with
    both workspaces starting at an odd address."""
    N, Nk, d, dv, B = shape
    r = device_run(fa, *shape, dtype)
    L = fa.lib()
    code = fa.DTYPES[DT[dtype]]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def odd_ws(n):
        raw = torch.empty(n + 2, dtype=torch.uint8, device="cuda")   # never empty, also when n == 0
        assert raw[1:].data_ptr() % 2 == 1
        return raw[1:]

    Oo = fa.jl_empty(r["O"].shape, DT[dtype]).fill_(777.0)
    l = fa.jl_empty(r["l"].shape, torch.float32).fill_(777.0)
    m = fa.jl_empty(r["m"].shape, torch.float32).fill_(777.0)
    nws = L.fa_causal_fwd_workspace(code, N, Nk, d, dv, B)
    ws = odd_ws(nws)
    rc = L.fa_causal_fwd(code, P(r["Q"]), P(r["K"]), P(r["V"]), P(Oo), P(l), P(m), N, Nk, d, dv, B, 0.0,
                         P(ws), nws, stream)
    assert rc == 0, L.fa_last_error()
    outs = [fa.jl_empty(r[nm].shape, DT[dtype]).fill_(777.0) for nm in ("dQ", "dK", "dV")]
    nwb = L.fa_causal_bwd_workspace(code, N, Nk, d, dv, B)
    wb = odd_ws(nwb)
    rc = L.fa_causal_bwd(code, P(r["Q"]), P(r["K"]), P(r["V"]), P(Oo), P(r["dO"]), P(l), P(m),
                         P(outs[0]), P(outs[1]), P(outs[2]), N, Nk, d, dv, B, 0.0, P(wb), nwb, stream)
    assert rc == 0, L.fa_last_error()
    torch.cuda.synchronize()
    for nm, t in zip(("O", "l", "m", "dQ", "dK", "dV"), [Oo, l, m] + outs):
        assert torch.equal(t, r[nm]), nm
    st = ctypes.c_int(-2)
    assert L.fa_dense_bwd_handoff_status(P(wb), nwb, stream, ctypes.byref(st)) == 0 and st.value == -1


@pytest.mark.parametrize("dtype", [BF, F32])
def test_causal_dpa_against_causal_fa(fa, dtype):
    shape = (256, 296, 64, 64, 2)
    N, Nk = shape[:2]
    r = device_run(fa, *shape, dtype, backward=False)
    Od, P = fa.causal_dpa(r["Q"], r["K"], r["V"])
    torch.cuda.synchronize()
    assert_close(_np(Od), _np(r["O"]), dtype, "causal_dpa O vs causal_fa O")
    assert_close(_np(Od), fwd_ref(*shape)[0], dtype, "causal_dpa O")
    hidden = torch.arange(Nk, device="cuda")[None, :] > torch.arange(N, device="cuda")[:, None] + (Nk - N)
    assert int(torch.count_nonzero(P[hidden])) == 0
    assert torch.allclose(P.float().sum(1), torch.ones((N, shape[4]), device="cuda"), atol=2e-2)


@pytest.mark.parametrize("shape,dtype", [((512, 576, 64, 64, 1), BF), ((200, 333, 48, 40, 2), F32)])
def test_explicit_scale(fa, shape, dtype):
    r = device_run(fa, *shape, dtype, scale=0.05)
    assert_fwd_close(r, fwd_ref(*shape, 0.05), dtype)
    check_bwd_vs_ref(r, *shape, dtype, scale=0.05)
