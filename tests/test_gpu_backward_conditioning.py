"""GPU parity of every dense, causal and circulant backward route under explicit scales and
ill-conditioned scores: the five input families of tests/cond_inputs.py (hot, cold, offset,
anti, hotkeys) crossed with the routes of ROUTES below.  Each case runs the forward and the
backward on the device with the family's scale, asserts that the intended route ran (hand-off
status, the fa_debug_dense_bwd_plan query on the knobs in force, fa_debug_last_circ_bwd_kernel)
and compares dQ, dK, dV with the float64 reference evaluated on the device's own O, l, m
(Float64: on the reference's own statistics, as that path recomputes them in double).

Tolerance: the two metrics of assert_grad_close (tests/test_gpu_backward.py: max|x-y| / max|y|
and ||x-y|| / ||y||, each denominator floored at 1e-2) within max(GTOL, 2 e_ref), GTOL = 2e-5 /
2e-2 / 5e-3 for fp32 / bf16 / fp16.  e_ref is what the kernels' formulation costs on the very
case (cond_inputs.e_ref: float32 scores and statistics, 16-bit P and dS, against float64; no
device value enters it), and the factor 2 covers the summation order and the MFMA accumulation.
Float64 keeps 1e-12 relative to max(|y|, 1) (tests/test_gpu_float64.py).  Each case prints a
COND line with e_ref, the device error and its ratio to the budget.

Shapes are the smallest that reach each route; none has more than 520 rows."""
from __future__ import annotations

import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import cond_inputs as C
from causal_ref import causal_bwd_ref
from circ_bwd_ref import circulant_bwd_ref
from conftest import assert_lm_close
from oracle import fa_oracle as O

pytestmark = pytest.mark.gpu
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16, "float64": torch.float64}
BF, F16, F32, F64T = "bfloat16", "float16", "float32", "float64"
ELEM64 = 1e-12
# fa::DenseBwdKernel (csrc/fa_dense_plan.h)
K_F64, K_GENERIC, K_F32MFMA, K_TWOPASS, K_SINGLE = range(5)
CIRC_MFMA, CIRC_SIMT, CIRC_F64 = 1, 2, 3   # fa_debug_last_circ_bwd_kernel()

# route -> (knobs, the plan's kernel, padded, hand-off status (None: not asked))
DENSE_ROUTES = {
    "twopass": (dict(bwd_mode=1), K_TWOPASS, 0, -1),
    "single": (dict(bwd_mode=2), K_SINGLE, 0, 0),
    "padded": (dict(), K_TWOPASS, 1, -1),
    "padded_single": (dict(bwd_mode=2), K_SINGLE, 1, 0),   # the single pass on the zero-padded copies
    "generic": (dict(bwd_generic=1), K_GENERIC, 0, None),
    "f32mfma": (dict(), K_F32MFMA, 0, None),
    "f64": (dict(), K_F64, 0, None),
}
MFMA3 = [(512, 512, 64, 64, 2), (256, 512, 128, 128, 2), (256, 256, 32, 64, 2)]
# (entry, route, shape, dtypes); dense and causal shapes are (N, Nk, d, dv, B), circulant ones
# (N, d, dv, W, B) with W <= N, so that the band is a mask
ROUTES = [
    ("dense", "twopass", MFMA3[0], (BF, F16)), ("dense", "twopass", MFMA3[1], (BF,)), ("dense", "twopass", MFMA3[2], (BF,)),
    ("dense", "single", MFMA3[0], (BF, F16)), ("dense", "single", MFMA3[1], (BF, F16)), ("dense", "single", MFMA3[2], (BF,)),
    ("dense", "padded", (200, 137, 96, 48, 2), (BF,)), ("dense", "padded", (30, 30, 12, 6, 2), (BF, F16)),
    ("dense", "padded_single", (200, 137, 96, 48, 2), (BF, F16)),
    ("dense", "generic", (200, 136, 128, 128, 2), (BF,)),
    ("dense", "f32mfma", (256, 256, 64, 64, 2), (F32,)), ("dense", "f32mfma", (130, 200, 128, 128, 2), (F32,)),
    ("dense", "f64", (100, 77, 12, 6, 2), (F64T,)), ("dense", "f64", (128, 128, 64, 64, 1), (F64T,)),
    ("causal", "twopass", (256, 256, 64, 64, 2), (BF, F16)), ("causal", "twopass", (200, 328, 128, 64, 2), (BF,)),
    ("causal", "padded", (77, 130, 40, 24, 1), (BF,)),
    ("causal", "generic", (200, 328, 128, 64, 2), (BF,)),
    ("causal", "f32mfma", (256, 256, 64, 64, 2), (F32,)), ("causal", "f32mfma", (77, 130, 40, 24, 1), (F32,)),
    ("causal", "f64", (77, 130, 40, 24, 1), (F64T,)),
    ("circulant", "mfma", (256, 64, 64, 129, 2), (BF,)), ("circulant", "mfma", (136, 48, 40, 33, 1), (BF,)),
    ("circulant", "simt", (256, 64, 64, 129, 2), (F32,)), ("circulant", "simt", (30, 12, 6, 7, 1), (BF,)),
    ("circulant", "f64", (256, 64, 64, 129, 2), (F64T,)), ("circulant", "f64", (30, 12, 6, 7, 1), (F64T,)),
]
PARAMS = [pytest.param(entry, route, shape, dt, name, id=f"{entry}-{route}-{'-'.join(map(str, shape))}-{dt}-{name}")
          for entry, route, shape, dts in ROUTES for dt in dts for name in C.FAMILIES]


@pytest.fixture(scope="module")
def fa():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    L = fa_hip.lib()
    i64, ci, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    L.fa_debug_dense_bwd_plan.restype = ci
    L.fa_debug_dense_bwd_plan.argtypes = [ci] + [i64] * 5 + [ci] * 6 + [sz, ci, ctypes.POINTER(i64)]
    L.fa_debug_set_bwd_hoff.restype = ci
    L.fa_debug_set_bwd_hoff.argtypes = [ci]
    return fa_hip


@contextlib.contextmanager
def knobs(L, **kw):
    """fa_debug_set_<name>(value) for every keyword, restored on the way out."""
    old = {}
    try:
        for name, v in kw.items():
            old[name] = getattr(L, "fa_debug_set_" + name)(v)
        yield
    finally:
        for name, v in old.items():
            getattr(L, "fa_debug_set_" + name)(v)


def _np(t):
    return t.detach().double().cpu().numpy()


def _geometry(entry, shape):
    """(N, Nk, d, dv, B, W, mask) of a ROUTES shape."""
    if entry == "circulant":
        N, d, dv, W, B = shape
        return N, N, d, dv, B, W, C.band_mask(N, W)
    N, Nk, d, dv, B = shape
    return N, Nk, d, dv, B, None, (C.causal_mask(N, Nk) if entry == "causal" else None)


@functools.lru_cache(maxsize=None)
def case(entry, shape, dtype, name):
    """Inputs, scale and e_ref of a case (shared between routes, never modified)."""
    N, Nk, d, dv, B, W, mask = _geometry(entry, shape)
    q, k, v, do, scale = C.family(name, N, Nk, d, dv, B, dtype, mask=mask)
    eref = None if dtype == F64T else C.e_ref(q, k, v, do, scale, dtype, mask)
    return q, k, v, do, scale, eref


def device_run(fa, entry, route, shape, dtype, q, k, v, do, scale):
    """Forward + backward on the device under the route's knobs.  Returns the tensors; asserts
    the route."""
    L = fa.lib()
    N, Nk, d, dv, B, W, _ = _geometry(entry, shape)
    code = fa.DTYPES[DT[dtype]]
    Q, K, V, dO = (fa.jl_tensor(a, DT[dtype]) for a in (q, k, v, do))
    if entry == "circulant":
        Oo, l, m = fa.circulant_fa(Q, K, V, W, scale)
        g = fa.circulant_fa_backward(Q, K, V, Oo, dO, l, m, W, scale)
        kind = L.fa_debug_last_circ_bwd_kernel()
        torch.cuda.synchronize()
        assert kind == {"mfma": CIRC_MFMA, "simt": CIRC_SIMT, "f64": CIRC_F64}[route], (route, kind)
        return Oo, l, m, g
    causal = entry == "causal"
    kn, kernel, padded, status = DENSE_ROUTES[route]
    kn = dict(kn)
    if kn.get("bwd_mode") == 2:
        # the single pass needs hoff * ceil(Nk / 256) <= ceil(N / 64) (csrc/fa_dense_plan.h): the
        # default step offset 3 where it fits, else the largest that does (2 at (256, 512))
        kn["bwd_hoff"] = min(3, -(-N // 64) // -(-Nk // 256))
        assert kn["bwd_hoff"] >= 1
    fwd, bwd = (fa.causal_fa, fa.causal_fa_backward) if causal else (fa.dense_fa, fa.dense_fa_backward)
    Oo, l, m = fwd(Q, K, V, scale)
    with knobs(L, **kn):
        nws = (L.fa_causal_bwd_workspace if causal else L.fa_dense_bwd_workspace)(code, N, Nk, d, dv, B)
        g = bwd(Q, K, V, Oo, dO, l, m, scale)
        torch.cuda.synchronize()
        if status is not None:
            assert fa.backward_handoff_status() == status, (route, fa.backward_handoff_status())
    out = (ctypes.c_int64 * 25)()
    cus = torch.cuda.get_device_properties(Q.device).multi_processor_count
    aligned = int(all(t.data_ptr() % 16 == 0 for t in (Q, K, V, dO)))
    got = L.fa_debug_dense_bwd_plan(code, N, Nk, d, dv, B, int(causal), kn.get("bwd_generic", 0), kn.get("bwd_mode", 0),
                                    kn.get("bwd_hoff", 3), -1, aligned, nws, cus, out)
    assert (got, out[0]) == (kernel, padded), f"{entry} {route}: plan kernel {got}, padded {out[0]}"
    return Oo, l, m, g


def reference(entry, shape, dtype, q, k, v, do, scale, Oo, l, m):
    N, Nk, d, dv, B, W, _ = _geometry(entry, shape)
    f64 = dtype == F64T
    if entry == "dense":
        if f64:
            _, l, m = O.dense_fa3(q, k, v, scale=scale)
        return O.dense_fa_backward(q, k, v, Oo, do, l, m, scale=scale)
    if entry == "causal":
        return causal_bwd_ref(q, k, v, Oo, do, None if f64 else l, None if f64 else m, scale)
    return circulant_bwd_ref(q, k, v, Oo, do, None if f64 else l, None if f64 else m, W, scale)


def check_grads(got, ref, dtype, eref, tag):
    """The two metrics within max(GTOL, 2 e_ref); Float64 elementwise 1e-12.  Prints the COND line."""
    worst = 0.0
    for x, y, nm in zip(got, ref, ("dQ", "dK", "dV")):
        x = _np(x) if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)
        assert x.shape == y.shape and np.all(np.isfinite(x)), f"{tag} {nm}: shape or non-finite values"
        if dtype == F64T:
            worst = max(worst, np.abs(x - y).max() / max(np.abs(y).max(), 1.0))
        else:
            worst = max(worst, *C.grad_metrics(x, y))
    bud = ELEM64 if dtype == F64T else C.budget(dtype, eref)
    print(f"COND {tag} e_ref {0.0 if eref is None else eref:.2e} device {worst:.2e} budget {bud:.2e} ratio {worst / bud:.3f}")
    assert worst <= bud, f"{tag}: device error {worst:.3e} > budget {bud:.3e}"


@pytest.mark.parametrize("entry,route,shape,dtype,name", PARAMS)
def test_backward_route_under_family(fa, entry, route, shape, dtype, name):
    q, k, v, do, scale, eref = case(entry, shape, dtype, name)
    Oo, l, m, g = device_run(fa, entry, route, shape, dtype, q, k, v, do, scale)
    # the forward's statistics under the family's scale (the backward reads them)
    N, Nk, d, dv, B, W, mask = _geometry(entry, shape)
    _, lr, mr = C.forward_f64(q, k, v, scale, mask)
    lm_dt = F32 if dtype == F64T else dtype      # l, m leave every kernel as float32
    assert_lm_close(_np(m), mr, lm_dt, "m")
    # l at conftest's rule where float32 scores allow it (cond_inputs.l_rtol)
    l_rtol = C.l_rtol(mr, lm_dt)
    l_err = (np.abs(_np(l) - lr) / (1 + np.abs(lr))).max()
    assert l_err <= l_rtol, f"l: rel err {l_err:.3e} > {l_rtol:.1e}"
    ref = reference(entry, shape, dtype, q, k, v, do, scale, _np(Oo), _np(l), _np(m))
    check_grads(g, ref, dtype, eref, f"{entry}/{route} {'-'.join(map(str, shape))} {dtype} {name}")


def test_every_route_gets_every_family():
    """The table above: each (entry, route) of the issue's list is there, under all five families."""
    have = {(e, r) for e, r, _, _ in ROUTES}
    assert have == {("dense", r) for r in DENSE_ROUTES} | {("causal", r) for r in ("twopass", "padded", "generic", "f32mfma", "f64")} \
        | {("circulant", r) for r in ("mfma", "simt", "f64")}
    assert {p.values[4] for p in PARAMS} == set(C.FAMILIES)
    assert max(s[0] for _, _, s, _ in ROUTES) <= 520


SMALL = (256, 256, 64, 64, 2)


@pytest.mark.parametrize("entry", ["dense", "causal", "circulant"])
def test_nonpositive_scale_is_the_default(fa, entry):
    """scale <= 0 means 1/sqrt(d): scale = -1 gives the bits of scale = 0, forward (causal,
    circulant; the dense forward has its own tests) and backward."""
    shape = (256, 64, 64, 129, 2) if entry == "circulant" else SMALL
    q, k, v, do, _, _ = case(entry, shape, BF, "hotkeys")
    Q, K, V, dO = (fa.jl_tensor(a, torch.bfloat16) for a in (q, k, v, do))
    outs = []
    for s in (0.0, -1.0):
        if entry == "dense":
            Oo, l, m = fa.dense_fa(Q, K, V)
            g = fa.dense_fa_backward(Q, K, V, Oo, dO, l, m, s)
        elif entry == "causal":
            Oo, l, m = fa.causal_fa(Q, K, V, s)
            g = fa.causal_fa_backward(Q, K, V, Oo, dO, l, m, s)
        else:
            Oo, l, m = fa.circulant_fa(Q, K, V, 129, s)
            g = fa.circulant_fa_backward(Q, K, V, Oo, dO, l, m, 129, s)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (Oo, l, m, *g)])
    for a, b, nm in zip(outs[0], outs[1], ("O", "l", "m", "dQ", "dK", "dV")):
        assert torch.equal(a, b), f"{entry} {nm}: scale -1 differs from scale 0"


@pytest.mark.parametrize("name", ["hot", "offset"])
def test_routes_agree_under_family(fa, name):
    """(512, 512, 64, 64, 2) bf16: single pass vs two passes, fast vs generic, within GTOL on
    both metrics (the check test_backward_single_pass / test_backward_fast_matches_generic make
    on N(0, 1) inputs)."""
    shape = MFMA3[0]
    q, k, v, do, scale, _ = case("dense", shape, BF, name)
    two = device_run(fa, "dense", "twopass", shape, BF, q, k, v, do, scale)[3]
    one = device_run(fa, "dense", "single", shape, BF, q, k, v, do, scale)[3]
    # the generic route at this (fast) shape: forced, the plan says so
    L = fa.lib()
    Q, K, V, dO = (fa.jl_tensor(a, torch.bfloat16) for a in (q, k, v, do))
    Oo, l, m = fa.dense_fa(Q, K, V, scale)
    with knobs(L, bwd_generic=1):
        gen = fa.dense_fa_backward(Q, K, V, Oo, dO, l, m, scale)
        torch.cuda.synchronize()
    for pair, what in (((one, two), "single vs two-pass"), ((two, gen), "fast vs generic")):
        for a, b, nm in zip(*pair, ("dQ", "dK", "dV")):
            err, rel = C.grad_metrics(_np(a), _np(b))
            print(f"{name} {what} {nm}: max err/max|y| {err:.2e}, norm rel {rel:.2e}")
            assert err <= C.GTOL[BF] and rel <= C.GTOL[BF], f"{name} {what} {nm}: {err:.2e}, {rel:.2e}"
