"""GPU parity of the windowed forward and backward kernels, each forced in turn
(fa_debug_set_win_composed), under explicit scales and ill-conditioned scores: the five input
families of tests/cond_inputs.py on two geometries whose edge windows hang over the image, so
that zero-padded keys (score 0) take part in the softmax.  Under `offset` the real scores are
near +9 sqrt(d) and the pad keys weigh e^-70: edge windows behave like interior ones.  Under
`anti` the real scores are near -9 sqrt(d) and the pad keys carry almost all the weight of an
edge window: y there is about 0 and finite, its gradients are at the floor, and NaN appears
only where no window covers a pixel.  `hot` and `cold` pass an explicit scale, which no other
windowed test does.

Forward: y, l, m against oracle.windowed_fa(scale=...) under conftest's assert_close /
assert_lm_close.  Backward: dq, dk, dv against oracle.windowed_fa_backward(scale=...) on the two
metrics of assert_grad_close (floor 1e-2) within max(GTOL, 2 e_ref); e_ref is cond_inputs'
lowp_backward against float64, window by window through oracle.window / unwindow (no device
value enters it).  Float64: 1e-12.  The kernel that ran is the fa_debug_win_*_plan answer for
the forced mode, asserted per case; each backward prints a COND line."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import cond_inputs as C
from conftest import assert_close, assert_lm_close
from oracle import fa_oracle as O

pytestmark = pytest.mark.gpu
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float64": torch.float64}
BF, F32, F64T = "bfloat16", "float32", "float64"
ELEM64 = 1e-12

GEOMS = [(32, 20, 7, 7, 3), (16, 16, 3, 3, 1)]   # (W, H, ws, stride, pad); the first leaves rows 18, 19 uncovered
DIMS = [(64, 64), (20, 48), (128, 128)]
B = 2
# fa::WinFwdKernel / fa::WinBwdKernel (csrc/fa_windowed.h)
(F_COMPOSED, F_FUSED, F_FUSED_WS, F_ROWS, F_ROWS1, F_SHIFT1, F_SHIFT2, F_SHIFT3, F_SHIFT128, F_STRIP, F_F32) = range(11)
B_COMPOSED, B_ROWS1, B_ROWS2, B_ROWS128, B_STRIP, B_STRIP_PARTIAL, B_F32 = range(7)
# (forward mode, backward mode) run together in one case
PAIRS = [(1, 1), (3, 3), (6, 0), (10, 10)]
gid = lambda g: "W{}H{}ws{}s{}p{}".format(*g)


def fwd_kernel(dtype, d, dv, mode):
    """The kernel a forced mode must reach on GEOMS (2-D, stride == ws <= 7, width % 8 == 0)."""
    wide = max(d, dv) > 64
    if mode == 1 or dtype == F64T:
        return {F_COMPOSED}
    if dtype == F32:
        return {F_COMPOSED if wide else F_F32}
    return {F_SHIFT128} if wide else {{3: F_SHIFT1, 6: F_SHIFT2, 10: F_STRIP}[mode]}


def bwd_kernel(dtype, d, dv, mode):
    wide = max(d, dv) > 64
    if mode == 1 or dtype == F64T:
        return {B_COMPOSED}
    if dtype == F32:
        return {B_COMPOSED if wide else B_F32}
    # 30 and 72 windows: two per workgroup in auto mode; the strip kernel in either store form
    return {B_ROWS128} if wide else {0: {B_ROWS2}, 3: {B_ROWS1}, 10: {B_STRIP, B_STRIP_PARTIAL}}[mode]


@pytest.fixture(scope="module")
def fa():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    L = fa_hip.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    geom = [ci, ci, ctypes.POINTER(i64), i64, i64, i64, i64, i64, i64]
    L.fa_debug_win_fwd_plan.restype = ci
    L.fa_debug_win_fwd_plan.argtypes = geom + [ci, ci, ci]
    L.fa_debug_win_bwd_plan.restype = ci
    L.fa_debug_win_bwd_plan.argtypes = geom + [ci, ci, ci, ci]
    return fa_hip


def _np(t):
    return t.detach().double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def same_window(geom):
    """(P, P) bool over the column-major flattened pixels: i and j lie in one window."""
    W, H, ws, st, pad = geom
    idx = O.window_index((W, H), ws, st, pad)
    mk = np.zeros((W * H, W * H), dtype=bool)
    for w in range(idx.shape[1]):
        pix = idx[:, w][idx[:, w] >= 0]
        mk[np.ix_(pix, pix)] = True
    return mk


@functools.lru_cache(maxsize=None)
def case(geom, d, dv, dtype, name):
    """Inputs (W, H, d | dv, B), scale, the oracle's forward and backward, e_ref (shared, never
    modified)."""
    W, H, ws, st, pad = geom
    P = W * H
    # the hot (query, key) pairs share a window (hot_pairs' keys lie in covered image rows)
    q, k, v, dy, scale = C.family(name, P, P, d, dv, B, dtype, mask=same_window(geom))
    q, k = (np.reshape(a, (W, H, d, B), order="F") for a in (q, k))
    v, dy = (np.reshape(a, (W, H, dv, B), order="F") for a in (v, dy))
    with np.errstate(invalid="ignore", divide="ignore"):
        fwd = O.windowed_fa(q, k, v, ws, st, pad, scale=scale)
        bwd = O.windowed_fa_backward(q, k, v, dy, ws, st, pad, scale=scale)
    eref = None if dtype == F64T else windowed_e_ref(q, k, v, dy, geom, scale, dtype, bwd)
    return q, k, v, dy, scale, fwd, bwd, eref


def windowed_e_ref(q, k, v, dy, geom, scale, dtype, ref):
    """cond_inputs.e_ref for the windowed chain rule: lowp_backward window by window (zero pad
    keys included, as in the kernels), folded, against the float64 windowed backward."""
    W, H, ws, st, pad = geom
    d, dv = q.shape[2], v.shape[2]
    r = lambda a: np.reshape(a, (a.shape[0], a.shape[1], -1), order="F")
    qw, kw, vw = (r(O.window(a, ws, st, pad)) for a in (q, k, v))
    div = O.coverage((W, H), ws, st, pad)
    with np.errstate(invalid="ignore", divide="ignore"):
        dyw = r(O.window(dy / div.reshape(div.shape + (1, 1)), ws, st, pad))
    o, l, m = C.forward_f64(qw, kw, vw, scale)
    o = C.round_to(o, dtype) if dtype == BF else o.astype(np.float32).astype(np.float64)
    l, m = l.astype(np.float32), m.astype(np.float32)
    low = C.lowp_backward(qw, kw, vw, dyw, o, l, m, scale, C.ROUND16[dtype])
    T, Lw = qw.shape[0], qw.shape[2] // B
    worst = 0.0
    for g, y, c in zip(low, ref, (d, d, dv)):
        x = O.unwindow(np.reshape(g, (T, c, Lw, B), order="F"), (W, H, c, B), ws, st, pad)
        worst = max(worst, *C.grad_metrics(x, y))
    return worst


def _plan_args(fa, geom, d, dv, dtype):
    W, H, ws, st, pad = geom
    return (fa.DTYPES[DT[dtype]], 2, (ctypes.c_int64 * 2)(W, H), d, dv, B, ws, st, pad)


def run_forward(fa, geom, d, dv, dtype, name, mode):
    W, H, ws, st, pad = geom
    q, k, v, dy, scale, (yr, lr, mr), _, _ = case(geom, d, dv, dtype, name)
    L = fa.lib()
    Q, K, V = (fa.jl_tensor(a, DT[dtype]) for a in (q, k, v))
    old = L.fa_debug_set_win_composed(mode)
    try:
        y, l, m = fa.windowed_fa(Q, K, V, ws, stride=st, pad=pad, scale=scale)
        torch.cuda.synchronize()
    finally:
        L.fa_debug_set_win_composed(old)
    al = lambda *ts: int(all(t.data_ptr() % 16 == 0 for t in ts))
    plan = L.fa_debug_win_fwd_plan(*_plan_args(fa, geom, d, dv, dtype), mode, al(Q, K, V), al(y))
    tag = f"fwd mode {mode} {gid(geom)} d {d} dv {dv} {dtype} {name}"
    assert plan in fwd_kernel(dtype, d, dv, mode), f"{tag}: plan {plan}"
    if dtype == F64T:
        yd, yy = _np(y), yr
        assert np.array_equal(np.isnan(yd), np.isnan(yy)), f"{tag}: NaN pattern"
        err = np.nanmax(np.abs(yd - yy)) / max(np.nanmax(np.abs(yy)), 1.0)
        assert err <= ELEM64, f"{tag}: y err {err:.3e}"
        assert_lm_close(_np(l), lr, F32, f"l ({tag})")
        assert_lm_close(_np(m), mr, F32, f"m ({tag})")
    else:
        # nan_ok: NaN exactly where the oracle has it, i.e. where no window covers a pixel
        assert_close(_np(y), yr, dtype, f"y ({tag})", nan_ok=True)
        assert_lm_close(_np(l), lr, dtype, f"l ({tag})")
        assert_lm_close(_np(m), mr, dtype, f"m ({tag})")
    return Q, K, V, y, l, m


def run_backward(fa, geom, d, dv, dtype, name, mode, fwd):
    W, H, ws, st, pad = geom
    q, k, v, dy, scale, _, ref, eref = case(geom, d, dv, dtype, name)
    L = fa.lib()
    Q, K, V, y, l, m = fwd
    DY = fa.jl_tensor(dy, DT[dtype])
    old = L.fa_debug_set_win_composed(mode)
    try:
        g = fa.windowed_fa_backward(Q, K, V, y, DY, l, m, ws, stride=st, pad=pad, scale=scale)
        torch.cuda.synchronize()
    finally:
        L.fa_debug_set_win_composed(old)
    al = lambda *ts: int(all(t.data_ptr() % 16 == 0 for t in ts))
    cus = torch.cuda.get_device_properties(Q.device).multi_processor_count
    plan = L.fa_debug_win_bwd_plan(*_plan_args(fa, geom, d, dv, dtype), mode, al(Q, K, V, y, DY), al(*g), cus)
    tag = f"windowed/bwd{mode} {gid(geom)} d {d} dv {dv} {dtype} {name}"
    assert plan in bwd_kernel(dtype, d, dv, mode), f"{tag}: plan {plan}"
    worst = 0.0
    for a, b_, nm in zip(g, ref, ("dq", "dk", "dv")):
        x = _np(a)
        assert x.shape == b_.shape and np.all(np.isfinite(x)), f"{tag} {nm}: shape or non-finite values"
        if dtype == F64T:
            worst = max(worst, np.abs(x - b_).max() / max(np.abs(b_).max(), 1.0))
        else:
            worst = max(worst, *C.grad_metrics(x, b_))
    bud = ELEM64 if dtype == F64T else C.budget(dtype, eref)
    print(f"COND {tag} e_ref {0.0 if eref is None else eref:.2e} device {worst:.2e} budget {bud:.2e} ratio {worst / bud:.3f}")
    assert worst <= bud, f"{tag}: device error {worst:.3e} > budget {bud:.3e}"


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"fwd{p[0]}-bwd{p[1]}")
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_windowed_bf16_paths_under_family(fa, geom, pair, name):
    for d, dv in DIMS:
        fwd = run_forward(fa, geom, d, dv, BF, name, pair[0])
        run_backward(fa, geom, d, dv, BF, name, pair[1], fwd)


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_windowed_f32_paths_under_family(fa, geom, mode, name):
    """fp32: the fused exact-f32 MFMA kernels (mode 0) and the composed path (1)."""
    for d, dv in DIMS[:2]:
        fwd = run_forward(fa, geom, d, dv, F32, name, mode)
        run_backward(fa, geom, d, dv, F32, name, mode, fwd)


@pytest.mark.parametrize("name", C.FAMILIES)
def test_windowed_f64_under_family(fa, name):
    """Float64 (the composed path under either mode) at 1e-12."""
    geom, (d, dv) = GEOMS[1], DIMS[1]
    for mode in (0, 1):
        fwd = run_forward(fa, geom, d, dv, F64T, name, mode)
        run_backward(fa, geom, d, dv, F64T, name, mode, fwd)


@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_anti_edge_windows_are_pad_dominated(geom):
    """What the `anti` family is there for, on the oracle: in every window with a pad key the
    pad keys hold all but e^-50 of the weight (m = 0, l = their number), so y is about 0 there."""
    q, k, v, dy, scale, (yr, lr, mr), _, _ = case(geom, 64, 64, BF, "anti")
    W, H, ws, st, pad = geom
    idx = O.window_index((W, H), ws, st, pad)                           # (T, L), -1: padding
    npad = (idx < 0).sum(axis=0)                                        # per window
    edge = npad > 0
    assert edge.any() and (~edge).any()
    assert np.all(mr[:, 0, edge] == 0.0) and np.all(mr[:, 0, ~edge] < -50.0)
    # a real query's l counts the pad keys; a pad query (q = 0) scores 0 on all ws^2 keys
    want = np.where(idx >= 0, npad[None, :], idx.shape[0])[:, edge]
    assert np.allclose(lr[:, 0, edge], want[:, :, None], rtol=0, atol=1e-15)


def test_windowed_nonpositive_scale_is_the_default(fa):
    """scale <= 0 means 1/sqrt(d): scale = -1 gives the bits of scale = 0, forward and backward."""
    geom = GEOMS[1]
    W, H, ws, st, pad = geom
    q, k, v, dy, _, _, _, _ = case(geom, 64, 64, BF, "hotkeys")
    Q, K, V, DY = (fa.jl_tensor(a, torch.bfloat16) for a in (q, k, v, dy))
    outs = []
    for s in (0.0, -1.0):
        y, l, m = fa.windowed_fa(Q, K, V, ws, stride=st, pad=pad, scale=s)
        g = fa.windowed_fa_backward(Q, K, V, y, DY, l, m, ws, stride=st, pad=pad, scale=s)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (y, l, m, *g)])
    for a, b_, nm in zip(outs[0], outs[1], ("y", "l", "m", "dq", "dk", "dv")):
        assert torch.equal(a, b_), f"{nm}: scale -1 differs from scale 0"
