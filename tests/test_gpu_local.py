"""GPU tests of local (sliding-window) attention (fa_local_fwd / fa_local_bwd through
fa_hip.local_fa, local_fa_backward, local_dpa) against the float64 yardstick tests/local_ref.py
on bf16-representable inputs seeded per shape.

Tolerances are the project's existing ones, as test_gpu_causal.py restates them:
  * forward: conftest.assert_close and its l, m rule (1e-5 fp32 / 1e-4 16-bit); Float64
    1e-12 relative to max(|y|, 1);
  * backward: max|x-y| / max|y| and ||x-y|| / ||y|| (each floored at 1e-2) within
    GTOL = 2e-5 / 2e-2 / 5e-3 for fp32 / bf16 / fp16, and 1e-12 for Float64, whose device path
    recomputes the row statistics in double, so its reference does too (l = m = None).
The backward reference is evaluated on the device's own O, l, m.  Every shape is the smallest
that reaches what CASES says it reaches."""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from conftest import assert_close, assert_lm_close
from local_ref import local_bwd_ref, local_fwd_ref, unseen_keys, visible

pytestmark = pytest.mark.gpu
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16, "float64": torch.float64}
GTOL = {"float32": 2e-5, "bfloat16": 2e-2, "float16": 5e-3}
ELEM64 = 1e-12

BF, F16, F32, F64T = "bfloat16", "float16", "float32", "float64"
BIG = 1 << 40
# (N, Nk, d, dv, B; left, right), dtypes, what it reaches
CASES = [
    ((1024, 1024, 64, 64, 2, 100, 0), (BF, F16, F32, F64T)),  # two 512-row workgroups, jt0 > 0 in the second; left edge mid-fragment; 392 rows hidden whole in their wave's first tile
    ((1024, 1024, 64, 64, 2, 63, 64), (BF, F16)),              # two-sided band; right edge one tile past the diagonal tile; jt1 clipped at NT
    ((512, 576, 64, 64, 1, 128, 0), (BF, F16)),                # off = 64, both edges tile-aligned; odd tile count
    ((256, 296, 64, 64, 2, 23, 17), (BF,)),                    # off and off - left not multiples of 8
    ((520, 520, 64, 64, 1, 200, 0), (BF, F16)),                # _wide with a ragged last tile: three masks can meet
    ((500, 500, 64, 64, 1, 70, 5), (BF, F32)),                 # Nk % 8 != 0: padded forward and backward, window from the real extents
    ((200, 333, 48, 40, 2, 50, 20), (BF, F32, F64T)),          # head dims inside a class, ragged both ways; 83 keys nobody sees
    ((512, 512, 128, 128, 1, 96, 32), (BF, F16)),              # d = 128 class, 256-row workgroups, backward register budget
    ((384, 384, 32, 32, 2, 31, 0), (BF,)),                     # d = 32 class
    ((8, 1000, 64, 64, 2, 100, 0), (BF, F32)),                 # decode-like: 892 unseen keys, dK/dV blocks with an empty query range, forward jt0 = 13
    ((128, 640, 128, 128, 1, 64, 0), (BF,)),                   # the same at d = 128 with off - left tile-aligned (448 unseen keys)
    ((64, 64, 64, 64, 1, 0, 0), (BF, F32)),                    # one key per query
    ((5, 5, 8, 8, 1, 2, 1), (BF, F32, F64T)),                  # degenerate
    ((1, 1, 16, 8, 3, 0, 0), (BF, F32, F64T)),
    ((256, 296, 64, 64, 2, BIG, BIG), (BF,)),                  # clamping; equals dense within tolerance
]
ident = lambda case: "-".join("2p40" if x == BIG else str(x) for x in case)
PARAMS = [pytest.param(case, dt, id=ident(case) + "-" + dt) for case, dts in CASES for dt in dts]
# the cases with keys that no query sees (j < off - left), and how many
UNSEEN = {(200, 333, 48, 40, 2, 50, 20): 83, (8, 1000, 64, 64, 2, 100, 0): 892, (128, 640, 128, 128, 1, 64, 0): 448,
          (256, 296, 64, 64, 2, 23, 17): 17}


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
def fwd_ref(case, scale=0.0):
    q, k, v, _ = inputs(*case[:5])
    return local_fwd_ref(q, k, v, case[5], case[6], scale)


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


def device_run(fa, case, dtype, scale=0.0, kv=None, backward=True):
    """Forward (+ backward) on the device.  kv: replaces the (k, v) float64 inputs."""
    left, right = case[5:]
    q, k, v, do = inputs(*case[:5])
    if kv is not None:
        k, v = kv
    Q, K, V, dO = (fa.jl_tensor(a, DT[dtype]) for a in (q, k, v, do))
    Oo, l, m = fa.local_fa(Q, K, V, left, right, scale)
    r = dict(Q=Q, K=K, V=V, dO=dO, O=Oo, l=l, m=m)
    if backward:
        r["dQ"], r["dK"], r["dV"] = fa.local_fa_backward(Q, K, V, Oo, dO, l, m, left, right, scale)
    torch.cuda.synchronize()
    return r


def check_bwd_vs_ref(r, case, dtype, scale=0.0):
    q, k, v, do = inputs(*case[:5])
    f64 = dtype == "float64"
    ref = local_bwd_ref(q, k, v, _np(r["O"]), do, None if f64 else _np(r["l"]), None if f64 else _np(r["m"]),
                        case[5], case[6], scale)
    for nm, y in zip(("dQ", "dK", "dV"), ref):
        assert_grad_close(_np(r[nm]), y, dtype, nm)


def test_the_table_reaches_what_it_says():
    """The masks of the table, on the CPU: every row sees a key; the counts of unseen keys; the
    rows hidden whole in their wave's first computed tile (64 rows per wave at d <= 64)."""
    for case, _ in CASES:
        N, Nk, _, _, _, left, right = case
        vis = visible(0, N, 0, Nk, Nk - N, -1 if left >= Nk else left, -1 if right >= Nk else right)
        assert vis.any(axis=1).all(), case
        assert (~vis.any(axis=0)).sum() == UNSEEN.get(case, 0) == unseen_keys(N, Nk, left, right).sum(), case
    N, Nk, left = 1024, 1024, 100
    vis = visible(0, N, 0, Nk, 0, left, 0)
    hidden = 0
    for w0 in range(0, N, 64):                       # a wave's 64 rows
        first = max(0, w0 - left) // 64              # its first computed tile
        hidden += int((~vis[w0:w0 + 64, first * 64:first * 64 + 64].any(axis=1)).sum())
    assert hidden == 392


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_forward_and_backward_vs_reference(fa, case, dtype):
    r = device_run(fa, case, dtype)
    assert fa.lib().fa_debug_fwd_last_path() != 30
    assert_fwd_close(r, fwd_ref(case), dtype)
    check_bwd_vs_ref(r, case, dtype)


@pytest.mark.parametrize("case,dtype", [(c, dt) for c in UNSEEN for dt in dict(CASES)[c]],
                         ids=lambda x: ident(x) if isinstance(x, tuple) else x)
def test_unseen_keys_get_exact_zero_gradients(fa, case, dtype):
    """dK, dV filled with NaN before the raw-ABI call: the rows of keys that no query sees are
    bitwise 0 afterwards and nothing is left unwritten."""
    N, Nk, d, dv, B, left, right = case
    r = device_run(fa, case, dtype, backward=False)
    L = fa.lib()
    code = fa.DTYPES[DT[dtype]]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dQ, dK, dV = (fa.jl_empty(s, DT[dtype]).fill_(float("nan")) for s in ((N, d, B), (Nk, d, B), (Nk, dv, B)))
    nwb = L.fa_local_bwd_workspace(code, N, Nk, d, dv, B)
    wb = torch.empty(nwb, dtype=torch.uint8, device="cuda")
    rc = L.fa_local_bwd(code, P(r["Q"]), P(r["K"]), P(r["V"]), P(r["O"]), P(r["dO"]), P(r["l"]), P(r["m"]),
                        P(dQ), P(dK), P(dV), N, Nk, d, dv, B, left, right, 0.0, P(wb), nwb, stream)
    assert rc == 0, L.fa_last_error()
    torch.cuda.synchronize()
    un = torch.tensor(unseen_keys(N, Nk, left, right), device="cuda")
    assert int(un.sum()) == UNSEEN[case]
    for nm, t in (("dQ", dQ), ("dK", dK), ("dV", dV)):
        assert bool(torch.isfinite(t).all()), nm + " not fully written"
    for nm, t in (("dK", dK), ("dV", dV)):
        rows = t[un]
        bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[rows.element_size()]
        assert int(torch.count_nonzero(rows.contiguous().view(bits))) == 0, nm
        assert int(torch.count_nonzero(t[~un])) > 0, nm


@pytest.mark.parametrize("case,dtype", [((64, 64, 64, 64, 1, 0, 0), BF), ((64, 64, 64, 64, 1, 0, 0), F32),
                                        ((1, 1, 16, 8, 3, 0, 0), BF), ((1, 1, 16, 8, 3, 0, 0), F32),
                                        ((1, 1, 16, 8, 3, 0, 0), F64T), ((8, 1000, 64, 64, 2, 0, 0), BF)],
                         ids=lambda x: ident(x) if isinstance(x, tuple) else x)
def test_one_key_per_query(fa, case, dtype):
    """(0, 0): O = V[off:] bitwise, l = 1, m = tau q_i.k_{i+off}; dV[off:] = dO, dQ = dK = 0."""
    N, Nk, d, dv, B, _, _ = case
    off = Nk - N
    q, k, v, do = inputs(*case[:5])
    r = device_run(fa, case, dtype)
    assert torch.equal(r["O"], r["V"][off:])
    assert bool((r["l"] == 1.0).all())
    mref = (q * k[off:]).sum(axis=1, keepdims=True) / math.sqrt(d)
    assert_lm_close(_np(r["m"]), mref, F32 if dtype == F64T else dtype, "m")
    assert_grad_close(_np(r["dV"][off:]), do, dtype, "dV[off:]")
    assert int(torch.count_nonzero(r["dV"][:off])) == 0
    assert_grad_close(_np(r["dQ"]), np.zeros((N, d, B)), dtype, "dQ")
    assert_grad_close(_np(r["dK"]), np.zeros((Nk, d, B)), dtype, "dK")


LEAK = [((1024, 1024, 64, 64, 2, 100, 0), (515, 650)), ((256, 296, 64, 64, 2, 23, 17), (70, 139)),
        ((512, 512, 128, 128, 1, 96, 32), (130, 301))]


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("case,rows", LEAK, ids=[ident(c) for c, _ in LEAK])
def test_nothing_leaks_from_outside_the_window(fa, case, rows, dtype):
    """K and V overwritten with +-3e4 at every key outside the union of the windows of the rows
    [a, b) (not tile-aligned), on both sides: O, l, m and dQ of those rows are bitwise unchanged.
    A single leaked key would dominate the softmax."""
    N, Nk, d, dv, B, left, right = case
    a, b = rows
    off = Nk - N
    q, k, v, do = inputs(*case[:5])
    base = device_run(fa, case, dtype)
    lo, hi = max(0, a + off - left), min(Nk - 1, b - 1 + off + right)      # the union of the rows' windows
    outside = np.ones(Nk, dtype=bool)
    outside[lo:hi + 1] = False
    assert outside[:lo].any() and outside[hi + 1:].any() and lo % 64 and (hi + 1) % 64
    sign = np.where(np.arange(Nk) % 2 == 0, 1.0, -1.0)[:, None, None]
    k2, v2 = k.copy(), v.copy()
    k2[outside] = (3e4 * sign * np.ones_like(k))[outside]
    v2[outside] = (-3e4 * sign * np.ones_like(v))[outside]
    pert = device_run(fa, case, dtype, kv=(k2, v2))
    for nm in ("O", "l", "m", "dQ"):
        assert torch.equal(pert[nm][a:b], base[nm][a:b]), nm
    for nm in ("O", "l", "m", "dQ", "dK", "dV"):
        assert bool(torch.isfinite(pert[nm]).all()), nm


@pytest.mark.parametrize("shape,dtype", [((520, 520, 64, 64, 1), BF), ((200, 333, 48, 40, 2), F32)])
def test_matches_causal_and_dense(fa, shape, dtype):
    """(-1, 0) against causal_fa / causal_fa_backward, (-1, -1) against dense_fa /
    dense_fa_backward, within the forward and gradient tolerances (other kernels: not bitwise)."""
    for window, fwd, bwd in (((-1, 0), fa.causal_fa, fa.causal_fa_backward), ((-1, -1), fa.dense_fa, fa.dense_fa_backward)):
        r = device_run(fa, shape + window, dtype)
        Oo, l, m = fwd(r["Q"], r["K"], r["V"])
        g = bwd(r["Q"], r["K"], r["V"], Oo, r["dO"], l, m)
        torch.cuda.synchronize()
        assert_close(_np(r["O"]), _np(Oo), dtype, f"{window} O")
        assert_lm_close(_np(r["l"]), _np(l), dtype, f"{window} l")
        assert_lm_close(_np(r["m"]), _np(m), dtype, f"{window} m")
        for nm, x in zip(("dQ", "dK", "dV"), g):
            assert_grad_close(_np(r[nm]), _np(x), dtype, f"{window} {nm}")


def test_kernel_choice(fa):
    """Through fa_debug_local_fwd_plan / fa_debug_local_bwd_plan (fa_dense_plan.h's enumerators),
    with the facts of real tensors: aligned bf16 takes the tiled MFMA forward (never p4, never
    split, on a grid the dense plan splits) and bwd_dq_fast / bwd_dkdv_fast; Nk % 8 != 0 the
    padded fast path; fp32 and Float64 their own families.  The planned call then runs."""
    L = fa.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out, b = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 6)()

    def plans(dtype, N, Nk, d, dv, B):
        code = fa.DTYPES[DT[dtype]]
        nf, nb = L.fa_local_fwd_workspace(code, N, Nk, d, dv, B), L.fa_local_bwd_workspace(code, N, Nk, d, dv, B)
        return (L.fa_debug_local_fwd_plan(code, N, Nk, d, dv, B, 1, 1, nf, cus, out),
                L.fa_debug_local_bwd_plan(code, N, Nk, d, dv, B, 1, nb, cus, b))

    assert plans(BF, 2048, 2048, 64, 64, 1) == (6, 3) and out[0] == 1 and out[4] == 1 and out[2] == 0 and b[0] == 0
    dense = (ctypes.c_int64 * 17)()
    assert L.fa_debug_dense_fwd_plan(1, 2048, 2048, 64, 64, 1, 0, 0, 2, 1, 1, 1 << 40, cus, dense) in (7, 8)
    assert plans(BF, 512, 512, 128, 128, 1) == (4, 3)
    assert plans(BF, 500, 500, 64, 64, 1) == (5, 3) and out[2] == 1 and b[0] == 1
    assert plans(F32, 500, 500, 64, 64, 1) == (1, 2)
    assert plans(F64T, 200, 333, 48, 40, 2) == (2, 0)
    case = (2048, 2048, 64, 64, 1, 100, 0)
    r = device_run(fa, case, BF)
    assert L.fa_debug_fwd_last_path() != 30 and fa.backward_handoff_status() == -1
    assert_fwd_close(r, fwd_ref(case), BF)
    check_bwd_vs_ref(r, case, BF)


@pytest.mark.parametrize("case,dtype", [((1024, 1024, 64, 64, 2, 100, 0), BF), ((200, 333, 48, 40, 2, 50, 20), F32)],
                         ids=lambda x: ident(x) if isinstance(x, tuple) else x)
def test_bitwise_deterministic(fa, case, dtype):
    a = device_run(fa, case, dtype)
    b = device_run(fa, case, dtype)
    for nm in ("O", "l", "m", "dQ", "dK", "dV"):
        assert torch.equal(a[nm], b[nm]), nm


@pytest.mark.parametrize("case,dtype", [((520, 520, 64, 64, 1, 200, 0), BF), ((200, 333, 48, 40, 2, 50, 20), F32)],
                         ids=lambda x: ident(x) if isinstance(x, tuple) else x)
def test_raw_abi_workspace_at_an_odd_address(fa, case, dtype):
    """Sentinel-filled outputs are overwritten everywhere, bitwise the mirror's result, with
    both workspaces starting at an odd address; the hand-off status reads -1."""
    N, Nk, d, dv, B, left, right = case
    r = device_run(fa, case, dtype)
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
    nws = L.fa_local_fwd_workspace(code, N, Nk, d, dv, B)
    ws = odd_ws(nws)
    rc = L.fa_local_fwd(code, P(r["Q"]), P(r["K"]), P(r["V"]), P(Oo), P(l), P(m), N, Nk, d, dv, B, left, right, 0.0,
                        P(ws), nws, stream)
    assert rc == 0, L.fa_last_error()
    outs = [fa.jl_empty(r[nm].shape, DT[dtype]).fill_(777.0) for nm in ("dQ", "dK", "dV")]
    nwb = L.fa_local_bwd_workspace(code, N, Nk, d, dv, B)
    wb = odd_ws(nwb)
    rc = L.fa_local_bwd(code, P(r["Q"]), P(r["K"]), P(r["V"]), P(Oo), P(r["dO"]), P(l), P(m),
                        P(outs[0]), P(outs[1]), P(outs[2]), N, Nk, d, dv, B, left, right, 0.0, P(wb), nwb, stream)
    assert rc == 0, L.fa_last_error()
    torch.cuda.synchronize()
    for nm, t in zip(("O", "l", "m", "dQ", "dK", "dV"), [Oo, l, m] + outs):
        assert torch.equal(t, r[nm]), nm
    st = ctypes.c_int(-2)
    assert L.fa_dense_bwd_handoff_status(P(wb), nwb, stream, ctypes.byref(st)) == 0 and st.value == -1


@pytest.mark.parametrize("case,dtype", [((512, 576, 64, 64, 1, 128, 0), BF), ((200, 333, 48, 40, 2, 50, 20), F32)],
                         ids=lambda x: ident(x) if isinstance(x, tuple) else x)
def test_explicit_scale(fa, case, dtype):
    r = device_run(fa, case, dtype, scale=0.05)
    assert_fwd_close(r, fwd_ref(case, 0.05), dtype)
    check_bwd_vs_ref(r, case, dtype, scale=0.05)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_local_dpa_against_local_fa(fa, dtype):
    case = (256, 296, 64, 64, 2, 23, 17)
    N, Nk, left, right = case[0], case[1], case[5], case[6]
    r = device_run(fa, case, dtype, backward=False)
    Od, P = fa.local_dpa(r["Q"], r["K"], r["V"], left, right)
    torch.cuda.synchronize()
    assert_close(_np(Od), _np(r["O"]), dtype, "local_dpa O vs local_fa O")
    assert_close(_np(Od), fwd_ref(case)[0], dtype, "local_dpa O")
    hidden = torch.tensor(~visible(0, N, 0, Nk, Nk - N, left, right), device="cuda")
    assert int(torch.count_nonzero(P[hidden])) == 0
    assert torch.allclose(P.float().sum(1), torch.ones((N, case[4]), device="cuda"), atol=2e-2)
