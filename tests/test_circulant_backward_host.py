"""CPU tests of the circulant backward: the float64 yardstick (tests/circ_bwd_ref.py)
against the existing dense oracle and torch autograd, the C ABI's checks before any
launch (fa_circulant_bwd, fa_circulant_bwd_workspace) and the Python mirror's argument
validation.  No device is touched."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch

import fa_hip
from fa_hip import DimensionMismatch
from circ_bwd_ref import band_index, circulant_bwd_ref, circulant_fwd_ref
from oracle import fa_oracle as O


def _inputs(N, d, dv, B, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, d, B)), rng.standard_normal((N, d, B)),
            rng.standard_normal((N, dv, B)), rng.standard_normal((N, dv, B)))


# ---- the yardstick ----------------------------------------------------------------
@pytest.mark.parametrize("N,mult", [(24, 1), (24, 2), (25, 1)])
def test_ref_equals_dense_oracle_when_the_band_covers_every_key(N, mult):
    """W = N (2N): the band holds every key once (twice), so P, and with it every
    gradient, is the dense one."""
    q, k, v, do = _inputs(N, 8, 6, 2, N + mult)
    o, l, m = O.dense_fa3(q, k, v)
    dqr, dkr, dvr = O.dense_fa_backward(q, k, v, o, do, l, m)
    oc, lc, mc = circulant_fwd_ref(q, k, v, mult * N)
    assert np.abs(oc - o).max() <= 1e-13
    dq, dk, dv = circulant_bwd_ref(q, k, v, oc, do, lc, mc, mult * N)
    for a, b in ((dq, dqr), (dk, dkr), (dv, dvr)):
        assert np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1.0)


@pytest.mark.parametrize("N,W,scale", [(40, 7, 0.0), (24, 12, 0.0), (20, 29, 0.0), (16, 1, 0.0), (24, 48, 0.3)])
def test_ref_equals_torch_autograd_through_the_gather_form(N, W, scale):
    """W < N, even W, W > N with W no multiple of N, W = 1, an explicit scale."""
    d, dv, B = 8, 5, 2
    q, k, v, do = _inputs(N, d, dv, B, 100 * N + W)
    tau = scale if scale > 0 else 1.0 / math.sqrt(d)
    J = torch.as_tensor(band_index(N, W))
    Q, K, V = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    S = tau * torch.einsum("ifb,itfb->itb", Q, K[J])            # K[J]: (N, W, d, B)
    P = torch.softmax(S, dim=1)
    Ot = torch.einsum("itb,itcb->icb", P, V[J])
    Ot.backward(torch.tensor(do))
    o, l, m = circulant_fwd_ref(q, k, v, W, scale)
    assert np.abs(o - Ot.detach().numpy()).max() <= 1e-13
    dq, dk, dv_ = circulant_bwd_ref(q, k, v, o, do, l, m, W, scale)
    for a, t in ((dq, Q), (dk, K), (dv_, V)):
        b = t.grad.numpy()
        assert np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1.0)
    # l = m = None recomputes the statistics (the Float64 device path's contract)
    for a, b in zip(circulant_bwd_ref(q, k, v, o, do, None, None, W, scale), (dq, dk, dv_)):
        assert np.array_equal(a, b)


def test_ref_scatter_equals_np_add_at():
    """The helper's W indexed adds are the scatter-add over J, also with repeated keys."""
    N, W, d, dv = 20, 29, 8, 5
    q, k, v, do = _inputs(N, d, dv, 1, 9)
    o, l, m = circulant_fwd_ref(q, k, v, W)
    dq, dk, dv_ = circulant_bwd_ref(q, k, v, o, do, l, m, W)
    J, tau = band_index(N, W), 1.0 / math.sqrt(d)
    S = tau * np.einsum("if,itf->it", q[:, :, 0], k[J, :, 0])
    P = np.exp(S - m[:, 0]) / l[:, 0]
    dS = P * (np.einsum("ic,itc->it", do[:, :, 0], v[J, :, 0]) - (do[:, :, 0] * o[:, :, 0]).sum(1)[:, None])
    dk2, dv2 = np.zeros((N, d)), np.zeros((N, dv))
    np.add.at(dk2, J, tau * dS[:, :, None] * q[:, None, :, 0])
    np.add.at(dv2, J, P[:, :, None] * do[:, None, :, 0])
    assert np.abs(dk2 - dk[:, :, 0]).max() <= 1e-13 and np.abs(dv2 - dv_[:, :, 0]).max() <= 1e-13


def test_ref_band_of_one_key():
    """W = 1: P = 1, so dS = dP − D = 0 and dV = dO."""
    q, k, v, do = _inputs(16, 8, 4, 2, 5)
    o, l, m = circulant_fwd_ref(q, k, v, 1)
    dq, dk, dv = circulant_bwd_ref(q, k, v, o, do, l, m, 1)
    assert np.abs(dq).max() <= 1e-14 and np.abs(dk).max() <= 1e-14
    assert np.array_equal(dv, do)


# ---- the C ABI, before any launch ------------------------------------------------------
def _bwd(L, dtype, ptrs, N, d, dv, B, W, ws=None, nws=0):
    return L.fa_circulant_bwd(dtype, *ptrs, N, d, dv, B, W, 0.0, ws, nws, None)


def test_abi_rejections_carry_status_and_message():
    L = fa_hip.lib()
    P = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    ok10 = [P] * 10
    rc = _bwd(L, 9, ok10, 64, 32, 32, 1, 7)
    assert rc == fa_hip.FA_ERR_INVALID_ARG and b"dtype" in L.fa_last_error()
    rc = _bwd(L, 1, ok10, 64, 32, 32, 1, 0)
    assert rc == fa_hip.FA_ERR_INVALID_ARG and b"DimensionMismatch" in L.fa_last_error()
    assert b"window size" in L.fa_last_error()
    for N, d, dv, B in ((64, 0, 32, 1), (64, 32, 0, 1), (-1, 32, 32, 1), (64, 32, 32, -1)):
        rc = _bwd(L, 1, ok10, N, d, dv, B, 7)
        assert rc == fa_hip.FA_ERR_INVALID_ARG and b"DimensionMismatch" in L.fa_last_error()
    for i in range(10):   # Q K V O dO l m dQ dK dV
        ptrs = list(ok10)
        ptrs[i] = None
        rc = _bwd(L, 1, ptrs, 64, 32, 32, 1, 7, P, 1 << 20)
        assert rc == fa_hip.FA_ERR_INVALID_ARG and b"null" in L.fa_last_error(), i
    for d, dv in ((129, 32), (32, 129)):
        rc = _bwd(L, 1, ok10, 64, d, dv, 1, 7)
        assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"head dimension" in L.fa_last_error()
    rc = _bwd(L, 1, ok10, 1 << 30, 4, 4, 1, 7)          # 8 GiB slab
    assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"32-bit" in L.fa_last_error()
    rc = _bwd(L, 1, ok10, 64, 32, 32, 1, 1 << 31)       # band width
    assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"32-bit" in L.fa_last_error()


def test_abi_workspace_is_checked_before_any_launch():
    L = fa_hip.lib()
    P = ctypes.c_void_p(16)
    need = L.fa_circulant_bwd_workspace(1, 256, 64, 64, 2, 129)
    assert need > 0
    rc = _bwd(L, 1, [P] * 10, 256, 64, 64, 2, 129)
    assert rc == fa_hip.FA_ERR_WORKSPACE and b"fa_circulant_bwd_workspace" in L.fa_last_error()
    rc = _bwd(L, 1, [P] * 10, 256, 64, 64, 2, 129, P, need - 1)
    assert rc == fa_hip.FA_ERR_WORKSPACE


def test_abi_empty_inputs_are_a_noop_that_dereferences_nothing():
    L = fa_hip.lib()
    none10 = [None] * 10
    assert _bwd(L, 1, none10, 0, 32, 32, 1, 5) == 0
    assert _bwd(L, 1, none10, 64, 32, 32, 0, 5) == 0
    assert L.fa_last_error() == b""
    # ... but the band width is validated first, as in the forward
    assert _bwd(L, 1, none10, 0, 32, 32, 1, 0) == fa_hip.FA_ERR_INVALID_ARG


def test_abi_workspace_query_is_positive_and_monotone():
    L = fa_hip.lib()
    q = lambda dt, N, B: L.fa_circulant_bwd_workspace(dt, N, 64, 64, B, 129)
    assert 0 < q(1, 256, 1) < q(1, 4096, 1) < q(1, 4096, 8)
    assert q(1, 4096, 8) >= 2 * 4 * 4096 * 8 + 256            # two fp32 statistics + slack
    assert q(3, 4096, 8) >= 2 * 8 * 4096 * 8 + 256            # Float64: statistics in double
    assert q(9, 4096, 8) == 0                                 # bad dtype
    assert L.fa_circulant_bwd_workspace(1, 4096, 64, 64, 8, 0) == 0
    assert L.fa_abi_version() == 1


def test_debug_export_reports_no_launch_yet_on_a_fresh_thread():
    import threading
    L = fa_hip.lib()
    seen = []
    t = threading.Thread(target=lambda: seen.append(L.fa_debug_last_circ_bwd_kernel()))
    t.start()
    t.join()
    assert seen == [0]


# ---- the Python mirror ---------------------------------------------------------------
def jl(shape, dtype=torch.bfloat16):
    return fa_hip.jl_empty(shape, dtype, device="cpu")


def _good(N=16, d=8, dv=4, B=2):
    f = lambda s: jl(s, torch.float32)
    return dict(Q=jl((N, d, B)), K=jl((N, d, B)), V=jl((N, dv, B)), O=jl((N, dv, B)), dO=jl((N, dv, B)),
                l=f((N, 1, B)), m=f((N, 1, B)))


def _call(a, W=5):
    return fa_hip.circulant_fa_backward(a["Q"], a["K"], a["V"], a["O"], a["dO"], a["l"], a["m"], W)


def test_mirror_is_exported():
    assert "circulant_fa_backward" in fa_hip.__all__


def test_mirror_rejects_bad_shapes():
    N, d, dv, B = 16, 8, 4, 2
    f = lambda s: jl(s, torch.float32)
    bad = {"K": jl((N + 1, d, B)), "V": jl((N, dv, B + 1)), "O": jl((N, dv + 1, B)), "dO": jl((N - 1, dv, B)),
           "l": f((N, B, 1)), "m": f((N - 1, 1, B)), "Q": jl((N, d))}
    for name, t in bad.items():
        a = _good(N, d, dv, B)
        a[name] = t
        with pytest.raises(DimensionMismatch):
            _call(a)
    for W in (0, -3):
        with pytest.raises(DimensionMismatch, match="W"):
            _call(_good(), W)


def test_mirror_rejects_non_f32_stats():
    for bad in (torch.bfloat16, torch.float16, torch.float64):
        for name in ("l", "m"):
            a = _good()
            a[name] = jl(tuple(a[name].shape), bad)
            with pytest.raises(DimensionMismatch, match="float32"):
                _call(a)


def test_mirror_valid_call_stops_only_at_the_device_check():
    with pytest.raises(TypeError, match="ROCm device"):
        _call(_good())
    with pytest.raises(TypeError, match="ROCm device"):
        _call(_good(), W=40)   # W > N is valid
