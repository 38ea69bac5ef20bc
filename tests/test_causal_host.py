"""CPU tests of causal attention: the float64 yardstick (tests/causal_ref.py) against the
dense oracle on each query's visible prefix and against torch autograd through an explicitly
masked softmax, the C ABI's checks before any launch (fa_causal_fwd, fa_causal_bwd and their
workspace queries) and the Python mirror's argument validation.  No device is touched."""
from __future__ import annotations

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import fa_hip
from fa_hip import DimensionMismatch
from causal_ref import causal_bwd_ref, causal_fwd_ref
from conftest import ROOT
from oracle import fa_oracle as O

SYMBOLS = ("fa_causal_fwd", "fa_causal_fwd_workspace", "fa_causal_bwd", "fa_causal_bwd_workspace")


def _inputs(N, Nk, d, dv, B, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, d, B)), rng.standard_normal((Nk, d, B)),
            rng.standard_normal((Nk, dv, B)), rng.standard_normal((N, dv, B)))


# ---- the yardstick ----------------------------------------------------------------
@pytest.mark.parametrize("N,Nk", [(24, 24), (17, 30), (1, 9)])
def test_ref_row_equals_dense_oracle_on_the_visible_prefix(N, Nk):
    """Row i is dense attention of q[i] over the keys 0 .. i + off."""
    q, k, v, _ = _inputs(N, Nk, 8, 6, 2, 7 * N + Nk)
    off = Nk - N
    o, l, m = causal_fwd_ref(q, k, v)
    for i in range(N):
        oi, li, mi = O.dense_fa3(q[i:i + 1], k[:i + off + 1], v[:i + off + 1])
        assert np.abs(o[i:i + 1] - oi).max() <= 1e-13
        assert np.abs(l[i:i + 1] - li).max() <= 1e-13 * max(np.abs(li).max(), 1.0)
        assert np.abs(m[i:i + 1] - mi).max() <= 1e-13 * max(np.abs(mi).max(), 1.0)


@pytest.mark.parametrize("N,Nk,scale", [(24, 24, 0.0), (20, 33, 0.0), (1, 6, 0.0), (16, 21, 0.3)])
def test_ref_equals_torch_autograd_through_a_masked_softmax(N, Nk, scale):
    """N = Nk, Nk > N with odd off, N = 1, an explicit scale."""
    d, dv, B = 8, 5, 2
    q, k, v, do = _inputs(N, Nk, d, dv, B, 100 * N + Nk)
    tau = scale if scale > 0 else 1.0 / math.sqrt(d)
    Q, K, V = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    S = tau * torch.einsum("ifb,jfb->ijb", Q, K)
    hidden = torch.arange(Nk)[None, :] > torch.arange(N)[:, None] + (Nk - N)
    P = torch.softmax(S.masked_fill(hidden[:, :, None], float("-inf")), dim=1)
    Ot = torch.einsum("ijb,jcb->icb", P, V)
    Ot.backward(torch.tensor(do))
    close = lambda a, b: np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1.0)
    o, l, m = causal_fwd_ref(q, k, v, scale)
    assert close(o, Ot.detach().numpy())
    Sm = S.detach().masked_fill(hidden[:, :, None], float("-inf")).numpy()
    assert close(m[:, 0, :], Sm.max(axis=1)) and close(l[:, 0, :], np.exp(Sm - Sm.max(axis=1, keepdims=True)).sum(axis=1))
    dq, dk, dv_ = causal_bwd_ref(q, k, v, o, do, l, m, scale)
    for a, t in ((dq, Q), (dk, K), (dv_, V)):
        assert close(a, t.grad.numpy())
    # l = m = None recomputes the statistics (the Float64 device path's contract)
    for a, b in zip(causal_bwd_ref(q, k, v, o, do, None, None, scale), (dq, dk, dv_)):
        assert np.array_equal(a, b)


# ---- the C ABI, before any launch ------------------------------------------------------
def test_header_declares_and_library_exports_the_four_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa_hip.h")).read(), flags=re.S)
    L = fa_hip.lib()
    for f in SYMBOLS:
        assert re.search(r"\b" + f + r"\s*\(", src), f"{f} not declared in fa_hip.h"
        assert hasattr(L, f), f"{f} not exported"
    assert L.fa_abi_version() == 1


P16 = ctypes.c_void_p(16)   # never dereferenced: validation fails first


def _fwd(L, dtype, ptrs, N, Nk, d, dv, B, ws=None, nws=0):
    return L.fa_causal_fwd(dtype, *ptrs, N, Nk, d, dv, B, 0.0, ws, nws, None)


def _bwd(L, dtype, ptrs, N, Nk, d, dv, B, ws=None, nws=0):
    return L.fa_causal_bwd(dtype, *ptrs, N, Nk, d, dv, B, 0.0, ws, nws, None)


def test_abi_fewer_keys_than_queries_is_unsupported():
    L = fa_hip.lib()
    for call, n in ((_fwd, 6), (_bwd, 10)):
        rc = call(L, 1, [P16] * n, 64, 63, 32, 32, 1, P16, 1 << 20)
        assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"causal" in L.fa_last_error()
    assert L.fa_causal_fwd_workspace(1, 64, 63, 32, 32, 1) == 0
    assert L.fa_causal_bwd_workspace(1, 64, 63, 32, 32, 1) == 0


def test_abi_rejections_carry_status_and_message():
    L = fa_hip.lib()
    for call, n in ((_fwd, 6), (_bwd, 10)):
        rc = call(L, 9, [P16] * n, 64, 64, 32, 32, 1)
        assert rc == fa_hip.FA_ERR_INVALID_ARG and b"dtype" in L.fa_last_error()
        for N, Nk, d, dv, B in ((64, 64, 0, 32, 1), (64, 64, 32, 0, 1), (-1, 64, 32, 32, 1), (64, 64, 32, 32, -1)):
            rc = call(L, 1, [P16] * n, N, Nk, d, dv, B)
            assert rc == fa_hip.FA_ERR_INVALID_ARG and b"DimensionMismatch" in L.fa_last_error()
        for i in range(n):
            ptrs = [P16] * n
            ptrs[i] = None
            rc = call(L, 1, ptrs, 64, 64, 32, 32, 1, P16, 1 << 20)
            assert rc == fa_hip.FA_ERR_INVALID_ARG and b"null" in L.fa_last_error(), i
        for d, dv in ((129, 32), (32, 129)):
            rc = call(L, 1, [P16] * n, 64, 64, d, dv, 1, P16, 1 << 20)
            assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"head dimension" in L.fa_last_error()
        rc = call(L, 1, [P16] * n, 1 << 30, 1 << 30, 4, 4, 1, P16, 1 << 20)      # 8 GiB slab
        assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"32-bit" in L.fa_last_error()


def test_abi_check_order_and_names():
    """dtype, DimensionMismatch, empty inputs, null pointer, head dimension, Nk >= N, 32-bit
    extents, workspace: each check wins over every later one, and fa_last_error() begins with
    the function's own name."""
    L = fa_hip.lib()
    for call, n, name in ((_fwd, 6, b"fa_causal_fwd: "), (_bwd, 10, b"fa_causal_bwd: ")):
        bad = [None] + [P16] * (n - 1)
        assert call(L, 9, [None] * n, 0, 64, 0, 32, 1) == fa_hip.FA_ERR_INVALID_ARG
        assert L.fa_last_error() == name + b"unknown dtype"
        assert call(L, 1, [None] * n, 0, 64, 0, 32, 1) == fa_hip.FA_ERR_INVALID_ARG      # over the empty no-op
        assert L.fa_last_error().startswith(name + b"DimensionMismatch")
        assert call(L, 1, [None] * n, 0, 64, 129, 32, 1) == 0                              # empty over everything later
        for N, Nk, d in ((64, 64, 129), (64, 63, 32), (1 << 30, 1 << 30, 4)):              # null over the shape checks
            assert call(L, 1, bad, N, Nk, d, 32, 1) == fa_hip.FA_ERR_INVALID_ARG
            assert L.fa_last_error() == name + b"null pointer"
        assert call(L, 1, [P16] * n, 64, 63, 129, 32, 1) == fa_hip.FA_ERR_UNSUPPORTED       # head dimension over Nk >= N
        assert L.fa_last_error().startswith(name + b"head dimension")
        assert call(L, 1, [P16] * n, 1 << 30, (1 << 30) - 1, 4, 4, 1) == fa_hip.FA_ERR_UNSUPPORTED   # Nk >= N over the extents
        assert L.fa_last_error() == name + b"causal attention needs Nk >= N (a query would see no key)"
        assert call(L, 1, [P16] * n, 1 << 30, 1 << 30, 4, 4, 1) == fa_hip.FA_ERR_UNSUPPORTED          # extents over the workspace
        assert L.fa_last_error() == name + b"extent exceeds the kernels' 32-bit addressing"
    # the backward rejects a null workspace even when told it holds the bytes; the forward
    # rejects a missing one only when the shape needs one
    need = L.fa_causal_bwd_workspace(1, 256, 256, 64, 64, 2)
    assert _bwd(L, 1, [P16] * 10, 256, 256, 64, 64, 2, None, need) == fa_hip.FA_ERR_WORKSPACE
    assert L.fa_last_error() == b"fa_causal_bwd: workspace missing or smaller than fa_causal_bwd_workspace()"
    need = L.fa_causal_fwd_workspace(1, 250, 250, 64, 64, 2)
    assert _fwd(L, 1, [P16] * 6, 250, 250, 64, 64, 2, None, need) == fa_hip.FA_ERR_WORKSPACE
    assert L.fa_last_error() == b"fa_causal_fwd: workspace missing or smaller than fa_causal_fwd_workspace()"


def test_abi_workspace_is_checked_before_any_launch():
    L = fa_hip.lib()
    need = L.fa_causal_bwd_workspace(1, 256, 256, 64, 64, 2)
    assert need >= 256 + 2 * 4 * 256 * 2 + 256               # header, two fp32 statistics, slack
    assert _bwd(L, 1, [P16] * 10, 256, 256, 64, 64, 2) == fa_hip.FA_ERR_WORKSPACE
    assert b"fa_causal_bwd_workspace" in L.fa_last_error()
    assert _bwd(L, 1, [P16] * 10, 256, 256, 64, 64, 2, P16, need - 1) == fa_hip.FA_ERR_WORKSPACE
    # the forward needs one only for the padded K / V copies of a 16-bit ragged Nk
    assert L.fa_causal_fwd_workspace(1, 256, 256, 64, 64, 2) == 0
    assert L.fa_causal_fwd_workspace(0, 250, 250, 64, 64, 2) == 0
    need = L.fa_causal_fwd_workspace(1, 250, 250, 64, 64, 2)
    assert need >= 2 * 256 * 64 * 2 * 2 + 256
    assert _fwd(L, 1, [P16] * 6, 250, 250, 64, 64, 2) == fa_hip.FA_ERR_WORKSPACE
    assert b"fa_causal_fwd_workspace" in L.fa_last_error()
    assert _fwd(L, 1, [P16] * 6, 250, 250, 64, 64, 2, P16, need - 1) == fa_hip.FA_ERR_WORKSPACE


def test_abi_empty_inputs_are_a_noop_that_dereferences_nothing():
    L = fa_hip.lib()
    for call, n in ((_fwd, 6), (_bwd, 10)):
        assert call(L, 1, [None] * n, 0, 0, 32, 32, 1) == 0
        assert call(L, 1, [None] * n, 0, 64, 32, 32, 1) == 0
        assert call(L, 1, [None] * n, 64, 64, 32, 32, 0) == 0
        assert L.fa_last_error() == b""


def test_causal_backward_workspace_holds_no_running_sums():
    """(1024, 1024, 64, 64, 64) bf16 is a shape fa_dense_bwd's single pass takes.  The causal
    workspace is exactly header + statistics + slack, independent of the device and of the
    dense plan; the dense answer under fa_debug_set_bwd_mode(2) adds the single pass's
    counters and running sums whenever a device is visible to plan it on (the plan asks for
    the CU count), and is never smaller."""
    L = fa_hip.lib()
    shape = (1, 1024, 1024, 64, 64, 64)
    causal = L.fa_causal_bwd_workspace(*shape)
    assert causal == 256 + 2 * 4 * 1024 * 64 + 256
    old = L.fa_debug_set_bwd_mode(2)
    try:
        dense2 = L.fa_dense_bwd_workspace(*shape)
        assert L.fa_causal_bwd_workspace(*shape) == causal
    finally:
        L.fa_debug_set_bwd_mode(old)
    L.fa_debug_set_bwd_mode(1)
    try:
        dense1 = L.fa_dense_bwd_workspace(*shape)
    finally:
        L.fa_debug_set_bwd_mode(old)
    assert causal <= dense1 <= dense2
    if dense2 > dense1:            # a device was there to plan the single pass on
        assert causal < dense2 and dense2 - causal >= 2 * 4 * 1024 * 64 * 64


# ---- the Python mirror ---------------------------------------------------------------
def jl(shape, dtype=torch.bfloat16):
    return fa_hip.jl_empty(shape, dtype, device="cpu")


def test_mirror_is_exported():
    for name in ("causal_fa", "causal_fa_", "causal_fa_backward", "causal_dpa"):
        assert name in fa_hip.__all__ and callable(getattr(fa_hip, name))


def _good(N=16, Nk=20, d=8, dv=4, B=2):
    f = lambda s: jl(s, torch.float32)
    return dict(Q=jl((N, d, B)), K=jl((Nk, d, B)), V=jl((Nk, dv, B)), O=jl((N, dv, B)), dO=jl((N, dv, B)),
                l=f((N, 1, B)), m=f((N, 1, B)))


def _back(a):
    return fa_hip.causal_fa_backward(a["Q"], a["K"], a["V"], a["O"], a["dO"], a["l"], a["m"])


def _fwd_(a):
    return fa_hip.causal_fa_(a["O"], a["l"], a["m"], a["Q"], a["K"], a["V"])


def test_mirror_rejects_bad_shapes_without_a_device():
    N, Nk, d, dv, B = 16, 20, 8, 4, 2
    f = lambda s: jl(s, torch.float32)
    bad = {"K": jl((Nk, d + 1, B)), "V": jl((Nk, dv, B + 1)), "O": jl((N, dv + 1, B)), "dO": jl((N - 1, dv, B)),
           "l": f((N, B, 1)), "m": f((N - 1, 1, B)), "Q": jl((N, d))}
    for name, t in bad.items():
        a = _good(N, Nk, d, dv, B)
        a[name] = t
        with pytest.raises(DimensionMismatch):
            _back(a)
        if name != "dO":
            with pytest.raises(DimensionMismatch):
                _fwd_(a)
    a = _good()
    with pytest.raises(DimensionMismatch):
        fa_hip.causal_fa(a["Q"], a["K"], jl((21, 4, 2)))
    with pytest.raises(DimensionMismatch):
        fa_hip.causal_dpa(a["Q"], jl((20, 9, 2)), a["V"])
    for name in ("l", "m"):
        a = _good()
        a[name] = jl(tuple(a[name].shape), torch.float64)
        with pytest.raises(DimensionMismatch, match="float32"):
            _back(a)


def test_mirror_reports_fewer_keys_than_queries_without_a_device():
    a = _good(N=16, Nk=12)
    for call in (_back, _fwd_, lambda a: fa_hip.causal_fa(a["Q"], a["K"], a["V"]),
                 lambda a: fa_hip.causal_dpa(a["Q"], a["K"], a["V"])):
        with pytest.raises(fa_hip.FlashAttentionError, match="causal") as e:
            call(a)
        assert e.value.status == fa_hip.FA_ERR_UNSUPPORTED


def test_mirror_valid_call_stops_only_at_the_device_check():
    for call in (_back, _fwd_, lambda a: fa_hip.causal_dpa(a["Q"], a["K"], a["V"])):
        with pytest.raises(TypeError, match="ROCm device"):
            call(_good())
