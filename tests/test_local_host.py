"""CPU tests of local (sliding-window) attention: the float64 yardstick (tests/local_ref.py)
against torch autograd through an explicitly masked softmax, against causal_ref at (-1, 0) and
the dense oracle at (-1, -1), its exact zeros on unseen keys; the C ABI's checks before any
launch (fa_local_fwd, fa_local_bwd and their workspace queries, which do not depend on the
window) and the Python mirror's argument validation.  No device is touched."""
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
from local_ref import local_bwd_ref, local_fwd_ref, unseen_keys, visible
from oracle import fa_oracle as O

SYMBOLS = ("fa_local_fwd", "fa_local_fwd_workspace", "fa_local_bwd", "fa_local_bwd_workspace")


def _inputs(N, Nk, d, dv, B, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, d, B)), rng.standard_normal((Nk, d, B)),
            rng.standard_normal((Nk, dv, B)), rng.standard_normal((N, dv, B)))


close = lambda a, b: np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1.0)


# ---- the yardstick ----------------------------------------------------------------
@pytest.mark.parametrize("N,Nk,left,right,scale", [(24, 24, 5, 0, 0.0), (20, 33, 3, 4, 0.0), (1, 6, 0, 0, 0.0),
                                                   (16, 21, 2, -1, 0.3), (12, 40, 7, 2, 0.0), (9, 9, -1, 3, 0.0)])
def test_ref_equals_torch_autograd_through_a_masked_softmax(N, Nk, left, right, scale):
    """Two-sided, one-sided on either side, one key per query, unseen keys, an explicit scale."""
    d, dv, B = 8, 5, 2
    q, k, v, do = _inputs(N, Nk, d, dv, B, 100 * N + Nk)
    tau = scale if scale > 0 else 1.0 / math.sqrt(d)
    Q, K, V = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    S = tau * torch.einsum("ifb,jfb->ijb", Q, K)
    i, j = torch.arange(N)[:, None] + (Nk - N), torch.arange(Nk)[None, :]
    hidden = torch.zeros((N, Nk), dtype=torch.bool)
    if right >= 0:
        hidden |= j > i + right
    if left >= 0:
        hidden |= j < i - left
    assert np.array_equal(~hidden.numpy(), visible(0, N, 0, Nk, Nk - N, left, right))
    P = torch.softmax(S.masked_fill(hidden[:, :, None], float("-inf")), dim=1)
    Ot = torch.einsum("ijb,jcb->icb", P, V)
    Ot.backward(torch.tensor(do))
    o, l, m = local_fwd_ref(q, k, v, left, right, scale)
    assert close(o, Ot.detach().numpy())
    Sm = S.detach().masked_fill(hidden[:, :, None], float("-inf")).numpy()
    assert close(m[:, 0, :], Sm.max(axis=1)) and close(l[:, 0, :], np.exp(Sm - Sm.max(axis=1, keepdims=True)).sum(axis=1))
    dq, dk, dv_ = local_bwd_ref(q, k, v, o, do, l, m, left, right, scale)
    for a, t in ((dq, Q), (dk, K), (dv_, V)):
        assert close(a, t.grad.numpy())
    # l = m = None recomputes the statistics (the Float64 device path's contract)
    for a, b in zip(local_bwd_ref(q, k, v, o, do, None, None, left, right, scale), (dq, dk, dv_)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("N,Nk", [(24, 24), (17, 30), (600, 700)])
def test_ref_contains_causal_and_dense(N, Nk):
    """(-1, 0) is causal_ref, (-1, -1) the dense oracle; a side >= Nk is unbounded too."""
    q, k, v, do = _inputs(N, Nk, 8, 6, 2, 7 * N + Nk)
    oc, lc, mc = causal_fwd_ref(q, k, v)
    for left in (-1, Nk, 1 << 40):
        o, l, m = local_fwd_ref(q, k, v, left, 0)
        assert close(o, oc) and close(l, lc) and close(m, mc)
        for a, b in zip(local_bwd_ref(q, k, v, o, do, l, m, left, 0), causal_bwd_ref(q, k, v, oc, do, lc, mc)):
            assert close(a, b)
    od, ld, md = O.dense_fa3(q, k, v)
    for left, right in ((-1, -1), (Nk, 1 << 40)):
        o, l, m = local_fwd_ref(q, k, v, left, right)
        assert close(o, od) and close(l, ld) and close(m, md)
        for a, b in zip(local_bwd_ref(q, k, v, o, do, l, m, left, right), O.dense_fa_backward(q, k, v, od, do, ld, md)):
            assert close(a, b)


@pytest.mark.parametrize("N,Nk,left,right,count", [(8, 100, 10, 0, 82), (20, 33, 5, 2, 8), (16, 16, 3, 0, 0),
                                                   (600, 1300, 50, 20, 650)])
def test_ref_gives_exact_zero_gradients_on_unseen_keys(N, Nk, left, right, count):
    """The keys j < off - left are seen by no query (a KV cache longer than the window)."""
    q, k, v, do = _inputs(N, Nk, 8, 6, 2, N + Nk)
    un = unseen_keys(N, Nk, left, right)
    assert un.sum() == count == max(0, Nk - N - left)
    assert np.array_equal(un, np.arange(Nk) < Nk - N - left)
    o, l, m = local_fwd_ref(q, k, v, left, right)
    _, dk, dv_ = local_bwd_ref(q, k, v, o, do, l, m, left, right)
    assert np.all(dk[un] == 0.0) and np.all(dv_[un] == 0.0)
    if count:
        assert np.all(np.abs(dv_[~un]).max(axis=(1, 2)) > 0.0)


# ---- the C ABI, before any launch ------------------------------------------------------
def test_header_declares_and_library_exports_the_four_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa_hip.h")).read(), flags=re.S)
    L = fa_hip.lib()
    for f in SYMBOLS:
        assert re.search(r"\b" + f + r"\s*\(", src), f"{f} not declared in fa_hip.h"
        assert hasattr(L, f), f"{f} not exported"
    assert L.fa_abi_version() == 1


P16 = ctypes.c_void_p(16)   # never dereferenced: validation fails first
WINDOWS = ((100, 0), (0, 0), (-1, -1), (0, 1 << 40), (1 << 40, 1 << 40))


def _fwd(L, dtype, ptrs, N, Nk, d, dv, B, ws=None, nws=0, window=(100, 0)):
    return L.fa_local_fwd(dtype, *ptrs, N, Nk, d, dv, B, *window, 0.0, ws, nws, None)


def _bwd(L, dtype, ptrs, N, Nk, d, dv, B, ws=None, nws=0, window=(100, 0)):
    return L.fa_local_bwd(dtype, *ptrs, N, Nk, d, dv, B, *window, 0.0, ws, nws, None)


def test_abi_fewer_keys_than_queries_is_unsupported():
    L = fa_hip.lib()
    for call, n in ((_fwd, 6), (_bwd, 10)):
        for w in WINDOWS:
            rc = call(L, 1, [P16] * n, 64, 63, 32, 32, 1, P16, 1 << 20, window=w)
            assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"local attention needs Nk >= N" in L.fa_last_error()
    assert L.fa_local_fwd_workspace(1, 64, 63, 32, 32, 1) == 0
    assert L.fa_local_bwd_workspace(1, 64, 63, 32, 32, 1) == 0


def test_abi_rejections_carry_status_and_message_in_the_causal_order():
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
        # a null pointer comes before Nk < N, the head dimension before it too
        ptrs = [P16] * n
        ptrs[0] = None
        assert call(L, 1, ptrs, 64, 63, 32, 32, 1, P16, 1 << 20) == fa_hip.FA_ERR_INVALID_ARG
        for d, dv in ((129, 32), (32, 129)):
            for Nk in (64, 63):
                rc = call(L, 1, [P16] * n, 64, Nk, d, dv, 1, P16, 1 << 20)
                assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"head dimension" in L.fa_last_error()
        rc = call(L, 1, [P16] * n, 1 << 30, 1 << 30, 4, 4, 1, P16, 1 << 20)      # 8 GiB slab
        assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"32-bit" in L.fa_last_error()
        assert b"fa_local_" in L.fa_last_error()


def test_abi_check_order_and_names():
    """As the causal pair's (tests/test_causal_host.py): each check wins over every later one,
    fa_last_error() begins with the function's own name, and the Nk >= N message says "local"."""
    L = fa_hip.lib()
    for call, n, name in ((_fwd, 6, b"fa_local_fwd: "), (_bwd, 10, b"fa_local_bwd: ")):
        bad = [None] + [P16] * (n - 1)
        assert call(L, 9, [None] * n, 0, 64, 0, 32, 1) == fa_hip.FA_ERR_INVALID_ARG
        assert L.fa_last_error() == name + b"unknown dtype"
        assert call(L, 1, [None] * n, 0, 64, 0, 32, 1) == fa_hip.FA_ERR_INVALID_ARG      # over the empty no-op
        assert L.fa_last_error().startswith(name + b"DimensionMismatch")
        assert call(L, 1, [None] * n, 0, 64, 129, 32, 1) == 0                              # empty over everything later
        for N, Nk, d in ((64, 64, 129), (64, 63, 32), (1 << 30, 1 << 30, 4)):              # null over the shape checks
            assert call(L, 1, bad, N, Nk, d, 32, 1) == fa_hip.FA_ERR_INVALID_ARG
            assert L.fa_last_error() == name + b"null pointer"
        assert call(L, 1, [P16] * n, 1 << 30, (1 << 30) - 1, 4, 4, 1) == fa_hip.FA_ERR_UNSUPPORTED   # Nk >= N over the extents
        assert L.fa_last_error() == name + b"local attention needs Nk >= N (a query would see no key)"
        assert call(L, 1, [P16] * n, 1 << 30, 1 << 30, 4, 4, 1) == fa_hip.FA_ERR_UNSUPPORTED          # extents over the workspace
        assert L.fa_last_error() == name + b"extent exceeds the kernels' 32-bit addressing"
    need = L.fa_local_bwd_workspace(1, 256, 256, 64, 64, 2)
    assert _bwd(L, 1, [P16] * 10, 256, 256, 64, 64, 2, None, need) == fa_hip.FA_ERR_WORKSPACE     # null, whatever the bytes
    assert L.fa_last_error() == b"fa_local_bwd: workspace missing or smaller than fa_local_bwd_workspace()"
    need = L.fa_local_fwd_workspace(1, 250, 250, 64, 64, 2)
    assert _fwd(L, 1, [P16] * 6, 250, 250, 64, 64, 2, None, need) == fa_hip.FA_ERR_WORKSPACE
    assert L.fa_last_error() == b"fa_local_fwd: workspace missing or smaller than fa_local_fwd_workspace()"


def test_abi_workspace_is_checked_before_any_launch_and_names_the_query():
    L = fa_hip.lib()
    need = L.fa_local_bwd_workspace(1, 256, 256, 64, 64, 2)
    assert need == 256 + 2 * 4 * 256 * 2 + 256                 # header, two fp32 statistics, slack
    assert _bwd(L, 1, [P16] * 10, 256, 256, 64, 64, 2) == fa_hip.FA_ERR_WORKSPACE
    assert b"fa_local_bwd_workspace" in L.fa_last_error()
    assert _bwd(L, 1, [P16] * 10, 256, 256, 64, 64, 2, P16, need - 1) == fa_hip.FA_ERR_WORKSPACE
    # the forward needs one only for the padded K / V copies of a 16-bit ragged Nk
    assert L.fa_local_fwd_workspace(1, 256, 256, 64, 64, 2) == 0
    assert L.fa_local_fwd_workspace(0, 250, 250, 64, 64, 2) == 0
    need = L.fa_local_fwd_workspace(1, 250, 250, 64, 64, 2)
    assert need >= 2 * 256 * 64 * 2 * 2 + 256
    assert _fwd(L, 1, [P16] * 6, 250, 250, 64, 64, 2) == fa_hip.FA_ERR_WORKSPACE
    assert b"fa_local_fwd_workspace" in L.fa_last_error()
    assert _fwd(L, 1, [P16] * 6, 250, 250, 64, 64, 2, P16, need - 1) == fa_hip.FA_ERR_WORKSPACE


SHAPES = [(1, 256, 256, 64, 64, 2), (1, 250, 250, 64, 64, 2), (2, 200, 333, 48, 40, 2), (0, 500, 500, 64, 64, 1),
          (3, 200, 333, 48, 40, 2), (1, 2048, 2048, 64, 64, 1), (1, 1024, 1024, 64, 64, 64), (1, 8, 1000, 64, 64, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_workspace_answers_are_the_causal_ones_and_ignore_the_window(shape):
    """The queries take no window; the entry points, given one byte less than the answer, reject
    every window alike (0 and 2^40 included: no window value changes what is required), and the
    answers equal fa_causal_*_workspace's for the shape, under every backward mode."""
    L = fa_hip.lib()
    dtype, dims = shape[0], shape[1:]
    nf, nb = L.fa_local_fwd_workspace(*shape), L.fa_local_bwd_workspace(*shape)
    assert nf == L.fa_causal_fwd_workspace(*shape) and nb == L.fa_causal_bwd_workspace(*shape)
    for mode in (1, 2):
        old = L.fa_debug_set_bwd_mode(mode)
        try:
            assert L.fa_local_bwd_workspace(*shape) == nb
        finally:
            L.fa_debug_set_bwd_mode(old)
    for w in WINDOWS:
        assert _bwd(L, dtype, [P16] * 10, *dims, P16, nb - 1, window=w) == fa_hip.FA_ERR_WORKSPACE, w
        assert b"fa_local_bwd_workspace" in L.fa_last_error()
        if nf:
            assert _fwd(L, dtype, [P16] * 6, *dims, P16, nf - 1, window=w) == fa_hip.FA_ERR_WORKSPACE, w
            assert b"fa_local_fwd_workspace" in L.fa_last_error()


def test_abi_empty_inputs_are_a_noop_that_dereferences_nothing():
    L = fa_hip.lib()
    for call, n in ((_fwd, 6), (_bwd, 10)):
        for w in WINDOWS:
            assert call(L, 1, [None] * n, 0, 0, 32, 32, 1, window=w) == 0
            assert call(L, 1, [None] * n, 0, 64, 32, 32, 1, window=w) == 0
            assert call(L, 1, [None] * n, 64, 64, 32, 32, 0, window=w) == 0
            assert L.fa_last_error() == b""


def test_plan_hooks_answer_without_a_device():
    """The kernel families of a local call (fa_dense_plan.h's enumerators), readable on the host."""
    L = fa_hip.lib()
    out = (ctypes.c_int64 * 8)()
    AMPLE = 1 << 40
    # aligned bf16 at d <= 64: the two-query-block tiled kernel, LDS-staged; never split (the
    # dense plan splits this grid), never p4
    assert L.fa_debug_local_fwd_plan(1, 2048, 2048, 64, 64, 1, 1, 1, AMPLE, 256, out) == 6
    assert list(out)[:3] == [1, 0, 0] and out[4] == 1 and out[5] == 512
    dense = (ctypes.c_int64 * 17)()
    assert L.fa_debug_dense_fwd_plan(1, 2048, 2048, 64, 64, 1, 0, 0, 2, 1, 1, AMPLE, 256, dense) == 8 and dense[3] > 1
    # d = 128, a grid that fills the chip: dense takes p4 (9), local the 256-row tiled kernel
    assert L.fa_debug_dense_fwd_plan(1, 4096, 4096, 128, 128, 16, 0, 0, 2, 1, 1, AMPLE, 256, dense) == 9
    assert L.fa_debug_local_fwd_plan(1, 4096, 4096, 128, 128, 16, 1, 1, AMPLE, 256, out) == 4 and out[5] == 256
    # Nk % 8 != 0: padded K / V copies and still a tiled kernel; without room, the generic one
    assert L.fa_debug_local_fwd_plan(1, 500, 500, 64, 64, 1, 1, 1, AMPLE, 256, out) == 5 and out[2] == 1 and out[3] == 504
    assert L.fa_debug_local_fwd_plan(1, 500, 500, 64, 64, 1, 1, 1, 0, 256, out) == 0
    assert L.fa_debug_local_fwd_plan(0, 500, 500, 64, 64, 1, 1, 1, AMPLE, 256, out) == 1    # fp32
    assert L.fa_debug_local_fwd_plan(3, 500, 500, 64, 64, 1, 1, 1, AMPLE, 256, out) == 2    # Float64
    assert L.fa_debug_local_fwd_plan(1, 64, 63, 64, 64, 1, 1, 1, AMPLE, 256, out) == -1
    b = (ctypes.c_int64 * 6)()
    # single-pass-eligible for dense: local runs the two passes
    assert L.fa_debug_local_bwd_plan(1, 1024, 1024, 64, 64, 64, 1, AMPLE, 256, b) == 3 and b[0] == 0
    assert L.fa_debug_local_bwd_plan(1, 500, 500, 64, 64, 1, 1, AMPLE, 256, b) == 3 and list(b)[:3] == [1, 504, 504]
    assert L.fa_debug_local_bwd_plan(1, 512, 512, 64, 64, 1, 0, AMPLE, 256, b) == 1   # misaligned: generic
    assert L.fa_debug_local_bwd_plan(0, 500, 500, 64, 64, 1, 1, AMPLE, 256, b) == 2   # fp32 MFMA
    assert L.fa_debug_local_bwd_plan(3, 500, 500, 64, 64, 1, 1, AMPLE, 256, b) == 0   # Float64


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_dense_plan_hooks_at_mask_2_agree_with_the_local_hooks(shape):
    """fa_debug_dense_fwd_plan / fa_debug_dense_bwd_plan read their `causal` argument as the
    mask (0 dense, 1 causal, 2 local): at 2, under the default knobs, they return the local
    hooks' kernel and every field both report, with and without room in the workspace, with
    aligned and misaligned tensors."""
    L = fa_hip.lib()
    ci, i64, sz, out_p = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64)
    L.fa_debug_dense_fwd_plan.restype = L.fa_debug_dense_bwd_plan.restype = ci
    L.fa_debug_dense_fwd_plan.argtypes = [ci] + [i64] * 5 + [ci] * 5 + [sz, ci, out_p]
    L.fa_debug_dense_bwd_plan.argtypes = [ci] + [i64] * 5 + [ci] * 6 + [sz, ci, out_p]
    lf, lb = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 6)()
    df, db = (ctypes.c_int64 * 17)(), (ctypes.c_int64 * 25)()
    for nws in (1 << 40, 0):
        for al in (1, 0):
            k = L.fa_debug_local_fwd_plan(*shape, al, al, nws, 256, lf)
            assert k == L.fa_debug_dense_fwd_plan(*shape, 2, 0, 2, al, al, nws, 256, df) and k >= 0
            # local out: local, causal bits, pad, ldk, nsplit, rows, grid, total
            assert list(lf) == [1, df[0], df[1], df[2], df[3], df[5], df[8], df[16]] and df[0] == 0
            k = L.fa_debug_local_bwd_plan(*shape, al, nws, 256, lb)
            assert k == L.fa_debug_dense_bwd_plan(*shape, 2, 0, 0, 3, -1, al, nws, 256, db) and k >= 0
            # local out: padded, N, Nk, d, dv as run, total
            assert list(lb) == list(db)[:5] + [db[24]]
    # the mask is a value, not a flag: anything else is an invalid argument, and 2 needs Nk >= N
    assert L.fa_debug_dense_fwd_plan(1, 64, 64, 64, 64, 1, 3, 0, 2, 1, 1, 0, 256, df) == -1
    assert L.fa_debug_dense_bwd_plan(1, 64, 64, 64, 64, 1, -1, 0, 0, 3, -1, 1, 0, 256, db) == -1
    assert L.fa_debug_dense_fwd_plan(1, 64, 63, 64, 64, 1, 2, 0, 2, 1, 1, 0, 256, df) == -1


# ---- the Python mirror ---------------------------------------------------------------
def jl(shape, dtype=torch.bfloat16):
    return fa_hip.jl_empty(shape, dtype, device="cpu")


def test_mirror_is_exported():
    for name in ("local_fa", "local_fa_", "local_fa_backward", "local_dpa"):
        assert name in fa_hip.__all__ and callable(getattr(fa_hip, name))


def _good(N=16, Nk=20, d=8, dv=4, B=2):
    f = lambda s: jl(s, torch.float32)
    return dict(Q=jl((N, d, B)), K=jl((Nk, d, B)), V=jl((Nk, dv, B)), O=jl((N, dv, B)), dO=jl((N, dv, B)),
                l=f((N, 1, B)), m=f((N, 1, B)))


def _back(a):
    return fa_hip.local_fa_backward(a["Q"], a["K"], a["V"], a["O"], a["dO"], a["l"], a["m"], 3, 1)


def _fwd_(a):
    return fa_hip.local_fa_(a["O"], a["l"], a["m"], a["Q"], a["K"], a["V"], 3, 1)


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
        fa_hip.local_fa(a["Q"], a["K"], jl((21, 4, 2)), 3, 1)
    with pytest.raises(DimensionMismatch):
        fa_hip.local_dpa(a["Q"], jl((20, 9, 2)), a["V"], 3, 1)
    for name in ("l", "m"):
        a = _good()
        a[name] = jl(tuple(a[name].shape), torch.float64)
        with pytest.raises(DimensionMismatch, match="float32"):
            _back(a)


def test_mirror_reports_fewer_keys_than_queries_without_a_device():
    a = _good(N=16, Nk=12)
    for call in (_back, _fwd_, lambda a: fa_hip.local_fa(a["Q"], a["K"], a["V"], 3, 1),
                 lambda a: fa_hip.local_dpa(a["Q"], a["K"], a["V"], 3, 1)):
        with pytest.raises(fa_hip.FlashAttentionError, match="local") as e:
            call(a)
        assert e.value.status == fa_hip.FA_ERR_UNSUPPORTED


def test_mirror_valid_call_stops_only_at_the_device_check():
    for call in (_back, _fwd_, lambda a: fa_hip.local_dpa(a["Q"], a["K"], a["V"], 3, 1)):
        with pytest.raises(TypeError, match="ROCm device"):
            call(_good())
