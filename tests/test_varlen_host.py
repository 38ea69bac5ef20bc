"""CPU tests of varlen attention (per-slab lengths in a padded batch): the float64 yardstick
(tests/varlen_ref.py) against local_ref at full lengths and on the sliced slabs, and against
torch autograd through an explicitly masked softmax (slabs with nk < nq and nk = 0 included);
the C ABI's checks before any launch (fa_varlen_fwd, fa_varlen_bwd and their workspace queries),
the plan and clamp hooks, the Python mirror's validation of host lengths, and the table of
tests/test_gpu_varlen.py pinned from the reference alone.  No device is touched."""
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
from conftest import ROOT
from local_ref import local_bwd_ref, local_fwd_ref
from varlen_ref import keyless_rows, lengths, slab_visible, unseen_keys, varlen_bwd_ref, varlen_fwd_ref

SYMBOLS = ("fa_varlen_fwd", "fa_varlen_fwd_workspace", "fa_varlen_bwd", "fa_varlen_bwd_workspace")

# The GPU cases of tests/test_gpu_varlen.py: (N, Nk, d, dv, B, left, right), q_lens, k_lens, dtypes
GPU_CASES = {
    "a": ((1024, 1024, 64, 64, 4, -1, 0), (1024, 700, 513, 0), (1024, 700, 600, 37), ("bfloat16", "float16")),
    "b": ((512, 640, 128, 128, 3, 64, 0), (512, 257, 1), (640, 300, 200), ("bfloat16",)),
    "c": ((256, 256, 64, 64, 3, -1, 0), (256, 200, 100), (256, 120, 0), ("bfloat16", "float32")),
    "d": ((200, 333, 48, 40, 2, -1, -1), (200, 77), (333, 130), ("bfloat16", "float32")),
    "e": ((256, 296, 64, 64, 2, 23, 17), (256, 150), (296, 171), ("bfloat16",)),
    "f": ((100, 140, 32, 48, 2, 10, 5), (100, 41), (140, 63), ("float64",)),
}


def _inputs(N, Nk, d, dv, B, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, d, B)), rng.standard_normal((Nk, d, B)),
            rng.standard_normal((Nk, dv, B)), rng.standard_normal((N, dv, B)))


close = lambda a, b: np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1.0)


# ---- the yardstick ----------------------------------------------------------------
@pytest.mark.parametrize("N,Nk,left,right", [(24, 24, 5, 0), (20, 33, 3, 4), (16, 21, -1, 0), (12, 40, -1, -1)])
def test_ref_at_full_lengths_is_local_ref(N, Nk, left, right):
    q, k, v, do = _inputs(N, Nk, 8, 5, 2, 11 * N + Nk)
    for ql, kl in ((None, None), ((N, N), (Nk, Nk)), ((N + 3, N), None)):        # past the extent: clamped
        o, l, m = varlen_fwd_ref(q, k, v, ql, kl, left, right)
        o2, l2, m2 = local_fwd_ref(q, k, v, left, right)
        assert close(o, o2) and close(l, l2) and close(m, m2)
        for a, b in zip(varlen_bwd_ref(q, k, v, o, do, l, m, ql, kl, left, right),
                        local_bwd_ref(q, k, v, o2, do, l2, m2, left, right)):
            assert close(a, b)


@pytest.mark.parametrize("left,right", [(5, 0), (-1, 0), (-1, -1), (3, 4)])
def test_ref_per_slab_is_local_ref_on_the_sliced_arrays(left, right):
    N, Nk, d, dv = 24, 30, 8, 5
    ql, kl = (24, 10, 7), (30, 18, 7)                                            # nk >= nq in every slab
    q, k, v, do = _inputs(N, Nk, d, dv, 3, 5)
    o, l, m = varlen_fwd_ref(q, k, v, ql, kl, left, right)
    dq, dk, dv_ = varlen_bwd_ref(q, k, v, o, do, l, m, ql, kl, left, right)
    for b, (nq, nk) in enumerate(zip(ql, kl)):
        sl = lambda a, n: a[:n, :, b:b + 1]
        o2, l2, m2 = local_fwd_ref(sl(q, nq), sl(k, nk), sl(v, nk), left, right)
        assert close(sl(o, nq), o2) and close(sl(l, nq), l2) and close(sl(m, nq), m2)
        g = local_bwd_ref(sl(q, nq), sl(k, nk), sl(v, nk), o2, sl(do, nq), l2, m2, left, right)
        assert close(sl(dq, nq), g[0]) and close(sl(dk, nk), g[1]) and close(sl(dv_, nk), g[2])
        # everything past the lengths is the empty-row state / zero
        assert not o[nq:, :, b].any() and not l[nq:, 0, b].any() and np.all(m[nq:, 0, b] == -np.inf)
        assert not dq[nq:, :, b].any() and not dk[nk:, :, b].any() and not dv_[nk:, :, b].any()


@pytest.mark.parametrize("left,right,scale", [(-1, 0, 0.0), (-1, -1, 0.0), (4, 0, 0.3), (3, 2, 0.0), (-1, 3, 0.0)])
def test_ref_equals_torch_autograd_through_a_masked_softmax(left, right, scale):
    """Slabs with nk < nq (key-less queries under a right bound), nk = 0, nq = 0 and nq = 1."""
    N, Nk, d, dv = 20, 26, 8, 5
    ql, kl = (20, 15, 9, 0, 1, 12), (26, 6, 0, 11, 26, 12)
    B = len(ql)
    q, k, v, do = _inputs(N, Nk, d, dv, B, 77)
    tau = scale if scale > 0 else 1.0 / math.sqrt(d)
    Q, K, V = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    S = tau * torch.einsum("ifb,jfb->ijb", Q, K)
    vis = np.stack([slab_visible(N, Nk, nq, nk, left, right) for nq, nk in zip(ql, kl)], axis=2)
    i, j = np.arange(N)[:, None, None], np.arange(Nk)[None, :, None]
    nq, nk = np.asarray(ql)[None, None, :], np.asarray(kl)[None, None, :]
    want = (i < nq) & (j < nk)
    if right >= 0:
        want &= j <= i + (nk - nq) + right
    if left >= 0:
        want &= j >= i + (nk - nq) - left
    assert np.array_equal(vis, want)
    empty = ~vis.any(axis=1)                                                       # (N, B)
    assert empty[: ql[1], 1].any() or right < 0                                   # nk < nq hides rows under a right bound
    hidden = torch.tensor(~vis)
    # rows whose softmax is all -inf are compared after the empty-row convention: P = 0 there
    Sm = S.masked_fill(hidden, float("-inf"))
    Sm = torch.where(torch.tensor(empty)[:, None, :], torch.zeros_like(Sm), Sm)
    P = torch.softmax(Sm, dim=1) * torch.tensor(~empty, dtype=torch.float64)[:, None, :]
    P = P.masked_fill(hidden, 0.0)
    Ot = torch.einsum("ijb,jcb->icb", P, V)
    Ot.backward(torch.tensor(do))
    o, l, m = varlen_fwd_ref(q, k, v, ql, kl, left, right, scale)
    assert close(o, Ot.detach().numpy())
    Sn = np.where(vis, S.detach().numpy(), -np.inf)
    mx = Sn.max(axis=1)
    assert np.all(m[:, 0, :][empty] == -np.inf) and np.all(l[:, 0, :][empty] == 0.0) and not o.transpose(0, 2, 1)[empty].any()
    assert close(m[:, 0, :][~empty], mx[~empty])
    assert close(l[:, 0, :][~empty], np.exp(Sn - np.where(empty, 0.0, mx)[:, None, :]).sum(axis=1)[~empty])
    dq, dk, dv_ = varlen_bwd_ref(q, k, v, o, do, l, m, ql, kl, left, right, scale)
    for a, t in ((dq, Q), (dk, K), (dv_, V)):
        assert close(a, t.grad.numpy())
    assert not dq.transpose(0, 2, 1)[empty].any()
    for a, b in zip(varlen_bwd_ref(q, k, v, o, do, None, None, ql, kl, left, right, scale), (dq, dk, dv_)):
        assert np.array_equal(a, b)
    # padding contents never enter: overwrite everything past the lengths
    q2, k2, v2, do2 = (a.copy() for a in (q, k, v, do))
    for b in range(B):
        q2[ql[b]:, :, b] = 3e4; do2[ql[b]:, :, b] = -3e4; k2[kl[b]:, :, b] = -3e4; v2[kl[b]:, :, b] = 3e4
    for a, b in zip(varlen_fwd_ref(q2, k2, v2, ql, kl, left, right, scale), (o, l, m)):
        assert np.array_equal(a, b)
    for a, b in zip(varlen_bwd_ref(q2, k2, v2, o, do2, l, m, ql, kl, left, right, scale), (dq, dk, dv_)):
        assert np.array_equal(a, b)


def test_the_table_reaches_what_it_says():
    """What the GPU cases must contain, from the reference alone."""
    all_q = [n for c in GPU_CASES.values() for n in c[1]]
    all_k = [n for c in GPU_CASES.values() for n in c[2]]
    assert any(n % 8 for n in all_q + all_k) and any(n % 64 for n in all_q + all_k)
    # one past a workgroup's row block: 512 rows at d <= 64, 256 at d = 128
    assert 513 in GPU_CASES["a"][1] and GPU_CASES["a"][0][2] <= 64
    assert 257 in GPU_CASES["b"][1] and GPU_CASES["b"][0][2] == 128
    # a query block (512 / 256 forward rows, 128 backward rows) wholly past nq, a key block (128) wholly past nk
    (N, Nk, *_), ql, kl, _ = GPU_CASES["a"]
    assert any((N - 1) // 512 * 512 >= nq for nq in ql) and any((Nk - 1) // 128 * 128 >= nk for nk in kl)
    (N, Nk, *_), ql, kl, _ = GPU_CASES["b"]
    assert any((N - 1) // 256 * 256 >= nq for nq in ql) and any((Nk - 1) // 128 * 128 >= nk for nk in kl)
    assert 0 in all_q and 0 in all_k and 1 in all_q
    # the exact counts of key-less rows in case c: nk < nq under right = 0, and nk = 0
    (N, Nk, _, _, _, left, right), ql, kl, _ = GPU_CASES["c"]
    counts = [int(keyless_rows(N, Nk, nq, nk, left, right).sum()) for nq, nk in zip(ql, kl)]
    assert counts == [0, 80, 100]
    # ... which the reference turns into the empty-row state
    q, k, v, do = _inputs(N, Nk, 8, 8, 3, 3)
    o, l, m = varlen_fwd_ref(q, k, v, ql, kl, left, right)
    for b, (nq, nk) in enumerate(zip(ql, kl)):
        kr = keyless_rows(N, Nk, nq, nk, left, right)
        assert np.all(l[kr, 0, b] == 0.0) and np.all(m[kr, 0, b] == -np.inf) and np.all(l[:nq, 0, b][~kr[:nq]] > 0.0)
    # case a's slab 3 has no query at all; case d's padded routes: ragged key count, odd head dims
    assert GPU_CASES["a"][1][3] == 0 and GPU_CASES["d"][0][1] % 8
    assert GPU_CASES["d"][0][2] not in (32, 64, 128) and GPU_CASES["d"][0][3] not in (32, 64, 128)
    # unseen keys exist under a left bound with a long cache (case b, slab 2: nk - nq - left = 135)
    (N, Nk, _, _, _, left, right), ql, kl, _ = GPU_CASES["b"]
    assert int(unseen_keys(N, Nk, ql[2], kl[2], left, right).sum()) == 135
    assert np.array_equal(lengths((-3, 0, N, N + 5), N, 4), (0, 0, N, N))


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
LENS = ((None, None), (P16, P16), (P16, None))


def _fwd(L, dtype, ptrs, N, Nk, d, dv, B, ws=None, nws=0, window=(100, 0), lens=(P16, P16)):
    return L.fa_varlen_fwd(dtype, *ptrs, N, Nk, d, dv, B, *lens, *window, 0.0, ws, nws, None)


def _bwd(L, dtype, ptrs, N, Nk, d, dv, B, ws=None, nws=0, window=(100, 0), lens=(P16, P16)):
    return L.fa_varlen_bwd(dtype, *ptrs, N, Nk, d, dv, B, *lens, *window, 0.0, ws, nws, None)


def test_abi_fewer_keys_than_queries_is_unsupported():
    L = fa_hip.lib()
    for call, n in ((_fwd, 6), (_bwd, 10)):
        for w in WINDOWS:
            for lens in LENS:
                rc = call(L, 1, [P16] * n, 64, 63, 32, 32, 1, P16, 1 << 20, window=w, lens=lens)
                assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"varlen attention needs Nk >= N" in L.fa_last_error()
    assert L.fa_varlen_fwd_workspace(1, 64, 63, 32, 32, 1) == 0
    assert L.fa_varlen_bwd_workspace(1, 64, 63, 32, 32, 1) == 0


def test_abi_check_order_and_messages_are_the_local_ones_under_the_new_names():
    L = fa_hip.lib()
    local = {b"fa_varlen_fwd: ": lambda *a: L.fa_local_fwd(*a[:12], *a[14:]),
             b"fa_varlen_bwd: ": lambda *a: L.fa_local_bwd(*a[:16], *a[18:])}
    for call, n, name in ((_fwd, 6, b"fa_varlen_fwd: "), (_bwd, 10, b"fa_varlen_bwd: ")):
        bad = [None] + [P16] * (n - 1)
        assert call(L, 9, [None] * n, 0, 64, 0, 32, 1) == fa_hip.FA_ERR_INVALID_ARG
        assert L.fa_last_error() == name + b"unknown dtype"
        assert call(L, 1, [None] * n, 0, 64, 0, 32, 1) == fa_hip.FA_ERR_INVALID_ARG      # over the empty no-op
        assert L.fa_last_error().startswith(name + b"DimensionMismatch")
        for N, B in ((0, 1), (64, 0)):                                                    # empty: nothing is dereferenced
            assert call(L, 1, [None] * n, N, 64, 129, 32, B, lens=(None, None)) == 0
            assert call(L, 1, [None] * n, N, 64, 129, 32, B) == 0
        for N, Nk, d in ((64, 64, 129), (64, 63, 32), (1 << 30, 1 << 30, 4)):              # null over the shape checks
            assert call(L, 1, bad, N, Nk, d, 32, 1) == fa_hip.FA_ERR_INVALID_ARG
            assert L.fa_last_error() == name + b"null pointer"
        for i in range(n):
            ptrs = [P16] * n
            ptrs[i] = None
            assert call(L, 1, ptrs, 64, 64, 32, 32, 1, P16, 1 << 20) == fa_hip.FA_ERR_INVALID_ARG, i
        for d, dv in ((129, 32), (32, 129)):
            for Nk in (64, 63):
                rc = call(L, 1, [P16] * n, 64, Nk, d, dv, 1, P16, 1 << 20)
                assert rc == fa_hip.FA_ERR_UNSUPPORTED and b"head dimension" in L.fa_last_error()
        assert call(L, 1, [P16] * n, 1 << 30, (1 << 30) - 1, 4, 4, 1) == fa_hip.FA_ERR_UNSUPPORTED   # Nk >= N over the extents
        assert L.fa_last_error() == name + b"varlen attention needs Nk >= N (a query would see no key)"
        assert call(L, 1, [P16] * n, 1 << 30, 1 << 30, 4, 4, 1) == fa_hip.FA_ERR_UNSUPPORTED          # extents over the workspace
        assert L.fa_last_error() == name + b"extent exceeds the kernels' 32-bit addressing"
        # every refusal above carries the local entry point's status and message, the names apart
        for args in ((9, [None] * n, 0, 64, 0, 32, 1), (1, [None] * n, -1, 64, 32, 32, 1), (1, bad, 64, 64, 32, 32, 1),
                     (1, [P16] * n, 64, 64, 129, 32, 1), (1, [P16] * n, 64, 63, 32, 32, 1),
                     (1, [P16] * n, 1 << 30, 1 << 30, 4, 4, 1), (1, [P16] * n, 250, 250, 64, 64, 2)):   # the last: no workspace
            rc = call(L, args[0], args[1], *args[2:])
            msg = L.fa_last_error()
            full = (args[0], *args[1], *args[2:], P16, P16, 100, 0, 0.0, None, 0, None)
            rc2 = local[name](*full)
            assert rc == rc2 and rc != 0
            assert msg.replace(b"varlen", b"local") == L.fa_last_error()
    need = L.fa_varlen_bwd_workspace(1, 256, 256, 64, 64, 2)
    assert _bwd(L, 1, [P16] * 10, 256, 256, 64, 64, 2, None, need) == fa_hip.FA_ERR_WORKSPACE     # null, whatever the bytes
    assert L.fa_last_error() == b"fa_varlen_bwd: workspace missing or smaller than fa_varlen_bwd_workspace()"
    assert _bwd(L, 1, [P16] * 10, 256, 256, 64, 64, 2, P16, need - 1) == fa_hip.FA_ERR_WORKSPACE
    need = L.fa_varlen_fwd_workspace(1, 250, 250, 64, 64, 2)
    assert _fwd(L, 1, [P16] * 6, 250, 250, 64, 64, 2, None, need) == fa_hip.FA_ERR_WORKSPACE
    assert L.fa_last_error() == b"fa_varlen_fwd: workspace missing or smaller than fa_varlen_fwd_workspace()"
    assert _fwd(L, 1, [P16] * 6, 250, 250, 64, 64, 2, P16, need - 1) == fa_hip.FA_ERR_WORKSPACE


SHAPES = [(dt, N, Nk, d, dv, B) for dt in range(4) for N, Nk, d, dv, B in
          ((256, 256, 64, 64, 2), (250, 250, 64, 64, 2), (200, 333, 48, 40, 2), (1024, 1024, 64, 64, 4), (512, 640, 128, 128, 3),
           (100, 140, 32, 48, 2), (64, 63, 32, 32, 1), (0, 5, 8, 8, 1))]


def test_workspace_answers_are_the_local_ones():
    L = fa_hip.lib()
    for s in SHAPES:
        assert L.fa_varlen_fwd_workspace(*s) == L.fa_local_fwd_workspace(*s), s
        assert L.fa_varlen_bwd_workspace(*s) == L.fa_local_bwd_workspace(*s), s
    assert L.fa_varlen_bwd_workspace(1, 256, 256, 64, 64, 2) == 256 + 2 * 4 * 256 * 2 + 256


def test_plan_hooks_answer_without_a_device_and_treat_varlen_as_local():
    L = fa_hip.lib()
    f, fl, b, bl = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 6)()
    for dt, N, Nk, d, dv, B in SHAPES:
        if N < 1 or Nk < N:
            assert L.fa_debug_varlen_fwd_plan(dt, N, Nk, d, dv, B, 1, 1, 0, 256, f) == -1
            assert L.fa_debug_varlen_bwd_plan(dt, N, Nk, d, dv, B, 1, 0, 256, b) == -1
            continue
        nf, nb = L.fa_varlen_fwd_workspace(dt, N, Nk, d, dv, B), L.fa_varlen_bwd_workspace(dt, N, Nk, d, dv, B)
        for al in (0, 1):
            kf = L.fa_debug_varlen_fwd_plan(dt, N, Nk, d, dv, B, al, al, nf, 256, f)
            assert kf == L.fa_debug_local_fwd_plan(dt, N, Nk, d, dv, B, al, al, nf, 256, fl)
            assert f[0] == 1 and list(f)[1:] == list(fl)[1:] and f[4] == 1 and f[1] == 0   # varlen; never split, no causal order
            kb = L.fa_debug_varlen_bwd_plan(dt, N, Nk, d, dv, B, al, nb, 256, b)
            assert kb == L.fa_debug_local_bwd_plan(dt, N, Nk, d, dv, B, al, nb, 256, bl) and list(b) == list(bl)
            assert kb != 4                                                                  # never the single pass
    # the 16-bit GPU cases run the tiled MFMA forward (4, 5: one query block per wave; 6, 7: two) and the
    # two-pass MFMA backward (3), d's ragged shape through the padded slabs
    for name, ((N, Nk, d, dv, B, _, _), _, _, dts) in GPU_CASES.items():
        for dt in (1, 2):
            if ("bfloat16", "float16")[dt - 1] not in dts:
                continue
            nf, nb = L.fa_varlen_fwd_workspace(dt, N, Nk, d, dv, B), L.fa_varlen_bwd_workspace(dt, N, Nk, d, dv, B)
            kf = L.fa_debug_varlen_fwd_plan(dt, N, Nk, d, dv, B, 1, 1, nf, 256, f)
            kb = L.fa_debug_varlen_bwd_plan(dt, N, Nk, d, dv, B, 1, nb, 256, b)
            assert kf in (4, 5, 6, 7) and kb == 3, (name, kf, kb)
            assert (f[2], b[0]) == ((1, 1) if name == "d" else (0, 0)), name
    # the existing dense hooks keep refusing mask value 3
    out = (ctypes.c_int64 * 25)()
    assert L.fa_debug_dense_fwd_plan(1, 256, 256, 64, 64, 1, 3, 0, 2, 1, 1, 0, 256, out) == -1
    assert L.fa_debug_dense_bwd_plan(1, 256, 256, 64, 64, 1, 3, 0, 0, 3, -1, 1, 1 << 30, 256, out) == -1


def test_clamp_hook():
    L = fa_hip.lib()
    for N in (1, 100, 1 << 30):
        assert [L.fa_debug_varlen_clamp(x, N) for x in (-3, 0, N, N + 5)] == [0, 0, N, N]
        assert L.fa_debug_varlen_clamp(N - 1, N) == N - 1 and L.fa_debug_varlen_clamp(-(1 << 31), N) == 0


# ---- the Python mirror -----------------------------------------------------------------
def test_mirror_validates_host_lengths_before_any_device_is_touched():
    q, k, v = torch.zeros(8, 4, 2), torch.zeros(10, 4, 2), torch.zeros(10, 4, 2)
    for bad_q, bad_k in (((9, 1), None), ((-1, 1), None), (None, (11, 0)), (None, (0, -2)), ((1,), None), (None, (1, 2, 3)),
                         (torch.tensor([1.0, 2.0]), None), ([[1, 2]], None)):
        with pytest.raises(DimensionMismatch):
            fa_hip.varlen_fa(q, k, v, bad_q, bad_k)
        with pytest.raises(DimensionMismatch):
            fa_hip.varlen_fa_backward(q, k, v, q, q, torch.zeros(8, 1, 2), torch.zeros(8, 1, 2), bad_q, bad_k)
        with pytest.raises(DimensionMismatch):
            fa_hip.varlen_dpa(q, k, v, bad_q, bad_k)
    # valid host lengths pass that check: the next refusal is the device's (CPU arrays: no fallback)
    with pytest.raises(TypeError):
        fa_hip.varlen_fa(q, k, v, None, None)
    with pytest.raises(fa_hip.FlashAttentionError):
        fa_hip.varlen_fa(k, q, q[:, :, :], None, None)       # Nk < N
    for name in ("varlen_fa", "varlen_fa_", "varlen_fa_backward", "varlen_dpa"):
        assert name in fa_hip.__all__ and callable(getattr(fa_hip, name))
