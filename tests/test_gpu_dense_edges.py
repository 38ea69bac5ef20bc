"""Prologue / epilogue edges of the LDS-staged forward (`w8q2_wide`, `w8b64_wide`).

The default path brings Q in by LDS-DMA and sends O out through the same LDS image
(token-pair b32 image writes, each wave storing the 16-B chunks of its own tokens).
Every case compares it bitwise with variant 20 (the same geometries with per-element
Q gathers and O stores) on O, l and m, and with the float64 oracle at the suite's
tolerances.  Shapes: one 512-row block, one full block plus an 8-token one, two full
blocks plus an 8-token one; one key tile and one plus an 8-key ragged one; every head
dim class and a padded one; three slabs; bf16 and f16.  Grids stay under the split-KV
threshold's tile count (fewer than 4 key tiles) or at >= 256 workgroups, so neither
run of a pair takes the split path.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from conftest import assert_close, assert_lm_close
from oracle import fa_oracle as O

pytestmark = pytest.mark.gpu

DT = {"bfloat16": torch.bfloat16, "float16": torch.float16}


@pytest.fixture(scope="module")
def fa():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    fa_hip.lib()
    return fa_hip


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _round(a, dtype):
    return torch.tensor(a).to(DT[dtype]).double().numpy()


def _variant20(fa, fn):
    L = fa.lib()
    old = L.fa_debug_set_fwd_variant(20)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.fa_debug_set_fwd_variant(old)
    return out


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("d,dv", [(64, 64), (48, 32), (32, 64), (128, 128)])
@pytest.mark.parametrize("Nk", [64, 72])
@pytest.mark.parametrize("N", [512, 520, 1032])
def test_edges_bitwise_and_oracle(fa, N, Nk, d, dv, dtype):
    B = 3
    rng = np.random.default_rng(N * 7 + Nk * 3 + d + dv)
    q, k, v = (_round(rng.standard_normal(sh), dtype) for sh in ((N, d, B), (Nk, d, B), (Nk, dv, B)))
    Q, K, V = (fa.jl_tensor(a, DT[dtype]) for a in (q, k, v))
    a = [t.clone() for t in fa.dense_fa(Q, K, V)]
    b = _variant20(fa, lambda: fa.dense_fa(Q, K, V))
    for x, y, nm in zip(a, b, ("y", "l", "m")):
        assert torch.equal(x, y), nm
    yr, lr, mr = O.dense_fa3(q, k, v)
    assert_close(_np(a[0]), yr, dtype, "y")
    assert_lm_close(_np(a[1]), lr, dtype, "l")
    assert_lm_close(_np(a[2]), mr, dtype, "m")


def test_edges_forced_rescale(fa):
    """Rescale threshold 0 (fa_debug_set_rescale_threshold, as test_gpu_dense.py's
    lazy-rescale test) on scores whose max climbs over the key sweep: every tile
    rescales O and l before the epilogue normalises them.  128 slabs of 520 rows
    (256 workgroups, no split-KV); the oracle is checked on four slabs."""
    L = fa.lib()
    rng = np.random.default_rng(23)
    N, Nk, d, B = 520, 640, 64, 128
    u = rng.standard_normal(d); u /= np.linalg.norm(u)
    q = np.repeat((u * 8.0)[None, :, None], N, 0).repeat(B, 2) + 0.3 * rng.standard_normal((N, d, B))
    t = np.linspace(-1.0, 1.0, Nk) * 60.0 * math.sqrt(d) / 8.0 / 2.0
    k = t[:, None, None] * u[None, :, None] + 0.3 * rng.standard_normal((Nk, d, B))
    v = rng.uniform(-4, 4, (Nk, d, B))
    q, k, v = (_round(a, "bfloat16") for a in (q, k, v))
    Q, K, V = (fa.jl_tensor(a, torch.bfloat16) for a in (q, k, v))
    old = L.fa_debug_set_rescale_threshold(0.0)
    try:
        a = [x.clone() for x in fa.dense_fa(Q, K, V)]
        b = _variant20(fa, lambda: fa.dense_fa(Q, K, V))
    finally:
        L.fa_debug_set_rescale_threshold(old)
    for x, y, nm in zip(a, b, ("y", "l", "m")):
        assert torch.equal(x, y), nm
    S = [0, 1, 77, 127]
    yr, lr, mr = O.dense_fa3(q[:, :, S], k[:, :, S], v[:, :, S])
    assert_close(_np(a[0][:, :, S]), yr, "bfloat16", "y")
    assert_lm_close(_np(a[1][:, :, S]), lr, "bfloat16", "l")
    assert_lm_close(_np(a[2][:, :, S]), mr, "bfloat16", "m")


@pytest.mark.parametrize("N,d,dv", [(520, 64, 64), (1032, 48, 32), (520, 128, 128)])
def test_edges_rows_past_n_untouched(fa, N, d, dv):
    """O, l and m are views of larger allocations filled with a sentinel: one guard slab
    before and one after.  The last block holds 8 tokens of 512 (256 at d = 128); a store
    of a row at or past N would land in the next feature row (caught by the comparison
    with variant 20) or, from the last feature row of the last slab, in the guard."""
    B, Nk = 3, 72
    rng = np.random.default_rng(N + d)
    Q, K, V = (fa.jl_tensor(rng.standard_normal(sh), torch.bfloat16) for sh in ((N, d, B), (Nk, d, B), (Nk, dv, B)))
    SENT = -768.0   # exact in bf16
    big = [fa.jl_empty((N, c, B + 2), dt) for c, dt in ((dv, torch.bfloat16), (1, torch.float32), (1, torch.float32))]
    for t in big:
        t.fill_(SENT)
    Ov, lv, mv = (t[:, :, 1:B + 1] for t in big)
    assert all(fa.is_jl_contiguous(t) for t in (Ov, lv, mv)) and Ov.data_ptr() % 16 == 0
    fa.dense_fa_(Ov, lv, mv, Q, K, V)
    torch.cuda.synchronize()
    ref = _variant20(fa, lambda: fa.dense_fa(Q, K, V))
    for x, y, nm in zip((Ov, lv, mv), ref, ("y", "l", "m")):
        assert torch.equal(x, y), nm
    for t, nm in zip(big, ("O", "l", "m")):
        assert bool((t[:, :, 0] == SENT).all()) and bool((t[:, :, B + 1] == SENT).all()), f"{nm}: guard slab written"
