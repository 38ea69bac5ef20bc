"""CPU checks of the ill-conditioned input families (tests/cond_inputs.py) and of the oracle's
scale keyword.  For every family at (N, Nk) = (256, 256), d = dv in {64, 128}:

  * the float64 gradients are not degenerate (a test on them can fail): max|dQ|, max|dK| and
    max|dV| >= 0.05 (anti: max|dV| only; there P barely depends on q);
  * the kernels' formulation itself (lowp_backward: float32 scores and statistics, P and dS
    rounded to the 16-bit type) stays within GTOL = 2e-5 / 2e-2 / 5e-3 of the float64 backward
    on both metrics of assert_grad_close, so the GPU tests' budget max(GTOL, 2 e_ref) is within
    a factor 2 of GTOL at these shapes (it is GTOL in every probe but one).
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import cond_inputs as C
from oracle import fa_oracle as O

N = NK = 256
B = 2
DTYPE_OF = {None: "float32", "bf16": "bfloat16", "fp16": "float16"}


@functools.lru_cache(maxsize=None)
def case(name, d, dtype):
    """Inputs, the oracle's forward and float64 backward (shared, never modified)."""
    q, k, v, do, scale = C.family(name, N, NK, d, d, B, dtype)
    o, l, m = O.dense_fa3(q, k, v, scale=scale)
    ref = O.dense_fa_backward(q, k, v, o, do, l, m, scale=scale)
    return (q, k, v, do, scale), (o, l, m), ref


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", C.FAMILIES)
def test_family_is_representable_and_seeded(name, d):
    for dtype in ("bfloat16", "float16", "float32"):
        a = C.family(name, N, NK, d, d, B, dtype)
        b = C.family(name, N, NK, d, d, B, dtype)
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(x, y)
            assert np.array_equal(C.round_to(x, dtype), x), f"{name}: not representable in {dtype}"
        assert a[4] == b[4] and (a[4] > 0) == (name in ("hot", "cold"))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", C.FAMILIES)
def test_family_regime(name, d):
    """The regime each family is there for."""
    (q, k, v, do, scale), (o, l, m), _ = case(name, d, "bfloat16")
    pmax = 1.0 / l            # the largest probability of a row: exp(m - m) / l
    print(f"{name} d {d}: m {m.min():.1f}..{m.max():.1f}, median max P {np.median(pmax):.3f}")
    if name == "hot":
        assert np.median(pmax) >= 0.3 and m.min() >= 5.0
    elif name == "cold":
        assert pmax.max() <= 0.05
    elif name == "offset":
        assert m.min() >= 8.0 * math.sqrt(d)
    elif name == "anti":
        assert m.max() <= -7.0 * math.sqrt(d)
    else:
        pairs = C.hot_pairs(N, NK, B)
        assert len({j // 64 for _, j, _ in pairs}) == 3 and len({b for _, _, b in pairs}) == B
        for i, j, b in pairs:
            assert m[i, 0, b] >= 6.0 * math.sqrt(d) and pmax[i, 0, b] >= 0.99
            # the hot key draws weight from many rows: it is the heaviest key of a tenth of them
            s = C.tau_of(scale, d) * (q[:, :, b] @ k[:, :, b].T)
            assert np.count_nonzero(s.argmax(axis=1) == j) >= N // 10


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", C.FAMILIES)
def test_gradients_not_degenerate(name, d):
    _, _, (dq, dk, dv) = case(name, d, "bfloat16")
    mx = [float(np.abs(g).max()) for g in (dq, dk, dv)]
    print(f"{name} d {d}: max|dQ| {mx[0]:.3g}, max|dK| {mx[1]:.3g}, max|dV| {mx[2]:.3g}")
    assert mx[2] >= 0.05
    if name != "anti":
        assert mx[0] >= 0.05 and mx[1] >= 0.05


@pytest.mark.parametrize("round16", [None, "bf16", "fp16"], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", C.FAMILIES)
def test_formulation_within_gtol(name, d, round16):
    dtype = DTYPE_OF[round16]
    (q, k, v, do, scale), (o, l, m), ref = case(name, d, dtype)
    low = C.lowp_backward(q, k, v, do, o, l, m, scale, round16)
    for x, y, nm in zip(low, ref, ("dQ", "dK", "dV")):
        err, rel = C.grad_metrics(x, y)
        print(f"{name} d {d} {dtype} {nm}: max err/max|y| {err:.2e}, norm rel {rel:.2e}")
        assert err <= C.GTOL[dtype] and rel <= C.GTOL[dtype], (nm, err, rel)
    # e_ref restates the same on the rounded forward outputs.  2 e_ref exceeds GTOL in one
    # probe only (offset, d = 64, bf16, dQ's norm metric at 1.1e-2: budget 2.2e-2)
    e = C.e_ref(q, k, v, do, scale, dtype)
    print(f"{name} d {d} {dtype}: e_ref {e:.2e}, budget {C.budget(dtype, e):.2e}")
    assert e <= C.GTOL[dtype]


def test_helper_references_agree_with_the_oracle():
    """cond_inputs' own float64 forward / backward (they take a mask) equal the oracle's
    where there is no mask, and causal_ref / circ_bwd_ref where there is one."""
    from causal_ref import causal_bwd_ref, causal_fwd_ref
    from circ_bwd_ref import circulant_bwd_ref, circulant_fwd_ref
    q, k, v, do, scale = C.family("hot", 40, 56, 16, 8, 2, "bfloat16")
    o, l, m = C.forward_f64(q, k, v, scale)
    for x, y in zip((o, l, m), O.dense_fa3(q, k, v, scale=scale)):
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)
    for x, y in zip(C.backward_f64(q, k, v, do, o, l, m, scale),
                    O.dense_fa_backward(q, k, v, o, do, l, m, scale=scale)):
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)
    mk = C.causal_mask(40, 56)
    o, l, m = C.forward_f64(q, k, v, scale, mk)
    for x, y in zip((o, l, m), causal_fwd_ref(q, k, v, scale)):
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)
    for x, y in zip(C.backward_f64(q, k, v, do, o, l, m, scale, mk), causal_bwd_ref(q, k, v, o, do, l, m, scale)):
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)
    q, k, v, do, scale = C.family("cold", 40, 40, 16, 8, 2, "bfloat16")
    mk = C.band_mask(40, 9)
    o, l, m = C.forward_f64(q, k, v, scale, mk)
    for x, y in zip((o, l, m), circulant_fwd_ref(q, k, v, 9, scale)):
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)
    for x, y in zip(C.backward_f64(q, k, v, do, o, l, m, scale, mk),
                    circulant_bwd_ref(q, k, v, o, do, l, m, 9, scale)):
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)


# ---- the forward yardstick (tests/test_gpu_forward_conditioning.py) --------------------------
def _forward_rows():
    """Every (entry, shape, dtype) of the GPU table once (the yardstick does not depend on the
    route), Float64 aside: there the reference is its own yardstick."""
    import test_gpu_forward_conditioning as G
    rows = sorted({(e, s, dt) for e, _, s, dts in G.ROUTES for dt in dts if dt != "float64"})
    return [pytest.param(e, s, dt, name, id=f"{e}-{G._sid(s)}-{dt}-{name}") for e, s, dt in rows for name in C.FAMILIES]


@pytest.mark.parametrize("entry,shape,dtype,name", _forward_rows())
def test_forward_formulation_leaves_headroom(entry, shape, dtype, name):
    """The condition on the inputs of the GPU forward cases, checked before any GPU run: the
    kernels' formulation alone (lowp_forward, with m_used at and 8 log2 units below the row
    maximum) uses at most half of each limit that the GPU test applies (O norm-wise and
    elementwise, l, m), on the slabs that test checks.  A case above 0.5 needs another shape or
    seed, not another limit."""
    import test_gpu_forward_conditioning as G
    eref = G.case(entry, G.resolve(shape, G.MI355X_CUS), dtype, name)[5]
    print(f"{entry} {G._sid(shape)} {dtype} {name}: " + ", ".join(f"{nm} {s:.3f}" for nm, s in eref.items()))
    assert max(eref.values()) <= 0.5, eref


@pytest.mark.parametrize("lag", [0.0, 8.0])
def test_lowp_forward_mask_is_a_restriction_to_the_visible_keys(lag):
    """lowp_forward with a mask (or counts of 0 / 1) gives each row what the unmasked call gives
    on that row's visible keys alone (float32 scores: equal up to the summation order)."""
    q, k, v, _, scale = C.family("hot", 40, 56, 16, 8, 2, "bfloat16")
    close = lambda x, y: np.abs(x - y).max() <= 1e-5 * max(np.abs(y).max(), 1.0)
    for mk in (C.causal_mask(40, 56), C.band_mask(40, 9)):
        kk, vv = (k, v) if mk.shape[1] == 56 else (k[:40], v[:40])
        full = C.lowp_forward(q, kk, vv, scale, None, mk, lag_log2=lag)
        same = C.lowp_forward(q, kk, vv, scale, None, counts=mk.astype(np.int64), lag_log2=lag)
        for x, y in zip(full, same):
            assert np.array_equal(x, y)
        for i in (0, 7, 39):
            vis = np.flatnonzero(mk[i])
            row = C.lowp_forward(q[i:i + 1], kk[vis], vv[vis], scale, None, lag_log2=lag)
            for x, y in zip(row, full):
                assert close(x, y[i:i + 1])
    # and the model is the float64 forward up to float32 rounding
    for x, y in zip(C.lowp_forward(q, k, v, scale, None, lag_log2=lag), C.forward_f64(q, k, v, scale)):
        assert np.abs(x - y).max() <= 1e-4 * max(np.abs(y).max(), 1.0)


@pytest.mark.parametrize("N,W", [(40, 9), (40, 40), (12, 30), (7, 15), (30, 7)])
def test_band_counts_agree_with_the_oracle(N, W):
    """band_counts against the reference's own band index (oracle.circulant_index), against
    band_mask where W <= N, and, through forward_f64(counts=), against circulant_fa3."""
    cnt = C.band_counts(N, W)
    J = O.circulant_index(N, W)                       # (W, N)
    want = np.zeros((N, N), dtype=np.int64)
    np.add.at(want, (np.broadcast_to(np.arange(N)[None, :], (W, N)), J), 1)
    assert np.array_equal(cnt, want) and np.all(cnt.sum(axis=1) == W)
    if W <= N:
        assert np.array_equal(cnt, C.band_mask(N, W).astype(np.int64))
    else:
        assert cnt.max() >= 2 and cnt.min() >= 1
    q, k, v, _, _ = C.family("hotkeys", N, N, 16, 8, 2, "bfloat16", mask=cnt > 0)
    for x, y in zip(C.forward_f64(q, k, v, 0.0, counts=cnt), O.circulant_fa3(q, k, v, W)):
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)


def test_hot_pairs_follow_the_mask():
    for mk in (C.causal_mask(200, 328), C.band_mask(136, 33)):
        for i, j, b in C.hot_pairs(mk.shape[0], mk.shape[1], 2, mk):
            assert mk[i, j]


def test_hot_pairs_are_unchanged_where_every_key_is_seen():
    """hot_pairs takes its keys from the thirds of the SEEN keys.  Where every key is seen (no
    mask, a causal mask, a circulant band) that is the thirds of [0, Nk): the values below are the
    ones the helper returned before it learned of unseen keys, and the hotkeys inputs built on them
    are the same bits (CRC-32 of k's bytes)."""
    import zlib
    assert C.hot_pairs(256, 256, 2) == [(51, 42, 0), (161, 129, 1), (8, 215, 0)]
    assert C.hot_pairs(30, 2, 3) == [(13, 0, 0), (3, 1, 1)]
    assert C.hot_pairs(200, 328, 2, C.causal_mask(200, 328)) == [(100, 54, 0), (118, 165, 1), (173, 275, 0)]
    assert C.hot_pairs(520, 584, 2, C.causal_mask(520, 584)) == [(276, 97, 0), (374, 293, 1), (472, 488, 0)]
    assert C.hot_pairs(77, 130, 1, C.causal_mask(77, 130)) == [(38, 21, 0), (45, 66, 0), (67, 110, 0)]
    assert C.hot_pairs(136, 136, 1, C.band_mask(136, 33)) == [(22, 22, 0), (69, 69, 0), (115, 115, 0)]
    assert C.hot_pairs(64, 64, 2, C.band_counts(64, 150) > 0) == [(32, 10, 0), (32, 33, 1), (32, 55, 0)]
    q, k, _, _, _ = C.family("hotkeys", 200, 328, 128, 64, 2, "bfloat16", mask=C.causal_mask(200, 328))
    assert (zlib.crc32(k.tobytes()), zlib.crc32(q.tobytes())) == (3780295603, 2238232506)
    q, k, _, _, _ = C.family("hotkeys", 256, 256, 64, 64, 2, "float16")
    assert (zlib.crc32(k.tobytes()), zlib.crc32(q.tobytes())) == (2961104623, 436521518)
    # a per-slab mask that is the same in every slab is the shared mask
    mk = C.causal_mask(200, 328)
    assert C.hot_pairs(200, 328, 2, np.repeat(mk[:, :, None], 2, axis=2)) == C.hot_pairs(200, 328, 2, mk)


@pytest.mark.parametrize("s", [0.05, 0.7])
def test_oracle_scale_is_a_rescaling_of_q_and_k(s):
    rng = np.random.default_rng(7)
    N_, Nk_, d, dv = 50, 70, 12, 6
    q, k, v = rng.standard_normal((N_, d, 2)), rng.standard_normal((Nk_, d, 2)), rng.standard_normal((Nk_, dv, 2))
    f = math.sqrt(s * math.sqrt(d))
    for x, y in zip(O.dense_fa3(q, k, v, scale=s), O.dense_fa3(q * f, k * f, v)):
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)
    # scale <= 0 is the default
    for sc in (0.0, -1.0):
        for x, y in zip(O.dense_fa3(q, k, v, scale=sc), O.dense_fa3(q, k, v)):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("s", [0.05, 0.7])
def test_oracle_backward_scale_vs_autograd(s):
    rng = np.random.default_rng(8)
    N_, Nk_, d, dv, B_ = 50, 70, 12, 6, 2
    q, k = rng.standard_normal((N_, d, B_)), rng.standard_normal((Nk_, d, B_))
    v, do = rng.standard_normal((Nk_, dv, B_)), rng.standard_normal((N_, dv, B_))
    o, l, m = O.dense_fa3(q, k, v, scale=s)
    got = O.dense_fa_backward(q, k, v, o, do, l, m, scale=s)
    tq, tk, tv = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    P = torch.softmax(s * torch.einsum("nfb,kfb->bnk", tq, tk), dim=-1)
    out = torch.einsum("bnk,kcb->ncb", P, tv)
    assert np.abs(out.detach().numpy() - o).max() <= 1e-12
    out.backward(torch.tensor(do))
    for x, t, nm in zip(got, (tq, tk, tv), ("dQ", "dK", "dV")):
        y = t.grad.numpy()
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0), nm


@pytest.mark.parametrize("s", [0.0, 0.3])
def test_oracle_windowed_scale(s):
    """windowed_fa / windowed_fa_backward pass scale through: equal to the rescaled inputs'
    default-scale results (dq, dk pick up the factor by the chain rule)."""
    rng = np.random.default_rng(9)
    d, dv = 8, 6
    q, k = rng.standard_normal((8, 5, d, 2)), rng.standard_normal((8, 5, d, 2))
    v, dy = rng.standard_normal((8, 5, dv, 2)), rng.standard_normal((8, 5, dv, 2))
    f = math.sqrt(C.tau_of(s, d) * math.sqrt(d))
    a = O.windowed_fa(q, k, v, 3, 3, 1, scale=s)
    b = O.windowed_fa(q * f, k * f, v, 3, 3, 1)
    for x, y in zip(a, b):
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)
    ga = O.windowed_fa_backward(q, k, v, dy, 3, 3, 1, scale=s)
    gb = O.windowed_fa_backward(q * f, k * f, v, dy, 3, 3, 1)
    for x, y, g in zip(ga, gb, (f, f, 1.0)):
        assert np.abs(x - g * y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)
