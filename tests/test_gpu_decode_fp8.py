"""GPU tests of decode attention over an fp8 cache (fa_decode_fp8_fwd through
fa_hip.decode_fp8_fa): K and V as e4m3fn bytes plus one float32 scale per KV slab, against the
float64 yardstick tests/varlen_ref.py on the DEQUANTISED cache (k8 * ks, v8 * vs, exact in
float64) repeated `group` times, on bf16-representable queries seeded per shape.  Every e4m3fn
value is exact in bf16 and fp16 and the scales enter through fp32 factors only, so live rows
meet conftest's tolerances for the Q dtype; empty rows (past nq, or key-less) are exact: O = 0
and l = 0 bitwise, m = -inf."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from conftest import assert_close, assert_lm_close
from varlen_ref import keyless_rows, varlen_fwd_ref

pytestmark = pytest.mark.gpu
DT = {"bfloat16": torch.bfloat16, "float16": torch.float16}
BF, F16 = "bfloat16", "float16"
# (N, G, Nk, d, dv, B), q_lens, k_lens, (left, right), dtypes
CASES = {
    1: ((1, 1, 528, 64, 64, 6), None, [0, 1, 63, 64, 65, 528], (-1, 0), (BF, F16)),   # wide loads; tile and share edges; empty slab
    2: ((4, 8, 256, 64, 64, 4), [4, 2, 0, 3], [256, 1, 100, 130], (-1, 0), (BF,)),     # full 32-row tile; dead rows
    3: ((3, 5, 333, 48, 40, 2), [3, 1], [333, 200], (-1, -1), (BF, F16)),              # byte loads; odd head dims
    4: ((2, 2, 264, 32, 32, 3), None, None, (-1, 0), (BF,)),                           # Nk % 8 == 0 but % 16 != 0: byte loads
    5: ((8, 4, 1088, 128, 128, 2), [8, 5], [1088, 700], (100, 0), (BF,)),              # D = 128 image; left window
    6: ((1, 1, 16, 16, 8, 1), None, [5], (-1, 0), (BF,)),                              # one partial tile
}
HAS_EMPTY = (1, 2, 3, 5)   # the cases with rows past nq or key-less queries
NSPLITS = (0, 1, 3, 7)


@pytest.fixture(scope="module")
def fa():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    fa_hip.lib()
    return fa_hip


def _np(t):
    return t.detach().double().cpu().numpy()


def e4m3(a):
    """float64 array rounded to e4m3fn on the CPU, as float64."""
    return torch.tensor(a, dtype=torch.float32).to(torch.float8_e4m3fn).to(torch.float32).double().numpy()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """bf16-representable q (N, d, B*G), e4m3fn-representable k8 (Nk, d, B), v8 (Nk, dv, B), and
    per-slab scales in [0.25, 2), no power of two: float64 / float32, shared, never modified."""
    N, G, Nk, d, dv, B = CASES[case][0]
    rng = np.random.default_rng(N * 131 + Nk * 17 + d * 7 + dv + G)
    q = torch.tensor(rng.standard_normal((N, d, B * G))).to(torch.bfloat16).double().numpy()
    k8, v8 = e4m3(rng.standard_normal((Nk, d, B))), e4m3(rng.standard_normal((Nk, dv, B)))
    ks, vs = (rng.uniform(0.25, 2.0, B).astype(np.float32) for _ in range(2))
    return q, k8, v8, ks, vs


def rep(x, G):
    return None if x is None else np.repeat(np.asarray(x), G)


@functools.lru_cache(maxsize=None)
def reference(case, scaled=True):
    """(O, l, m) float64 and the (N, B*G) mask of empty rows."""
    (N, G, Nk, d, dv, B), ql, kl, (left, right), _ = CASES[case]
    q, k8, v8, ks, vs = inputs(case)
    k = k8 * ks.astype(np.float64) if scaled else k8
    v = v8 * vs.astype(np.float64) if scaled else v8
    ref = varlen_fwd_ref(q, np.repeat(k, G, axis=2), np.repeat(v, G, axis=2), rep(ql, G), rep(kl, G), left, right)
    nq = rep(ql, G) if ql is not None else [N] * (B * G)
    nk = rep(kl, G) if kl is not None else [Nk] * (B * G)
    er = np.stack([(np.arange(N) >= nq[b]) | keyless_rows(N, Nk, nq[b], nk[b], left, right) for b in range(B * G)], axis=1)
    return ref, er


def cache(fa, a, odd=False):
    """A float64 array of e4m3fn values as a Julia-layout fp8 device tensor; odd: as uint8, in a
    buffer that starts one byte past an aligned address."""
    by = torch.tensor(a, dtype=torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)
    if not odd:
        return fa.jl_tensor(by, torch.uint8).view(torch.float8_e4m3fn)
    buf = torch.empty(by.numel() + 1, dtype=torch.uint8, device="cuda")
    t = buf[1:].view(tuple(reversed(by.shape))).permute(2, 1, 0)
    t.copy_(by)
    assert t.data_ptr() % 2 == 1
    return t


def run(fa, case, dtype, nsplit, arrays=None, scaled=True, odd=False):
    (N, G, Nk, d, dv, B), ql, kl, (left, right), _ = CASES[case]
    q, k8, v8, ks, vs = inputs(case)
    if arrays is not None:
        q, k8, v8 = arrays
    Q, K8, V8 = fa.jl_tensor(q, DT[dtype]), cache(fa, k8, odd), cache(fa, v8, odd)
    dev = lambda x, t: None if x is None else torch.tensor(np.asarray(x), dtype=t, device="cuda")
    KS, VS = (dev(ks, torch.float32), dev(vs, torch.float32)) if scaled else (None, None)
    old = fa.lib().fa_debug_set_decode_nsplit(nsplit)
    try:
        out = fa.decode_fp8_fa(Q, K8, V8, KS, VS, dev(kl, torch.int32), dev(ql, torch.int32), G, left, right)
    finally:
        fa.lib().fa_debug_set_decode_nsplit(old)
    torch.cuda.synchronize()
    return out


def bitwise_zero(t):
    t = t.contiguous()
    return int(torch.count_nonzero(t.view({2: torch.int16, 4: torch.int32}[t.element_size()]))) == 0


def assert_matches(out, case, dtype, what, scaled=True):
    (o, l, m), er = reference(case, scaled)
    O, L, M = out
    live = ~er
    assert live.any(), "the case has no live row"
    assert er.any() == (case in HAS_EMPTY)
    for t in out:
        assert not torch.isnan(t).any()
    ert = torch.tensor(er, device="cuda")[:, None, :]
    assert bitwise_zero(torch.where(ert, O, torch.zeros_like(O))) and bitwise_zero(torch.where(ert, L, torch.zeros_like(L)))
    assert bool((M[ert] == float("-inf")).all())
    sel = lambda a: np.where(live[:, None, :], a, 0.0)
    print(f"{what}: max |dO| {np.abs(sel(_np(O)) - sel(o)).max():.3e}, max |dl| {np.abs(sel(_np(L)) - sel(l)).max():.3e}, "
          f"max |dm| {np.abs(sel(_np(M)) - sel(m)).max():.3e}")
    assert_close(sel(_np(O)), sel(o), dtype, what + " O")
    assert_lm_close(sel(_np(L)), sel(l), dtype, what + " l")
    assert_lm_close(sel(_np(M)), sel(m), dtype, what + " m")


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("case,dtype", [(c, dt) for c in CASES for dt in CASES[c][4]])
def test_forward_vs_reference(fa, case, dtype, nsplit):
    assert_matches(run(fa, case, dtype, nsplit), case, dtype, f"case {case} {dtype} nsplit {nsplit}")


@pytest.mark.parametrize("case", (2, 3))
def test_no_scales_mean_one(fa, case):
    assert_matches(run(fa, case, BF, 3, scaled=False), case, BF, f"case {case} without scales", scaled=False)


@pytest.mark.parametrize("case", (1, 2, 5))
def test_m_is_bitwise_equal_across_split_counts(fa, case):
    m1, m3, m7 = (run(fa, case, BF, n)[2] for n in (1, 3, 7))
    assert torch.equal(m1, m3) and torch.equal(m1, m7)


@pytest.mark.parametrize("case", (1, 3, 5))
def test_nothing_leaks_from_the_padding(fa, case):
    (N, G, Nk, d, dv, B), ql, kl, _, _ = CASES[case]
    base = run(fa, case, BF, 3)
    for fill in (0.0, 448.0):
        q, k8, v8 = (a.copy() for a in inputs(case)[:3])
        for b in range(B):
            nq, nk = (N if ql is None else ql[b]), (Nk if kl is None else kl[b])
            q[nq:, :, b * G:(b + 1) * G] = fill * np.where(np.arange(N - nq) % 2 == 0, 1.0, -1.0)[:, None, None]
            for a in (k8, v8):
                a[nk:, :, b] = fill * np.where(np.arange(Nk - nk) % 2 == 0, 1.0, -1.0)[:, None]
        got = run(fa, case, BF, 3, arrays=(q, k8, v8))
        for x, y in zip(got, base):
            assert torch.equal(x, y), f"fill {fill}"


@pytest.mark.parametrize("case,nsplit", [(5, 0), (5, 3), (3, 3)])
def test_two_runs_are_bitwise_equal(fa, case, nsplit):
    a, b = run(fa, case, BF, nsplit), run(fa, case, BF, nsplit)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("case", (1, 5))
def test_cache_at_an_odd_byte_offset(fa, case):
    """Shapes that take the wide loads when aligned: a uint8 view one byte off must take the
    byte loads (a wide load there would be misaligned) and match the reference."""
    assert_matches(run(fa, case, BF, 3, odd=True), case, BF, f"case {case} at an odd byte offset")
