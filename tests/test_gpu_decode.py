"""GPU tests of decode attention (fa_decode_fwd through fa_hip.decode_fa): split-KV with `group`
query slabs per KV slab, against the float64 yardstick tests/varlen_ref.py called on the cache
repeated `group` times (the definition of grouping), on bf16-representable inputs seeded per
shape.  Live rows under conftest's tolerances; empty rows (past nq, or key-less) exactly:
O = 0 and l = 0 bitwise, m = -inf."""
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
    1: ((1, 1, 520, 64, 64, 6), None, [0, 1, 63, 64, 65, 520], (-1, 0), (BF, F16)),
    2: ((4, 8, 256, 64, 64, 4), [4, 2, 0, 3], [256, 1, 100, 130], (-1, 0), (BF,)),
    3: ((3, 5, 333, 48, 40, 2), [3, 1], [333, 200], (-1, -1), (BF, F16)),
    4: ((8, 4, 1088, 128, 128, 2), [8, 5], [1088, 700], (100, 0), (BF,)),
    5: ((2, 2, 192, 32, 32, 3), None, None, (-1, 0), (BF,)),
    6: ((1, 1, 8, 16, 8, 1), None, [5], (-1, 0), (BF,)),
}
HAS_EMPTY = (1, 2, 3, 4)   # the cases with rows past nq or key-less queries (5 and 6: every row sees a key)
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


@functools.lru_cache(maxsize=None)
def inputs(case):
    """bf16-representable q (N, d, B*G), k (Nk, d, B), v (Nk, dv, B): float64, shared, never modified."""
    N, G, Nk, d, dv, B = CASES[case][0]
    rng = np.random.default_rng(N * 131 + Nk * 17 + d * 7 + dv + G)
    bf = lambda a: torch.tensor(a).to(torch.bfloat16).double().numpy()
    return tuple(bf(rng.standard_normal(s)) for s in ((N, d, B * G), (Nk, d, B), (Nk, dv, B)))


def rep(x, G):
    return None if x is None else np.repeat(np.asarray(x), G)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(O, l, m) float64 and the (N, B*G) mask of empty rows."""
    (N, G, Nk, d, dv, B), ql, kl, (left, right), _ = CASES[case]
    q, k, v = inputs(case)
    ref = varlen_fwd_ref(q, np.repeat(k, G, axis=2), np.repeat(v, G, axis=2), rep(ql, G), rep(kl, G), left, right)
    nq = rep(ql, G) if ql is not None else [N] * (B * G)
    nk = rep(kl, G) if kl is not None else [Nk] * (B * G)
    er = np.stack([(np.arange(N) >= nq[b]) | keyless_rows(N, Nk, nq[b], nk[b], left, right) for b in range(B * G)], axis=1)
    return ref, er


def run(fa, case, dtype, nsplit, arrays=None, group=None, lens=None):
    (N, G, Nk, d, dv, B), ql, kl, (left, right), _ = CASES[case]
    q, k, v = inputs(case) if arrays is None else arrays
    ql, kl = (ql, kl) if lens is None else lens
    Q, K, V = (fa.jl_tensor(a, DT[dtype]) for a in (q, k, v))
    dev = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=torch.int32, device="cuda")
    old = fa.lib().fa_debug_set_decode_nsplit(nsplit)
    try:
        out = fa.decode_fa(Q, K, V, dev(kl), dev(ql), G if group is None else group, left, right)
    finally:
        fa.lib().fa_debug_set_decode_nsplit(old)
    torch.cuda.synchronize()
    return out


def bitwise_zero(t):
    t = t.contiguous()
    return int(torch.count_nonzero(t.view({2: torch.int16, 4: torch.int32}[t.element_size()]))) == 0


def assert_matches(out, case, dtype, what):
    (o, l, m), er = reference(case)
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


@pytest.mark.parametrize("case", (1, 2, 4))
def test_m_is_bitwise_equal_across_split_counts(fa, case):
    m1, m3, m7 = (run(fa, case, BF, n)[2] for n in (1, 3, 7))
    assert torch.equal(m1, m3) and torch.equal(m1, m7)


@pytest.mark.parametrize("case", (1, 2, 4))
def test_nothing_leaks_from_the_padding(fa, case):
    (N, G, Nk, d, dv, B), ql, kl, _, _ = CASES[case]
    base = run(fa, case, BF, 3)
    for fill in (0.0, 3e4):
        q, k, v = (a.copy() for a in inputs(case))
        for b in range(B):
            nq, nk = (N if ql is None else ql[b]), (Nk if kl is None else kl[b])
            q[nq:, :, b * G:(b + 1) * G] = fill * np.where(np.arange(N - nq) % 2 == 0, 1.0, -1.0)[:, None, None]
            for a in (k, v):
                a[nk:, :, b] = fill * np.where(np.arange(Nk - nk) % 2 == 0, 1.0, -1.0)[:, None]
        got = run(fa, case, BF, 3, arrays=(q, k, v))
        for x, y in zip(got, base):
            assert torch.equal(x, y), f"fill {fill}"


@pytest.mark.parametrize("nsplit", (0, 3))
def test_two_runs_are_bitwise_equal(fa, nsplit):
    a, b = run(fa, 4, BF, nsplit), run(fa, 4, BF, nsplit)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_group_equals_repeated_cache(fa):
    (N, G, Nk, d, dv, B), ql, kl, _, _ = CASES[2]
    q, k, v = inputs(2)
    got = run(fa, 2, BF, 0, arrays=(q, np.repeat(k, G, axis=2), np.repeat(v, G, axis=2)), group=1, lens=(rep(ql, G), rep(kl, G)))
    assert_matches(got, 2, BF, "group 1 on the repeated cache")
    (O8, l8, m8), (_, er) = run(fa, 2, BF, 0), reference(2)
    sel = lambda t: np.where(~er[:, None, :], _np(t), 0.0)
    assert_close(sel(O8), sel(got[0]), BF, "group 8 vs group 1: O")
    assert_lm_close(sel(l8), sel(got[1]), BF, "group 8 vs group 1: l")
    assert_lm_close(sel(m8), sel(got[2]), BF, "group 8 vs group 1: m")
