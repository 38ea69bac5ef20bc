"""GPU tests of paged decode attention (fa_decode_paged_fwd through fa_hip.paged_decode_fa): the
cache scattered into a pool of pages through a shuffled page table, against the float64
yardstick tests/varlen_ref.py on the logical (gathered, `group`-repeated) cache, on
bf16-representable inputs seeded per shape.  The pool is larger than what is used; pages that no
read entry names hold NaN, unused table entries name such a page, and the rows of a slab's last
page past nk hold +-3e4.  Live rows under conftest's tolerances; empty rows exactly."""
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
# page_size: (N, G, max_pages, d, dv, B), q_lens, k_lens, (left, right), dtypes
CASES = {
    64: ((1, 1, 9, 64, 64, 6), None, [0, 1, 63, 64, 65, 576], (-1, 0), (BF, F16)),      # page = tile edge, empty slabs
    128: ((8, 4, 9, 128, 128, 2), [8, 5], [1152, 700], (100, 0), (BF,)),                # second tile of a page, left edge mid-page
    192: ((2, 2, 3, 32, 32, 3), None, None, (-1, 0), (BF,)),                            # a page of 3 tiles
    16: ((4, 8, 21, 64, 64, 4), [4, 2, 0, 3], [336, 1, 100, 130], (-1, 0), (BF,)),      # chunk path, cap % 64 != 0
    24: ((3, 5, 14, 48, 40, 2), None, [336, 200], (-1, -1), (BF, F16)),                 # pages cut tiles unevenly
    8: ((1, 1, 1, 16, 8, 1), None, [5], (-1, 0), (BF,)),                                # the smallest call
}
HAS_EMPTY = (64, 128, 16)   # the cases with rows past nq or key-less queries
NSPLITS = (0, 1, 3, 7)
SPARE = 3                   # pages of the pool that no table entry of a live key names


@pytest.fixture(scope="module")
def fa():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    fa_hip.lib()
    return fa_hip


def _np(t):
    return t.detach().double().cpu().numpy()


def k_lengths(ps):
    (N, G, mp, d, dv, B), _, kl, _, _ = CASES[ps]
    return [mp * ps] * B if kl is None else kl


@functools.lru_cache(maxsize=None)
def inputs(ps):
    """bf16-representable q (N, d, B*G) and the logical cache k (cap, d, B), v (cap, dv, B): float64, never modified."""
    N, G, mp, d, dv, B = CASES[ps][0]
    rng = np.random.default_rng(N * 131 + mp * ps * 17 + d * 7 + dv + G)
    bf = lambda a: torch.tensor(a).to(torch.bfloat16).double().numpy()
    return tuple(bf(rng.standard_normal(s)) for s in ((N, d, B * G), (mp * ps, d, B), (mp * ps, dv, B)))


@functools.lru_cache(maxsize=None)
def pools(ps, shuffle=0, fill="nan", share=0, private=False):
    """(k_pages, v_pages, table) as numpy: the logical cache scattered through a table shuffled by
    `shuffle`.  fill "nan": NaN in unnamed pages, +-3e4 past nk; "zero": zeros in both.  share > 0:
    slab 1's first `share` pages equal slab 0's, and slab 1 names slab 0's (its own copies stay
    unnamed) unless `private`."""
    (N, G, mp, d, dv, B), _, _, _, _ = CASES[ps]
    _, k, v = inputs(ps) if share == 0 else shared_inputs(ps, share)
    used = [-(-nk // ps) for nk in k_lengths(ps)]
    P = sum(used) + SPARE
    perm = np.random.default_rng(1000 + shuffle).permutation(P)
    unnamed = float("nan") if fill == "nan" else 0.0
    kp, vp = np.full((ps, d, P), unnamed), np.full((ps, dv, P), unnamed)
    table = np.full((mp, B), perm[P - 1], dtype=np.int32)           # unused entries: a page no live key is in
    nxt = 0
    for b in range(B):
        nk = k_lengths(ps)[b]
        tail = (0.0 if fill == "zero" else 3e4) * np.where(np.arange(ps) % 2 == 0, 1.0, -1.0)[:, None]
        for j in range(used[b]):
            page, nxt = perm[nxt], nxt + 1
            if b == 1 and j < share and not private:
                table[j, b] = table[j, 0]
                continue
            table[j, b] = page
            past = np.arange(j * ps, (j + 1) * ps)[:, None] >= nk
            kp[:, :, page] = np.where(past, tail, k[j * ps:(j + 1) * ps, :, b])
            vp[:, :, page] = np.where(past, tail, v[j * ps:(j + 1) * ps, :, b])
    return kp, vp, table


@functools.lru_cache(maxsize=None)
def shared_inputs(ps, share):
    q, k, v = (a.copy() for a in inputs(ps))
    k[:share * ps, :, 1], v[:share * ps, :, 1] = k[:share * ps, :, 0], v[:share * ps, :, 0]
    return q, k, v


def rep(x, G):
    return None if x is None else np.repeat(np.asarray(x), G)


@functools.lru_cache(maxsize=None)
def reference(ps):
    """(O, l, m) float64 on the logical cache and the (N, B*G) mask of empty rows."""
    (N, G, mp, d, dv, B), ql, kl, (left, right), _ = CASES[ps]
    q, k, v = inputs(ps)
    ref = varlen_fwd_ref(q, np.repeat(k, G, axis=2), np.repeat(v, G, axis=2), rep(ql, G), rep(kl, G), left, right)
    nq = rep(ql, G) if ql is not None else [N] * (B * G)
    nk = rep(k_lengths(ps), G)
    er = np.stack([(np.arange(N) >= nq[b]) | keyless_rows(N, mp * ps, nq[b], nk[b], left, right) for b in range(B * G)], axis=1)
    return ref, er


def run(fa, ps, dtype, nsplit, shuffle=0, fill="nan", share=0, private=False, gather=False):
    (N, G, mp, d, dv, B), ql, kl, (left, right), _ = CASES[ps]
    q = inputs(ps)[0]
    kp, vp, table = pools(ps, shuffle, fill, share, private)
    Q, KP, VP = (fa.jl_tensor(a, DT[dtype]) for a in (q, kp, vp))
    T = fa.jl_tensor(table, torch.int32)
    dev = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=torch.int32, device="cuda")
    old = fa.lib().fa_debug_set_decode_nsplit(nsplit)
    try:
        if gather:
            out = fa.decode_fa(Q, *fa.paged_kv_gather(KP, VP, T), dev(kl), dev(ql), G, left, right)
        else:
            out = fa.paged_decode_fa(Q, KP, VP, T, dev(kl), dev(ql), G, left, right)
    finally:
        fa.lib().fa_debug_set_decode_nsplit(old)
    torch.cuda.synchronize()
    return out


def bitwise_zero(t):
    t = t.contiguous()
    return int(torch.count_nonzero(t.view({2: torch.int16, 4: torch.int32}[t.element_size()]))) == 0


def assert_matches(out, ps, dtype, what):
    (o, l, m), er = reference(ps)
    O, L, M = out
    live = ~er
    assert live.any(), "the case has no live row"
    assert er.any() == (ps in HAS_EMPTY)
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


def assert_same_bits(a, b, what):
    for x, y in zip(a, b):
        assert torch.equal(x, y), what


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("ps,dtype", [(c, dt) for c in CASES for dt in CASES[c][4]])
def test_forward_vs_reference(fa, ps, dtype, nsplit):
    assert_matches(run(fa, ps, dtype, nsplit), ps, dtype, f"page {ps} {dtype} nsplit {nsplit}")


@pytest.mark.parametrize("ps", (64, 128, 16, 24))
def test_m_is_bitwise_equal_across_split_counts(fa, ps):
    m1, m3, m7 = (run(fa, ps, BF, n)[2] for n in (1, 3, 7))
    assert torch.equal(m1, m3) and torch.equal(m1, m7)


@pytest.mark.parametrize("ps", (128, 16))
@pytest.mark.parametrize("nsplit", (0, 3))
def test_two_runs_are_bitwise_equal(fa, ps, nsplit):
    assert_same_bits(run(fa, ps, BF, nsplit), run(fa, ps, BF, nsplit), "second run")


@pytest.mark.parametrize("ps", sorted(CASES))
def test_outputs_do_not_depend_on_where_the_pages_lie(fa, ps):
    assert not np.array_equal(pools(ps, 0)[2], pools(ps, 1)[2]) or ps == 8
    assert_same_bits(run(fa, ps, BF, 3, shuffle=1), run(fa, ps, BF, 3), "another shuffle of the same logical cache")


@pytest.mark.parametrize("ps", sorted(CASES))
def test_nothing_leaks_from_unnamed_pages_or_the_tail(fa, ps):
    assert_same_bits(run(fa, ps, BF, 3, fill="zero"), run(fa, ps, BF, 3), "zeros for the NaN pages and the +-3e4 tail")


@pytest.mark.parametrize("ps,share", [(128, 5), (192, 2), (24, 8)])   # slab 1 is longer than the shared prefix
def test_a_shared_prefix_equals_private_copies(fa, ps, share):
    shared, private = pools(ps, 0, "nan", share)[2], pools(ps, 0, "nan", share, True)[2]
    assert (shared[:share, 1] == shared[:share, 0]).all() and (private[:share, 1] != private[:share, 0]).all()
    assert_same_bits(run(fa, ps, BF, 0, share=share), run(fa, ps, BF, 0, share=share, private=True), "shared pages")


@pytest.mark.parametrize("ps,dtype", [(c, dt) for c in CASES for dt in CASES[c][4]])
def test_gather_then_decode_agrees(fa, ps, dtype):
    assert_matches(run(fa, ps, dtype, 0, fill="zero", gather=True), ps, dtype, f"page {ps} {dtype} gather + decode_fa")
