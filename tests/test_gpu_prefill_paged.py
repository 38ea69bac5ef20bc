"""GPU tests of chunked prefill over a paged cache (fa_prefill_paged_fwd through
fa_hip.paged_prefill_fa), in the style of tests/test_gpu_decode_paged.py: the logical cache
scattered into a pool through a shuffled table, against the float64 yardstick tests/varlen_ref.py
on the gathered, `group`-repeated cache, on bf16-representable inputs seeded per case.  The pool
holds 3 spare pages; unnamed pages hold NaN, unused table entries name such a page, rows of a
slab's last page past nk hold +-3e4.  Live rows under conftest's tolerances; empty rows exactly.
The shapes are the smallest that reach each edge of the 128-row blocks."""
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
# page_size, (N, G, max_pages, d, dv, B), q_lens, k_lens, (left, right), dtypes
CASES = [
    (64, (40, 4, 5, 64, 64, 3), None, [320, 100, 0], (-1, 0), (BF, F16)),   # two row blocks, the second ragged; off > 0; an empty slab
    (128, (96, 2, 3, 128, 128, 2), [96, 50], [384, 200], (100, 0), (BF,)),  # second tile of a page; left edge mid-page; rows i >= nq; 64 KiB of LDS
    (16, (33, 1, 13, 64, 64, 2), None, [208, 20], (-1, 0), (BF,)),          # one row past decode's limit; chunk path; cap % 64 != 0; key-less queries
    (24, (30, 5, 10, 48, 40, 2), None, [240, 130], (-1, -1), (BF, F16)),    # G divides no block; pages cut tiles unevenly; odd head dims
    (256, (130, 1, 1, 32, 128, 2), None, None, (64, 0), (BF,)),             # the contiguous cache as one page per slab; a block of 2 rows
    (64, (2, 8, 3, 64, 64, 2), None, [192, 70], (-1, 0), (BF,)),            # N * G <= 32: paged_decode_fa's ground
    (8, (1, 1, 1, 16, 8, 1), None, [5], (-1, 0), (BF,)),                    # the smallest call
]
IDS = range(len(CASES))
HAS_EMPTY = (0, 1, 2)       # the cases with an empty slab, rows past nq or key-less queries
DECODE_CASE = 5
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


def k_lengths(c):
    ps, (N, G, mp, d, dv, B), _, kl, _, _ = CASES[c]
    return [mp * ps] * B if kl is None else kl


@functools.lru_cache(maxsize=None)
def inputs(c, share=0):
    """bf16-representable q (N, d, B*G) and the logical cache k (cap, d, B), v (cap, dv, B): float64, never
    modified.  share > 0: slab 1's first `share` pages equal slab 0's."""
    ps, (N, G, mp, d, dv, B) = CASES[c][:2]
    rng = np.random.default_rng(N * 131 + mp * ps * 17 + d * 7 + dv + G)
    bf = lambda a: torch.tensor(a).to(torch.bfloat16).double().numpy()
    q, k, v = (bf(rng.standard_normal(s)) for s in ((N, d, B * G), (mp * ps, d, B), (mp * ps, dv, B)))
    if share:
        k[:share * ps, :, 1], v[:share * ps, :, 1] = k[:share * ps, :, 0], v[:share * ps, :, 0]
    return q, k, v


@functools.lru_cache(maxsize=None)
def pools(c, shuffle=0, fill="nan", share=0, private=False):
    """(k_pages, v_pages, table) as numpy: the logical cache scattered through a table shuffled by
    `shuffle`.  fill "nan": NaN in unnamed pages, +-3e4 past nk; "zero": zeros in both.  share > 0:
    slab 1 names slab 0's first `share` pages (its own copies stay unnamed) unless `private`."""
    ps, (N, G, mp, d, dv, B) = CASES[c][:2]
    _, k, v = inputs(c, share)
    used = [-(-nk // ps) for nk in k_lengths(c)]
    P = sum(used) + SPARE
    perm = np.random.default_rng(1000 + shuffle).permutation(P)
    unnamed = float("nan") if fill == "nan" else 0.0
    kp, vp = np.full((ps, d, P), unnamed), np.full((ps, dv, P), unnamed)
    table = np.full((mp, B), perm[P - 1], dtype=np.int32)           # unused entries: a page no live key is in
    tail = (0.0 if fill == "zero" else 3e4) * np.where(np.arange(ps) % 2 == 0, 1.0, -1.0)[:, None]
    nxt = 0
    for b in range(B):
        for j in range(used[b]):
            page, nxt = perm[nxt], nxt + 1
            if b == 1 and j < share and not private:
                table[j, b] = table[j, 0]
                continue
            table[j, b] = page
            past = np.arange(j * ps, (j + 1) * ps)[:, None] >= k_lengths(c)[b]
            kp[:, :, page] = np.where(past, tail, k[j * ps:(j + 1) * ps, :, b])
            vp[:, :, page] = np.where(past, tail, v[j * ps:(j + 1) * ps, :, b])
    return kp, vp, table


def rep(x, G):
    return None if x is None else np.repeat(np.asarray(x), G)


@functools.lru_cache(maxsize=None)
def reference(c):
    """(O, l, m) float64 on the logical cache and the (N, B*G) mask of empty rows."""
    ps, (N, G, mp, d, dv, B), ql, kl, (left, right), _ = CASES[c]
    q, k, v = inputs(c)
    ref = varlen_fwd_ref(q, np.repeat(k, G, axis=2), np.repeat(v, G, axis=2), rep(ql, G), rep(kl, G), left, right)
    nq = rep(ql, G) if ql is not None else [N] * (B * G)
    nk = rep(k_lengths(c), G)
    er = np.stack([(np.arange(N) >= nq[b]) | keyless_rows(N, mp * ps, nq[b], nk[b], left, right) for b in range(B * G)], axis=1)
    return ref, er


def run(fa, c, dtype, nsplit, shuffle=0, fill="nan", share=0, private=False, decode=False):
    ps, (N, G, mp, d, dv, B), ql, kl, (left, right), _ = CASES[c]
    kp, vp, table = pools(c, shuffle, fill, share, private)
    Q, KP, VP = (fa.jl_tensor(a, DT[dtype]) for a in (inputs(c, share)[0], kp, vp))
    T = fa.jl_tensor(table, torch.int32)
    dev = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=torch.int32, device="cuda")
    old = fa.lib().fa_debug_set_decode_nsplit(nsplit)
    try:
        out = (fa.paged_decode_fa if decode else fa.paged_prefill_fa)(Q, KP, VP, T, dev(kl), dev(ql), G, left, right)
    finally:
        fa.lib().fa_debug_set_decode_nsplit(old)
    torch.cuda.synchronize()
    return out


def bitwise_zero(t):
    t = t.contiguous()
    return int(torch.count_nonzero(t.view({2: torch.int16, 4: torch.int32}[t.element_size()]))) == 0


def assert_matches(out, c, dtype, what, ref=None):
    (o, l, m), er = reference(c)
    if ref is not None:
        o, l, m = (_np(t) for t in ref)
    O, L, M = out
    live = ~er
    assert live.any(), "the case has no live row"
    assert er.any() == (c in HAS_EMPTY)
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


@pytest.mark.parametrize("nsplit", (0, 1, 3))
@pytest.mark.parametrize("c,dtype", [(c, dt) for c in IDS for dt in CASES[c][5]])
def test_forward_vs_reference(fa, c, dtype, nsplit):
    assert_matches(run(fa, c, dtype, nsplit), c, dtype, f"case {c} {dtype} nsplit {nsplit}")


def test_rows_within_decodes_limit_agree_with_paged_decode(fa):
    assert_matches(run(fa, DECODE_CASE, BF, 0), DECODE_CASE, BF, "against paged_decode_fa", ref=run(fa, DECODE_CASE, BF, 0, decode=True))


@pytest.mark.parametrize("c", (0, 1, 2, 3))
def test_m_is_bitwise_equal_across_split_counts(fa, c):
    m1, m3, m7 = (run(fa, c, BF, n)[2] for n in (1, 3, 7))
    assert torch.equal(m1, m3) and torch.equal(m1, m7)


@pytest.mark.parametrize("c", (1, 2))
@pytest.mark.parametrize("nsplit", (0, 3))
def test_two_runs_are_bitwise_equal(fa, c, nsplit):
    assert_same_bits(run(fa, c, BF, nsplit), run(fa, c, BF, nsplit), "second run")


@pytest.mark.parametrize("c", IDS)
def test_outputs_do_not_depend_on_where_the_pages_lie(fa, c):
    assert not np.array_equal(pools(c, 0)[2], pools(c, 1)[2])
    assert_same_bits(run(fa, c, BF, 3, shuffle=1), run(fa, c, BF, 3), "another shuffle of the same logical cache")


@pytest.mark.parametrize("c", IDS)
def test_nothing_leaks_from_unnamed_pages_or_the_tail(fa, c):
    assert_same_bits(run(fa, c, BF, 3, fill="zero"), run(fa, c, BF, 3), "zeros for the NaN pages and the +-3e4 tail")


@pytest.mark.parametrize("c,share", [(1, 1), (3, 4)])   # slab 1 is longer than the shared prefix
def test_a_shared_prefix_equals_private_copies(fa, c, share):
    shared, private = pools(c, 0, "nan", share)[2], pools(c, 0, "nan", share, True)[2]
    assert (shared[:share, 1] == shared[:share, 0]).all() and (private[:share, 1] != private[:share, 0]).all()
    assert_same_bits(run(fa, c, BF, 0, share=share), run(fa, c, BF, 0, share=share, private=True), "shared pages")
