"""GPU tests of chunked prefill over a paged fp8 cache (fa_hip.paged_prefill_fp8_fa), in the manner of
test_gpu_prefill_paged.py and test_gpu_decode_paged_fp8.py: the e4m3fn logical cache scattered into
byte pools through a shuffled table, against varlen_ref.py in float64 on the dequantised,
`group`-repeated cache.  3 spare pages; unnamed pages hold 0x7F, unused entries name such a page,
rows past nk hold +-448; scales in [0.25, 2), no powers of two.  Live rows under conftest's
tolerances (the fp8 decode tests': the arithmetic after the exact convert is the same); empty rows exactly."""
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
    (64, (40, 4, 8, 64, 64, 3), None, [512, 100, 0], (-1, 0), (BF, F16)),   # two row blocks, the second ragged; 8 tiles: the ring wraps; an empty slab
    (128, (96, 2, 3, 128, 128, 2), [96, 50], [384, 200], (100, 0), (BF,)),  # second tile of a page; left edge mid-page; rows i >= nq; most LDS and registers
    (16, (33, 1, 13, 64, 64, 2), None, [208, 20], (-1, 0), (BF,)),          # one row past decode's limit; chunk path; cap % 64 != 0; nk inside a chunk; key-less queries
    (48, (30, 5, 5, 48, 40, 2), None, [240, 130], (-1, -1), (BF, F16)),     # G divides no block; pages cut tiles unevenly; odd head dims
    (256, (130, 1, 1, 32, 128, 2), None, None, (64, 0), (BF,)),             # the contiguous byte cache as one page per slab; a block of 2 rows
    (64, (2, 8, 3, 64, 64, 2), None, [192, 70], (-1, 0), (BF,)),            # N * G <= 32: paged_decode_fp8_fa's ground
    (16, (1, 1, 1, 16, 8, 1), None, [5], (-1, 0), (BF,)),                   # the smallest call
]
IDS = range(len(CASES))
HAS_EMPTY = (0, 1, 2)       # the cases with an empty slab, rows past nq or key-less queries
DECODE_CASE = 5
SPARE = 3                   # pages of the pool that no table entry of a live key names
NAN8, MAX8 = 0x7F, 0x7E     # e4m3fn NaN and +448 (0xFE: -448)


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
    return torch.tensor(a, dtype=torch.float32).to(torch.float8_e4m3fn)


def k_lengths(c):
    ps, (N, G, mp, d, dv, B), _, kl, _, _ = CASES[c]
    return [mp * ps] * B if kl is None else kl


@functools.lru_cache(maxsize=None)
def inputs(c, share=0):
    """bf16-representable q (N, d, B*G), the e4m3fn-representable k8 (cap, d, B), v8 (cap, dv, B) as float64, the
    per-slab scales.  share > 0: slab 1's first `share` pages and its scales equal slab 0's.  Never modified."""
    ps, (N, G, mp, d, dv, B) = CASES[c][:2]
    rng = np.random.default_rng(N * 131 + mp * ps * 17 + d * 7 + dv + G)
    q = torch.tensor(rng.standard_normal((N, d, B * G))).to(torch.bfloat16).double().numpy()
    k8, v8 = (e4m3(rng.standard_normal((mp * ps, f, B))).to(torch.float32).double().numpy() for f in (d, dv))
    ks, vs = (rng.uniform(0.25, 2.0, B).astype(np.float32) for _ in range(2))
    if share:
        k8[:share * ps, :, 1], v8[:share * ps, :, 1] = k8[:share * ps, :, 0], v8[:share * ps, :, 0]
        ks[1], vs[1] = ks[0], vs[0]
    return q, k8, v8, ks, vs


@functools.lru_cache(maxsize=None)
def pools(c, shuffle=0, fill="nan", share=0, private=False):
    """(k8_pages, v8_pages, table) as numpy: the logical cache scattered through a table shuffled by `shuffle`.
    fill "nan": 0x7F in unnamed pages, +-448 past nk; "zero": zeros.  share > 0: slab 1 names slab 0's first pages."""
    ps, (N, G, mp, d, dv, B) = CASES[c][:2]
    k, v = (e4m3(a).view(torch.uint8).numpy() for a in inputs(c, share)[1:3])
    used = [-(-nk // ps) for nk in k_lengths(c)]
    P = sum(used) + SPARE
    perm = np.random.default_rng(1000 + shuffle).permutation(P)
    kp, vp = (np.full((ps, f, P), NAN8 if fill == "nan" else 0, dtype=np.uint8) for f in (d, dv))
    table = np.full((mp, B), perm[P - 1], dtype=np.int32)           # unused entries: a page no live key is in
    tail = np.where(np.arange(ps) % 2 == 0, MAX8, MAX8 | 0x80).astype(np.uint8)[:, None] * (fill != "zero")
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
def reference(c, scaled=True):
    """(O, l, m) float64 on the dequantised logical cache and the (N, B*G) mask of empty rows."""
    ps, (N, G, mp, d, dv, B), ql, kl, (left, right), _ = CASES[c]
    q, k8, v8, ks, vs = inputs(c)
    k, v = (k8 * ks.astype(np.float64), v8 * vs.astype(np.float64)) if scaled else (k8, v8)
    ref = varlen_fwd_ref(q, np.repeat(k, G, axis=2), np.repeat(v, G, axis=2), rep(ql, G), rep(kl, G), left, right)
    nq = rep(ql, G) if ql is not None else [N] * (B * G)
    nk = rep(k_lengths(c), G)
    er = np.stack([(np.arange(N) >= nq[b]) | keyless_rows(N, mp * ps, nq[b], nk[b], left, right) for b in range(B * G)], axis=1)
    return ref, er


def run(fa, c, dtype, nsplit, shuffle=0, fill="nan", share=0, private=False, decode=False, scaled=True):
    ps, (N, G, mp, d, dv, B), ql, kl, (left, right), _ = CASES[c]
    q, _, _, ks, vs = inputs(c, share)
    kp, vp, table = pools(c, shuffle, fill, share, private)
    Q, T = fa.jl_tensor(q, DT[dtype]), fa.jl_tensor(table, torch.int32)
    KP, VP = (fa.jl_tensor(a, torch.uint8).view(torch.float8_e4m3fn) for a in (kp, vp))
    dev = lambda x, t=torch.int32: None if x is None else torch.tensor(np.asarray(x), dtype=t, device="cuda")
    KS, VS = (dev(ks, torch.float32), dev(vs, torch.float32)) if scaled else (None, None)
    old = fa.lib().fa_debug_set_decode_nsplit(nsplit)
    try:
        out = (fa.paged_decode_fp8_fa if decode else fa.paged_prefill_fp8_fa)(Q, KP, VP, T, KS, VS, dev(kl), dev(ql), G, left, right)
    finally:
        fa.lib().fa_debug_set_decode_nsplit(old)
    torch.cuda.synchronize()
    return out


def bitwise_zero(t):
    t = t.contiguous()
    return int(torch.count_nonzero(t.view({2: torch.int16, 4: torch.int32}[t.element_size()]))) == 0


def assert_matches(out, c, dtype, what, ref=None, scaled=True):
    (o, l, m), er = reference(c, scaled)
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


def test_rows_within_decodes_limit_agree_with_paged_decode_fp8(fa):
    assert_matches(run(fa, DECODE_CASE, BF, 0), DECODE_CASE, BF, "against paged_decode_fp8_fa",
                   ref=run(fa, DECODE_CASE, BF, 0, decode=True))


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
    assert_same_bits(run(fa, c, BF, 3, fill="zero"), run(fa, c, BF, 3), "zeros for the 0x7F pages and the +-448 tail")


@pytest.mark.parametrize("c,share", [(1, 1), (3, 2)])   # slab 1 is longer than the shared prefix
def test_a_shared_prefix_equals_private_copies(fa, c, share):
    shared, private = pools(c, 0, "nan", share)[2], pools(c, 0, "nan", share, True)[2]
    assert (shared[:share, 1] == shared[:share, 0]).all() and (private[:share, 1] != private[:share, 0]).all()
    assert_same_bits(run(fa, c, BF, 0, share=share), run(fa, c, BF, 0, share=share, private=True), "shared pages")


@pytest.mark.parametrize("c", (1, 3))
def test_no_scales_mean_one(fa, c):
    assert_matches(run(fa, c, BF, 3, scaled=False), c, BF, f"case {c} without scales", scaled=False)
