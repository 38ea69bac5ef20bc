"""GPU tests of decode attention over a paged fp8 cache (fa_decode_paged_fp8_fwd through
fa_hip.paged_decode_fp8_fa): the e4m3fn cache scattered into pools of byte pages through a
shuffled page table, against the float64 yardstick tests/varlen_ref.py on the dequantised logical
cache (k8 * ks, v8 * vs, `group`-repeated), on bf16-representable queries seeded per shape.  The
pools are larger than what is used; pages that no read entry names hold the NaN byte 0x7F, unused
table entries name such a page, and the rows of a slab's last page past nk hold +-448.  Live rows
under conftest's tolerances (those of test_gpu_decode_fp8.py: the arithmetic after the convert is
the same); empty rows exactly."""
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
# name: page_size, (N, G, max_pages, d, dv, B), q_lens, k_lens, (left, right), dtypes
CASES = {
    "p64": (64, (1, 1, 9, 64, 64, 6), None, [0, 1, 63, 64, 65, 576], (-1, 0), (BF, F16)),   # page = tile edge, empty slab
    "p128": (128, (8, 4, 9, 128, 128, 2), [8, 5], [1152, 700], (100, 0), (BF,)),            # second tile of a page, left edge mid-page
    "p192": (192, (2, 2, 3, 32, 32, 3), None, None, (-1, 0), (BF,)),                        # a page of three tiles
    "p16": (16, (4, 8, 21, 64, 64, 4), [4, 2, 0, 3], [336, 1, 100, 130], (-1, 0), (BF,)),   # chunk path, cap % 64 != 0, nk inside a chunk
    "p48": (48, (3, 5, 7, 48, 40, 2), None, [336, 200], (-1, -1), (BF, F16)),               # pages cut tiles unevenly, odd head dims
    "min": (16, (1, 1, 1, 16, 8, 1), None, [5], (-1, 0), (BF,)),                            # the smallest call
}
HAS_EMPTY = ("p64", "p128", "p16")   # the cases with rows past nq or key-less queries
NSPLITS = (0, 1, 3, 7)
SPARE = 3                            # pages of the pool that no table entry of a live key names
NAN8, MAX8 = 0x7F, 0x7E              # e4m3fn NaN and +448 (0xFE: -448)


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


def k_lengths(case):
    ps, (N, G, mp, d, dv, B), _, kl, _, _ = CASES[case]
    return [mp * ps] * B if kl is None else kl


@functools.lru_cache(maxsize=None)
def inputs(case, share=0):
    """bf16-representable q (N, d, B*G), the e4m3fn-representable logical cache k8 (cap, d, B), v8
    (cap, dv, B) as float64, and per-slab scales in [0.25, 2), no power of two.  share > 0: slab
    1's first `share` pages and its scales equal slab 0's.  Never modified."""
    ps, (N, G, mp, d, dv, B) = CASES[case][:2]
    rng = np.random.default_rng(N * 131 + mp * ps * 17 + d * 7 + dv + G)
    q = torch.tensor(rng.standard_normal((N, d, B * G))).to(torch.bfloat16).double().numpy()
    k8, v8 = (e4m3(rng.standard_normal((mp * ps, f, B))).to(torch.float32).double().numpy() for f in (d, dv))
    ks, vs = (rng.uniform(0.25, 2.0, B).astype(np.float32) for _ in range(2))
    if share:
        k8[:share * ps, :, 1], v8[:share * ps, :, 1] = k8[:share * ps, :, 0], v8[:share * ps, :, 0]
        ks[1], vs[1] = ks[0], vs[0]
    return q, k8, v8, ks, vs


@functools.lru_cache(maxsize=None)
def pools(case, shuffle=0, fill="nan", share=0, private=False):
    """(k8_pages, v8_pages, table) as numpy bytes / int32: the logical cache scattered through a
    table shuffled by `shuffle`.  fill "nan": 0x7F in unnamed pages, +-448 past nk; "zero": zeros in
    both.  share > 0: slab 1 names slab 0's first `share` pages (its own copies stay unnamed)
    unless `private`."""
    ps, (N, G, mp, d, dv, B) = CASES[case][:2]
    k, v = (e4m3(a).view(torch.uint8).numpy() for a in inputs(case, share)[1:3])
    used = [-(-nk // ps) for nk in k_lengths(case)]
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
            past = np.arange(j * ps, (j + 1) * ps)[:, None] >= k_lengths(case)[b]
            kp[:, :, page] = np.where(past, tail, k[j * ps:(j + 1) * ps, :, b])
            vp[:, :, page] = np.where(past, tail, v[j * ps:(j + 1) * ps, :, b])
    return kp, vp, table


def rep(x, G):
    return None if x is None else np.repeat(np.asarray(x), G)


@functools.lru_cache(maxsize=None)
def reference(case, scaled=True):
    """(O, l, m) float64 on the dequantised logical cache and the (N, B*G) mask of empty rows."""
    ps, (N, G, mp, d, dv, B), ql, kl, (left, right), _ = CASES[case]
    q, k8, v8, ks, vs = inputs(case)
    k, v = (k8 * ks.astype(np.float64), v8 * vs.astype(np.float64)) if scaled else (k8, v8)
    ref = varlen_fwd_ref(q, np.repeat(k, G, axis=2), np.repeat(v, G, axis=2), rep(ql, G), rep(kl, G), left, right)
    nq = rep(ql, G) if ql is not None else [N] * (B * G)
    nk = rep(k_lengths(case), G)
    er = np.stack([(np.arange(N) >= nq[b]) | keyless_rows(N, mp * ps, nq[b], nk[b], left, right) for b in range(B * G)], axis=1)
    return ref, er


def run(fa, case, dtype, nsplit, shuffle=0, fill="nan", share=0, private=False, gather=False, scaled=True):
    ps, (N, G, mp, d, dv, B), ql, kl, (left, right), _ = CASES[case]
    q, _, _, ks, vs = inputs(case, share)
    kp, vp, table = pools(case, shuffle, fill, share, private)
    Q, T = fa.jl_tensor(q, DT[dtype]), fa.jl_tensor(table, torch.int32)
    KP, VP = (fa.jl_tensor(a, torch.uint8).view(torch.float8_e4m3fn) for a in (kp, vp))
    dev = lambda x, t=torch.int32: None if x is None else torch.tensor(np.asarray(x), dtype=t, device="cuda")
    KS, VS = (dev(ks, torch.float32), dev(vs, torch.float32)) if scaled else (None, None)
    old = fa.lib().fa_debug_set_decode_nsplit(nsplit)
    try:
        if gather:
            out = fa.decode_fp8_fa(Q, *fa.paged_kv_gather(KP, VP, T), KS, VS, dev(kl), dev(ql), G, left, right)
        else:
            out = fa.paged_decode_fp8_fa(Q, KP, VP, T, KS, VS, dev(kl), dev(ql), G, left, right)
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


def assert_same_bits(a, b, what):
    for x, y in zip(a, b):
        assert torch.equal(x, y), what


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("case,dtype", [(c, dt) for c in CASES for dt in CASES[c][5]])
def test_forward_vs_reference(fa, case, dtype, nsplit):
    assert_matches(run(fa, case, dtype, nsplit), case, dtype, f"{case} {dtype} nsplit {nsplit}")


@pytest.mark.parametrize("nsplit", (0, 3))
@pytest.mark.parametrize("case", CASES)
def test_bitwise_equal_to_decode_fp8_on_the_gathered_pools(fa, case, nsplit):
    """The same plan and the same arithmetic: any difference is an addressing error.  Zero-filled
    pools, which the gathered slabs may read past nk where the paged kernel looks nothing up."""
    assert_same_bits(run(fa, case, BF, nsplit, fill="zero"), run(fa, case, BF, nsplit, fill="zero", gather=True),
                     "paged_kv_gather + decode_fp8_fa")


@pytest.mark.parametrize("case", CASES)
def test_outputs_do_not_depend_on_where_the_pages_lie(fa, case):
    assert not np.array_equal(pools(case, 0)[2], pools(case, 1)[2])
    assert_same_bits(run(fa, case, BF, 3, shuffle=1), run(fa, case, BF, 3), "another shuffle of the same logical cache")


@pytest.mark.parametrize("case", CASES)
def test_nothing_leaks_from_unnamed_pages_or_the_tail(fa, case):
    assert_same_bits(run(fa, case, BF, 3, fill="zero"), run(fa, case, BF, 3), "zeros for the NaN pages and the +-448 tail")


def test_a_shared_prefix_equals_private_copies(fa):
    case, share = "p128", 5            # slab 1 (700 keys) is longer than the shared 640
    shared, private = pools(case, 0, "nan", share)[2], pools(case, 0, "nan", share, True)[2]
    assert (shared[:share, 1] == shared[:share, 0]).all() and (private[:share, 1] != private[:share, 0]).all()
    assert_same_bits(run(fa, case, BF, 0, share=share), run(fa, case, BF, 0, share=share, private=True), "shared pages")


@pytest.mark.parametrize("case", ("p128", "p48"))
def test_no_scales_mean_one(fa, case):
    assert_matches(run(fa, case, BF, 3, scaled=False), case, BF, f"{case} without scales", scaled=False)
