"""CPU checks behind tests/test_gpu_masked_conditioning.py: the extended helpers of
tests/cond_inputs.py (per-slab masks, empty rows, the LOCAL exponent form) against local_ref.py and
varlen_ref.py, the condition on the inputs of every GPU case (the formulation alone leaves half of
each forward limit; no backward budget buys itself room), and that the tables reach what they
say.  Nothing here needs a device; the cases are the GPU file's own (shared through its cache)."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import cond_inputs as C
import test_gpu_masked_conditioning as G
from local_ref import local_bwd_ref, local_fwd_ref
from varlen_ref import keyless_rows, unseen_keys, varlen_bwd_ref, varlen_fwd_ref

F64T = "float64"


def close(x, y):
    """1e-12 relative to max(|y|, 1); an m = -inf of y must be one of x."""
    inf = np.isneginf(y)
    if not np.array_equal(np.isneginf(x), inf):
        return False
    x, y = np.where(inf, 0.0, x), np.where(inf, 0.0, y)
    return np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0)


# ---- the helpers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hot", "anti"])
@pytest.mark.parametrize("left,right", [(20, 5), (-1, 0), (7, -1), (0, 0), (-1, -1)])
def test_forward_and_backward_f64_agree_with_local_ref(left, right, name):
    N, Nk = 40, 56
    mk = C.local_mask(N, Nk, left, right)
    q, k, v, do, scale = C.family(name, N, Nk, 16, 8, 2, "bfloat16", mask=mk)
    o, l, m = C.forward_f64(q, k, v, scale, mk)
    for x, y in zip((o, l, m), local_fwd_ref(q, k, v, left, right, scale)):
        assert close(x, y)
    for x, y in zip(C.backward_f64(q, k, v, do, o, l, m, scale, mk), local_bwd_ref(q, k, v, o, do, l, m, left, right, scale)):
        assert close(x, y)


VARLEN_HOST = [   # (q_lens, k_lens, left, right) at (N, Nk, B) = (40, 56, 4): nk < nq, nk = 0, nq = 0, full
    ((40, 30, 25, 0), (56, 12, 0, 33), -1, 0),
    ((40, 30, 25, 0), (56, 12, 0, 33), 5, 3),
    ((17, 40, 1, 40), (9, 56, 56, 40), -1, -1),
    ((40, 30, 25, 0), None, 7, -1),
]


@pytest.mark.parametrize("name", ["hot", "hotkeys", "anti"])
@pytest.mark.parametrize("ql,kl,left,right", VARLEN_HOST)
def test_forward_and_backward_f64_agree_with_varlen_ref(ql, kl, left, right, name):
    N, Nk, B = 40, 56, 4
    mk = C.varlen_masks(N, Nk, ql, kl, left, right)
    assert mk.shape == (N, Nk, B)
    q, k, v, do, scale = C.family(name, N, Nk, 16, 8, B, "bfloat16", mask=mk)
    o, l, m = C.forward_f64(q, k, v, scale, mk)
    ro, rl, rm = varlen_fwd_ref(q, k, v, ql, kl, left, right, scale)
    assert np.array_equal(np.isneginf(m), np.isneginf(rm)) and np.isneginf(rm).any()
    assert np.all(o.transpose(0, 2, 1)[np.isneginf(m)[:, 0, :]] == 0.0) and np.all(l[np.isneginf(m)] == 0.0)
    for x, y in zip((o, l, m), (ro, rl, rm)):
        assert close(x, y)
    ref = varlen_bwd_ref(q, k, v, o, do, l, m, ql, kl, left, right, scale)
    for x, y in zip(C.backward_f64(q, k, v, do, o, l, m, scale, mk), ref):
        assert close(x, y)
    # an empty row comes from the mask, never from the l, m that are passed in
    l2, m2 = np.where(np.isneginf(m), 3.0, l), np.where(np.isneginf(m), 1.0, m)
    for x, y in zip(C.backward_f64(q, k, v, do, o, l2, m2, scale, mk), ref):
        assert close(x, y)
    low = C.lowp_backward(q, k, v, do, o, l, m, scale, "bf16", mk)
    low2 = C.lowp_backward(q, k, v, do, o, l2, m2, scale, "bf16", mk)
    for x, y, z in zip(low, low2, ref):
        assert np.array_equal(x, y) and np.all(np.isfinite(x))
        assert max(C.grad_metrics(x, z)) <= 5e-2
    # the error metrics: empty rows add nothing, and e_ref / e_ref_fwd are finite
    assert np.isfinite(C.e_ref(q, k, v, do, scale, "bfloat16", mk))
    sh = C.e_ref_fwd(q, k, v, scale, "bfloat16", mk, local_exponent=True)
    assert all(np.isfinite(s) for s in sh.values()) and max(sh.values()) <= 1.0


def test_a_3d_mask_is_its_slabs_and_a_2d_mask_is_shared():
    N, Nk, B = 40, 56, 3
    mk3 = C.varlen_masks(N, Nk, (40, 30, 25), (56, 12, 40), 9, 2)
    q, k, v, do, scale = C.family("hot", N, Nk, 16, 8, B, "bfloat16")
    full = C.forward_f64(q, k, v, scale, mk3)
    lowf = C.lowp_forward(q, k, v, scale, "bf16", mk3, exponent="sub")
    bw = C.backward_f64(q, k, v, do, *full, scale, mk3)
    for b in range(B):
        sl = slice(b, b + 1)
        one = C.forward_f64(q[:, :, sl], k[:, :, sl], v[:, :, sl], scale, mk3[:, :, b])
        for x, y in zip(full, one):
            assert np.array_equal(x[:, :, sl], y)
        for x, y in zip(lowf, C.lowp_forward(q[:, :, sl], k[:, :, sl], v[:, :, sl], scale, "bf16", mk3[:, :, b], exponent="sub")):
            assert np.array_equal(x[:, :, sl], y)
        one = C.backward_f64(q[:, :, sl], k[:, :, sl], v[:, :, sl], do[:, :, sl], *(a[:, :, sl] for a in full), scale, mk3[:, :, b])
        for x, y in zip(bw, one):
            assert np.array_equal(x[:, :, sl], y)
    mk2 = C.local_mask(N, Nk, 9, 2)
    for x, y in zip(C.forward_f64(q, k, v, scale, mk2), C.forward_f64(q, k, v, scale, np.repeat(mk2[:, :, None], B, axis=2))):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("lag", [0.0, 8.0])
def test_lowp_forward_local_exponent(lag):
    """The `sub` form: the float64 forward up to float32 rounding, as the fma form is; with no lag a
    row with one visible key has l = 1 and O = that key's V exactly (what the kernels' comment asks
    of the form); empty rows keep O = 0, l = 0, m = -inf in both forms."""
    N, Nk, B = 40, 56, 2
    mk = C.varlen_masks(N, Nk, (40, 30), (56, 12), 0, 0)          # one key per live query; slab 1: 12 live rows
    q, k, v, _, scale = C.family("offset", N, Nk, 16, 8, B, "float32", mask=mk)
    ref = C.forward_f64(q, k, v, scale, mk)
    empty = np.isneginf(ref[2])[:, 0, :]
    assert empty.sum() == 28 and not empty[:, 0].any()
    for form in ("fma", "sub"):
        o, l, m = C.lowp_forward(q, k, v, scale, None, mk, lag_log2=lag, exponent=form)
        assert np.array_equal(np.isneginf(m)[:, 0, :], empty)
        assert np.all(l[:, 0, :][empty] == 0.0) and np.all(o.transpose(0, 2, 1)[empty] == 0.0)
        for x, y in zip((o, l, m), ref):
            x, y = x.transpose(0, 2, 1)[~empty], y.transpose(0, 2, 1)[~empty]
            assert np.abs(x - y).max() <= 1e-4 * max(np.abs(y).max(), 1.0)
        if form == "sub" and lag == 0.0:
            assert np.all(l[:, 0, :][~empty] == 1.0)
            for b in range(B):
                i, j = np.nonzero(mk[:, :, b])
                assert np.array_equal(o[i, :, b], v[j, :, b])


def test_hot_pairs_take_seen_keys():
    """A local window with off - left > 0 hides the first keys from every query, a varlen slab the
    keys past nk: the pairs sit on seen keys, one per third of them, each visible to its query."""
    mk = C.local_mask(77, 130, 20, 5)
    pairs = C.hot_pairs(77, 130, 1, mk)
    seen = np.flatnonzero(mk.any(axis=0))
    assert seen[0] == 33 and [j for _, j, _ in pairs] == [int(seen[min(96, ((2 * t + 1) * 97) // 6 + t)]) for t in range(3)]
    assert all(mk[i, j] for i, j, _ in pairs)
    mk3 = C.varlen_masks(256, 256, (256, 200, 100), (256, 120, 0), -1, 0)
    pairs = C.hot_pairs(256, 256, 3, mk3)
    assert [b for _, _, b in pairs] == [0, 1] and all(mk3[i, j, b] for i, j, b in pairs)   # slab 2 sees no key: no pair
    assert pairs[1][1] < 120


# ---- the getter --------------------------------------------------------------------------------------
def test_last_launch_getter_is_a_debug_hook_and_starts_empty():
    """fa_debug_dense_last_launch is exported, is not in the public header, refuses a null
    pointer, and on a thread that has launched nothing reports -1 everywhere (what it reports
    after a launch is tests/test_gpu_masked_conditioning.py's, against the plan hooks)."""
    import threading
    import fa_hip
    L = fa_hip.lib()
    L.fa_debug_dense_last_launch.restype = ctypes.c_int
    L.fa_debug_dense_last_launch.argtypes = [ctypes.POINTER(ctypes.c_int)]
    assert L.fa_debug_dense_last_launch(None) == -1
    got = []

    def fresh():
        out = (ctypes.c_int * 6)(*([7] * 6))
        got.append((L.fa_debug_dense_last_launch(out), list(out)))

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert got == [(0, [-1] * 6)]
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fa_hip.h")) as f:
        assert "fa_debug_dense_last_launch" not in f.read()


# ---- the condition on the GPU cases ---------------------------------------------------------------------
def _rows(f64):
    return [p for p in G.PARAMS if (p.values[2] == F64T) == f64]


@pytest.mark.parametrize("entry,route,dtype,name", _rows(False))
def test_formulation_leaves_headroom_and_budgets_stay_near_gtol(entry, route, dtype, name):
    """Before any GPU run: the kernels' formulation alone (lowp_forward in both exponent forms,
    m_used at and 8 log2 units below the row maximum) uses at most half of each forward limit on
    the live rows; and the backward budget max(GTOL, 2 e_ref) stays within 1.5 GTOL and within
    2.5e-2 / 5e-3 / 2e-5 (bf16 / fp16 / fp32), so no case buys itself room.  A case above needs
    another draw (G.SEEDS), not another limit."""
    _, _, _, _, _, _, eref_f, eref_b = G.case(entry, route, dtype, name)
    bud = C.budget(dtype, eref_b)
    print(f"HEADROOM {entry} {route} {dtype} {name}: " + ", ".join(f"{nm} {s:.3f}" for nm, s in eref_f.items())
          + f"; e_ref {eref_b:.2e} budget {bud:.2e}")
    assert max(eref_f.values()) <= 0.5, eref_f
    assert bud <= 1.5 * C.GTOL[dtype] and bud <= {"bfloat16": 2.5e-2, "float16": 5e-3, "float32": 2e-5}[dtype], (eref_b, bud)


def test_seeds_name_table_cases():
    for entry, route, dtype, name in G.SEEDS:
        assert dtype in G.ROWS[(entry, route)][2] and name in C.FAMILIES


def test_every_route_gets_every_family():
    """The GPU file's tables: each row of the issue's two lists is there, under all five families."""
    assert set(G.ROWS) == {("local", r) for r in G.ROUTES} | {("varlen", r) for r in G.ROUTES if r not in ("w8q2", "w8b64")}
    for key, row in G.ROWS.items():
        for dt in row[2]:
            assert {p.values[3] for p in G.PARAMS if p.values[:3] == (*key, dt)} == set(C.FAMILIES)
    assert len(G.PARAMS) == sum(len(row[2]) for row in G.ROWS.values()) * len(C.FAMILIES)
    assert max(row[0][0] for row in G.ROWS.values()) <= 520


# ---- the tables reach what they say ------------------------------------------------------------------
def test_tables_reach_what_they_say():
    for (entry, route), (shape, lens, dts, _, _) in G.ROWS.items():
        N, Nk, d, dv, B, left, right = shape
        mk = G.mask_of(entry, route)
        er, ek = G.empty_rows(mk, B)
        assert N <= 520 and Nk >= N
        if entry == "local":
            assert mk.shape == (N, Nk) and not er.any(), (route, "every local row sees a key")
            assert ek[:, 0].sum() == max(0, Nk - N - left), route
        else:
            assert mk.shape == (N, Nk, B)
            for b, (nq, nk) in enumerate(zip(*lens)):
                keyless = keyless_rows(N, Nk, nq, nk, left, right)
                want = nq if nk == 0 else max(0, min(nq, nq - nk - right)) if right >= 0 else 0
                assert keyless.sum() == want and er[:, b].sum() == (N - nq) + want, (route, b)
                assert np.array_equal(ek[:, b], (np.arange(Nk) >= nk) | unseen_keys(N, Nk, nq, nk, left, right)), (route, b)
    ek = G.empty_rows(G.mask_of("local", "padded"), 1)[1]
    assert ek.sum() == 33 and ek[:33].all()
    er = G.empty_rows(G.mask_of("varlen", "w8q2_wide"), 3)[0]
    assert er[:513, 1].sum() == 113 and er[:113, 1].all() and er[513:, 1].all() and not er[:, 0].any()
    er, ek = G.empty_rows(G.mask_of("varlen", "f32"), 3)
    assert er[:, 2].all() and ek[:, 2].all() and er[:, 1].sum() == (256 - 200) + 80


def test_local_w8q2_wide_hides_whole_rows_in_a_waves_first_tile():
    """(520, 584; 100, 0): a wave of the 512-row workgroup holds 64 consecutive queries and computes
    the 64-key tiles that one of them sees.  In the first of those tiles some of its rows see no key
    (their windows begin in the next tile): the rows whose running maximum is still -inf when a
    wave-mate rescales.  The second workgroup (8 rows) starts at key tile 7."""
    mk = G.mask_of("local", "w8q2_wide")
    hidden = 0
    for r0 in range(0, 520, 64):
        rows = mk[r0:min(r0 + 64, 520)]
        t0 = int(np.flatnonzero(rows.any(axis=0))[0]) // 64
        hidden += int((~rows[:, 64 * t0:64 * t0 + 64].any(axis=1)).sum())
    assert hidden > 0
    print("rows hidden whole in their wave's first tile:", hidden)
    assert int(np.flatnonzero(mk[512:].any(axis=0))[0]) // 64 == 7


def test_generic_rows_reach_the_generic_kernels_by_the_shift_alone():
    """The generic rows' shape is one the fast kernels take (Nk % 8 == 0, head dims of a class, no
    workspace needed): what sends the forward to dense_fwd_generic is the one-element shift of K and
    V, 2 bytes off a 16-B boundary."""
    for entry in ("local", "varlen"):
        (N, Nk, d, dv, B, _, _), _, dts, fwd, bwd = G.ROWS[(entry, "generic")]
        assert Nk % 8 == 0 and N % 8 == 0 and d in (32, 64, 128) and dv in (32, 64, 128)
        assert all(G.DT[dt].itemsize == 2 for dt in dts) and (16 + 2) % 16 != 0
        assert fwd == (G.K_GENERIC, 0) and bwd == (G.KB_GENERIC, 0)


@pytest.mark.parametrize("key", list(G.ROWS), ids=lambda k: "-".join(k))
def test_hotkeys_pairs_sit_on_visible_pairs_in_every_slab(key):
    (N, Nk, d, dv, B, _, _), _, dts, _, _ = G.ROWS[key]
    mk = G.mask_of(*key)
    pairs = C.hot_pairs(N, Nk, B, mk)
    assert len(pairs) == (2 if key == ("varlen", "f32") else 3)         # that row's slab 2 has no key
    q, k, _, _, _, _, _, _ = G.case(*key, dts[0], "hotkeys")
    for i, j, b in pairs:
        assert (mk[i, j] if mk.ndim == 2 else mk[i, j, b])
        assert np.array_equal(k[j, :, b], 8.0 * q[i, :, b])
    if B > 1:
        assert len({b for _, _, b in pairs}) == min(B, len(pairs))
