"""GPU parity of local and varlen attention (fa_local_fwd / fa_local_bwd, fa_varlen_fwd /
fa_varlen_bwd), forward and backward, under explicit scales and ill-conditioned scores: the five
input families of tests/cond_inputs.py (hot, cold, offset, anti, hotkeys) crossed with the routes
of ROWS below.  One test per (entry, route, dtype, family) runs the forward and, on the device's
own O, l, m, the backward, and asserts both routes from fa_debug_dense_last_launch (the kernel,
the mask and the pad / padded flag the launchers recorded).

The masked bodies differ from their dense parents in the arithmetic (csrc/fa_fwd.hip: a row-local
lazy rescale with alpha = 1 for a row that stays, exponent (s - m_used) c with offset 0 while
m_used = -inf; csrc/fa_bwd.hip: the varlen pre-pass, the zero keys of the padded slabs).  N(0, 1)
inputs at the default scale (row maxima 2..5) exercise none of it; `hot` and `hotkeys` make the
rescale fire again and again, `anti` puts every visible score near -70 (d = 64) or -100 (d = 128),
where a state that starts from 0 instead of -inf, or a masked score that is finite, decides.

Tolerances, none new and none derived from device output.  Forward, on the live rows:
test_gpu_forward_conditioning.check_forward (assert_close on O, assert_lm_close on m,
cond_inputs.l_rtol on l; Float64 1e-12 relative to max(|y|, 1)).  Backward:
test_gpu_backward_conditioning.check_grads (both grad_metrics within max(GTOL, 2 e_ref), e_ref
from cond_inputs.e_ref on the very case and mask; Float64 1e-12) against cond_inputs.backward_f64
on the device's O, l, m (Float64: the reference's own statistics).  Every empty row is checked
exactly, bitwise: O = 0, l = 0, m = -inf, dQ = 0; dK = dV = 0 for keys that no query sees and for
rows past nk.  Whether the limits are fair on these inputs is tests/test_masked_conditioning_host.py's
headroom check.  Each case prints an FCOND and a COND line.

Shapes are (N, Nk, d, dv, B; left, right); none has more than 520 rows."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import cond_inputs as C
from conftest import assert_close
from test_gpu_backward_conditioning import K_F32MFMA, K_GENERIC as KB_GENERIC, K_TWOPASS, check_grads
from test_gpu_backward_conditioning import K_F64 as KB_F64
from test_gpu_forward_conditioning import (BF, DT, F16, F32, F64T, K_F64, K_GENERIC, K_GENERIC_F32, K_W8B64, K_W8B64_WIDE,
                                           K_W8Q2, K_W8Q2_WIDE, _np, _shifted, check_forward, knobs)

pytestmark = pytest.mark.gpu
MASK_LOCAL, MASK_VARLEN = 2, 3     # fa::DenseMask (csrc/fa_internal.h)
OUTS = ("O", "l", "m", "dQ", "dK", "dV")

# (entry, route) -> (shape, (q_lens, k_lens) or None, dtypes,
#                    forward (kernel, pad), backward (kernel, padded) as fa_debug_dense_last_launch reports them)
# "generic": the forward is the raw C call with K / V views shifted one element and no workspace
# (dense_fwd_generic<LOCAL / VARLEN>), the backward runs under fa_debug_set_bwd_generic(1)
# (bwd_generic_dq / bwd_generic_dkdv<float, LOCAL / VARLEN>).
ROWS = {
    # off 64; the second workgroup has 8 rows and starts at key tile 7; rows hidden whole in their wave's first tile
    ("local", "w8q2_wide"): ((520, 584, 64, 64, 2, 100, 0), None, (BF, F16), (K_W8Q2_WIDE, 0), (K_TWOPASS, 0)),
    # narrow Q / O, two-sided, neither edge a multiple of 8
    ("local", "w8q2"): ((300, 328, 32, 32, 2, 23, 17), None, (BF,), (K_W8Q2, 0), (K_TWOPASS, 1)),
    ("local", "w8b64_wide"): ((264, 320, 128, 128, 2, 96, 32), None, (BF, F16), (K_W8B64_WIDE, 0), (K_TWOPASS, 0)),
    ("local", "w8b64"): ((130, 192, 128, 64, 2, 40, 0), None, (BF,), (K_W8B64, 0), (K_TWOPASS, 1)),
    # Nk % 8 != 0, odd head dims; 33 unseen keys; forward pad and backward padded slabs
    ("local", "padded"): ((77, 130, 40, 24, 1, 20, 5), None, (BF,), (K_W8Q2, 1), (K_TWOPASS, 1)),
    ("local", "generic"): ((200, 328, 128, 64, 2, 50, 20), None, (BF,), (K_GENERIC, 0), (KB_GENERIC, 0)),
    ("local", "f32"): ((256, 256, 64, 64, 2, 63, 64), None, (F32,), (K_GENERIC_F32, 0), (K_F32MFMA, 0)),
    ("local", "f64"): ((77, 130, 40, 24, 1, 20, 5), None, (F64T,), (K_F64, 0), (KB_F64, 0)),
    # slab 1: nk < nq under right = 0, 113 key-less queries; 513 is one past the 512-row workgroup
    ("varlen", "w8q2_wide"): ((520, 584, 64, 64, 3, -1, 0), ((520, 513, 77), (584, 400, 130)), (BF, F16),
                              (K_W8Q2_WIDE, 0), (K_TWOPASS, 0)),
    ("varlen", "w8b64_wide"): ((264, 320, 128, 128, 2, 64, 0), ((264, 257), (320, 300)), (BF, F16),
                               (K_W8B64_WIDE, 0), (K_TWOPASS, 0)),
    ("varlen", "padded"): ((200, 333, 48, 40, 2, -1, -1), ((200, 77), (333, 130)), (BF,), (K_W8Q2_WIDE, 1), (K_TWOPASS, 1)),
    ("varlen", "generic"): ((200, 328, 128, 64, 2, 50, 20), ((200, 41), (328, 63)), (BF,), (K_GENERIC, 0), (KB_GENERIC, 0)),
    # a slab with nk = 0
    ("varlen", "f32"): ((256, 256, 64, 64, 3, -1, 0), ((256, 200, 100), (256, 120, 0)), (F32,),
                        (K_GENERIC_F32, 0), (K_F32MFMA, 0)),
    ("varlen", "f64"): ((100, 140, 32, 48, 2, 10, 5), ((100, 41), (140, 63)), (F64T,), (K_F64, 0), (KB_F64, 0)),
}
ROUTES = ("w8q2_wide", "w8q2", "w8b64_wide", "w8b64", "padded", "generic", "f32", "f64")
# Draws other than the family's first (cond_inputs.family's seed), by (entry, route, dtype, family).
# fp16 inputs at d = 128 under `offset` / `anti`: 128 fp16 products near 9 summed in float32 to
# about +-1150 leave each score a rounding error near 3e-5 after the scale, and the yardstick's l
# then uses up to half of its limit (test_gpu_forward_conditioning.SEEDS documents the same).
# The yardstick's worst share (always l; the two exponent forms give the same figure) on the first
# draws, from tests/test_masked_conditioning_host.py, which asserts at most 0.5:
#     local  w8b64_wide fp16 offset 0.500 (draws 1..8: 0.553 0.444 0.467 0.405 0.405 0.454 0.494 0.496)
#     local  w8b64_wide fp16 anti   0.444          varlen w8b64_wide fp16 offset 0.469
#     varlen w8b64_wide fp16 anti   0.468          every other case at most 0.28
# The row on the cap takes draw 4; the others keep their first.  These four are the cases with the
# least room in this file.
SEEDS = {
    ("local", "w8b64_wide", F16, "offset"): 4,
}
PARAMS = [pytest.param(entry, route, dt, name, id=f"{entry}-{route}-{'-'.join(map(str, row[0]))}-{dt}-{name}")
          for (entry, route), row in ROWS.items() for dt in row[2] for name in C.FAMILIES]


@pytest.fixture(scope="module")
def fa():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    L = fa_hip.lib()
    L.fa_debug_dense_last_launch.restype = ctypes.c_int
    L.fa_debug_dense_last_launch.argtypes = [ctypes.POINTER(ctypes.c_int)]
    return fa_hip


def last_launch(L):
    """((forward kernel, mask, pad), (backward kernel, mask, padded)) of this thread's last launches."""
    out = (ctypes.c_int * 6)()
    assert L.fa_debug_dense_last_launch(out) == 0
    return tuple(out[:3]), tuple(out[3:])


@functools.lru_cache(maxsize=None)
def mask_of(entry, route):
    """The (N, Nk) local or (N, Nk, B) varlen mask of a row, from the references' own rule."""
    (N, Nk, _, _, _, left, right), lens, _, _, _ = ROWS[(entry, route)]
    mk = C.local_mask(N, Nk, left, right) if lens is None else C.varlen_masks(N, Nk, lens[0], lens[1], left, right)
    mk.setflags(write=False)
    return mk


def empty_rows(mask, B):
    """(N, B) bool: queries that see no key (rows past nq included); (Nk, B) bool: keys that no
    query sees (rows past nk included)."""
    m3 = mask[:, :, None].repeat(B, axis=2) if mask.ndim == 2 else mask
    return ~m3.any(axis=1), ~m3.any(axis=0)


@functools.lru_cache(maxsize=None)
def case(entry, route, dtype, name):
    """Inputs, scale, the float64 forward and the yardsticks of a case (shared, never modified):
    q, k, v, do, scale, (O, l, m) reference, e_ref_fwd shares, e_ref (None for Float64)."""
    (N, Nk, d, dv, B, _, _), _, _, _, _ = ROWS[(entry, route)]
    mask = mask_of(entry, route)
    q, k, v, do, scale = C.family(name, N, Nk, d, dv, B, dtype, mask=mask, seed=SEEDS.get((entry, route, dtype, name), 0))
    ref = C.forward_f64(q, k, v, scale, mask)
    eref_f = C.e_ref_fwd(q, k, v, scale, dtype, mask, ref=ref, local_exponent=True)
    eref_b = None if dtype == F64T else C.e_ref(q, k, v, do, scale, dtype, mask)
    for a in (q, k, v, do, *ref):
        a.setflags(write=False)
    return q, k, v, do, scale, ref, eref_f, eref_b


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _lens_dev(lens):
    return [None if x is None else x if isinstance(x, torch.Tensor) else torch.tensor(x, dtype=torch.int32, device="cuda")
            for x in lens]


def run(fa, entry, route, dtype, arrays, scale, lens="row", window=None, knob=None, expect=True):
    """Forward, then the backward on the device's own O, l, m, under the route's knobs (and
    `knob`, more fa_debug_set_* values for both).  lens: "row" (the row's, as device tensors), or
    (q_lens, k_lens) of None / sequences / int32 device tensors.  Asserts both routes from
    fa_debug_dense_last_launch.  Returns the six outputs and the inputs as device tensors."""
    L = fa.lib()
    (N, Nk, d, dv, B, left, right), row_lens, _, efwd, ebwd = ROWS[(entry, route)]
    if window is not None:
        left, right = window
    varlen = entry == "varlen"
    Q, K, V, dO = (fa.jl_tensor(np.array(a), DT[dtype]) for a in arrays)   # a copy: the shared cases are read-only
    QL, KL = _lens_dev(row_lens if lens == "row" else lens) if varlen else (None, None)
    code = fa.DTYPES[Q.dtype]
    stream = ctypes.c_void_p(torch.cuda.current_stream(Q.device).cuda_stream)
    with knobs(L, **(knob or {})):
        if route == "generic":
            Ks, Vs = _shifted(fa, K), _shifted(fa, V)
            Oo = fa.jl_empty((N, dv, B), Q.dtype, Q.device)
            l, m = (fa.jl_empty((N, 1, B), torch.float32, Q.device) for _ in range(2))
            head = (code, _ptr(Q), _ptr(Ks), _ptr(Vs), _ptr(Oo), _ptr(l), _ptr(m), N, Nk, d, dv, B)
            tail = (left, right, float(scale), ctypes.c_void_p(0), 0, stream)
            rc = L.fa_varlen_fwd(*head, _ptr(QL), _ptr(KL), *tail) if varlen else L.fa_local_fwd(*head, *tail)
            assert rc == 0, L.fa_last_error().decode(errors="replace")
        elif varlen:
            Oo, l, m = fa.varlen_fa(Q, K, V, QL, KL, left, right, scale)
        else:
            Oo, l, m = fa.local_fa(Q, K, V, left, right, scale)
        with knobs(L, **(dict(bwd_generic=1) if route == "generic" else {})):
            if varlen:
                g = fa.varlen_fa_backward(Q, K, V, Oo, dO, l, m, QL, KL, left, right, scale)
            else:
                g = fa.local_fa_backward(Q, K, V, Oo, dO, l, m, left, right, scale)
        torch.cuda.synchronize()
        got = last_launch(L)
    if expect:
        mk = MASK_VARLEN if varlen else MASK_LOCAL
        assert got == ((efwd[0], mk, efwd[1]), (ebwd[0], mk, ebwd[1])), f"{entry}/{route}: launched {got}"
    return dict(Q=Q, K=K, V=V, dO=dO, O=Oo, l=l, m=m, dQ=g[0], dK=g[1], dV=g[2])


@functools.lru_cache(maxsize=None)
def base_run(entry, route, dtype, name):
    """The unmodified run of a table case (shared between the tests, never modified)."""
    import fa_hip
    q, k, v, do, scale = case(entry, route, dtype, name)[:5]
    return run(fa_hip, entry, route, dtype, (q, k, v, do), scale)


def bitwise_zero(t):
    t = t.contiguous()
    bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return int(torch.count_nonzero(t.view(bits))) == 0


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check_empty_exact(r, er, ek, tag):
    """Empty rows bitwise: O = 0, l = 0, m = -inf, dQ = 0; unseen keys and rows past nk: dK = dV = 0.
    Every other row has l > 0 and a finite m; nothing anywhere is NaN."""
    er_t, ek_t = torch.tensor(er, device="cuda"), torch.tensor(ek, device="cuda")
    rows = lambda t, sel: t.permute(0, 2, 1)[sel]          # (rows, C)
    if er.any():
        assert bitwise_zero(rows(r["O"], er_t)) and bitwise_zero(rows(r["l"], er_t)), f"{tag}: O, l of empty rows"
        assert bool((rows(r["m"], er_t) == float("-inf")).all()), f"{tag}: m of empty rows"
        assert bitwise_zero(rows(r["dQ"], er_t)), f"{tag}: dQ of empty rows"
    if ek.any():
        assert bitwise_zero(rows(r["dK"], ek_t)) and bitwise_zero(rows(r["dV"], ek_t)), f"{tag}: dK, dV of unseen keys"
    for nm in OUTS:
        assert not bool(torch.isnan(r[nm]).any()), f"{tag}: NaN in {nm}"
    assert bool((rows(r["l"], ~er_t) > 0).all()) and bool(torch.isfinite(rows(r["m"], ~er_t)).all()), f"{tag}: live rows' l, m"


def live_only(o, l, m, er):
    """(O, l, m) as float64 with the empty rows' state (checked exactly elsewhere) replaced by 0."""
    live = ~er[:, None, :]
    return tuple(np.where(live, np.asarray(a, dtype=np.float64), 0.0) for a in (o, l, m))


def check_case(r, entry, route, dtype, arrays, scale, mask, ref, eref_f, eref_b, tag):
    """Empty rows exactly, the forward under check_forward's rule, the backward under check_grads'."""
    q, k, v, do = arrays
    er, ek = empty_rows(mask, q.shape[2])
    check_empty_exact(r, er, ek, tag)
    check_forward(live_only(_np(r["O"]), _np(r["l"]), _np(r["m"]), er), live_only(*ref, er), eref_f, dtype, tag)
    f64 = dtype == F64T
    gref = C.backward_f64(q, k, v, do, _np(r["O"]), ref[1] if f64 else _np(r["l"]), ref[2] if f64 else _np(r["m"]), scale, mask)
    check_grads((r["dQ"], r["dK"], r["dV"]), gref, dtype, eref_b, tag)


@pytest.mark.parametrize("entry,route,dtype,name", PARAMS)
def test_masked_route_under_family(fa, entry, route, dtype, name):
    q, k, v, do, scale, ref, eref_f, eref_b = case(entry, route, dtype, name)
    r = base_run(entry, route, dtype, name)
    tag = f"{entry}/{route} {'-'.join(map(str, ROWS[(entry, route)][0]))} {dtype} {name}"
    check_case(r, entry, route, dtype, (q, k, v, do), scale, mask_of(entry, route), ref, eref_f, eref_b, tag)


def test_last_launch_agrees_with_the_plan_hooks(fa):
    """fa_debug_dense_last_launch against fa_debug_local_*_plan / fa_debug_varlen_*_plan on shapes
    under the default knobs, where both can answer: the same kernel and pad / padded flag."""
    L = fa.lib()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    for entry, route in (("local", "w8q2_wide"), ("local", "padded"), ("varlen", "w8b64_wide"), ("varlen", "padded")):
        (N, Nk, d, dv, B, _, _), _, dts, _, _ = ROWS[(entry, route)]
        dtype = dts[0]
        run(fa, entry, route, dtype, case(entry, route, dtype, "cold")[:4], 0.0)
        fwd, bwd = last_launch(L)
        code = fa.DTYPES[DT[dtype]]
        fo, bo = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 6)()
        nwf = getattr(L, f"fa_{entry}_fwd_workspace")(code, N, Nk, d, dv, B)
        nwb = getattr(L, f"fa_{entry}_bwd_workspace")(code, N, Nk, d, dv, B)
        kf = getattr(L, f"fa_debug_{entry}_fwd_plan")(code, N, Nk, d, dv, B, 1, 1, nwf, cus, fo)
        kb = getattr(L, f"fa_debug_{entry}_bwd_plan")(code, N, Nk, d, dv, B, 1, nwb, cus, bo)
        mk = MASK_VARLEN if entry == "varlen" else MASK_LOCAL
        assert fo[0] == 1 and fwd == (kf, mk, fo[2]), (entry, route, fwd, kf, list(fo))
        assert bwd == (kb, mk, bo[0]), (entry, route, bwd, kb, list(bo))


# ---- the existing claims, where they have not been tried ----------------------------------------
@pytest.mark.parametrize("name", ["hot", "hotkeys"])
@pytest.mark.parametrize("entry", ["local", "varlen"])
def test_rescale_threshold_under_family(fa, entry, name):
    """Lazy-rescale threshold 0 (rescale on every increase of a row's maximum) against the default
    8 on the w8q2_wide rows, bf16: m bitwise equal, O of both within tolerance of the reference,
    the empty rows exact in both."""
    q, k, v, do, scale, ref, _, _ = case(entry, "w8q2_wide", BF, name)
    mask = mask_of(entry, "w8q2_wide")
    er, ek = empty_rows(mask, q.shape[2])
    outs = []
    for thr in (0.0, 8.0):
        r = run(fa, entry, "w8q2_wide", BF, (q, k, v, do), scale, knob=dict(rescale_threshold=thr))
        check_empty_exact(r, er, ek, f"{entry} threshold {thr} ({name})")
        assert_close(live_only(_np(r["O"]), _np(r["l"]), _np(r["m"]), er)[0], live_only(*ref, er)[0], BF,
                     f"O at threshold {thr} ({entry}, {name})")
        outs.append(r)
    assert bits_equal(outs[0]["m"], outs[1]["m"]), f"{entry} {name}: m differs between thresholds 0 and 8"


def _filled(entry, route, arrays, fill):
    """The inputs with the rows past the lengths set to `fill` (+-: alternating sign per row)."""
    _, (ql, kl), _, _, _ = ROWS[(entry, route)]
    q, k, v, do = (a.copy() for a in arrays)
    for b in range(q.shape[2]):
        for a, n in ((q, ql[b]), (do, ql[b]), (k, kl[b]), (v, kl[b])):
            a[n:, :, b] = fill * np.where(np.arange(a.shape[0] - n) % 2 == 0, 1.0, -1.0)[:, None]
    return q, k, v, do


@pytest.mark.parametrize("name", ["offset", "anti"])
@pytest.mark.parametrize("route,dtype", [("w8q2_wide", F16), ("padded", BF), ("generic", BF), ("f32", F32)])
def test_nothing_leaks_from_the_varlen_padding(fa, route, dtype, name):
    """Padding rows of Q, K, V, dO zeroed, then filled with +-3e4: all six outputs bitwise equal
    between the fills and equal to the unmodified run, and finite (m = -inf on empty rows).  The
    zero fill under `anti` is the case csrc/fa_dense_plan.h names: exp(0 - lse) overflows."""
    q, k, v, do, scale = case("varlen", route, dtype, name)[:5]
    z = run(fa, "varlen", route, dtype, _filled("varlen", route, (q, k, v, do), 0.0), scale)
    f = run(fa, "varlen", route, dtype, _filled("varlen", route, (q, k, v, do), 3e4), scale)
    b = base_run("varlen", route, dtype, name)
    er, _ = empty_rows(mask_of("varlen", route), q.shape[2])
    er_t = torch.tensor(er, device="cuda")[:, None, :]
    for nm in OUTS:
        assert bits_equal(z[nm], f[nm]), f"{nm}: the fills differ"
        assert torch.equal(z[nm], b[nm]), f"{nm}: differs from the unmodified run"
        if nm == "m":
            assert torch.equal(torch.isneginf(f[nm]), er_t) and bool(torch.isfinite(f[nm][~er_t]).all()), nm
        else:
            assert bool(torch.isfinite(f[nm]).all()), nm


AGREE = ("hot", "offset", "anti")
AGREE_SHAPES = {BF: (520, 520, 64, 64, 1), F32: (200, 333, 48, 40, 2)}


def _agree(a, b, dtype, mr, eref_b, tag):
    """a against b (dicts of device outputs): the forward under check_forward's limits with b as
    the reference, the gradients under max(GTOL, 2 e_ref) on both metrics."""
    assert_close(_np(a["O"]), _np(b["O"]), dtype, f"O ({tag})")
    m_err = (np.abs(_np(a["m"]) - _np(b["m"])) / (1 + np.abs(_np(b["m"])))).max()
    assert m_err <= C.TOL[dtype]["lm"], f"{tag}: m {m_err:.3e}"
    l_err = (np.abs(_np(a["l"]) - _np(b["l"])) / (1 + np.abs(_np(b["l"])))).max()
    assert l_err <= C.l_rtol(mr, dtype), f"{tag}: l {l_err:.3e}"
    bud = C.budget(dtype, eref_b)
    for nm in ("dQ", "dK", "dV"):
        err, rel = C.grad_metrics(_np(a[nm]), _np(b[nm]))
        print(f"AGREE {tag} {nm}: {err:.2e} {rel:.2e} budget {bud:.2e}")
        assert err <= bud and rel <= bud, f"{tag} {nm}: {err:.2e}, {rel:.2e} > {bud:.2e}"


@pytest.mark.parametrize("name", AGREE)
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("window", [(-1, 0), (-1, -1)], ids=["causal", "dense"])
def test_local_matches_causal_and_dense_under_family(fa, window, dtype, name):
    """local_fa at (-1, 0) against causal_fa and at (-1, -1) against dense_fa, both directions
    (tests/test_gpu_local.py's test_matches_causal_and_dense, on N(0, 1) inputs there)."""
    N, Nk, d, dv, B = AGREE_SHAPES[dtype]
    causal = window == (-1, 0)
    mask = C.causal_mask(N, Nk) if causal else None
    q, k, v, do, scale = C.family(name, N, Nk, d, dv, B, dtype)
    mr = C.forward_f64(q, k, v, scale, mask)[2]
    eref_b = C.e_ref(q, k, v, do, scale, dtype, mask)
    Q, K, V, dO = (fa.jl_tensor(a, DT[dtype]) for a in (q, k, v, do))
    Oo, l, m = fa.local_fa(Q, K, V, *window, scale)
    g = fa.local_fa_backward(Q, K, V, Oo, dO, l, m, *window, scale)
    fwd, bwd = (fa.causal_fa, fa.causal_fa_backward) if causal else (fa.dense_fa, fa.dense_fa_backward)
    Or, lr, mr_d = fwd(Q, K, V, scale)
    gr = bwd(Q, K, V, Or, dO, lr, mr_d, scale)
    torch.cuda.synchronize()
    _agree(dict(zip(OUTS, (Oo, l, m, *g))), dict(zip(OUTS, (Or, lr, mr_d, *gr))), dtype, mr, eref_b,
           f"local {window} vs {'causal' if causal else 'dense'} {dtype} {name}")


@pytest.mark.parametrize("name", AGREE)
@pytest.mark.parametrize("route,dtype", [("w8q2_wide", BF), ("f32", F32)])
def test_varlen_null_lengths_match_local_fa_under_family(fa, route, dtype, name):
    """varlen_fa with NULL lengths (every slab full) against local_fa with the same window."""
    (N, Nk, d, dv, B, left, right), _, _, _, _ = ROWS[("varlen", route)]
    mask = C.local_mask(N, Nk, left, right)
    q, k, v, do, scale = case("varlen", route, dtype, name)[:5]
    mr = C.forward_f64(q, k, v, scale, mask)[2]
    eref_b = C.e_ref(q, k, v, do, scale, dtype, mask)
    a = run(fa, "varlen", route, dtype, (q, k, v, do), scale, lens=(None, None))
    Oo, l, m = fa.local_fa(a["Q"], a["K"], a["V"], left, right, scale)
    g = fa.local_fa_backward(a["Q"], a["K"], a["V"], Oo, a["dO"], l, m, left, right, scale)
    torch.cuda.synchronize()
    _agree(a, dict(zip(OUTS, (Oo, l, m, *g))), dtype, mr, eref_b, f"varlen NULL lengths vs local {route} {dtype} {name}")


@pytest.mark.parametrize("route,dtype,bad,clamped", [
    ("padded", BF, ((1200, -5), (340, -2147483648)), ((200, 0), (333, 0))),
    ("f32", F32, ((265, -1, 100), (-7, 120, 2147483647)), ((256, 0, 100), (0, 120, 256))),
])
def test_device_lengths_out_of_range_are_clamped(fa, route, dtype, bad, clamped):
    """int32 device lengths with negative entries and entries above N / Nk: all six outputs
    bitwise equal to the run with the lengths clamped to [0, N] / [0, Nk] (include/fa_hip.h; every
    VARLEN instantiation takes its extents from fa::varlen_extents, the only reader of the arrays)."""
    q, k, v, do, scale = case("varlen", route, dtype, "hot")[:5]
    a = run(fa, "varlen", route, dtype, (q, k, v, do), scale, lens=bad)
    b = run(fa, "varlen", route, dtype, (q, k, v, do), scale, lens=clamped)
    for nm in OUTS:
        assert bits_equal(a[nm], b[nm]), nm
    (N, Nk, _, _, _, left, right), _, _, _, _ = ROWS[("varlen", route)]
    er, ek = empty_rows(C.varlen_masks(N, Nk, clamped[0], clamped[1], left, right), q.shape[2])
    check_empty_exact(a, er, ek, f"varlen {route} out-of-range lengths")


@pytest.mark.parametrize("entry", ["local", "varlen"])
def test_bitwise_deterministic_under_hotkeys(fa, entry):
    q, k, v, do, scale = case(entry, "w8q2_wide", BF, "hotkeys")[:5]
    a = base_run(entry, "w8q2_wide", BF, "hotkeys")
    b = run(fa, entry, "w8q2_wide", BF, (q, k, v, do), scale)
    for nm in OUTS:
        assert bits_equal(a[nm], b[nm]), nm
