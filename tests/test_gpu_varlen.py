"""GPU tests of varlen attention (fa_varlen_fwd / fa_varlen_bwd through fa_hip.varlen_fa,
varlen_fa_backward, varlen_dpa): per-slab lengths in a padded batch, against the float64
yardstick tests/varlen_ref.py on bf16-representable inputs seeded per shape.

Tolerances and norms are tests/test_gpu_local.py's (GTOL, assert_fwd_close, assert_grad_close,
Float64 as it tests it), imported.  The backward is fed the device's own O, l, m.  The forward is
compared on the rows that see a key; every other row (past nq, or key-less) is checked exactly:
O = 0, l = 0, m = -inf, bitwise.  The cases are tests/test_varlen_host.py's GPU_CASES, whose
contents that file pins on the CPU."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_local import DT, assert_fwd_close, assert_grad_close, fa, _np  # noqa: F401  (fa: the module fixture)
from conftest import assert_close, assert_lm_close
from test_varlen_host import GPU_CASES
from varlen_ref import keyless_rows, unseen_keys, varlen_bwd_ref, varlen_fwd_ref

pytestmark = pytest.mark.gpu
PARAMS = [pytest.param(name, dt, id=f"{name}-{dt}") for name, c in GPU_CASES.items() for dt in c[3]]
OUTS = ("O", "l", "m", "dQ", "dK", "dV")


@functools.lru_cache(maxsize=None)
def inputs(N, Nk, d, dv, B):
    """bf16-representable q, k, v, do (float64 arrays; shared, never modified)."""
    rng = np.random.default_rng(N * 131 + Nk * 17 + d * 7 + dv + 1)
    bf = lambda a: torch.tensor(a).to(torch.bfloat16).double().numpy()
    return tuple(bf(rng.standard_normal(s)) for s in ((N, d, B), (Nk, d, B), (Nk, dv, B), (N, dv, B)))


@functools.lru_cache(maxsize=None)
def fwd_ref(name):
    case, ql, kl, _ = GPU_CASES[name]
    q, k, v, _ = inputs(*case[:5])
    return varlen_fwd_ref(q, k, v, ql, kl, case[5], case[6])


def padded(name, fill):
    """The inputs with the rows past the lengths set to `fill` (+-: alternating sign per row)."""
    case, ql, kl, _ = GPU_CASES[name]
    q, k, v, do = (a.copy() for a in inputs(*case[:5]))
    for b in range(case[4]):
        for a, n in ((q, ql[b]), (do, ql[b]), (k, kl[b]), (v, kl[b])):
            rows = a.shape[0] - n
            a[n:, :, b] = fill * np.where(np.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]
    return q, k, v, do


def device_run(fa, name, dtype, arrays=None, lens="device", backward=True):
    case, ql, kl, _ = GPU_CASES[name]
    left, right = case[5:]
    q, k, v, do = inputs(*case[:5]) if arrays is None else arrays
    Q, K, V, dO = (fa.jl_tensor(a, DT[dtype]) for a in (q, k, v, do))
    if lens == "device":
        QL, KL = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in (ql, kl))
    else:
        QL, KL = lens
    Oo, l, m = fa.varlen_fa(Q, K, V, QL, KL, left, right)
    r = dict(Q=Q, K=K, V=V, dO=dO, O=Oo, l=l, m=m, QL=QL, KL=KL)
    if backward:
        r["dQ"], r["dK"], r["dV"] = fa.varlen_fa_backward(Q, K, V, Oo, dO, l, m, QL, KL, left, right)
    torch.cuda.synchronize()
    return r


@functools.lru_cache(maxsize=None)
def base_run(name, dtype):
    import fa_hip
    return device_run(fa_hip, name, dtype)


def bitwise_zero(t):
    t = t.contiguous()
    bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return int(torch.count_nonzero(t.view(bits))) == 0


def empty_rows(name):
    """(N, B) bool: rows past nq and key-less queries; (Nk, B) bool: rows past nk and unseen keys."""
    (N, Nk, _, _, B, left, right), ql, kl, _ = GPU_CASES[name]
    er = np.stack([(np.arange(N) >= ql[b]) | keyless_rows(N, Nk, ql[b], kl[b], left, right) for b in range(B)], axis=1)
    ek = np.stack([(np.arange(Nk) >= kl[b]) | unseen_keys(N, Nk, ql[b], kl[b], left, right) for b in range(B)], axis=1)
    return er, ek


@pytest.mark.parametrize("name,dtype", PARAMS)
def test_forward_and_backward_vs_reference(fa, name, dtype):
    case, ql, kl, _ = GPU_CASES[name]
    r = base_run(name, dtype)
    assert fa.lib().fa_debug_fwd_last_path() != 30
    o, l, m = fwd_ref(name)
    er, _ = empty_rows(name)
    live = ~er
    assert np.array_equal(live, l[:, 0, :] > 0)
    # the rows that see a key, under test_gpu_local's forward rule (the others: the next test, exactly)
    sel = lambda a: np.where(live[:, None, :], a, 0.0)
    got = {"O": torch.tensor(sel(_np(r["O"]))), "l": torch.tensor(sel(_np(r["l"]))),
           "m": torch.tensor(np.where(live[:, None, :], _np(r["m"]), 0.0))}
    assert_fwd_close(got, (sel(o), sel(l), np.where(live[:, None, :], m, 0.0)), dtype)
    q, k, v, do = inputs(*case[:5])
    f64 = dtype == "float64"
    ref = varlen_bwd_ref(q, k, v, _np(r["O"]), do, None if f64 else _np(r["l"]), None if f64 else _np(r["m"]),
                         ql, kl, case[5], case[6])
    for nm, y in zip(("dQ", "dK", "dV"), ref):
        assert_grad_close(_np(r[nm]), y, dtype, nm)


@pytest.mark.parametrize("name,dtype", PARAMS)
def test_exact_values_past_the_lengths_and_on_empty_rows(fa, name, dtype):
    r = base_run(name, dtype)
    er, ek = empty_rows(name)
    assert er.any() and ek.any()
    er_t, ek_t = torch.tensor(er, device="cuda"), torch.tensor(ek, device="cuda")
    rows = lambda t, mask: t.permute(0, 2, 1)[mask]          # (rows, C)
    assert bitwise_zero(rows(r["O"], er_t)) and bitwise_zero(rows(r["dQ"], er_t))
    assert bitwise_zero(rows(r["l"], er_t))
    assert bool((rows(r["m"], er_t) == float("-inf")).all())
    assert bitwise_zero(rows(r["dK"], ek_t)) and bitwise_zero(rows(r["dV"], ek_t))
    for nm in OUTS:
        assert not bool(torch.isnan(r[nm]).any()), nm
    assert bool((rows(r["l"], ~er_t) > 0).all()) and bool(torch.isfinite(rows(r["m"], ~er_t)).all())


@pytest.mark.parametrize("name,dtype", [("a", "bfloat16"), ("a", "float16"), ("d", "bfloat16"), ("d", "float32")])
def test_nothing_leaks_from_the_padding(fa, name, dtype):
    """Padding rows of Q, K, V, dO zeroed, then filled with +-3e4: every output bitwise equal."""
    z = device_run(fa, name, dtype, arrays=padded(name, 0.0))
    f = device_run(fa, name, dtype, arrays=padded(name, 3e4))
    b = base_run(name, dtype)
    for nm in OUTS:
        assert torch.equal(z[nm].contiguous().view(torch.uint8), f[nm].contiguous().view(torch.uint8)), nm
        assert torch.equal(z[nm], b[nm]), nm
        assert bool(torch.isfinite(f[nm]).all()) or nm == "m", nm


@pytest.mark.parametrize("name,dtype", [("a", "bfloat16"), ("b", "bfloat16"), ("d", "bfloat16"), ("d", "float32"), ("e", "bfloat16"),
                                        ("f", "float64")])
def test_null_lengths_are_full_lengths_and_agree_with_local_fa(fa, name, dtype):
    (N, Nk, d, dv, B, left, right), _, _, _ = GPU_CASES[name]
    full = (torch.full((B,), N, dtype=torch.int32, device="cuda"), torch.full((B,), Nk, dtype=torch.int32, device="cuda"))
    a = device_run(fa, name, dtype, lens=(None, None))
    b = device_run(fa, name, dtype, lens=full)
    c = device_run(fa, name, dtype, lens=([N] * B, None))        # a host sequence is copied to the device
    for nm in OUTS:
        assert torch.equal(a[nm], b[nm]) and torch.equal(a[nm], c[nm]), nm
    Oo, l, m = fa.local_fa(a["Q"], a["K"], a["V"], left, right)
    g = fa.local_fa_backward(a["Q"], a["K"], a["V"], Oo, a["dO"], l, m, left, right)
    torch.cuda.synchronize()
    assert_fwd_close(a, (_np(Oo), _np(l), _np(m)), dtype, "vs local_fa ")
    for nm, x in zip(("dQ", "dK", "dV"), g):
        assert_grad_close(_np(a[nm]), _np(x), dtype, "vs local_fa " + nm)
    print("bitwise equal to local_fa:", {nm: bool(torch.equal(a[nm], x)) for nm, x in zip(OUTS, (Oo, l, m) + tuple(g))})


@pytest.mark.parametrize("name,dtype", [("a", "bfloat16"), ("d", "bfloat16"), ("d", "float32")])
def test_bitwise_deterministic(fa, name, dtype):
    a, b = base_run(name, dtype), device_run(fa, name, dtype)
    for nm in OUTS:
        assert torch.equal(a[nm].contiguous().view(torch.uint8), b[nm].contiguous().view(torch.uint8)), nm


@pytest.mark.parametrize("name,dtype", [("a", "bfloat16"), ("d", "bfloat16"), ("d", "float32"), ("f", "float64")])
def test_raw_abi_workspace_at_an_odd_address(fa, name, dtype):
    """Sentinel-filled outputs are overwritten everywhere, bitwise the mirror's result, with both
    workspaces starting at an odd address; the hand-off status reads -1."""
    (N, Nk, d, dv, B, left, right), _, _, _ = GPU_CASES[name]
    r = base_run(name, dtype)
    L = fa.lib()
    code = fa.DTYPES[DT[dtype]]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def odd_ws(n):
        raw = torch.empty(n + 2, dtype=torch.uint8, device="cuda")   # never empty, also when n == 0
        assert raw[1:].data_ptr() % 2 == 1
        return raw[1:]

    Oo = fa.jl_empty(r["O"].shape, DT[dtype]).fill_(777.0)
    l = fa.jl_empty(r["l"].shape, torch.float32).fill_(777.0)
    m = fa.jl_empty(r["m"].shape, torch.float32).fill_(777.0)
    nws = L.fa_varlen_fwd_workspace(code, N, Nk, d, dv, B)
    ws = odd_ws(nws)
    rc = L.fa_varlen_fwd(code, P(r["Q"]), P(r["K"]), P(r["V"]), P(Oo), P(l), P(m), N, Nk, d, dv, B, P(r["QL"]), P(r["KL"]),
                         left, right, 0.0, P(ws), nws, stream)
    assert rc == 0, L.fa_last_error()
    outs = [fa.jl_empty(r[nm].shape, DT[dtype]).fill_(777.0) for nm in ("dQ", "dK", "dV")]
    nwb = L.fa_varlen_bwd_workspace(code, N, Nk, d, dv, B)
    wb = odd_ws(nwb)
    rc = L.fa_varlen_bwd(code, P(r["Q"]), P(r["K"]), P(r["V"]), P(Oo), P(r["dO"]), P(l), P(m),
                         P(outs[0]), P(outs[1]), P(outs[2]), N, Nk, d, dv, B, P(r["QL"]), P(r["KL"]), left, right, 0.0,
                         P(wb), nwb, stream)
    assert rc == 0, L.fa_last_error()
    torch.cuda.synchronize()
    for nm, t in zip(OUTS, [Oo, l, m] + outs):
        assert torch.equal(t, r[nm]), nm
    st = ctypes.c_int(-2)
    assert L.fa_dense_bwd_handoff_status(P(wb), nwb, stream, ctypes.byref(st)) == 0 and st.value == -1


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_varlen_dpa_against_varlen_fa(fa, dtype):
    name = "c"
    case, ql, kl, _ = GPU_CASES[name]
    r = base_run(name, dtype)
    Od, ld, md = fa.varlen_dpa(r["Q"], r["K"], r["V"], r["QL"], r["KL"], case[5], case[6])
    torch.cuda.synchronize()
    er, _ = empty_rows(name)
    er_t = torch.tensor(er, device="cuda")
    assert bitwise_zero(Od.permute(0, 2, 1)[er_t]) and bitwise_zero(ld.permute(0, 2, 1)[er_t])
    assert bool((md.permute(0, 2, 1)[er_t] == float("-inf")).all())
    assert torch.equal(torch.isinf(md), torch.isinf(r["m"]))
    live = ~er[:, None, :]
    sel = lambda t: np.where(live, _np(t), 0.0)
    assert_close(sel(Od), sel(r["O"]), dtype, "varlen_dpa O vs varlen_fa O")
    assert_close(sel(Od), np.where(live, fwd_ref(name)[0], 0.0), dtype, "varlen_dpa O")
    assert_lm_close(sel(ld), sel(r["l"]), dtype, "varlen_dpa l")
    assert_lm_close(sel(md), sel(r["m"]), dtype, "varlen_dpa m")
