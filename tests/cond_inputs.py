"""Ill-conditioned attention inputs and low-precision yardsticks for the backward and the
forward tests (helper for the tests, not a test).

family(): five input families that leave the regime of N(0, 1) inputs at scale 1/sqrt(d)
(unit-variance scores, row maxima of 2..5, the explicit scale argument unused):

    hot      N(0, 1) q, k at scale 4/sqrt(d): peaked rows (max P about 0.45), m = 7..20
    cold     N(0, 1) q, k at scale 0.25/sqrt(d): near-uniform P
    offset   q, k = 0.5 N(0, 1) + 3u, default scale: every score carries the common offset
             9 sqrt(d) (m = 70..80 at d = 64, 102..111 at d = 128; raw q.k = 600..1200)
    anti     q = 0.5 N(0, 1) + 3u, k = 0.5 N(0, 1) - 3u: the same offset, negative
    hotkeys  N(0, 1), then k[j] = 8 q[i] for three (i, j): those rows reach m = 8 |q_i|^2 /
             sqrt(d), and those keys draw weight from many other rows (scores 8 q_i'.q_i / sqrt(d))

u is a fixed +-1 vector of length d; v and do are N(0, 1) in every family.

lowp_backward(): the backward in the kernels' FORMULATION (not their code), in numpy: float32
raw scores, nlse = -(m + ln l) / tau in float32, P = exp2((s_raw + nlse) tau log2 e) in
float32, dS = P (dP - D) in float32, P and dS rounded to the 16-bit type before the three
gradient products (taken in float64).  Its distance to the float64 reference on a case is what
the formulation itself costs there: e_ref() measures it, budget() turns it into a tolerance.

lowp_forward(): the forward in the kernels' formulation (its docstring); fwd_shares() states an
(O, l, m) against the float64 forward as shares of the forward tests' limits (conftest's
assert_close and assert_lm_close, l_rtol() for l), and e_ref_fwd() is lowp_forward's shares: what
the limits leave to a device on a case.  band_counts(): a circulant band as key counts (W > N).

Masks: every helper that takes a mask takes (N, Nk) bool (key j visible to query i, the same in
every slab) or (N, Nk, B), one per slab: local_mask() and varlen_masks() build them from
local_ref.visible and varlen_ref.slab_visible.  A row with no visible key is an EMPTY row, as in
tests/varlen_ref.py: O = 0, l = 0, m = -inf in the forward helpers, P = 0 and no contribution in
the backward helpers whatever l, m are passed for it, and nothing in the numerator of a metric.
"""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch

from conftest import TOL
from local_ref import visible
from varlen_ref import lengths, slab_visible

FAMILIES = ("hot", "cold", "offset", "anti", "hotkeys")
GTOL = {"float32": 2e-5, "bfloat16": 2e-2, "float16": 5e-3}
ROUND16 = {"float32": None, "bfloat16": "bf16", "float16": "fp16", "float64": None}
LOG2E = 1.4426950408889634


def round_to(a, dtype: str) -> np.ndarray:
    """a rounded to `dtype` (bf16 for float32 and float64, as the other tests do), as float64."""
    t = torch.float16 if dtype == "float16" else torch.bfloat16
    return torch.tensor(np.asarray(a, dtype=np.float64)).to(t).double().numpy()


def _round16(a: np.ndarray, kind) -> np.ndarray:
    if kind is None:
        return a.astype(np.float64)
    assert kind in ("bf16", "fp16"), kind
    t = torch.bfloat16 if kind == "bf16" else torch.float16
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(t).double().numpy()


def sign_vector(d: int) -> np.ndarray:
    """The fixed +-1 vector u of length d."""
    return np.where(np.random.default_rng(1000 + d).random(d) < 0.5, -1.0, 1.0)


def _slab(mask, b: int):
    """Slab b's (N, Nk) mask of a 2-D (shared) or 3-D (per-slab) mask; None stays None."""
    if mask is None:
        return None
    mask = np.asarray(mask)
    assert mask.ndim in (2, 3), mask.shape
    return mask if mask.ndim == 2 else mask[:, :, b]


def hot_pairs(N: int, Nk: int, B: int, mask=None):
    """Three (i, j, slab) with the keys j in different thirds of the key range (different 64-key
    tiles from Nk = 192 up) and, at B > 1, different slabs.  With a mask (module docstring) the
    keys are taken from the thirds of the SEEN keys of the slab the pair goes to (those some
    query sees: all of them under a causal mask or a band, not under a local window with
    off - left > 0 or past a varlen slab's lengths), and the query is the middle one of those
    that see key j.  A slab that sees no key gets no pair."""
    out = []
    for t in range(min(3, Nk)):
        if mask is None:
            j = min(Nk - 1, ((2 * t + 1) * Nk) // 6 + t)
            i = (j * 7 + 13 * (t + 1)) % N
        else:
            mk = _slab(mask, t % B)
            seen = np.flatnonzero(mk.any(axis=0))
            if not seen.size:
                continue
            j = int(seen[min(seen.size - 1, ((2 * t + 1) * seen.size) // 6 + t)])
            rows = np.flatnonzero(mk[:, j])
            i = int(rows[rows.size // 2])
        out.append((i, j, t % B))
    return out


def family(name: str, N: int, Nk: int, d: int, dv: int, B: int, dtype: str, mask=None, seed: int = 0):
    """(q, k, v, do, scale): float64 arrays (N, d, B), (Nk, d, B), (Nk, dv, B), (N, dv, B) that
    are exactly representable in `dtype`, and the scale argument to pass (0: the default).
    Seeded from (name, N, Nk, d), and from `seed` where it is not 0 (another draw of the same
    family).  mask places the hotkeys pairs where query i sees key j."""
    assert name in FAMILIES, name
    rng = np.random.default_rng(zlib.crc32((f"{name}-{N}-{Nk}-{d}" + (f"-{seed}" if seed else "")).encode()))
    q, k = rng.standard_normal((N, d, B)), rng.standard_normal((Nk, d, B))
    v, do = rng.standard_normal((Nk, dv, B)), rng.standard_normal((N, dv, B))
    scale = 0.0
    # the C ABI takes scale as a float: the value returned is the float32 the device receives
    if name == "hot":
        scale = float(np.float32(4.0 / math.sqrt(d)))
    elif name == "cold":
        scale = float(np.float32(0.25 / math.sqrt(d)))
    elif name in ("offset", "anti"):
        u = sign_vector(d)[None, :, None]
        q = 0.5 * q + 3.0 * u
        k = 0.5 * k + (3.0 if name == "offset" else -3.0) * u
    q, k, v, do = (round_to(a, dtype) for a in (q, k, v, do))
    if name == "hotkeys":
        for i, j, b in hot_pairs(N, Nk, B, mask):
            k[j, :, b] = 8.0 * q[i, :, b]        # a power of two: still representable
    return q, k, v, do, scale


def tau_of(scale: float, d: int) -> float:
    return float(scale) if scale > 0 else 1.0 / math.sqrt(d)


def forward_f64(q, k, v, scale: float = 0.0, mask=None, counts=None):
    """O (N, dv, B), l, m (N, 1, B) in float64 of (masked) softmax(tau q k^T) v; statistics over
    the visible keys; an empty row is O = 0, l = 0, m = -inf.  counts: optional (N, Nk) integers,
    how often query i takes key j (a circulant band with W > N repeats keys); it replaces mask,
    keys with count 0 are hidden."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    N, d, B = q.shape
    tau = tau_of(scale, d)
    o = np.empty((N, v.shape[1], B))
    l = np.empty((N, 1, B))
    m = np.empty((N, 1, B))
    if counts is not None:
        assert mask is None
        mask = np.asarray(counts) > 0
    for b in range(B):
        S = tau * (q[:, :, b] @ k[:, :, b].T)
        if mask is not None:
            S = np.where(_slab(mask, b), S, -np.inf)
        mb = S.max(axis=1) if S.shape[1] else np.full(N, -np.inf)
        live = np.isfinite(mb)                      # an empty row: exp(-inf - 0) = 0 everywhere
        E = np.exp(S - np.where(live, mb, 0.0)[:, None])
        if counts is not None:
            E = E * counts
        lb = E.sum(axis=1)
        o[:, :, b] = (E / np.where(live, lb, 1.0)[:, None]) @ v[:, :, b]
        l[:, 0, b], m[:, 0, b] = lb, mb
    return o, l, m


def backward_f64(q, k, v, do, O, l, m, scale: float = 0.0, mask=None):
    """(dQ, dK, dV) in float64 on the O, l, m that are passed in.  Which rows are empty comes
    from the mask, never from l, m: an empty row has P = 0."""
    q, k, v, do, O = (np.asarray(a, dtype=np.float64) for a in (q, k, v, do, O))
    N, d, B = q.shape
    tau = tau_of(scale, d)
    l = np.asarray(l, dtype=np.float64).reshape(N, B)
    m = np.asarray(m, dtype=np.float64).reshape(N, B)
    dq, dk, dvv = np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    for b in range(B):
        S = tau * (q[:, :, b] @ k[:, :, b].T)
        mb, lb = m[:, b], l[:, b]
        if mask is not None:
            mk = _slab(mask, b)
            live = mk.any(axis=1)
            S = np.where(mk, S, -np.inf)
            mb, lb = np.where(live, mb, 0.0), np.where(live, lb, 1.0)
        P = np.exp(S - mb[:, None]) / lb[:, None]
        dP = do[:, :, b] @ v[:, :, b].T
        D = (do[:, :, b] * O[:, :, b]).sum(axis=1)
        dS = P * (dP - D[:, None])
        dq[:, :, b] = tau * (dS @ k[:, :, b])
        dk[:, :, b] = tau * (dS.T @ q[:, :, b])
        dvv[:, :, b] = P.T @ do[:, :, b]
    return dq, dk, dvv


def lowp_backward(q, k, v, do, O, l, m, scale, round16=None, mask=None):
    """(dQ, dK, dV) of the kernels' formulation (module docstring).  q (N, d, B), k (Nk, d, B),
    v (Nk, dv, B), do, O (N, dv, B), l, m (N, 1, B) or (N, B); round16: None, "bf16" or "fp16";
    mask: optional (module docstring); an empty row has P = 0 whatever its l, m."""
    f32 = np.float32
    q, k, v, do, O = (np.asarray(a, dtype=np.float64) for a in (q, k, v, do, O))
    N, d, B = q.shape
    tau = f32(tau_of(scale, d))
    tau_log2 = f32(tau * f32(LOG2E))
    l = np.asarray(l, dtype=f32).reshape(N, B)
    m = np.asarray(m, dtype=f32).reshape(N, B)
    dq, dk, dvv = np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    for b in range(B):
        qb, kb, vb, dob, ob = (a[:, :, b].astype(f32) for a in (q, k, v, do, O))
        s_raw = qb @ kb.T                                           # float32
        mb, lb = m[:, b], l[:, b]
        if mask is not None:
            mk = _slab(mask, b)
            live = mk.any(axis=1)
            mb, lb = np.where(live, mb, f32(0.0)), np.where(live, lb, f32(1.0))
        nlse = (-(mb + np.log(lb)) / tau).astype(f32)
        arg = ((s_raw + nlse[:, None]) * tau_log2).astype(f32)
        if mask is not None:
            arg = np.where(mk, arg, f32(-np.inf))
        P = np.exp2(arg).astype(f32)
        dP = dob @ vb.T
        D = (dob * ob).sum(axis=1, dtype=f32)
        dS = (P * (dP - D[:, None])).astype(f32)
        P16, dS16 = _round16(P, round16), _round16(dS, round16)
        dq[:, :, b] = float(tau) * (dS16 @ k[:, :, b])
        dk[:, :, b] = float(tau) * (dS16.T @ q[:, :, b])
        dvv[:, :, b] = P16.T @ do[:, :, b]
    return dq, dk, dvv


def grad_metrics(x, y, floor: float = 1e-2):
    """The two metrics of assert_grad_close (tests/test_gpu_backward.py): max|x - y| / max|y|
    and ||x - y|| / ||y||, each denominator floored (at `floor`, `floor` sqrt(size))."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    err = np.abs(x - y).max() / max(np.abs(y).max(), floor)
    rel = np.linalg.norm(x - y) / max(np.linalg.norm(y), floor * np.sqrt(y.size))
    return float(err), float(rel)


def e_ref(q, k, v, do, scale, dtype: str, mask=None) -> float:
    """What the formulation costs on this case: the larger metric, over dQ, dK, dV, of
    lowp_backward against the float64 backward, both on the float64 forward's O (rounded to
    `dtype`) and its l, m (rounded to float32).  Nothing here comes from a device."""
    o, l, m = forward_f64(q, k, v, scale, mask)
    if dtype in ("bfloat16", "float16"):
        o = round_to(o, dtype)
    elif dtype == "float32":
        o = o.astype(np.float32).astype(np.float64)
    l, m = l.astype(np.float32), m.astype(np.float32)
    ref = backward_f64(q, k, v, do, o, l, m, scale, mask)
    low = lowp_backward(q, k, v, do, o, l, m, scale, ROUND16[dtype], mask)
    return max(max(grad_metrics(x, y)) for x, y in zip(low, ref))


def budget(dtype: str, eref: float) -> float:
    """max(GTOL, 2 e_ref): the factor 2 is for the summation order and the MFMA accumulation,
    which lowp_backward does not model."""
    return max(GTOL[dtype], 2.0 * eref)


def l_rtol(m_ref, dtype: str) -> float:
    """The limit on |l - l_ref| / (1 + |l_ref|): conftest's rule where float32 scores allow it.
    A float32 score of size |s| moves its exponential by up to a few |s| 2^-24 (2.6e-5 at
    |s| = 110), whatever the kernel does.  dtype names the conftest row (float32 for Float64
    kernels: l, m leave every kernel as float32)."""
    a = np.abs(np.asarray(m_ref, dtype=np.float64))
    a = a[np.isfinite(a)]                           # empty rows (m = -inf) hold no score
    return max(TOL[dtype]["lm"], 8.0 * (float(a.max()) if a.size else 0.0) * 2.0 ** -24)


def lowp_forward(q, k, v, scale, round16=None, mask=None, counts=None, lag_log2: float = 0.0, exponent: str = "fma"):
    """(O, l, m) of the forward kernels' FORMULATION (not their code), in numpy: float32 raw
    scores s, c = tau log2(e) in float32, P = exp2(fma(s, c, -m_used c)) in float32 with m_used
    lag_log2 / c below the row maximum (the lazy rescale lets it lag by up to 8 log2 units), l
    summed in float32, P rounded to the 16-bit type before P V (taken in float64), O rounded
    to the output type (float32 where round16 is None), l = l_used 2^((m_used - m) c),
    m = max(s) tau.  mask, counts as in forward_f64 (a repeated key adds its rounded P each time);
    an empty row is O = 0, l = 0, m = -inf.  exponent: "fma" as above, or "sub" for the LOCAL / VARLEN
    bodies' row-local form P = exp2(fl(fl(s - m_used) c)) (two roundings, no product m_used c)."""
    assert exponent in ("fma", "sub"), exponent
    f32 = np.float32
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    N, d, B = q.shape
    tau = f32(tau_of(scale, d))
    c = f32(tau * f32(LOG2E))
    if counts is not None:
        assert mask is None
        counts = np.asarray(counts)
        mask = counts > 0
    o = np.empty((N, v.shape[1], B))
    l = np.empty((N, 1, B))
    m = np.empty((N, 1, B))
    for b in range(B):
        s_raw = q[:, :, b].astype(f32) @ k[:, :, b].astype(f32).T
        if mask is not None:
            s_raw = np.where(_slab(mask, b), s_raw, f32(-np.inf))
        m_true = s_raw.max(axis=1) if s_raw.shape[1] else np.full(N, f32(-np.inf))
        live = np.isfinite(m_true)
        m_used = np.where(live, (m_true - f32(lag_log2) / c).astype(f32), f32(0.0))   # an empty row: offset 0, P = 0
        if exponent == "fma":
            mc = (m_used * c).astype(f32)
            arg = (s_raw.astype(np.float64) * float(c) - mc.astype(np.float64)[:, None]).astype(f32)   # one rounding: the fma
        else:
            arg = ((s_raw - m_used[:, None]).astype(f32) * c).astype(f32)
        P = np.exp2(arg).astype(f32)
        P16 = _round16(P, round16)
        if counts is not None:
            P, P16 = (P * counts).astype(f32), P16 * counts
        l_used = P.sum(axis=1, dtype=f32)
        ob = (P16 @ v[:, :, b]) / np.where(live, l_used, f32(1.0)).astype(np.float64)[:, None]
        o[:, :, b] = ob.astype(f32) if round16 is None else _round16(ob, round16)
        l[:, 0, b] = (l_used * np.exp2(((m_used - np.where(live, m_true, f32(0.0))) * c).astype(f32))).astype(f32)
        m[:, 0, b] = (m_true * tau).astype(f32)
    return o, l, m


ELEM64 = 1e-12   # Float64 outputs: relative to max(|y|, 1) (tests/test_gpu_float64.py)


def fwd_shares(o, l, m, o_ref, l_ref, m_ref, dtype: str) -> dict:
    """What share of each forward limit (o, l, m) uses against the float64 (o_ref, l_ref,
    m_ref): conftest.assert_close's norm-wise and elementwise limits on O (Float64: ELEM64),
    assert_lm_close's on m, l_rtol on l.  A share above 1 fails the assertion it stands for."""
    x, y = np.asarray(o, dtype=np.float64), np.asarray(o_ref, dtype=np.float64)
    m, m_ref = np.asarray(m, dtype=np.float64), np.asarray(m_ref, dtype=np.float64)
    empty = np.isneginf(m_ref)                      # an empty row's m = -inf enters no metric
    if empty.any():
        assert np.array_equal(np.isneginf(m), empty), "m = -inf on other rows than the reference's empty ones"
        m, m_ref = np.where(empty, 0.0, m), np.where(empty, 0.0, m_ref)
    err = np.abs(x - y)
    out = {}
    if dtype == "float64":
        out["O elem"] = err.max() / max(np.abs(y).max(), 1.0) / ELEM64
        lm_dt = "float32"
    else:
        t = TOL[dtype]
        lm_dt = dtype
        out["O norm"] = np.linalg.norm(x - y) / (t["norm"] * max(np.linalg.norm(x), np.linalg.norm(y), 1e-30))
        if dtype == "float32":
            out["O elem"] = err.max() / (t["elem_rel_max"] * np.abs(y).max() + t["elem_abs"])
        else:
            out["O elem"] = (err / (t["elem"] * (1 + np.abs(y)))).max()
    rel = lambda a, r: (np.abs(np.asarray(a, dtype=np.float64) - r) / (1 + np.abs(r))).max()
    out["l"] = rel(l, l_ref) / l_rtol(m_ref, lm_dt)
    out["m"] = rel(m, m_ref) / TOL[lm_dt]["lm"]
    return {nm: float(s) for nm, s in out.items()}


def e_ref_fwd(q, k, v, scale, dtype: str, mask=None, counts=None, ref=None, local_exponent: bool = False) -> dict:
    """What the forward formulation costs on this case: fwd_shares of lowp_forward against the
    float64 forward (ref, if the caller has it), per limit the worse of no lag and a lag of 8
    log2 units, and with local_exponent (the LOCAL / VARLEN bodies) of lowp_forward's two exponent
    forms.  Nothing here comes from a device.  Float64: the reference itself, all 0."""
    ref = forward_f64(q, k, v, scale, mask, counts) if ref is None else ref
    if dtype == "float64":
        return dict.fromkeys(("O elem", "l", "m"), 0.0)
    worst = {}
    for form in (("fma", "sub") if local_exponent else ("fma",)):
        for lag in (0.0, 8.0):
            sh = fwd_shares(*lowp_forward(q, k, v, scale, ROUND16[dtype], mask, counts, lag, form), *ref, dtype)
            worst = {nm: max(s, worst.get(nm, 0.0)) for nm, s in sh.items()}
    return worst


def causal_mask(N: int, Nk: int) -> np.ndarray:
    return np.arange(Nk)[None, :] <= np.arange(N)[:, None] + (Nk - N)


def local_mask(N: int, Nk: int, left: int, right: int) -> np.ndarray:
    """(N, Nk) bool of local attention (local_ref.visible with off = Nk - N; a negative side unbounded)."""
    return visible(0, N, 0, Nk, Nk - N, left, right)


def varlen_masks(N: int, Nk: int, q_lens, k_lens, left: int, right: int) -> np.ndarray:
    """(N, Nk, B) bool of a varlen batch: varlen_ref.slab_visible on each slab's clamped lengths
    (one of q_lens, k_lens may be None: full)."""
    B = len(q_lens if q_lens is not None else k_lens)
    nqs, nks = lengths(q_lens, N, B), lengths(k_lens, Nk, B)
    return np.stack([slab_visible(N, Nk, int(nqs[b]), int(nks[b]), left, right) for b in range(B)], axis=2)


def band_mask(N: int, W: int) -> np.ndarray:
    """Circulant band of W <= N keys (i - p + t) mod N, p = (W - 1) // 2, as a mask."""
    assert W <= N
    p = (W - 1) // 2
    mk = np.zeros((N, N), dtype=bool)
    mk[np.arange(N)[:, None], (np.arange(N)[:, None] - p + np.arange(W)[None, :]) % N] = True
    return mk


def band_counts(N: int, W: int) -> np.ndarray:
    """(N, N) integers: how often the band (i - p + t) mod N, t < W, p = (W - 1) // 2, of query
    i takes key j.  W <= N: band_mask as 0 / 1; W > N: the keys repeat."""
    p = (W - 1) // 2
    cnt = np.zeros((N, N), dtype=np.int64)
    rows = np.broadcast_to(np.arange(N)[:, None], (N, W))
    np.add.at(cnt, (rows, (np.arange(N)[:, None] - p + np.arange(W)[None, :]) % N), 1)
    return cnt
