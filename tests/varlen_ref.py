"""Float64 numpy restatement of varlen attention (per-slab lengths in a padded batch), forward
and backward (helper for the tests, not a test), on top of local_ref.py.

Slab b is the leading nq = clamp(q_lens[b], 0, N) queries and nk = clamp(k_lens[b], 0, Nk) keys of
its (N, Nk) slab.  With off_b = nk - nq (of either sign) query i < nq attends the keys

    0 <= j < nk   and   i + off_b - left <= j <= i + off_b + right

(local_ref.visible with off_b; a negative side is unbounded).  A query that sees no key, and every
row i >= nq, is an EMPTY row: O = 0, l = 0, m = -inf, and it contributes to no gradient.  dQ rows
i >= nq, dK / dV rows j >= nk and the rows of keys that no query sees are 0.  Nothing past the
lengths is read: the padding rows of q, k, v, do never enter a product.
"""
from __future__ import annotations

import math

import numpy as np

from local_ref import visible


def lengths(lens, n: int, B: int) -> np.ndarray:
    """The clamped lengths of a batch (None: every slab full)."""
    if lens is None:
        return np.full(B, n, dtype=np.int64)
    out = np.clip(np.asarray(lens, dtype=np.int64), 0, n)
    assert out.shape == (B,)
    return out


def slab_visible(N: int, Nk: int, nq: int, nk: int, left: int, right: int) -> np.ndarray:
    """(N, Nk) bool of one slab: False past the lengths."""
    vis = np.zeros((N, Nk), dtype=bool)
    vis[:nq, :nk] = visible(0, nq, 0, nk, nk - nq, left, right)
    return vis


def varlen_fwd_ref(q, k, v, q_lens, k_lens, left: int, right: int, scale: float = 0.0):
    """O (N, dv, B), l (N, 1, B), m (N, 1, B) in float64; the empty-row state where a row is empty."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    N, d, B = q.shape
    Nk, dv = k.shape[0], v.shape[1]
    tau = float(scale) if scale > 0 else 1.0 / math.sqrt(d)
    nqs, nks = lengths(q_lens, N, B), lengths(k_lens, Nk, B)
    o = np.zeros((N, dv, B))
    l = np.zeros((N, 1, B))
    m = np.full((N, 1, B), -np.inf)
    for b in range(B):
        nq, nk = int(nqs[b]), int(nks[b])
        if nq == 0 or nk == 0:
            continue
        vis = visible(0, nq, 0, nk, nk - nq, left, right)
        S = np.where(vis, tau * (q[:nq, :, b] @ k[:nk, :, b].T), -np.inf)
        live = vis.any(axis=1)
        mb = S.max(axis=1)
        E = np.where(vis, np.exp(S - np.where(live, mb, 0.0)[:, None]), 0.0)
        lb = E.sum(axis=1)
        o[:nq, :, b] = np.where(live[:, None], (E / np.where(live, lb, 1.0)[:, None]) @ v[:nk, :, b], 0.0)
        l[:nq, 0, b] = lb
        m[:nq, 0, b] = mb
    return o, l, m


def varlen_bwd_ref(q, k, v, o, do, l, m, q_lens, k_lens, left: int, right: int, scale: float = 0.0):
    """(dQ, dK, dV) in float64.  l, m: (N, 1, B) or (N, B); None recomputes both in float64 (what
    the Float64 device path does).  D uses the o that is passed in (a device's own, rounded)."""
    q, k, v, o, do = (np.asarray(a, dtype=np.float64) for a in (q, k, v, o, do))
    N, d, B = q.shape
    Nk, dv = k.shape[0], v.shape[1]
    tau = float(scale) if scale > 0 else 1.0 / math.sqrt(d)
    if l is None or m is None:
        _, l, m = varlen_fwd_ref(q, k, v, q_lens, k_lens, left, right, scale)
    l = np.asarray(l, dtype=np.float64).reshape(N, B)
    m = np.asarray(m, dtype=np.float64).reshape(N, B)
    nqs, nks = lengths(q_lens, N, B), lengths(k_lens, Nk, B)
    dq = np.zeros((N, d, B))
    dk = np.zeros((Nk, d, B))
    dvv = np.zeros((Nk, dv, B))
    for b in range(B):
        nq, nk = int(nqs[b]), int(nks[b])
        if nq == 0 or nk == 0:
            continue
        vis = visible(0, nq, 0, nk, nk - nq, left, right)
        live = vis.any(axis=1)
        S = tau * (q[:nq, :, b] @ k[:nk, :, b].T)
        mb = np.where(live, m[:nq, b], 0.0)
        lb = np.where(live, l[:nq, b], 1.0)
        P = np.where(vis, np.exp(np.where(vis, S, 0.0) - mb[:, None]) / lb[:, None], 0.0)
        dP = do[:nq, :, b] @ v[:nk, :, b].T
        D = (do[:nq, :, b] * o[:nq, :, b]).sum(axis=1)
        dS = P * (dP - D[:, None])
        dq[:nq, :, b] = tau * (dS @ k[:nk, :, b])
        dk[:nk, :, b] = tau * (dS.T @ q[:nq, :, b])
        dvv[:nk, :, b] = P.T @ do[:nq, :, b]
    return dq, dk, dvv


def keyless_rows(N: int, Nk: int, nq: int, nk: int, left: int, right: int) -> np.ndarray:
    """(N,) bool: a query i < nq that sees no key."""
    out = np.zeros(N, dtype=bool)
    out[:nq] = ~slab_visible(N, Nk, nq, nk, left, right)[:nq].any(axis=1)
    return out


def unseen_keys(N: int, Nk: int, nq: int, nk: int, left: int, right: int) -> np.ndarray:
    """(Nk,) bool: a key j < nk that no query sees."""
    out = np.zeros(Nk, dtype=bool)
    out[:nk] = ~slab_visible(N, Nk, nq, nk, left, right)[:, :nk].any(axis=0)
    return out
