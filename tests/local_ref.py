"""Float64 numpy restatement of local (sliding-window) attention, forward and backward
(helper for the tests, not a test), in causal_ref.py's form.

With off = Nk - N >= 0 (bottom-right alignment), query i attends the keys

    0 <= j < Nk   and   i + off - left <= j <= i + off + right,

where a negative left / right means no bound on that side: (-1, 0) is causal attention,
(-1, -1) dense attention, (0, 0) one key per query.  With tau = scale (<= 0: 1/sqrt(d)):

    s_ij  = tau q_i.k_j  (j visible)      m_i = max_j s_ij      l_i = sum_j exp(s_ij - m_i)
    P_ij  = exp(s_ij - m_i) / l_i         O_i = sum_j P_ij v_j
    dP_ij = dO_i.v_j    D_i = dO_i.O_i    dS_ij = P_ij (dP_ij - D_i)
    dQ_i  = tau sum_j dS_ij k_j           dK_j = tau sum_i dS_ij q_i       dV_j = sum_i P_ij dO_i

The mask is a select: masked scores never enter a max, a sum or a product, so dK and dV of a
key that no query sees are exactly 0.  D uses the O that is passed in, so a device's own
(rounded) O can be given.
"""
from __future__ import annotations

import math

import numpy as np


CHUNK = 512   # queries scored at a time (bounds the (rows, keys) score blocks)


def visible(i0: int, i1: int, j0: int, j1: int, off: int, left: int, right: int) -> np.ndarray:
    """(i1 - i0, j1 - j0) bool: key j (j0 <= j < j1) is visible to query i (i0 <= i < i1)."""
    c = np.arange(i0, i1)[:, None] + off          # the causal diagonal's key of each query
    j = np.arange(j0, j1)[None, :]
    vis = np.ones((i1 - i0, j1 - j0), dtype=bool)
    if right >= 0:
        vis &= j <= c + right
    if left >= 0:
        vis &= j >= c - left
    return vis


def unseen_keys(N: int, Nk: int, left: int, right: int) -> np.ndarray:
    """(Nk,) bool: no query sees key j."""
    return ~visible(0, N, 0, Nk, Nk - N, left, right).any(axis=0)


def _key_range(i0: int, i1: int, Nk: int, off: int, left: int, right: int):
    """Keys [j0, j1) outside which nothing is visible to the queries i0 <= i < i1."""
    j0 = 0 if left < 0 else max(0, i0 + off - left)
    j1 = Nk if right < 0 else min(Nk, i1 - 1 + off + right + 1)
    return j0, j1


def local_fwd_ref(q, k, v, left: int, right: int, scale: float = 0.0):
    """O (N, dv, B), l (N, 1, B), m (N, 1, B) in float64, statistics over the visible keys."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    N, d, B = q.shape
    Nk = k.shape[0]
    assert Nk >= N, "local attention needs Nk >= N"
    off = Nk - N
    tau = float(scale) if scale > 0 else 1.0 / math.sqrt(d)
    o = np.empty((N, v.shape[1], B))
    l = np.empty((N, 1, B))
    m = np.empty((N, 1, B))
    for b in range(B):
        for i0 in range(0, N, CHUNK):
            i1 = min(i0 + CHUNK, N)
            j0, j1 = _key_range(i0, i1, Nk, off, left, right)
            vis = visible(i0, i1, j0, j1, off, left, right)
            S = np.where(vis, tau * (q[i0:i1, :, b] @ k[j0:j1, :, b].T), -np.inf)
            mb = S.max(axis=1)
            E = np.where(vis, np.exp(S - mb[:, None]), 0.0)
            lb = E.sum(axis=1)
            o[i0:i1, :, b] = (E / lb[:, None]) @ v[j0:j1, :, b]
            l[i0:i1, 0, b], m[i0:i1, 0, b] = lb, mb
    return o, l, m


def local_bwd_ref(q, k, v, o, do, l, m, left: int, right: int, scale: float = 0.0):
    """(dQ, dK, dV) in float64.  l, m: (N, 1, B) or (N, B); None recomputes both in float64
    from q, k (what the Float64 device path does)."""
    q, k, v, o, do = (np.asarray(a, dtype=np.float64) for a in (q, k, v, o, do))
    N, d, B = q.shape
    Nk, dv = k.shape[0], v.shape[1]
    assert Nk >= N, "local attention needs Nk >= N"
    off = Nk - N
    tau = float(scale) if scale > 0 else 1.0 / math.sqrt(d)
    if l is None or m is None:
        _, l, m = local_fwd_ref(q, k, v, left, right, scale)
    l = np.asarray(l, dtype=np.float64).reshape(N, B)
    m = np.asarray(m, dtype=np.float64).reshape(N, B)
    dq = np.zeros((N, d, B))
    dk = np.zeros((Nk, d, B))
    dvv = np.zeros((Nk, dv, B))
    for b in range(B):
        for i0 in range(0, N, CHUNK):
            i1 = min(i0 + CHUNK, N)
            j0, j1 = _key_range(i0, i1, Nk, off, left, right)
            vis = visible(i0, i1, j0, j1, off, left, right)
            S = tau * (q[i0:i1, :, b] @ k[j0:j1, :, b].T)
            P = np.where(vis, np.exp(np.where(vis, S, 0.0) - m[i0:i1, b][:, None]) / l[i0:i1, b][:, None], 0.0)
            dP = do[i0:i1, :, b] @ v[j0:j1, :, b].T
            D = (do[i0:i1, :, b] * o[i0:i1, :, b]).sum(axis=1)
            dS = P * (dP - D[:, None])
            dq[i0:i1, :, b] = tau * (dS @ k[j0:j1, :, b])
            dk[j0:j1, :, b] += tau * (dS.T @ q[i0:i1, :, b])
            dvv[j0:j1, :, b] += P.T @ do[i0:i1, :, b]
    return dq, dk, dvv
