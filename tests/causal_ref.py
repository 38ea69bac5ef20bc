"""Float64 numpy restatement of causal dense attention, forward and backward (helper for
the tests, not a test).

Query i attends the keys j <= i + off, off = Nk - N >= 0 (bottom-right alignment: the last
query sees every key; N == Nk is the lower triangle).  With tau = scale (<= 0: 1/sqrt(d)):

    s_ij  = tau q_i.k_j  (j visible)      m_i = max_j s_ij      l_i = sum_j exp(s_ij - m_i)
    P_ij  = exp(s_ij - m_i) / l_i         O_i = sum_j P_ij v_j
    dP_ij = dO_i.v_j    D_i = dO_i.O_i    dS_ij = P_ij (dP_ij - D_i)
    dQ_i  = tau sum_j dS_ij k_j           dK_j = tau sum_i dS_ij q_i       dV_j = sum_i P_ij dO_i

The mask is a select: masked scores never enter a max, a sum or a product.  D uses the O
that is passed in, so a device's own (rounded) O can be given, as the dense tests do.
"""
from __future__ import annotations

import math

import numpy as np


CHUNK = 512   # queries scored at a time (bounds the (rows, Nk) score blocks)


def _visible(i0: int, i1: int, Nk: int, off: int) -> np.ndarray:
    """(rows, Nk) bool: key j is visible to query i, i0 <= i < i1."""
    return np.arange(Nk)[None, :] <= np.arange(i0, i1)[:, None] + off


def causal_fwd_ref(q, k, v, scale: float = 0.0):
    """O (N, dv, B), l (N, 1, B), m (N, 1, B) in float64, statistics over the visible keys."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    N, d, B = q.shape
    Nk = k.shape[0]
    assert Nk >= N, "causal attention needs Nk >= N"
    off = Nk - N
    tau = float(scale) if scale > 0 else 1.0 / math.sqrt(d)
    o = np.empty((N, v.shape[1], B))
    l = np.empty((N, 1, B))
    m = np.empty((N, 1, B))
    for b in range(B):
        for i0 in range(0, N, CHUNK):
            i1 = min(i0 + CHUNK, N)
            kv = min(Nk, i1 + off)                       # no later key is visible to this chunk
            vis = _visible(i0, i1, kv, off)
            S = np.where(vis, tau * (q[i0:i1, :, b] @ k[:kv, :, b].T), -np.inf)
            mb = S.max(axis=1)
            E = np.where(vis, np.exp(S - mb[:, None]), 0.0)
            lb = E.sum(axis=1)
            o[i0:i1, :, b] = (E / lb[:, None]) @ v[:kv, :, b]
            l[i0:i1, 0, b], m[i0:i1, 0, b] = lb, mb
    return o, l, m


def causal_bwd_ref(q, k, v, o, do, l, m, scale: float = 0.0):
    """(dQ, dK, dV) in float64.  l, m: (N, 1, B) or (N, B); None recomputes both in float64
    from q, k (what the Float64 device path does)."""
    q, k, v, o, do = (np.asarray(a, dtype=np.float64) for a in (q, k, v, o, do))
    N, d, B = q.shape
    Nk, dv = k.shape[0], v.shape[1]
    assert Nk >= N, "causal attention needs Nk >= N"
    off = Nk - N
    tau = float(scale) if scale > 0 else 1.0 / math.sqrt(d)
    if l is None or m is None:
        _, l, m = causal_fwd_ref(q, k, v, scale)
    l = np.asarray(l, dtype=np.float64).reshape(N, B)
    m = np.asarray(m, dtype=np.float64).reshape(N, B)
    dq = np.zeros((N, d, B))
    dk = np.zeros((Nk, d, B))
    dvv = np.zeros((Nk, dv, B))
    for b in range(B):
        for i0 in range(0, N, CHUNK):
            i1 = min(i0 + CHUNK, N)
            kv = min(Nk, i1 + off)
            vis = _visible(i0, i1, kv, off)
            S = tau * (q[i0:i1, :, b] @ k[:kv, :, b].T)
            P = np.where(vis, np.exp(np.where(vis, S, 0.0) - m[i0:i1, b][:, None]) / l[i0:i1, b][:, None], 0.0)
            dP = do[i0:i1, :, b] @ v[:kv, :, b].T
            D = (do[i0:i1, :, b] * o[i0:i1, :, b]).sum(axis=1)
            dS = P * (dP - D[:, None])
            dq[i0:i1, :, b] = tau * (dS @ k[:kv, :, b])
            dk[:kv, :, b] += tau * (dS.T @ q[i0:i1, :, b])
            dvv[:kv, :, b] += P.T @ do[i0:i1, :, b]
    return dq, dk, dvv
