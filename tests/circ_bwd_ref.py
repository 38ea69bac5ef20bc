"""Float64 numpy restatement of the circulant (periodic banded) attention backward
(helper for the tests, not a test).

For query i, band entry t = 0..W-1 and key j(i, t) = (i - p + t) mod N, p = (W-1)//2,
tau = scale (<= 0: 1/sqrt(d)):

    s_it  = tau q_i.k_j        P_it = exp(s_it - m_i) / l_i
    dP_it = dO_i.v_j           D_i  = dO_i.O_i             dS_it = P_it (dP_it - D_i)
    dQ_i  = tau sum_t dS_it k_j
    dK_j  = tau sum_{(i,t): j(i,t)=j} dS_it q_i     dV_j = sum_{(i,t): j(i,t)=j} P_it dO_i

W > N repeats keys; every band entry counts once, as in the forward.  D uses the O
that is passed in, so a device's own (rounded) O can be given, as the dense tests do.
"""
from __future__ import annotations

import math

import numpy as np


CHUNK = 256   # queries gathered at a time (bounds the (rows, W, d) gathers)


def band_index(N: int, W: int) -> np.ndarray:
    """J[i, t] = (i - p + t) mod N, shape (N, W)."""
    p = (W - 1) // 2
    return (np.arange(N)[:, None] - p + np.arange(W)[None, :]) % N


def circulant_fwd_ref(Q, K, V, W: int, scale: float = 0.0):
    """O (N, dv, B), l (N, 1, B), m (N, 1, B) in float64 (m = max tau s, l = sum exp(tau s - m))."""
    Q, K, V = (np.asarray(a, dtype=np.float64) for a in (Q, K, V))
    N, d, B = Q.shape
    tau = float(scale) if scale > 0 else 1.0 / math.sqrt(d)
    J = band_index(N, W)
    O = np.empty((N, V.shape[1], B))
    l = np.empty((N, 1, B))
    m = np.empty((N, 1, B))
    for b in range(B):
        for i0 in range(0, N, CHUNK):
            r = slice(i0, min(i0 + CHUNK, N))
            S = tau * np.einsum("if,itf->it", Q[r, :, b], K[J[r], :, b])
            mb = S.max(axis=1)
            E = np.exp(S - mb[:, None])
            lb = E.sum(axis=1)
            O[r, :, b] = np.einsum("it,itc->ic", E / lb[:, None], V[J[r], :, b])
            l[r, 0, b], m[r, 0, b] = lb, mb
    return O, l, m


def circulant_bwd_ref(Q, K, V, O, dO, l, m, W: int, scale: float = 0.0):
    """(dQ, dK, dV) in float64.  l, m: (N, 1, B) or (N, B); None recomputes both in
    float64 from Q, K (what the Float64 device path does)."""
    Q, K, V, O, dO = (np.asarray(a, dtype=np.float64) for a in (Q, K, V, O, dO))
    N, d, B = Q.shape
    dv = V.shape[1]
    tau = float(scale) if scale > 0 else 1.0 / math.sqrt(d)
    J = band_index(N, W)
    if l is None or m is None:
        _, l, m = circulant_fwd_ref(Q, K, V, W, scale)
    l = np.asarray(l, dtype=np.float64).reshape(N, B)
    m = np.asarray(m, dtype=np.float64).reshape(N, B)
    dQ = np.zeros((N, d, B))
    dK = np.zeros((N, d, B))
    dV = np.zeros((N, dv, B))
    for b in range(B):
        P = np.empty((N, W))
        dS = np.empty((N, W))
        for i0 in range(0, N, CHUNK):
            r = slice(i0, min(i0 + CHUNK, N))
            Kg, Vg = K[J[r], :, b], V[J[r], :, b]             # (rows, W, d), (rows, W, dv)
            S = tau * np.einsum("if,itf->it", Q[r, :, b], Kg)
            P[r] = np.exp(S - m[r, b][:, None]) / l[r, b][:, None]
            dP = np.einsum("ic,itc->it", dO[r, :, b], Vg)
            D = (dO[r, :, b] * O[r, :, b]).sum(axis=1)
            dS[r] = P[r] * (dP - D[:, None])
            dQ[r, :, b] = tau * np.einsum("it,itf->if", dS[r], Kg)
        # scatter-add over J (np.add.at(dK, J, ...)): every column J[:, t] is a permutation
        # of the keys (i -> i + const mod N), so it is W plain indexed adds
        for t in range(W):
            dK[J[:, t], :, b] += tau * dS[:, t, None] * Q[:, :, b]
            dV[J[:, t], :, b] += P[:, t, None] * dO[:, :, b]
    return dQ, dK, dV
