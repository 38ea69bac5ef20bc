#!/usr/bin/env python
"""Time the cache writers against the plain-torch forms a caller would write without them.

    python tools/bench_kv_append.py [--rounds 5]

Shapes: the decode append (N = 1; 128 and 1024 slabs; d = dv = 128; pages of 16 and 64), a prefill
chunk (N = 2048, 8 slabs) and the quantise of a (8192, 128, 8) cache.  Both forms run in the same
process, alternating, after a warm-up of each; a time is the median over the rounds of a device-event
window of `iters` calls.  GB/s is over the algorithmic bytes: source read plus destination written."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flashattention.jl_amd"))
import fa_hip  # noqa: E402


def torch_append(kp, vp, table, kn, vn, kl, scales=None):
    """Every slab appends its N rows (q_lens = N) so that it ends at kl: index arithmetic in torch."""
    N, B, ps, P = kn.shape[0], kn.shape[2], kp.shape[0], kp.shape[2]
    j = (kl.long() - N)[None, :] + torch.arange(N, device=kn.device)[:, None]     # (N, B) logical positions
    page = table.long().gather(0, j // ps).clamp(0, P - 1)
    row = j % ps
    for pool, new, s in ((kp, kn, scales and scales[0]), (vp, vn, scales and scales[1])):
        if s is not None:
            new = (new.float() / s[None, None, :]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        pool[row, :, page] = new.permute(0, 2, 1)


def window(f, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us per call


def compare(name, hip, ref, nbytes, iters, rounds):
    for f in (hip, ref):
        window(f, max(3, iters // 10))
    th, tr = [], []
    for _ in range(rounds):
        th.append(window(hip, iters))
        tr.append(window(ref, iters))
    h, r = statistics.median(th), statistics.median(tr)
    print(f"{name:44s} hip {h:9.1f} us {nbytes / h / 1e3:8.1f} GB/s | torch {r:9.1f} us {nbytes / r / 1e3:8.1f} GB/s | x{r / h:6.2f}"
          f" | hip min..max {min(th):.1f}..{max(th):.1f}", flush=True)


def append_case(N, B, ps, context, fp8, iters, rounds, d=128, dv=128):
    dev, dt = "cuda", torch.bfloat16
    mp = -(-(context + N) // ps)
    P = B * mp
    pdt = torch.uint8 if fp8 else dt
    kp, vp = (fa_hip.jl_empty((ps, n, P), pdt, dev).zero_() for n in (d, dv))
    kn, vn = (fa_hip.jl_tensor(torch.randn(N, n, B), dt, dev) for n in (d, dv))
    table = fa_hip.jl_tensor(torch.randperm(P).int().reshape(B, mp).t(), torch.int32, dev)
    kl = (torch.randint(context // 2, context + 1, (B,)) + N).int().to(dev)
    sc = (torch.full((B,), 0.37, device=dev), torch.full((B,), 0.91, device=dev)) if fp8 else None
    if fp8:
        hip = lambda: fa_hip.paged_kv_append_fp8_(kp, vp, table, kn, vn, sc[0], sc[1], kl)
    else:
        hip = lambda: fa_hip.paged_kv_append_(kp, vp, table, kn, vn, kl)
    ref = lambda: torch_append(kp, vp, table, kn, vn, kl, sc)
    nbytes = N * (d + dv) * B * (3 if fp8 else 4)
    compare(f"append{'_fp8' if fp8 else ''} N={N} B={B} page={ps}", hip, ref, nbytes, iters, rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kv_append.py needs a ROCm device"
    torch.manual_seed(0)
    print(torch.cuda.get_device_name(0))
    for fp8 in (False, True):
        for B in (128, 1024):
            for ps in (16, 64):
                append_case(1, B, ps, 1024, fp8, 500, a.rounds)
        for ps in (16, 64):
            append_case(2048, 8, ps, 2048, fp8, 50, a.rounds)
    k, v = (fa_hip.jl_tensor(torch.randn(8192, 128, 8), torch.bfloat16, "cuda") for _ in range(2))
    compare("quantise Nk=8192 d=dv=128 B=8", lambda: fa_hip.quantize_kv_fp8_hip(k, v), lambda: fa_hip.quantize_kv_fp8(k, v),
            2 * k.numel() * 3, 50, a.rounds)


if __name__ == "__main__":
    main()
