"""A/B the dense forward of two builds of libfa_hip.so in ONE process, interleaved
rounds after a clock settle: configs[1] (4096, 64, 64 slabs) bf16, the same with 128
slabs, a ragged-key shape, configs[3] and configs[3] on the 8-wave kernel (variant 5,
w8b64_wide); y, l, m checked bitwise against the first build.  Prints every round (a gain counts when every round favours it and the median
gain exceeds the spread between rounds of one build).
Usage: python tools/exp/ab_fwd_libs.py LIB_A LIB_B"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flashattention.jl_amd")]
import torch
import fa_hip
from bench import _randn_jl

libs = []
for p in sys.argv[1:]:
    fa_hip._LIB = None
    os.environ["FA_HIP_LIB"] = os.path.abspath(p)
    libs.append(fa_hip.lib())


def use(i):
    fa_hip._LIB = libs[i]


g = torch.Generator(device="cuda").manual_seed(1)
# (N, Nk, d, slabs[, forward variant])
shapes = [(4096, 4096, 64, 64), (4096, 4096, 64, 128), (4096, 4000, 64, 64), (8192, 8192, 128, 64), (8192, 8192, 128, 64, 5)]
if os.environ.get("AB_SHAPES"):   # e.g. AB_SHAPES="4096,4096,64,64;8192,8192,128,64,5"
    shapes = [tuple(int(x) for x in sh.split(",")) for sh in os.environ["AB_SHAPES"].split(";")]
data = {}
for (N, Nk, d, BH) in sorted(set(sh[:4] for sh in shapes)):
    data[(N, Nk, d, BH)] = (_randn_jl(fa_hip, (N, d, BH), torch.bfloat16, g), _randn_jl(fa_hip, (Nk, d, BH), torch.bfloat16, g),
                            _randn_jl(fa_hip, (Nk, d, BH), torch.bfloat16, g))
use(0)
Q, K, V = data[shapes[0][:4]]
for _ in range(2000):
    fa_hip.dense_fa(Q, K, V)
torch.cuda.synchronize()
for sh in shapes:
    Q, K, V = data[sh[:4]]
    for L in libs:
        L.fa_debug_set_fwd_variant(sh[4] if len(sh) > 4 else 0)
    ref = None
    same = {}
    for i in range(len(libs)):
        use(i)
        out = [t.clone() for t in fa_hip.dense_fa(Q, K, V)]
        ref = ref or out
        same[i] = all(torch.equal(a, b) for a, b in zip(out, ref))
    ts = {i: [] for i in range(len(libs))}
    for rnd in range(8):
        for i in range(len(libs)):
            use(i)
            for _ in range(20):
                fa_hip.dense_fa(Q, K, V)
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(40):
                fa_hip.dense_fa(Q, K, V)
            e1.record(); torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1) / 40 * 1e3)
    N, Nk, d, BH = sh[:4]
    fl = 4.0 * BH * N * Nk * d
    for i in range(len(libs)):
        print(f"{sh} lib {i} rounds (us): " + " ".join(f"{t:.1f}" for t in ts[i]), flush=True)
    for i in range(len(libs)):
        v = sorted(ts[i])
        print(f"{sh} lib {i}: median {v[len(v) // 2]:8.1f} us  best {v[0]:8.1f}  ({fl / v[len(v) // 2] / 1e6:6.0f} TFLOP/s)  "
              f"bitwise equal to lib 0: {same[i]}", flush=True)
for L in libs:
    L.fa_debug_set_fwd_variant(0)
