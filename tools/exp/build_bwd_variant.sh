#!/bin/bash
# Build a copy of libfa_hip.so with extra flags on the dense backward's files (A/B builds):
#   tools/exp/build_bwd_variant.sh OUT.so "-mllvm ... -DFOO=1"
set -e
[ -n "$1" ] || { echo "usage: $0 OUT.so \"flags\"" >&2; exit 2; }
R=$(cd "$(dirname "$0")/../.." && pwd)
C=$R/flashattention.jl_amd/csrc
B=/tmp/bwdvar_$$
mkdir -p $B
objs=
for f in fa_bwd fa_bwd_simt_dq fa_bwd_simt_dkdv fa_bwd_f32 fa_bwd_dq fa_bwd_dkdv fa_bwd_fused; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -munsafe-fp-atomics $2 -x hip -c $C/$f.hip -o $B/$f.o &
    objs="$objs $B/$f.o"
done
wait
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o $1 $C/build/api.cpp.o $C/build/fa_fwd.hip.o $C/build/fa_fwd_p4.hip.o \
    $objs $C/build/fa_windowed_fwd.hip.o $C/build/fa_windowed_bwd.hip.o $C/build/fa_circulant.hip.o $C/build/fa_circulant_bwd.hip.o $C/build/fa_softmax.hip.o $C/build/fa_f64.hip.o
rm -rf $B
