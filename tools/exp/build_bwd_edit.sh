#!/bin/bash
# Build a copy of libfa_hip.so whose fa_bwd_fused.hip (the single pass) is edited by python
# scripts (A/B ablations); the flags also go to fa_bwd.hip, whose fused_setup reads -DFA_BWD_ABL:
#   tools/exp/build_bwd_edit.sh OUT.so "flags" edit1.py [edit2.py ...]
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
C=$R/flashattention.jl_amd/csrc
B=/tmp/bwded_$$
mkdir -p $B
out=$1; flags=$2; shift 2
cp $C/fa_bwd_fused.hip $B/fa_bwd_fused.hip
# (the copy's "../../include/fa_hip.h" has no meaning in $B; the csrc headers are found through -I)
sed -i "s#\"../../include/fa_hip.h\"#\"$R/include/fa_hip.h\"#" $B/fa_bwd_fused.hip
for e in "$@"; do python3 $e $B/fa_bwd_fused.hip; done
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -munsafe-fp-atomics $flags"
/opt/rocm/bin/hipcc $F -I$C -x hip -c $B/fa_bwd_fused.hip -o $B/fa_bwd_fused.o &
/opt/rocm/bin/hipcc $F -x hip -c $C/fa_bwd.hip -o $B/fa_bwd.o &
wait
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o $out $C/build/api.cpp.o $C/build/fa_fwd.hip.o $C/build/fa_fwd_p4.hip.o \
    $B/fa_bwd.o $B/fa_bwd_fused.o $C/build/fa_bwd_simt_dq.hip.o $C/build/fa_bwd_simt_dkdv.hip.o $C/build/fa_bwd_f32.hip.o $C/build/fa_bwd_dq.hip.o $C/build/fa_bwd_dkdv.hip.o \
    $C/build/fa_windowed_fwd.hip.o $C/build/fa_windowed_bwd.hip.o $C/build/fa_circulant.hip.o $C/build/fa_circulant_bwd.hip.o $C/build/fa_softmax.hip.o $C/build/fa_f64.hip.o
rm -rf $B
