#!/bin/bash
# tools/exp/lib_pw<tag>.so = the library with every pointwise object (csrc/pointwise*.hip) recompiled under extra -D switches, the other
# objects linked from the regular build: tools/build_pw_variant.sh tl "-DPP_TIMELINE"
R=$(cd $(dirname $0)/..; pwd); B=$R/p2p_bridge_amd/csrc/build
T=/tmp/pwvar/$1; mkdir -p $T $R/tools/exp
for s in $R/p2p_bridge_amd/csrc/pointwise*.hip; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -Wno-unused-function $2 -c $s -o $T/$(basename $s .hip).o &
done; wait
[ $(ls $T/*.o | wc -l) = $(ls $R/p2p_bridge_amd/csrc/pointwise*.hip | wc -l) ] &&
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/tools/exp/lib_pw$1.so $T/*.o $(ls $B/*.o | grep -v "/pointwise[^/]*\.o") && echo built pw$1
