#!/bin/bash
# tools/exp/lib_<tag>.so = the library with every voxel-convolution object (csrc/conv3d*.hip) recompiled under extra -D switches
# (timing ablations / variants), the other objects linked from the regular build;
# usage: tools/build_conv_variants.sh tag1:"-DX=1 -DY" tag2:"-DZ" ...   (built in parallel; run via P2PB_LIB_PATH)
R=$(cd $(dirname $0)/..; pwd)
B=$R/p2p_bridge_amd/csrc/build
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -Wno-unused-function"
mkdir -p $R/tools/exp
for spec in "$@"; do
  tag=${spec%%:*}; defs=${spec#*:}
  T=/tmp/convvar/$tag; mkdir -p $T
  ( for s in $R/p2p_bridge_amd/csrc/conv3d*.hip; do
      /opt/rocm/bin/hipcc $FLAGS $defs -c $s -o $T/$(basename $s .hip).o 2> $T/$(basename $s .hip).err &
    done; wait
    [ $(ls $T/*.o | wc -l) = $(ls $R/p2p_bridge_amd/csrc/conv3d*.hip | wc -l) ] &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/tools/exp/lib_$tag.so $T/*.o $(ls $B/*.o | grep -v "/conv3d[^/]*\.o") &&
    echo "built $tag" || { echo "FAILED $tag"; tail -5 $T/*.err; } ) &
done
wait
