#!/bin/bash
# dev tool (CPU box): a library variant with extra compiler defines for EVERY kernel file, into
# hcatgnet_amd/csrc/_variants/<name>.so (git-ignored, travels to the GPU box; load with HCG_LIB, tools/ab_lib.sh / ab_kernels.sh).
# usage: tools/build_variant_def.sh NAME "-DHCG_SPLIT_SCALAR"        (an empty define string = a copy of the product build)
#        tools/build_variant_def.sh twolaunch "-DHCG_NO_BWD_PAIR"    (the two-launch arm of the backward pair's A/B)
set -e
name=$1; defs=$2
C=$(cd "$(dirname "$0")/../hcatgnet_amd/csrc" && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
obj=$(mktemp -d)
mkdir -p $C/_variants
# the file list is the Makefile's (a variant must export every symbol of _lib.SIGNATURES)
files=$(sed -n 's/^SRCS := //p' $C/Makefile | sed 's/\.hip//g')
[ -n "$files" ] || { echo "no SRCS in $C/Makefile"; exit 1; }
n=0
for f in $files; do
  $HIPCC -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -fno-slp-vectorize $defs -c $C/$f.hip -o $obj/$f.o &
  n=$((n+1)); if [ $((n % 6)) -eq 0 ]; then wait; fi
done
wait
objs=""; for f in $files; do objs="$objs $obj/$f.o"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $C/_variants/$name.so $objs
rm -r $obj
echo built $C/_variants/$name.so
