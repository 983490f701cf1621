#!/bin/bash
# Build libsrlhip_<tag>.so of the current tree next to the product library with extra compiler flags on the GEMM / convolution
# sources (compile-time variants such as -DSRL_OBS_LINE_STORES=0), reusing every other object of the normal build.
#   scripts/build_variant.sh nolines -DSRL_OBS_LINE_STORES=0 ;  SRL_HIP_LIB=$PWD/srl_amd/csrc/libsrlhip_nolines.so python3 scripts/obs_fwd_bench.py
set -e
tag=$1; shift
cd "$(dirname "$0")/.."
make -j8 >/dev/null
d=srl_amd/csrc/build_$tag
mkdir -p $d
for f in gemm conv; do
  hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC "$@" -c -o $d/$f.o srl_amd/csrc/$f.hip &
done
wait
objs=$(ls srl_amd/csrc/build/*.o | grep -v -e /gemm.o -e /conv.o)
hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -shared -o srl_amd/csrc/libsrlhip_$tag.so $objs $d/gemm.o $d/conv.o
echo srl_amd/csrc/libsrlhip_$tag.so
