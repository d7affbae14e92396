#!/bin/bash
# Build a VARIANT of the library next to the product one, for same-box A/B runs:
#   scripts/build_variant.sh <name> "<extra hipcc flags, e.g. -DHZ_PROBE_EXTRA_LOADS=2>"
# -> horayzon_amd/libhorayzon_hip_<name>.so (git-ignored; travels with the gpurun snapshot).  Select it at run time with
#   HORAYZON_HIP_LIB=horayzon_amd/libhorayzon_hip_<name>.so python scripts/quick_perf.py ...
set -e
name=$1; shift
flags="$*"
R=$(cd "$(dirname "$0")/.." && pwd)
obj=/tmp/hz_variant_$name
mkdir -p $obj
cd $R/horayzon_amd/csrc
srcs=$(make -s print-srcs)      # the Makefile's SRCS: one list of sources
objs=
for f in $srcs; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-result $flags -c $f -o $obj/${f%.hip}.o &
  objs="$objs $obj/${f%.hip}.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/horayzon_amd/libhorayzon_hip_$name.so $objs
echo built horayzon_amd/libhorayzon_hip_$name.so
