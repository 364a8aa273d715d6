#!/bin/bash
# Build libghs_mst.so from the working tree with extra compile flags into
# distributed_ghs_implementation_amd/lib/exp/<name>.so (same-box A/B: tools/gpu/ab.sh with
# GHS_MST_LIB=...). The csrc Makefile does the build (its object list, its link line) into a
# temporary OUTDIR; the shipped lib/ is untouched.
# Usage: tools/build_variant.sh NAME "EXTRA_FLAGS"   e.g. tools/build_variant.sh o2 "-O2"
#        (-DGHS_AB_ENV=1 gives the `make AB=1` build)
set -e
NAME=$1; EXTRA=$2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
make -C "$ROOT/distributed_ghs_implementation_amd/csrc" OUTDIR="$T" \
  HIPFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-result $EXTRA"
mkdir -p "$ROOT/distributed_ghs_implementation_amd/lib/exp"
mv "$T/libghs_mst.so" "$ROOT/distributed_ghs_implementation_amd/lib/exp/$NAME.so"
echo "built $NAME.so with $EXTRA"
