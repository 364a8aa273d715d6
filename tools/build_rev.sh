#!/bin/bash
# Build libghs_mst.so from a git revision into distributed_ghs_implementation_amd/lib/exp/<name>.so
# (same-box A/B runs: tools/gpu/ab.sh with GHS_MST_LIB=...). The revision's own csrc Makefile does
# the build, so its object list is the revision's; a revision from before csrc/Makefile existed
# cannot be built this way. Usage: tools/build_rev.sh REV NAME
set -e -o pipefail
REV=${1:-HEAD}; NAME=${2:-base}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
git -C "$ROOT" archive "$REV" distributed_ghs_implementation_amd/csrc include | tar -x -C "$T"
make -C "$T/distributed_ghs_implementation_amd/csrc" OUTDIR="$T/out"
mkdir -p "$ROOT/distributed_ghs_implementation_amd/lib/exp"
mv "$T/out/libghs_mst.so" "$ROOT/distributed_ghs_implementation_amd/lib/exp/$NAME.so"
echo "built $NAME.so from $REV"
