#!/bin/bash
# Build a variant of the library beside the product build: tools/build_variant.sh <name> ["extra hipcc flags"] [source dir]
#   -> build_ab/libscasr_<name>.so  (objects in /tmp/scasr_build_<name>; the product's objects are not touched)
# Sources, compiler and flags are read from the source dir's Makefile (SRCS, HIPCC, CXXFLAGS with EXTRA = the given flags),
# so a variant is the product build plus those flags.
# e.g. tools/build_variant.sh phase "-DSC_PHASE_DBG -DSC_PHASE_MIN_GRID=200";  a worktree of another commit as source dir
set -e
NAME=$1; EXTRA=$2; ROOT=$(cd "$(dirname "$0")/.." && pwd); SRC=${3:-$ROOT/speechcatcher_amd/csrc}
OBJ=/tmp/scasr_build_$NAME; mkdir -p $OBJ $ROOT/build_ab
mkvar() { make -s --no-print-directory -C "$SRC" EXTRA="$EXTRA" --eval="print-$1: ; @echo \$($1)" print-$1; }
SRCS=$(mkvar SRCS); HIPCC=$(mkvar HIPCC); FLAGS=$(mkvar CXXFLAGS); ARCH=$(mkvar ARCH)
pids=(); objs=()
for f in $SRCS; do
  o=$OBJ/${f%.hip}.o; objs+=($o)
  $HIPCC $FLAGS -c $SRC/$f -o $o & pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=$ARCH -shared -fPIC "${objs[@]}" -o $ROOT/build_ab/libscasr_$NAME.so
echo "built build_ab/libscasr_$NAME.so"
