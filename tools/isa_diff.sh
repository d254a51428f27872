#!/usr/bin/env bash
# gfx950 device assembly of every libbnn source, revision REV against the working tree:
#   tools/isa_diff.sh HEAD~1
# Prints the files whose assembly differs and exits 1 if any does ("bit-identical, registers unchanged"
# as one command).  Both trees are compiled from the same relative paths with the Makefile's CXXFLAGS, so
# file directives cannot differ; the assembly is only diffed, never inspected.  JOBS=<n> (16 at most).
set -euo pipefail
REV=${1:?usage: tools/isa_diff.sh REV}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SUB=distributed-mnist-bnns_amd/csrc
JOBS=${JOBS:-16}
[ "$JOBS" -le 16 ] || JOBS=16
mkvar() { sed -n "s/^$1 *[:?]*= *//p" "$ROOT/$SUB/Makefile"; }
export HIPCC=${HIPCC:-/opt/rocm/bin/hipcc} FLAGS=$(mkvar CXXFLAGS)
SRCS=$(mkvar SRCS)
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$TMP/rev" "$TMP/work/$SUB" "$TMP/work/include"
git -C "$ROOT" archive "$REV" -- "$SUB" include | tar -x -C "$TMP/rev"
cp "$ROOT/$SUB"/*.hip "$ROOT/$SUB"/*.h "$TMP/work/$SUB/"
cp "$ROOT"/include/*.h "$TMP/work/include/"
# (no --save-temps: bnn_pack.hip does not survive its preprocessed intermediate)
for side in rev work; do
  for f in $SRCS; do echo "$TMP/$side/$SUB $f"; done
done | xargs -P "$JOBS" -L 1 sh -c \
  'cd "$0" && exec "$HIPCC" --offload-arch=gfx950 $FLAGS -w -I ../../include --offload-device-only -S "$1" -o "${1%.hip}.s"'
rc=0
for f in $SRCS; do
  if ! cmp -s "$TMP/rev/$SUB/${f%.hip}.s" "$TMP/work/$SUB/${f%.hip}.s"; then
    echo "differs: $f"
    rc=1
  fi
done
[ $rc -ne 0 ] || echo "isa_diff: the device assembly of all $(echo $SRCS | wc -w) files is identical to $REV"
exit $rc
