#!/bin/bash
# builds libsuma_hip from a git revision (default HEAD) with that revision's own Makefile, for A/B runs against the
# working tree:
#   tools/build_rev.sh <out.bin> [rev] [extra hipcc flags ...]
OUT=$(readlink -f "$1"); REV=${2:-HEAD}; shift; shift
D=$(mktemp -d)
git archive "$REV" semantic_suma_amd/csrc include | tar -x -C "$D" || exit 1
make -C "$D/semantic_suma_amd/csrc" -j16 HIPCC="hipcc $*" ../libsuma_hip.so >/dev/null &&
  cp "$D/semantic_suma_amd/libsuma_hip.so" "$OUT" && echo "built $OUT from $REV"
rc=$?
rm -rf "$D"
exit $rc
