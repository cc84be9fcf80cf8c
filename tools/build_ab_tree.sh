#!/bin/bash
# A clean, built checkout of a revision under abtree/NAME: tree A of tools/gpu_ab_tree.sh
# (whole-tree A/B: needed when the C ABI or the packed layouts differ, so a swapped library will not do).
# usage: tools/build_ab_tree.sh NAME [REV]   (REV defaults to HEAD; abtree/ is git-ignored)
set -e -o pipefail
NAME=$1; REV=${2:-HEAD}
R=$(cd "$(dirname "$0")/.." && pwd)
A=$R/abtree/$NAME
[ -e "$A" ] && { echo "$A exists"; exit 1; }
mkdir -p "$A"
git -C "$R" archive "$REV" | tar -x -C "$A"
make -C "$A/fast-cwdm_amd/csrc" -j"${MAX_JOBS:-8}"
echo "built $A at $(git -C "$R" rev-parse --short "$REV")"
