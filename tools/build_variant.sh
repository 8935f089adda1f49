#!/bin/bash
# Build libraymarch_hip.so from a git revision of the kernel source into lib/var/<name>.so, for
# same-box A/B timing (RM_LIB_PATH=burn_raymarching_amd/lib/var/<name>.so).
#   bash tools/build_variant.sh <rev|WT> <name> [extra hipcc flags]   (WT: the working tree)
# The revision's whole csrc/ and include/ are unpacked into a temporary directory and compiled
# there, so the variant sees its own revision of every header.
set -e
REV=$1; NAME=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/burn_raymarching_amd/lib/var"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
if [ "$REV" = WT ]; then  # the working tree
  mkdir -p "$tmp/burn_raymarching_amd"
  cp -r "$ROOT/burn_raymarching_amd/csrc" "$tmp/burn_raymarching_amd/csrc"
  cp -r "$ROOT/include" "$tmp/include"
else
  git -C "$ROOT" archive "$REV" burn_raymarching_amd/csrc include | tar -x -C "$tmp"
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wno-unused-result "$@" \
  -o "$ROOT/burn_raymarching_amd/lib/var/$NAME.so" "$tmp/burn_raymarching_amd/csrc/rm_kernels.hip"
echo "built lib/var/$NAME.so from $REV"
