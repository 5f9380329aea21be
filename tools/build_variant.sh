#!/bin/bash
# A/B builds for the lab: tools/build_variant.sh <out.so> [extra hipcc flags...]  — compiles every csrc/*.hip with the extra flags
# (e.g. -DGDR_ATTN_NO_XCD_REMAP) into a scratch directory and links <out.so>; run a tool with GDR_HIP_LIB=<out.so> to use it.
# GDR_CSRC=<dir> takes the sources from another tree (a checkout of the parent commit: `git worktree add`, `git archive | tar -x`).
set -e
out=$1; shift
here=$(cd "$(dirname "$0")/.." && pwd)
src=${GDR_CSRC:-$here/gdr_amd/csrc}
tmp=$(mktemp -d)
pids=()
for f in "$src"/*.hip; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -fno-gpu-rdc "$@" \
      -I"$src" -c "$f" -o "$tmp/$(basename "$f" .hip).o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$out" "$tmp"/*.o
rm -rf "$tmp"
echo "built $out"
