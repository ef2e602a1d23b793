#!/bin/bash
# Recompiles the device code with -Rpass-analysis=kernel-resource-usage and fails if a kernel of csrc/lsgpu_snf.hip.h
# (SurfaceNormalDataPointsFilter, with and without the densities of keepDensities 1) uses scratch: its lists and box_normal's work arrays are meant to live in registers and
# LDS ("Surface normals of every point"), which rests on compiler heuristics nothing else guards.
#   devtools/check_snf_resources.sh            prints VGPRs / scratch / LDS of every k_snf_* kernel
set -euo pipefail
HERE=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
"$HIPCC" --offload-arch=${ARCH:-gfx950} -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -c \
  -Rpass-analysis=kernel-resource-usage -o "$OUT/dev.o" "$HERE/laser_slam_amd/csrc/lsgpu_icp.hip" 2> "$OUT/remarks.txt"
awk '/Function Name:/ { name = $0; sub(/.*Function Name: /, "", name); sub(/ \[.*/, "", name); snf = name ~ /k_snf_/ }
     snf && / VGPRs:/ { v = $0; sub(/.* VGPRs: /, "", v); sub(/ .*/, "", v) }
     snf && /ScratchSize/ { s = $0; sub(/.*: /, "", s); sub(/ .*/, "", s) }
     snf && /LDS Size/ { l = $0; sub(/.*: /, "", l); sub(/ .*/, "", l); print name, "VGPRs", v, "scratch", s, "LDS", l; n++; if (s != 0) bad++ }
     END { if (n != 17) { print "expected 17 k_snf_* kernels (tile and fallback for 4 list lengths, each with and without densities, and k_snf_unpermute), saw " n; exit 1 } if (bad) { print bad " kernel(s) use scratch"; exit 1 } print "ok: no scratch in " n " kernels" }' "$OUT/remarks.txt"
