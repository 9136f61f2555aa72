#!/bin/bash
# Build an A/B variant of libavexhip.so and (optionally) run a command against it -- the one parametrised form of the per-experiment
# scripts earlier rounds kept under scripts/debug/ (ab_r04g.sh ... ab_r04x.sh each named variant libraries nothing in the tree built).
#
#   scripts/ab_variant.sh <suffix> "<extra cflags>" [-- command ...]
#
#   scripts/ab_variant.sh noepi "-DGEMM_NOEPI=1"                      # builds avex_amd/lib/libavexhip_noepi.so (objects in avex_amd/_build_noepi/)
#   scripts/ab_variant.sh noepi "-DGEMM_NOEPI=1" -- python scripts/gemm_ab.py --a avex_amd/lib/libavexhip_noepi.so --b avex_amd/lib/libavexhip.so --shapes qkv,fc1 --step
#   scripts/ab_variant.sh diag "-DATT_STAMPS=1" -- env AVEX_AMD_LIB=$PWD/avex_amd/lib/libavexhip_diag.so python scripts/attn_stamps.py
#
# The instrument switches the kernels read at compile time (all off in the product library; the rejected alternatives of rounds 1-6
# are in git history):
#   gemm.hip       GEMM_NOEPI=1  GEMM_NOSTORE=1
#   attention.hip  ATT_STAMPS=1 (with AVEX_AMD_DIAG=1)
#   attention16.hip knock-outs / stamps (A3_KO, A3_STAMPS): scripts/micro/att16_bench.hip, no library needed
#   melspec.hip    STFT_KNOCK=bits
# Run on the GPU box through gpurun: build here (hipcc cross-compiles), the .so travels with the snapshot.
set -e
[ $# -ge 2 ] || { sed -n 2,20p "$0"; exit 2; }
suffix=$1; cflags=$2; shift 2
cd "$(dirname "$0")/.."
AVEX_AMD_LIB_SUFFIX=$suffix AVEX_AMD_EXTRA_CFLAGS="$cflags" python -m avex_amd.build
echo "[ab_variant] avex_amd/lib/libavexhip_${suffix}.so  (select with AVEX_AMD_LIB=\$PWD/avex_amd/lib/libavexhip_${suffix}.so)"
if [ "$1" = "--" ]; then shift; exec "$@"; fi
