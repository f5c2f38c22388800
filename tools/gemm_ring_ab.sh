#!/bin/bash
# A/B of library builds on the plain int8 GEMM launches, interleaved rounds in one call: tools/gemm_ring_ab.sh tag ...
# ("default" = the shipped library; other tags are tools/_exp/libffq_<tag>.so from tools/build_variant.sh). Every step runs under its
# own time limit and the chain ends at the first step that fails.
set -o pipefail
for round in 1 2 3; do
  for tag in "$@"; do
    lib=""; [ "$tag" != default ] && lib="FFQ_LIB=tools/_exp/libffq_$tag.so"
    echo "== $tag round $round"
    env $lib timeout -k 10 240 python tools/gemm_ring_time.py 16384 2>&1 | grep -v amdgpu || exit 1
  done
done
