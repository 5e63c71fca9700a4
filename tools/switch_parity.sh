#!/bin/bash
# The one compile-time switch that selects a second form of product code: VK_HANDLE_ALWAYS_FENCED, the memory-model-correct
# arrival of vk_volume.hip. This keeps it honest (the experiments that lost are in git history, tools/patches/README.md):
#   in the container:  tools/switch_parity.sh build          — one libvk_hip_var_sw_<name>.so per switch
#   on the GPU box:    tools/switch_parity.sh run <outdir>   — the parity tests that cover the switched code, per build
# A switch whose build no longer passes is a bug, not a variant to be quoted.
set -e
root=$(cd $(dirname $0)/.. && pwd)
# name | source | flags | tests
table="
handle_fenced|vk_volume.hip|-DVK_HANDLE_ALWAYS_FENCED=1|tests/test_gpu_parity.py tests/test_gpu_set_view_rounds.py tests/test_gpu_banded_lists.py tests/test_gpu_edge_cases.py tests/test_gpu_round5.py
"
if [ "$1" = build ]; then
  echo "$table" | while IFS='|' read name src flags tests; do
    [ -z "$name" ] && continue
    bash $root/tools/build_variant.sh sw_$name $root/vulcan_amd/csrc/$src $flags
  done
else
  out=${2:-gpurun_out/switch_parity}; mkdir -p $out
  echo "$table" | while IFS='|' read name src flags tests; do
    [ -z "$name" ] && continue
    lib=$root/vulcan_amd/lib/libvk_hip_var_sw_$name.so
    [ -f $lib ] || { echo "== $name: not built"; continue; }
    if VK_HIP_LIBRARY=$lib timeout -k 10 600 python -m pytest $tests -m gpu -x -q > $out/$name.txt 2>&1; then verdict=ok; else verdict=FAILED; fi
    echo "== $name ($src $flags): $verdict: $(tail -1 $out/$name.txt)"
  done
fi
