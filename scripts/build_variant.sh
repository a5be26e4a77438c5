#!/bin/bash
# Builds escalator_amd/libescalator_hip_<NAME>.so: the library with esc_kernels.hip part 0
# compiled with extra flags (e.g. -DK1_PK_DS=8), for A/B timing through ESC_LIB_PATH.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../escalator_amd/csrc"
B=../../build/var_$NAME
mkdir -p $B
HIPCC=/opt/rocm/bin/hipcc
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result -I../../include -I."
$HIPCC $FL "$@" -DESC_PART=0 -c esc_kernels.hip -o $B/esc_kernels.o
O=../../build/csrc
# the host runtime's files (the Makefile's SRCS_RT)
RT_SRCS="esc_runtime esc_rebuild esc_pod_grow esc_pod_compact esc_pod_audit esc_pod_verify esc_node_verify"
RT_DIR=$O
if [ -n "$REBUILD_RT" ]; then            # flags that change the runtime's view too (e.g. -DESC_ORD_CHUNK)
    for f in $RT_SRCS; do $HIPCC $FL "$@" -c $f.hip -o $B/$f.o; done
    RT_DIR=$B
fi
RT=""
for f in $RT_SRCS; do RT="$RT $RT_DIR/$f.o"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libescalator_hip_$NAME.so $B/esc_kernels.o $RT \
    $O/esc_multi.o $O/esc_list.o $O/esc_pack.o $O/esc_synth.o -pthread
