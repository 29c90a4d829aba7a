#!/bin/bash
# Build the current sources into build/live/$1/libfognet_hip.so (A/B timing with
# FOGNET_LIB=... python tools/stage_timing.py); the product library is untouched.
# SRC=<dir>: another tree's csrc (a parent commit's export) instead of this one's.
set -e
cd "$(dirname "$0")/.."
d=build/live/$1; mkdir -p $d
S=${SRC:-fognetsimpp_amd/csrc}
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result $EXTRA -Iinclude -I$S -shared -o $d/libfognet_hip.so \
  $S/capi.hip $S/replay.hip $S/replay_wide.hip $S/replay_v2.hip $S/replay_region.hip $S/decide.hip $S/tracegen.hip $S/user_stats.hip $S/node_stats.hip $S/per_user_stats.hip $S/signal_vectors.hip $S/replay_assigned.hip $S/window_stats.hip $S/quantiles.hip $S/io.cpp
echo built $d
