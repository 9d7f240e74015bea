#!/usr/bin/env bash
# Host build of the workspace layout of csrc/mm_common.h for tests/test_gpu_spoly_loads.py (test infrastructure; see
# mm_ws_layout_host.cpp).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
hipcc -O2 -std=c++17 -fPIC -shared "${here}/mm_ws_layout_host.cpp" -o "${here}/libmm_ws_layout_host.so"
echo "built ${here}/libmm_ws_layout_host.so"
