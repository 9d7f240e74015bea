#!/usr/bin/env bash
# CPU build of csrc/mm_predict.h's schedule for tests/test_predict_host.py (test infrastructure; see mm_predict_host.hip).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
hipcc -O2 -std=c++17 --offload-arch=gfx950 -fPIC -shared "${here}/mm_predict_host.hip" -o "${here}/libmm_predict_host.so"
echo "built ${here}/libmm_predict_host.so"
