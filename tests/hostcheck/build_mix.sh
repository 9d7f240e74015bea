#!/usr/bin/env bash
# CPU build of csrc/mm_mix.h for tests/test_coregionalized.py (test infrastructure; see mm_mix_host.hip).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
hipcc -O2 -std=c++17 --offload-arch=gfx950 -fPIC -shared "${here}/mm_mix_host.hip" -o "${here}/libmm_mix_host.so"
echo "built ${here}/libmm_mix_host.so"
