#!/usr/bin/env bash
# CPU build of csrc/mm_gram_stats.h for tests/test_gram_stats_host.py (test infrastructure; see mm_gram_stats_host.hip).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
hipcc -O2 -std=c++17 --offload-arch=gfx950 -fPIC -shared "${here}/mm_gram_stats_host.hip" -o "${here}/libmm_gram_stats_host.so"
echo "built ${here}/libmm_gram_stats_host.so"
