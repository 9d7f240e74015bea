#!/usr/bin/env bash
# The stand-alone GPU driver of the one-wave dense solvers of csrc/mm_adjoint.h for tests/test_gpu_dense_small.py (test
# infrastructure; see dense_small.hip).  A program of its own: nothing here is linked into the product library.
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
csrc="$(cd "${here}/../../gpflowpilco_amd/csrc" && pwd)"
hipcc -O2 -std=c++17 --offload-arch=gfx950 -I "${csrc}" "${here}/dense_small.hip" -o "${here}/dense_small"
echo "built ${here}/dense_small"
