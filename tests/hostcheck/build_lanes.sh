#!/usr/bin/env bash
# CPU builds of the lane-count check of csrc/mm_adjoint.h, mm_adjoint_nd.h and mm_mix.h for tests/test_adjoint_lanes.py (test
# infrastructure; see adjoint_lanes.hip): one stand-alone program, three times -- plain, address + undefined-behaviour sanitizers,
# thread sanitizer.  Executables only: no shared object is built with a sanitizer and nothing is preloaded.
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
common=(-O1 -g -std=c++17 --offload-arch=gfx950 -pthread "${here}/adjoint_lanes.hip")
hipcc "${common[@]}" -o "${here}/adjoint_lanes" &
p0=$!
hipcc "${common[@]}" -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -o "${here}/adjoint_lanes_asan" &
p1=$!
hipcc "${common[@]}" -Xarch_host -fsanitize=thread -o "${here}/adjoint_lanes_tsan" &
p2=$!
wait "${p0}"; wait "${p1}"; wait "${p2}"      # a failed compile fails the build (set -e)
echo "built ${here}/adjoint_lanes ${here}/adjoint_lanes_asan ${here}/adjoint_lanes_tsan"
