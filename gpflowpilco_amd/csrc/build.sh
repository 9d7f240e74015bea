#!/usr/bin/env bash
# Build the gfx950 shared library in-tree (hipcc cross-compiles without a GPU).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="${OUT:-${here}/../libgpflowpilco_mm.so}"      # OUT=path: a variant build beside the default one
obj="${OBJDIR:-${here}/.obj}"
mkdir -p "${obj}"
common=(-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wno-unused-result)
objs=()
pids=()
for src in mm_kernels mm_mfma mm_f64 mm_moments mm_moments6 mm_compose mm_compose_nd mm_compose_bwd mm_compose_bwd_nd mm_pathwise mm_pathwise_mean mm_backward mm_bwd_f32 mm_route mm_pathwise_policy mm_pathwise_sample mm_gram mm_predict mm_gram_stats; do
  extra=()
  # mm_mfma.hip and mm_bwd_f32.hip are built with -fno-honor-nans: the per-tile range check max(|x|) then folds
  # into one v_max3_f32 per two entries (no canonicalising v_max x, x); inputs are finite by the
  # time they reach those kernels (k_prep's status word rejects non-PD / non-finite states).
  [[ "${src}" == mm_mfma || "${src}" == mm_bwd_f32 ]] && extra=(-fno-honor-nans)
  # mm_pathwise.hip without the SLP vectoriser: it pairs elements of different 16-byte loads into
  # v_pk_fma_f32 operands, and the shuffles it places on the loop back edge wait for the prefetched
  # (still in flight) weight blocks -- s_waitcnt vmcnt(0) per iteration instead of vmcnt(8)
  [[ "${src}" == mm_pathwise ]] && extra=(-fno-slp-vectorize)
  hipcc "${common[@]}" "${extra[@]}" -c "${here}/${src}.hip" -o "${obj}/${src}.o" "$@" &
  pids+=($!)
  objs+=("${obj}/${src}.o")
done
for p in "${pids[@]}"; do wait "${p}"; done   # a failed compile fails the build (set -e)
hipcc --offload-arch=gfx950 -fPIC -shared "${objs[@]}" -o "${out}"
echo "built ${out}"
