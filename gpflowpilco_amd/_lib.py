"""ctypes binding of ``libgpflowpilco_mm.so`` (include/gpflowpilco_mm.h).

There is NO CPU fallback: if the HIP library is missing the import of any op
raises, loudly.  Build it with ``gpflowpilco_amd/csrc/build.sh`` (or
``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPFLOWPILCO_MM_LIB: an alternative build of the same library (A/B experiments of kernel variants: csrc/build.sh
# with OUT=... and extra -D flags); the default is the in-tree build
LIB_PATH = os.environ.get("GPFLOWPILCO_MM_LIB") or os.path.join(_HERE, "libgpflowpilco_mm.so")

MM_F32, MM_F64 = 0, 1
MM_DMAX = 32
MM_M_ALIGN = 128
MM_FULL_OUTPUT_COV = 1
MM_MODEL_UNCERTAINTY = 2
MM_FORCE_GENERIC = 4
MM_STAGE_DIAG = 8
MM_STAGE_OFFDIAG = 16
MM_STAGE_FINALIZE = 32
MM_FORCE_WORST_TIER = 64
MM_WORKSPACE_CURRENT = 128
MM_FORCE_ROUTE = 256
MM_NO_ROUTE = 512
MM_SUMS_CURRENT = 1024
# internal A/B bits of the f32 off-diagonal sweep's bound-based tile skipping (csrc/mm_common.h; results are bit-identical):
# the Euclidean bound at every site / no bound-based skipping at all
MM_ISTAGE_OLD_SKIP_BOUND = 1 << 26
MM_ISTAGE_NO_BOUND_SKIP = 1 << 27
# internal A/B bit of the forward's f64 weight moments (csrc/mm_common.h; results are bit-identical): the 64 x 128 GEMM tiling and
# the one-workgroup-per-item contraction
MM_ISTAGE_OLD_WMOM = 1 << 28
# internal A/B bit of the degree-4..6 contraction (csrc/mm_common.h; results are bit-identical): every load where its value is used
MM_ISTAGE_OLD_SPOLY_LOADS = 1 << 29

ERRORS = {
    -1: "MM_E_ARG: NULL pointer or non-positive size",
    -2: "MM_E_DIM: input dimension d exceeds MM_DMAX=32 or unsupported shape",
    -3: "MM_E_DTYPE: dtype must be MM_F32 or MM_F64",
    -4: "MM_E_WORKSPACE: workspace/packed buffer too small",
    -5: "MM_E_NO_C: model_uncertainty requested but the model was packed without C",
    -6: "MM_E_STATE: Euler update / closed rollout needs d == L and a full output covariance",
}

# name -> (restype, argtypes); exactly the symbols include/gpflowpilco_mm.h declares
SIGNATURES = {
    "mm_abi_version": (C.c_int, []),
    "mm_packed_model_bytes": (C.c_size_t, [C.c_int] * 5),
    "mm_pack_model": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int]
                      + [C.c_void_p] * 6 + [C.c_void_p]),
    "mm_pack_perm": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mm_workspace_bytes": (C.c_size_t, [C.c_int] * 6),
    "mm_moment_match": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                  C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mm_q_forward": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mm_Q_reduce_forward": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_double, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "mm_euler_update": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 8),
    "mm_expected_cost": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "mm_offdiag_stats": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mm_offdiag_worklist_len": (C.c_int, [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mm_offdiag_skip_bounds": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mm_route_estimates": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mm_compose_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "mm_compose_nd_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "mm_compose_tape_bytes": (C.c_size_t, [C.c_int] * 6),
    "mm_compose_backward_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "mm_policy_grad_bytes": (C.c_size_t, [C.c_int] * 3),
    "mm_compose_tape_bytes_nd": (C.c_size_t, [C.c_int] * 7),
    "mm_compose_backward_workspace_bytes_nd": (C.c_size_t, [C.c_int] * 6),
    "mm_policy_grad_bytes_nd": (C.c_size_t, [C.c_int] * 4),
    "mm_compose_nd_mixed_workspace_bytes": (C.c_size_t, [C.c_int] * 6),
    "mm_compose_tape_bytes_nd_mixed": (C.c_size_t, [C.c_int] * 8),
    "mm_compose_backward_workspace_bytes_nd_mixed": (C.c_size_t, [C.c_int] * 7),
    "mm_bwd_f32_supported": (C.c_int, [C.c_int]),
    "mm_backward_pair_aggregates_bytes": (C.c_size_t, [C.c_int] * 5),
    "mm_backward_pair_aggregates": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mm_moment_match_backward_bytes": (C.c_size_t, [C.c_int] * 5),
    "mm_moment_match_backward_bytes_dtype": (C.c_size_t, [C.c_int] * 6),
    "mm_moment_match_backward": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p]),
    "mm_moment_match_with_sums": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                            C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_void_p]),
    "mm_backward_bytes": (C.c_size_t, [C.c_int] * 5),
    "mm_backward_sums": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mm_pathwise_eval": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 12),
    "mm_pathwise_rollout": (C.c_int, [C.c_int] * 7 + [C.c_double] + [C.c_void_p] * 13),
    "mm_pathwise_eval_jac": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 13),
    "mm_pathwise_eval_bound": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 13),
    "mm_pathwise_tape_bytes": (C.c_size_t, [C.c_int] * 6),
    "mm_pathwise_policy_rollout": (C.c_int, [C.c_int] * 5 + [C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 10
                                   + [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double]
                                   + [C.c_void_p] * 4 + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "mm_pathwise_backward_scratch_bytes": (C.c_size_t, [C.c_int] * 3),
    "mm_pathwise_policy_rollout_backward": (C.c_int, [C.c_int] * 3 + [C.c_double, C.c_int, C.c_int, C.c_void_p]
                                            + [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double]
                                            + [C.c_void_p] * 2 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
                                            + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mm_pathwise_policy_rollout_backward_seeded": (C.c_int, [C.c_int] * 3 + [C.c_double, C.c_int, C.c_int, C.c_void_p]
                                                   + [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double]
                                                   + [C.c_void_p] * 2 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4
                                                   + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mm_pathwise_tape_bytes_nd": (C.c_size_t, [C.c_int] * 7),
    "mm_pathwise_policy_rollout_nd": (C.c_int, [C.c_int] * 5 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                      + [C.c_void_p] * 9
                                      + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                      + [C.c_void_p] * 4 + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "mm_pathwise_backward_scratch_bytes_nd": (C.c_size_t, [C.c_int] * 4),
    "mm_pathwise_policy_rollout_backward_nd": (C.c_int, [C.c_int] * 3 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                               + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                               + [C.c_void_p] * 2 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
                                               + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mm_pathwise_policy_rollout_backward_nd_seeded": (C.c_int, [C.c_int] * 3 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                                      + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                                      + [C.c_void_p] * 2 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4
                                                      + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mm_pathwise_policy_rollout_wide": (C.c_int, [C.c_int] * 5 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                        + [C.c_void_p] * 9
                                        + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                        + [C.c_void_p] * 4 + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "mm_pathwise_backward_scratch_bytes_wide": (C.c_size_t, [C.c_int] * 4),
    "mm_pathwise_policy_rollout_backward_wide": (C.c_int, [C.c_int] * 3 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                                 + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                                 + [C.c_void_p] * 2 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
                                                 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mm_pathwise_policy_rollout_backward_wide_seeded": (C.c_int, [C.c_int] * 3 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                                        + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                                        + [C.c_void_p] * 2 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4
                                                        + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mm_pathwise_tape_bytes_mixed": (C.c_size_t, [C.c_int] * 8),
    "mm_pathwise_policy_rollout_mixed": (C.c_int, [C.c_int] * 5 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                         + [C.c_void_p] * 9
                                         + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                         + [C.c_void_p] * 4 + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
                                         + [C.c_int, C.c_void_p, C.c_void_p]),
    "mm_pathwise_policy_rollout_backward_mixed": (C.c_int, [C.c_int] * 3 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                                  + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                                  + [C.c_void_p] * 2 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4
                                                  + [C.c_void_p, C.c_size_t, C.c_void_p] + [C.c_int, C.c_void_p]),
    "mm_pathwise_eval_kern": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 12 + [C.c_int]),
    "mm_pathwise_rollout_kern": (C.c_int, [C.c_int] * 7 + [C.c_double] + [C.c_void_p] * 13 + [C.c_int]),
    "mm_pathwise_eval_jac_kern": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 13 + [C.c_int]),
    "mm_pathwise_eval_bound_kern": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 13 + [C.c_int]),
    "mm_pathwise_policy_rollout_kern": (C.c_int, [C.c_int] * 5 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                        + [C.c_void_p] * 9
                                        + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                        + [C.c_void_p] * 4 + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
                                        + [C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "mm_pathwise_mean_eval": (C.c_int, [C.c_int] * 5 + [C.c_void_p] * 10 + [C.c_int]),
    "mm_pathwise_policy_rollout_mean": (C.c_int, [C.c_int] * 4 + [C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
                                        + [C.c_void_p] * 6
                                        + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
                                        + [C.c_void_p] * 4 + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
                                        + [C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "mm_pathwise_basis": (C.c_int, [C.c_int] * 5 + [C.c_void_p] * 9),
    "mm_pathwise_pack_stream": (C.c_int, [C.c_int] * 5 + [C.c_void_p] * 4),
    "mm_gram_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "mm_gram_se": (C.c_int, [C.c_int] * 4 + [C.c_void_p] * 6),
    "mm_gram_se_backward": (C.c_int, [C.c_int] * 4 + [C.c_void_p] * 9 + [C.c_size_t, C.c_void_p]),
    "mm_predict_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "mm_predict_se": (C.c_int, [C.c_int] * 4 + [C.c_void_p] * 10 + [C.c_size_t, C.c_void_p]),
    "mm_gram_stats_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "mm_gram_stats_se": (C.c_int, [C.c_int] * 5 + [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p]),
    "mm_gram_stats_se_backward": (C.c_int, [C.c_int] * 5 + [C.c_void_p] * 11 + [C.c_size_t, C.c_void_p]),
    "mm_rollout_closed": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_double, C.c_int, C.c_double,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}


def _composed_rollout_signatures():
  """The eleven ``mm_rollout_composed*`` entries, from the pieces their argument lists share: prefix, head constants, target and
  precision, the role's own arguments, and -- the ``_nd_mixed`` entries -- the mixing."""
  P, Z, I, D = C.c_void_p, C.c_size_t, C.c_int, C.c_double
  prefix = [P, Z, I, I, I,  P, Z, I, I,  I, I, I, D, I, I, C.POINTER(C.c_int32)]   # drift pack; policy pack; dtype B H dt nx na active
  heads = {"": [D, D], "_nd": [I, C.POINTER(D), C.POINTER(D)]}                     # scale, shift | nu, scale[nu], shift[nu]
  buffers = lambda n: [P, Z] * n + [P, P]                                          # n (pointer, bytes) pairs; status, stream
  roles = {"": [P] * 5 + buffers(3),                          # mx Sxx cost traj_mu traj_S; drift / policy / compose workspaces
           "_taped": [P] * 3 + buffers(3),                    # mx Sxx cost; drift / policy workspaces, tape
           "_backward": [P, Z, P] + [P] * 3 + buffers(2),     # tape, g_cost; g_policy g_mx g_Sxx; drift / sweep workspaces
           "_backward_seeded": [P, Z, P, P, P] + [P] * 3 + buffers(2)}                 # ... g_cost, g_xm, g_xS; ...
  sigs = {}
  for role, args in roles.items():
    stem, seeded, _ = role.partition("_seeded")
    for nd, head in heads.items():
      sigs[f"mm_rollout_composed{stem}{nd}{seeded}"] = (I, prefix + head + [P, P] + args)
  for role, mixing in (("", [P, P]), ("_taped", [P, P]), ("_backward", [P])):        # mix_W, mix_c | mix_W: the one sweep is seeded
    args = roles["_backward_seeded" if role == "_backward" else role]
    sigs[f"mm_rollout_composed{role}_nd_mixed"] = (I, prefix + heads["_nd"] + [P, P] + args + mixing)
  return sigs


SIGNATURES.update(_composed_rollout_signatures())


def _compose_wide_signatures():
  """The reverse sweep for 8 < ne <= 16 (``mm_compose_wide_backward*``): the argument lists of the ``_nd`` sweeps of the same role,
  the mixed ones with mix_W appended; their two size queries; and the switch between their dense paths."""
  nd, seeded = (SIGNATURES[f"mm_rollout_composed_backward_nd{s}"][1] for s in ("", "_seeded"))
  return {"mm_compose_wide_backward": (C.c_int, list(nd)),
          "mm_compose_wide_backward_seeded": (C.c_int, list(seeded)),
          "mm_compose_wide_backward_mixed": (C.c_int, list(nd) + [C.c_void_p]),
          "mm_compose_wide_backward_mixed_seeded": (C.c_int, list(seeded) + [C.c_void_p]),
          "mm_compose_backward_workspace_bytes_wide": (C.c_size_t, [C.c_int] * 6),
          "mm_compose_backward_workspace_bytes_wide_mixed": (C.c_size_t, [C.c_int] * 7),
          "mm_compose_wide_dense_path": (C.c_int, [C.c_int])}


SIGNATURES.update(_compose_wide_signatures())

_lib = None


class MomentMatchingLibraryError(RuntimeError):
  pass


def lib():
  """Load the shared library once; raise if it is not built."""
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise MomentMatchingLibraryError(
          f"{LIB_PATH} is missing: the HIP extension is not built and there is no CPU "
          "fallback. Run gpflowpilco_amd/csrc/build.sh (needs hipcc).")
    handle = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
      fn = getattr(handle, name)
      fn.restype = res
      fn.argtypes = args
    _lib = handle
  return _lib


def check(rc: int, what: str):
  if rc == 0:
    return
  if rc < 0:
    raise ValueError(f"{what}: {ERRORS.get(rc, rc)}")
  raise MomentMatchingLibraryError(f"{what}: HIP error {rc}")
