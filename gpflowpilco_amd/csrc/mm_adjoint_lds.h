// Dynamic-LDS sizes of the reverse-sweep kernels that run several functions of mm_adjoint.h / mm_adjoint_nd.h back to back on one
// arena (mm_compose_bwd.hip, mm_compose_bwd_nd.hip).  They sit in a header of their own so that the lane-count check of
// tests/hostcheck/adjoint_lanes.hip carves its arenas with the launchers' own arithmetic (less the trailing + 8).
#pragma once
#include "mm_adjoint_nd.h"

// k_compose_tail_bwd: gme, gSee, gSxe, gm1, gS1, then the work area shared by cost -> encode -> step
static inline size_t mm_tail_bwd_lds(int nx, int ne, int nd) {
  int wk = mma_cost_bwd_scratch(ne);
  const int e = mma_encode_bwd_scratch(nx, ne - nx), st = mma_step_bwd_scratch(nx, nd);
  if (e > wk) wk = e;
  if (st > wk) wk = st;
  return (size_t)(ne + ne * ne + nx * ne + nx + nx * nx + wk + 8) * sizeof(double);
}

// k_policy_head_bwd_small
static inline size_t mm_policy_bwd_lds(int M, int ne) {
  const int nd = ne + 1;
  return (size_t)(4 * ne + 2 * ne * ne + 4 + nd + nd * nd + mma_policy_small_bwd_scratch(M, ne, 256) + 8) * sizeof(double);
}

// k_compose_tail_bwd_nd
static inline size_t mm_tail_bwd_nd_lds(int nx, int ne, int nd) {
  int wk = mma_cost_bwd_scratch(ne);
  const int e = mma_encode_bwd_scratch(nx, ne - nx), st = mma_step_bwd_scratch(nx, nd);
  if (e > wk) wk = e;
  if (st > wk) wk = st;
  return (size_t)(ne + ne * ne + nx * ne + nx + nx * nx + wk + 8) * sizeof(double);
}

// k_policy_head_bwd_nd
static inline size_t mm_policy_bwd_nd_lds(int M, int ne, int nu) {
  const int nd = ne + nu;
  return (size_t)(2 * ne + 2 * ne * ne + ne * nu + 3 * nu + nu * nu + mma_head_bwd_nd_scratch(ne, nu) + nd + nd * nd
                  + mma_policy_nd_bwd_scratch(M, ne, 256) + 8) * sizeof(double);
}

// the _wide entries' LDS: mm_policy_bwd_nd_lds, but with one action -- no pair item runs -- without the pair item's scratch
static inline size_t mm_policy_bwd_wide_lds(int M, int ne, int nu) {
  if (nu > 1) return mm_policy_bwd_nd_lds(M, ne, nu);
  const int nd = ne + nu;
  return (size_t)(2 * ne + 2 * ne * ne + ne * nu + 3 * nu + nu * nu + mma_head_bwd_nd_scratch(ne, nu) + nd + nd * nd
                  + mma_policy_small_bwd_scratch(M, ne, 256) + ne * ne + 2 * ne + 8) * sizeof(double);
}
