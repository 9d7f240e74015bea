// Output mixing of a coregionalised drift, f = W g + c (gpflow's LinearCoregionalization; gpflow_pilco/moment_matching/
// models.py:279-289), on the moments of one GP moment match, and its adjoint -- the step the composed rollouts of
// mm_compose_nd.hip / mm_compose_bwd_nd.hip insert between the drift's match with Lg latents and everything that reads a drift
// with nx outputs:
//   mma_mix_fwd   (g1 [Lg], Sgg [Lg][Lg], cross_g [nd][Lg]) -> f1 = W g1 + c [nx], Sff = W Sgg W^T [nx][nx] (i <= j computed,
//                 mirrored: exactly symmetric), cross = cross_g W^T [nd][nx] (pre-inverted cross terms mix like the mean)
//   mma_mix_bwd   (g f1, g Sff, g cross) -> g g1 = W^T g f1, g Sgg = W^T (g Sff) W, g cross_g = (g cross) W
// W [nx][Lg] row-major, c [nx] or null.  The map is linear: the adjoint needs nothing from the forward.  Arithmetic in f64
// whatever the moments' type T (rounded on store).  Inputs and outputs must not overlap.  Written for an execution context
// `Ctx` exactly as mm_adjoint.h (tests/hostcheck/mm_mix_host.hip is the CPU build that tests/test_coregionalized.py checks
// against torch).
#pragma once
#include "mm_adjoint.h"

// scratch of either map: nx * Lg doubles
__host__ __device__ inline int mma_mix_scratch(int nx, int Lg) { return nx * Lg; }

template <class Ctx, typename T>
__host__ __device__ inline void mma_mix_fwd(Ctx c, int nx, int Lg, int nd, const double* W, const double* mc, const T* g1,
                                            const T* Sgg, const T* cg, T* f1, T* Sff, T* cross, double* sm) {
  const int lane = c.lane(), nl = c.nl();
  double* WS = sm;                                          // W Sgg [nx][Lg]
  for (int idx = lane; idx < nx * Lg; idx += nl) {
    const int i = idx / Lg, l = idx - i * Lg;
    double s = 0.0;
    for (int k = 0; k < Lg; ++k) s = fma(W[i * Lg + k], (double)Sgg[k * Lg + l], s);
    WS[idx] = s;
  }
  for (int i = lane; i < nx; i += nl) {
    double s = mc ? mc[i] : 0.0;
    for (int k = 0; k < Lg; ++k) s = fma(W[i * Lg + k], (double)g1[k], s);
    f1[i] = (T)s;
  }
  for (int idx = lane; idx < nd * nx; idx += nl) {
    const int k = idx / nx, i = idx - k * nx;
    double s = 0.0;
    for (int l = 0; l < Lg; ++l) s = fma((double)cg[k * Lg + l], W[i * Lg + l], s);
    cross[idx] = (T)s;
  }
  c.sync();
  for (int idx = lane; idx < nx * nx; idx += nl) {
    const int i = idx / nx, j = idx - i * nx;
    if (i > j) continue;
    double s = 0.0;
    for (int l = 0; l < Lg; ++l) s = fma(WS[i * Lg + l], W[j * Lg + l], s);
    Sff[i * nx + j] = (T)s;
    Sff[j * nx + i] = (T)s;
  }
}

MMA_FN void mma_mix_bwd(Ctx c, int nx, int Lg, int nd, const double* W, const double* gf1, const double* gSff,
                        const double* gcross, double* gg1, double* gSgg, double* gcg, double* sm) {
  const int lane = c.lane(), nl = c.nl();
  double* GW = sm;                                          // (g Sff) W [nx][Lg]
  for (int idx = lane; idx < nx * Lg; idx += nl) {
    const int i = idx / Lg, l = idx - i * Lg;
    double s = 0.0;
    for (int j = 0; j < nx; ++j) s = fma(gSff[i * nx + j], W[j * Lg + l], s);
    GW[idx] = s;
  }
  for (int l = lane; l < Lg; l += nl) {
    double s = 0.0;
    for (int i = 0; i < nx; ++i) s = fma(W[i * Lg + l], gf1[i], s);
    gg1[l] = s;
  }
  for (int idx = lane; idx < nd * Lg; idx += nl) {
    const int k = idx / Lg, l = idx - k * Lg;
    double s = 0.0;
    for (int i = 0; i < nx; ++i) s = fma(gcross[k * nx + i], W[i * Lg + l], s);
    gcg[idx] = s;
  }
  c.sync();
  for (int idx = lane; idx < Lg * Lg; idx += nl) {
    const int k = idx / Lg, l = idx - k * Lg;
    double s = 0.0;
    for (int i = 0; i < nx; ++i) s = fma(W[i * Lg + k], GW[i * Lg + l], s);
    gSgg[idx] = s;
  }
}
