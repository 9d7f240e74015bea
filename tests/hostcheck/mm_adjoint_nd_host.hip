// CPU build of the multi-action adjoint arithmetic of csrc/mm_adjoint_nd.h (MMAHostCtx: one host thread, no barriers) -- TEST
// INFRASTRUCTURE ONLY, as mm_adjoint_host.hip: tests/test_adjoint_nd_host.py loads it to check the hand-derived adjoints against
// autograd without a GPU; nothing under gpflowpilco_amd/ loads or links it.
#include <vector>
#include "../../gpflowpilco_amd/csrc/mm_adjoint_nd.h"

extern "C" int hc_step_bwd_nd(int nx, int na, int nu, const int32_t* act, double dt, const double* Sxe, const double* cp,
                              const double* Sdd, const double* dcross, const double* gm1, const double* gS1, double* gSxe,
                              double* gcp, double* gSdd, double* gdf1, double* gdSff, double* gdcross) {
  MMComposeDims D;
  const int rc = mm_compose_dims_nd(nx, na, nu, act, D);
  if (rc) return rc;
  std::vector<double> sm(mma_step_bwd_scratch(nx, D.nd) + 8);
  mma_step_bwd_nd(MMAHostCtx(), D, dt, Sxe, cp, Sdd, dcross, gm1, gS1, gSxe, gcp, gSdd, gdf1, gdSff, gdcross, sm.data());
  return 0;
}

extern "C" void hc_head_bwd_nd(int ne, int nu, const double* scale, const double* shift, const double* pf1, const double* pSff,
                               const double* pcross, const double* See, const double* gmd, const double* gSdd, const double* gcp,
                               double* gme, double* gSee, double* gpcross, double* gpf1, double* gpSff) {
  std::vector<double> sm(mma_head_bwd_nd_scratch(ne, nu) + 8);
  mma_head_bwd_nd(MMAHostCtx(), ne, nu, scale, shift, pf1, pSff, pcross, See, gmd, gSdd, gcp, gme, gSee, gpcross, gpf1, gpSff,
                  sm.data());
}

extern "C" int hc_policy_pair_bwd(int M, int d, const double* Za, const double* betaa, const double* la2, double vara,
                                  const double* Zb, const double* betab, const double* lb2, double varb, const double* mu,
                                  const double* Sigma, double g, double* gmu, double* gSig, double* gpa, double* gpb) {
  std::vector<double> sm(mma_policy_pair_bwd_scratch(M, d, 1) + 8);
  bool ok = true;
  mma_policy_pair_bwd(MMAHostCtx(), M, d, Za, betaa, la2, vara, Zb, betab, lb2, varb, mu, Sigma, g, gmu, gSig, gpa, gpb, sm.data(),
                      &ok);
  return ok ? 0 : 1;
}

extern "C" int hc_policy_nd_bwd(int nu, int M, int d, const double* Z, const double* beta, const double* ls2, const double* var,
                                const double* mu, const double* Sigma, const double* gf1, const double* gSff, const double* gcross,
                                double* gmu, double* gSig, double* gpar) {
  std::vector<double> sm(mma_policy_nd_bwd_scratch(M, d, 1) + 8);
  bool ok = true;
  mma_policy_nd_bwd<MMAHostCtx, 8>(MMAHostCtx(), nu, M, d, Z, beta, ls2, var, mu, Sigma, gf1, gSff, gcross, gmu, gSig, gpar,
                                   sm.data(), &ok);
  return ok ? 0 : 1;
}
