// CPU build of the output mixing of a coregionalised drift and its adjoint (csrc/mm_mix.h; MMAHostCtx: one host thread, no
// barriers) -- TEST INFRASTRUCTURE ONLY, as mm_adjoint_nd_host.hip: tests/test_coregionalized.py loads it to check the two maps
// against torch without a GPU; nothing under gpflowpilco_amd/ loads or links it.
#include <vector>
#include "../../gpflowpilco_amd/csrc/mm_mix.h"

extern "C" void hc_mix_fwd(int nx, int Lg, int nd, const double* W, const double* mc, const double* g1, const double* Sgg,
                           const double* cg, double* f1, double* Sff, double* cross) {
  std::vector<double> sm(mma_mix_scratch(nx, Lg) + 8);
  mma_mix_fwd<MMAHostCtx, double>(MMAHostCtx(), nx, Lg, nd, W, mc, g1, Sgg, cg, f1, Sff, cross, sm.data());
}

// the same with the moments in float: f64 arithmetic, rounded on store
extern "C" void hc_mix_fwd_f32(int nx, int Lg, int nd, const double* W, const double* mc, const float* g1, const float* Sgg,
                               const float* cg, float* f1, float* Sff, float* cross) {
  std::vector<double> sm(mma_mix_scratch(nx, Lg) + 8);
  mma_mix_fwd<MMAHostCtx, float>(MMAHostCtx(), nx, Lg, nd, W, mc, g1, Sgg, cg, f1, Sff, cross, sm.data());
}

extern "C" void hc_mix_bwd(int nx, int Lg, int nd, const double* W, const double* gf1, const double* gSff, const double* gcross,
                           double* gg1, double* gSgg, double* gcg) {
  std::vector<double> sm(mma_mix_scratch(nx, Lg) + 8);
  mma_mix_bwd(MMAHostCtx(), nx, Lg, nd, W, gf1, gSff, gcross, gg1, gSgg, gcg, sm.data());
}
