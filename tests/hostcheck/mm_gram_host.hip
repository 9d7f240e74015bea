// CPU build of the per-entry arithmetic of the SE-ARD Gram matrix and its adjoint (csrc/mm_gram.h; one host thread, std::exp for
// the device exponential) -- TEST INFRASTRUCTURE ONLY, as mm_mix_host.hip: tests/test_gram_host.py loads it to check the maps against
// torch autograd without a GPU; nothing under gpflowpilco_amd/ loads or links it.  One latent per call; X == NULL is the self mode
// of mm_gram_se / mm_gram_se_backward (X = Z, N = M, G a general [M, M] matrix).
#include <vector>
#include "../../gpflowpilco_amd/csrc/mm_gram.h"

static double hc_entry(int d, const double* x, const double* z, const double* ls) {
  double acc = 0.0;
  for (int k = 0; k < d; ++k) acc = mmg_sq_acc(x[k], z[k], 1.0 / ls[k], acc);
  return mmg_profile(acc);
}

extern "C" void hc_gram_fwd(int M, int N, int d, const double* X, const double* Z, const double* ls, double var, double* K) {
  const double* Xp = X ? X : Z;
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) K[(size_t)m * N + n] = var * hc_entry(d, Xp + (size_t)n * d, Z + (size_t)m * d, ls);
}

extern "C" void hc_gram_bwd(int M, int N, int d, const double* G, const double* X, const double* Z, const double* ls, double var,
                            double* gZ, double* gls, double* gvar) {
  const bool self = X == nullptr;
  const double* Xp = self ? Z : X;
  std::vector<double> al_sum(d, 0.0);
  double gv = 0.0;
  for (int m = 0; m < M; ++m) {
    std::vector<double> az(d, 0.0), al(d, 0.0);
    for (int n = 0; n < N; ++n) {
      const double e = hc_entry(d, Xp + (size_t)n * d, Z + (size_t)m * d, ls);
      const double g = G[(size_t)m * N + n];
      gv = fma(g, e, gv);
      const double t = (self ? g + G[(size_t)n * M + m] : g) * (var * e);
      for (int k = 0; k < d; ++k) mmg_adj_acc(t, Xp[(size_t)n * d + k], Z[(size_t)m * d + k], az[k], al[k]);
    }
    for (int k = 0; k < d; ++k) {
      gZ[(size_t)m * d + k] = mmg_gz_scale(az[k], 1.0 / ls[k]);
      al_sum[k] += al[k];
    }
  }
  for (int k = 0; k < d; ++k) gls[k] = (self ? 0.5 : 1.0) * mmg_gl_scale(al_sum[k], 1.0 / ls[k]);
  *gvar = gv;
}
