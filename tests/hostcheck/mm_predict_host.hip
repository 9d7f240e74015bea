// CPU build of the predictive mean and variance (csrc/mm_predict.h's schedule, csrc/mm_gram.h's entries; one host thread, scalar fma
// for the matrix instruction, std::exp for the device exponential) -- TEST INFRASTRUCTURE ONLY, as mm_gram_host.hip:
// tests/test_predict_host.py loads it to check the schedule and its masks against torch without a GPU; nothing under
// gpflowpilco_amd/ loads or links it.  The arguments are mm_predict_se's without the workspace and the stream.
#include <algorithm>
#include <vector>
#include "../../gpflowpilco_amd/csrc/mm_predict.h"

// the visited blocks in the order of the walk: (ib, jb, weight) per visit; returns their number (fills at most cap of them)
extern "C" long long hc_predict_schedule(int M, int cap, int* ib, int* jb, double* weight) {
  long long n = 0;
  for (MMPBlock b = mmp_first(); !mmp_done(b, M); b = mmp_next(b), ++n)
    if (n < cap) { ib[n] = b.ib; jb[n] = b.jb; weight[n] = mmp_weight(b); }
  return n;
}

extern "C" int hc_predict_se(int L, int M, int N, int d, const double* X, const double* Z, const double* ls, const double* var,
                             const double* beta, const double* C, const double* mean_c, double* mean, double* fvar) {
  if ((C == nullptr) != (fvar == nullptr)) return -1;
  const int nb = mmp_blocks(M), tiles = mmp_tiles(N);
  std::vector<double> strip(mmp_strip(M)), acc((size_t)MMP_B * MMP_TN);
  for (long long item = 0; item < mmp_items(L, N); ++item) {
    const int l = (int)(item / tiles), t = (int)(item - (long long)l * tiles);
    const double* Zl = Z + (size_t)l * M * d;
    const double* Cl = C ? C + (size_t)l * M * M : nullptr;
    // phase 1: the strip (zero past M and N) and the mean: 4 row groups of 16 per block, added in index order
    double msum[4][MMP_TN] = {};
    for (int jb = 0; jb < nb; ++jb)
      for (int r = 0; r < MMP_B; ++r)
        for (int c = 0; c < MMP_TN; ++c) {
          double kv = 0.0, b = 0.0;
          if (mmp_row_valid(M, jb, r)) {
            b = beta[(size_t)l * M + jb * MMP_B + r];
            if (mmp_col_valid(N, t, c)) {
              double a = 0.0;
              for (int k = 0; k < d; ++k)
                a = mmg_sq_acc(X[((size_t)t * MMP_TN + c) * d + k], Zl[((size_t)jb * MMP_B + r) * d + k], 1.0 / ls[(size_t)l * d + k], a);
              kv = var[l] * mmg_profile(a);
            }
          }
          strip[((size_t)jb * MMP_B + r) * MMP_TN + c] = kv;
          msum[r >> 4][c] = fma(kv, b, msum[r >> 4][c]);
        }
    for (int c = 0; c < MMP_TN; ++c)
      if (mmp_col_valid(N, t, c)) {
        double s = msum[0][c];
        for (int j = 1; j < 4; ++j) s += msum[j][c];
        mean[((size_t)t * MMP_TN + c) * L + l] = mean_c ? s + mean_c[l] : s;
      }
    if (!C) continue;
    // phase 2: the walk; 16 partial sums per point (row group w = i / 16, residue kq = i % 4), rows in ascending order inside each
    double vs[16][MMP_TN] = {};
    for (MMPBlock blk = mmp_first(); !mmp_done(blk, M); blk = mmp_next(blk)) {
      if (blk.jb == 0) std::fill(acc.begin(), acc.end(), 0.0);
      const double scale = mmp_row_scale(blk);
      for (double& a : acc) a *= scale;
      for (int i = 0; i < MMP_B; ++i)
        for (int j = 0; j < MMP_B; ++j) {
          const double cij = (mmp_row_valid(M, blk.ib, i) && mmp_row_valid(M, blk.jb, j))
                                 ? Cl[((size_t)blk.ib * MMP_B + i) * M + (size_t)blk.jb * MMP_B + j] : 0.0;
          for (int c = 0; c < MMP_TN; ++c)
            acc[(size_t)i * MMP_TN + c] = fma(cij, strip[((size_t)blk.jb * MMP_B + j) * MMP_TN + c], acc[(size_t)i * MMP_TN + c]);
        }
      if (mmp_is_diagonal(blk))
        for (int i = 0; i < MMP_B; ++i) {
          const int p = (i >> 4) * 4 + (i & 3);
          for (int c = 0; c < MMP_TN; ++c)
            vs[p][c] = fma(strip[((size_t)blk.ib * MMP_B + i) * MMP_TN + c], acc[(size_t)i * MMP_TN + c], vs[p][c]);
        }
    }
    for (int c = 0; c < MMP_TN; ++c)
      if (mmp_col_valid(N, t, c)) {
        double s = vs[0][c];
        for (int j = 1; j < 16; ++j) s += vs[j][c];
        fvar[((size_t)t * MMP_TN + c) * L + l] = var[l] + s;
      }
  }
  return 0;
}
