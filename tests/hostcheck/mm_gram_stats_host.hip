// CPU build of the schedule of the streamed Gram statistics and their adjoint (csrc/mm_gram_stats.h; one host thread, scalar fma for
// the matrix instruction, std::exp for the device exponential) -- TEST INFRASTRUCTURE ONLY, as mm_predict_host.hip:
// tests/test_gram_stats_host.py loads it to check the items, blocks, chunks, splits and sums against torch without a GPU; nothing
// under gpflowpilco_amd/ loads or links it.
#include <vector>
#include "../../gpflowpilco_amd/csrc/mm_gram_stats.h"

static double hc_k(int d, const double* x, const double* z, const double* ls, double var) {
  double acc = 0.0;
  for (int k = 0; k < d; ++k) acc = mmg_sq_acc(x[k], z[k], 1.0 / ls[k], acc);
  return var * mmg_profile(acc);
}

// tile [64][64] of K: rows of block b, points of chunk ch, masked to zero past M and N
static void hc_tile(int M, int N, int d, int b, int ch, const double* X, const double* Zl, const double* lsl, double var, double* T) {
  for (int r = 0; r < MGS_B; ++r)
    for (int j = 0; j < MGS_TN; ++j) {
      const bool ok = mgs_row_valid(M, b, r) && mgs_col_valid(N, ch, j);
      T[r * MGS_TN + j] = ok ? hc_k(d, X + ((size_t)ch * MGS_TN + j) * d, Zl + ((size_t)b * MGS_B + r) * d, lsl, var) : 0.0;
    }
}

extern "C" int hc_stats_splits(int L, int M, int N) { return mgs_splits(L, M, N); }

// visits[l][pair][n] += 1 for every point the forward schedule hands to a block pair
extern "C" void hc_stats_schedule(int L, int M, int N, int* visits) {
  const long long pairs = mgs_pairs(M);
  const int S = mgs_splits(L, M, N), cps = mgs_chunks_per_split(L, M, N), nch = mgs_chunks(N);
  for (long long item = 0; item < (long long)L * pairs * S; ++item) {
    const int s = (int)(item % S);
    const long long lp = item / S;
    const int c0 = s * cps, c1 = c0 + cps < nch ? c0 + cps : nch;
    for (int ch = c0; ch < c1; ++ch)
      for (int j = 0; j < MGS_TN; ++j)
        if (mgs_col_valid(N, ch, j)) visits[(size_t)lp * N + (size_t)ch * MGS_TN + j] += 1;
  }
}

extern "C" void hc_stats_fwd(int L, int M, int N, int d, int Q, const double* X, const double* R, const double* Z, const double* ls,
                             const double* var, double* Phi, double* Psi) {
  const MGSWs w = mgs_workspace(L, M, d, Q);
  std::vector<double> ws(w.fwd_total, 0.0), Ti(MGS_B * MGS_TN), Tj(MGS_B * MGS_TN);
  const long long pairs = mgs_pairs(M);
  const int S = mgs_splits(L, M, N), cps = mgs_chunks_per_split(L, M, N), nch = mgs_chunks(N), nb = mgs_blocks(M);
  for (long long item = 0; item < (long long)L * pairs * S; ++item) {
    const int s = (int)(item % S);
    const long long lp = item / S;
    const int l = (int)(lp / pairs);
    int ib, jb;
    mgs_pair_blocks(lp - (long long)l * pairs, ib, jb);
    const int c0 = s * cps, c1 = c0 + cps < nch ? c0 + cps : nch;
    double* part = ws.data() + w.phi + ((size_t)lp * S + s) * (MGS_B * MGS_B);
    double* pp = ws.data() + w.psi + (((size_t)l * nb + ib) * S + s) * ((size_t)MGS_B * Q);
    for (int ch = c0; ch < c1; ++ch) {
      hc_tile(M, N, d, ib, ch, X, Z + (size_t)l * M * d, ls + (size_t)l * d, var[l], Ti.data());
      hc_tile(M, N, d, jb, ch, X, Z + (size_t)l * M * d, ls + (size_t)l * d, var[l], Tj.data());
      for (int r = 0; r < MGS_B; ++r)
        for (int c = 0; c < MGS_B; ++c) {
          double acc = part[r * MGS_B + c];
          for (int j = 0; j < MGS_TN; ++j) acc = fma(Ti[r * MGS_TN + j], Tj[c * MGS_TN + j], acc);
          part[r * MGS_B + c] = acc;
        }
      if (Q > 0 && jb == 0)
        for (int r = 0; r < MGS_B; ++r)
          for (int q = 0; q < Q; ++q) {
            double acc = pp[(size_t)r * Q + q];
            for (int j = 0; j < MGS_TN; ++j)
              if (mgs_col_valid(N, ch, j)) acc = fma(Ti[r * MGS_TN + j], R[((size_t)ch * MGS_TN + j) * Q + q], acc);
            pp[(size_t)r * Q + q] = acc;
          }
    }
  }
  // k_stats_fwd_sum
  for (int l = 0; l < L; ++l)
    for (int i = 0; i < M; ++i) {
      for (int j = 0; j < M; ++j) {
        const int a = i > j ? i : j, b = i > j ? j : i, ib = a / MGS_B, jb = b / MGS_B;
        const double* p = ws.data() + w.phi + (((size_t)l * pairs + (size_t)mgs_pair_index(ib, jb)) * S) * (MGS_B * MGS_B)
                          + (size_t)(a - ib * MGS_B) * MGS_B + (b - jb * MGS_B);
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += p[(size_t)s * (MGS_B * MGS_B)];
        Phi[((size_t)l * M + i) * M + j] = sum;
      }
      for (int q = 0; q < Q; ++q) {
        const int ib = i / MGS_B;
        const double* p = ws.data() + w.psi + (((size_t)l * nb + ib) * S) * ((size_t)MGS_B * Q) + (size_t)(i - ib * MGS_B) * Q + q;
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += p[(size_t)s * MGS_B * Q];
        Psi[((size_t)l * M + i) * Q + q] = sum;
      }
    }
}

extern "C" void hc_stats_bwd(int L, int M, int N, int d, int Q, const double* GPhi, const double* GPsi, const double* X,
                             const double* R, const double* Z, const double* ls, const double* var, double* gZ, double* gls,
                             double* gvar) {
  const int nb = mgs_blocks(M), nch = mgs_chunks(N), groups = mgs_bwd_groups(L, N);
  const size_t sl = mgs_slice(M, d), md = (size_t)M * d;
  std::vector<double> Gs((size_t)L * M * M), strip(mgs_strip(M)), slices((size_t)L * groups * sl, 0.0), t(MGS_B * MGS_TN);
  for (int l = 0; l < L; ++l)
    for (int a = 0; a < M; ++a)
      for (int b = 0; b < M; ++b)
        Gs[((size_t)l * M + a) * M + b] = GPhi[((size_t)l * M + a) * M + b] + GPhi[((size_t)l * M + b) * M + a];
  for (int l = 0; l < L; ++l)
    for (int w = 0; w < groups; ++w) {
      double* slZ = slices.data() + ((size_t)l * groups + w) * sl;
      double* slL = slZ + md;
      double* slV = slL + d;
      const double* Zl = Z + (size_t)l * M * d;
      for (int ch = w; ch < nch; ch += groups) {
        for (int jb = 0; jb < nb; ++jb)
          hc_tile(M, N, d, jb, ch, X, Zl, ls + (size_t)l * d, var[l], strip.data() + (size_t)jb * MGS_B * MGS_TN);
        for (int ib = 0; ib < nb; ++ib) {
          for (int r = 0; r < MGS_B; ++r)
            for (int j = 0; j < MGS_TN; ++j) {
              double acc = 0.0;
              if (mgs_row_valid(M, ib, r)) {
                const double* g = Gs.data() + ((size_t)l * M + (size_t)ib * MGS_B + r) * M;
                for (int m = 0; m < M; ++m) acc = fma(g[m], strip[(size_t)m * MGS_TN + j], acc);
                if (mgs_col_valid(N, ch, j))
                  for (int q = 0; q < Q; ++q)
                    acc = fma(GPsi[((size_t)l * M + (size_t)ib * MGS_B + r) * Q + q], R[((size_t)ch * MGS_TN + j) * Q + q], acc);
              }
              const double tv = acc * strip[((size_t)ib * MGS_B + r) * MGS_TN + j];
              t[r * MGS_TN + j] = tv;
              slV[0] += tv;
            }
          for (int r = 0; r < MGS_B; ++r) {
            if (!mgs_row_valid(M, ib, r)) continue;
            const size_t m = (size_t)ib * MGS_B + r;
            for (int k = 0; k < d; ++k) {
              double az = 0.0, al = 0.0;
              for (int j = 0; j < MGS_TN; ++j) {
                const double x = mgs_col_valid(N, ch, j) ? X[((size_t)ch * MGS_TN + j) * d + k] : 0.0;
                mmg_adj_acc(t[r * MGS_TN + j], x, Zl[m * d + k], az, al);
              }
              slZ[m * d + k] += az;
              slL[k] += al;
            }
          }
        }
      }
    }
  // k_stats_bwd_sum
  for (int l = 0; l < L; ++l) {
    for (size_t i = 0; i < md + d + 1; ++i) {
      double sum = 0.0;
      for (int w = 0; w < groups; ++w) sum += slices[((size_t)l * groups + w) * sl + i];
      if (i < md) gZ[(size_t)l * md + i] = mmg_gz_scale(sum, 1.0 / ls[(size_t)l * d + i % d]);
      else if (i < md + d) gls[(size_t)l * d + (i - md)] = mmg_gl_scale(sum, 1.0 / ls[(size_t)l * d + (i - md)]);
      else gvar[l] = sum / var[l];
    }
  }
}
