// Device bodies the composed rollouts share (mm_compose.hip: one action; mm_compose_nd.hip: several): the 48-point
// Gauss-Legendre rule of the NormalCDF head's quadratures and the trigonometric encoding of a state.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "mm_compose.h"

static __device__ const double MM_GL48_X[48] = {-9.98771007252426068e-01, -9.93530172266350764e-01, -9.84124583722826851e-01, -9.70591592546247273e-01, -9.52987703160430910e-01, -9.31386690706554332e-01, -9.05879136715569633e-01, -8.76572020274247854e-01, -8.43588261624393487e-01, -8.07066204029442624e-01, -7.67159032515740358e-01, -7.24034130923814634e-01, -6.77872379632663891e-01, -6.28867396776513599e-01, -5.77224726083972683e-01, -5.23160974722232996e-01, -4.66902904750958414e-01, -4.08686481990716721e-01, -3.48755886292160755e-01, -2.87362487355455554e-01, -2.24763790394689050e-01, -1.61222356068891709e-01, -9.70046992094626970e-02, -3.23801709628693674e-02, 3.23801709628693674e-02, 9.70046992094626970e-02, 1.61222356068891709e-01, 2.24763790394689050e-01, 2.87362487355455554e-01, 3.48755886292160755e-01, 4.08686481990716721e-01, 4.66902904750958414e-01, 5.23160974722232996e-01, 5.77224726083972683e-01, 6.28867396776513599e-01, 6.77872379632663891e-01, 7.24034130923814634e-01, 7.67159032515740358e-01, 8.07066204029442624e-01, 8.43588261624393487e-01, 8.76572020274247854e-01, 9.05879136715569633e-01, 9.31386690706554332e-01, 9.52987703160430910e-01, 9.70591592546247273e-01, 9.84124583722826851e-01, 9.93530172266350764e-01, 9.98771007252426068e-01};
static __device__ const double MM_GL48_W[48] = {3.15334605230917957e-03, 7.32755390127649234e-03, 1.14772345792349736e-02, 1.55793157229429276e-02, 1.96161604573552965e-02, 2.35707608393240925e-02, 2.74265097083568818e-02, 3.11672278327983394e-02, 3.47772225647706573e-02, 3.82413510658306741e-02, 4.15450829434645535e-02, 4.46745608566940997e-02, 4.76166584924902839e-02, 5.03590355538542783e-02, 5.28901894851934867e-02, 5.51995036999840538e-02, 5.72772921004029295e-02, 5.91148396983954827e-02, 6.07044391658935825e-02, 6.20394231598924636e-02, 6.31141922862537841e-02, 6.39242385846479494e-02, 6.44661644359498381e-02, 6.47376968126836816e-02, 6.47376968126836816e-02, 6.44661644359498381e-02, 6.39242385846479494e-02, 6.31141922862537841e-02, 6.20394231598924636e-02, 6.07044391658935825e-02, 5.91148396983954827e-02, 5.72772921004029295e-02, 5.51995036999840538e-02, 5.28901894851934867e-02, 5.03590355538542783e-02, 4.76166584924902839e-02, 4.46745608566940997e-02, 4.15450829434645535e-02, 3.82413510658306741e-02, 3.47772225647706573e-02, 3.11672278327983394e-02, 2.74265097083568818e-02, 2.35707608393240925e-02, 1.96161604573552965e-02, 1.55793157229429276e-02, 1.14772345792349736e-02, 7.32755390127649234e-03, 3.15334605230917957e-03};

// ---------------------------------------------------------------------------------------------
// mmc_encode_body: (mx, Sxx) -> moments of e = [sin a, cos a, x_inactive] and Cov(x, e)
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void mmc_encode_body(const MMComposeDims& D, const T* mx, const T* Sxx, T* me, T* See, double* Sxe,
                                                int b, int lane) {
  const int nx = D.nx, na = D.na, nb = D.nb, ne = D.ne, n2 = 2 * na;
  __shared__ double m[MMC_NX], S[MMC_NX * MMC_NX];
  __shared__ double s1[MMC_NA], c1[MMC_NA];
  __shared__ double Syy[4 * MMC_NA * MMC_NA];      // centred covariance of [sin a, cos a]
  __shared__ double Sxy[MMC_NX * 2 * MMC_NA];      // Cov(x, [sin a, cos a])
  for (int i = lane; i < nx; i += 64) m[i] = (double)mx[(size_t)b * nx + i];
  for (int i = lane; i < nx * nx; i += 64) S[i] = (double)Sxx[(size_t)b * nx * nx + i];
  __syncthreads();
  __shared__ double sa[MMC_NA], ca[MMC_NA];        // sin a_i, cos a_i: ONE sincos per angle, the pair terms by angle addition
  if (lane < na) {                                 // maths.py:143-176: first moments
    const int r = D.active[lane];
    const double a = m[r], ev = exp(-0.5 * S[r * nx + r]);
    double sv, cv;
    sincos(a, &sv, &cv);
    sa[lane] = sv; ca[lane] = cv;
    s1[lane] = ev * sv; c1[lane] = ev * cv;
  }
  __syncthreads();
  for (int idx = lane; idx < na * na; idx += 64) { // second moments (uncentred), then centred
    const int i = idx / na, j = idx - i * na;
    const int ri = D.active[i], rj = D.active[j];
    const double vi = S[ri * nx + ri], vj = S[rj * nx + rj];
    const double sij = 0.5 * (S[ri * nx + rj] + S[rj * nx + ri]);       // (Sxx + Sxx^T) / 2
    const double A = exp(-0.5 * (vi + vj) - sij), Bm = exp(-0.5 * (vi + vj) + sij);
    const double cc = ca[i] * ca[j], ss = sa[i] * sa[j];
    const double Acos = A * (cc - ss), Bcos = Bm * (cc + ss);           // cos(a_i + a_j), cos(a_i - a_j)
    const double s2 = 0.5 * (Bcos - Acos), c2 = 0.5 * (Bcos + Acos);
    const double sc = 0.5 * (sa[i] * ca[j] * (Bm + A) - sa[j] * ca[i] * (Bm - A));   // E[sin a_i cos a_j]
    Syy[i * n2 + j] = s2 - s1[i] * s1[j];
    Syy[(na + i) * n2 + na + j] = c2 - c1[i] * c1[j];
    Syy[i * n2 + na + j] = sc - s1[i] * c1[j];
    Syy[(na + j) * n2 + i] = sc - s1[i] * c1[j];
  }
  // Cov(x, y) = Sxa [diag(c1), diag(-s1)]   (pre-inverted cross of sincos, components.py:35-37)
  for (int idx = lane; idx < nx * na; idx += 64) {
    const int r = idx / na, j = idx - r * na;
    const double sra = S[r * nx + D.active[j]];
    Sxy[r * n2 + j] = sra * c1[j];
    Sxy[r * n2 + na + j] = -sra * s1[j];
  }
  __syncthreads();
  T* meb = me + (size_t)b * ne;
  T* Seb = See + (size_t)b * ne * ne;
  double* Sxeb = Sxe + (size_t)b * nx * ne;
  for (int k = lane; k < ne; k += 64)
    meb[k] = (T)(k < na ? s1[k] : k < n2 ? c1[k - na] : m[D.inactive[k - n2]]);
  for (int idx = lane; idx < ne * ne; idx += 64) {           // components.py:41-53
    const int i = idx / ne, j = idx - i * ne;
    double v;
    if (i < n2 && j < n2) v = Syy[i * n2 + j];
    else if (i >= n2 && j >= n2) v = S[D.inactive[i - n2] * nx + D.inactive[j - n2]];
    else if (i >= n2) v = Sxy[D.inactive[i - n2] * n2 + j];  // Sby
    else v = Sxy[D.inactive[j - n2] * n2 + i];               // Sby^T
    Seb[idx] = (T)v;
  }
  for (int idx = lane; idx < nx * ne; idx += 64) {
    const int r = idx / ne, k = idx - r * ne;
    Sxeb[idx] = k < n2 ? Sxy[r * n2 + k] : S[r * nx + D.inactive[k - n2]];
  }
}
