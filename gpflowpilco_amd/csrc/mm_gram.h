// Per-entry arithmetic of the SE-ARD Gram matrix and of its adjoint (mm_gram.hip; f64).  Written once for the device kernels and for
// the one-thread CPU build that tests/test_gram_host.py checks against torch autograd (tests/hostcheck/mm_gram_host.hip): the host
// side differs in the exponential alone (std::exp for mm_exp_f64).
//
//   K[m][n]  = var exp(-1/2 sum_k ((x_nk - z_mk) / l_k)^2)            the squared distance from DIFFERENCES: no a^2 + b^2 - 2ab
//   t        = G[m][n] K[m][n]
//   gZ[m][k] = sum_n t (x_nk - z_mk) / l_k^2,   gls[k] = sum_mn t (x_nk - z_mk)^2 / l_k^3,   gvar = sum_mn t / var = sum_mn G e
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#if defined(__HIP_DEVICE_COMPILE__)
#include "mm_exp_f64.h"
#endif

#define MMG_FN __host__ __device__ __forceinline__

// tile of one workgroup: MMG_TM rows (inducing points) x MMG_TN columns (data points), MMG_THREADS threads
#define MMG_TM 16
#define MMG_TN 128
#define MMG_THREADS 256
#define MMG_RPT (MMG_TM * MMG_TN / MMG_THREADS)      /* rows per thread of the entry phase: 8 */

// acc + ((x - z) il)^2, il = 1 / lengthscale
MMG_FN double mmg_sq_acc(double x, double z, double il, double acc) {
  const double t = (x - z) * il;
  return fma(t, t, acc);
}

// e^{-acc / 2}: the entry without its variance
MMG_FN double mmg_profile(double acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return mm_exp_f64(-0.5 * acc);
#else
  return exp(-0.5 * acc);
#endif
}

// one entry's contribution to the two sums of a (row, dimension) pair: az += t (x - z), al += t (x - z)^2
MMG_FN void mmg_adj_acc(double t, double x, double z, double& az, double& al) {
  const double diff = x - z;
  az = fma(t, diff, az);
  al = fma(t * diff, diff, al);
}

// ... and what turns the sums into gradients
MMG_FN double mmg_gz_scale(double az, double il) { return az * il * il; }
MMG_FN double mmg_gl_scale(double al, double il) { return al * il * il * il; }

// column chunks / row tiles of a [M, N] Gram matrix
static inline int mmg_chunks(int N) { return (N + MMG_TN - 1) / MMG_TN; }
static inline int mmg_tiles(int M) { return (M + MMG_TM - 1) / MMG_TM; }
// workspace of mm_gram_se_backward, in doubles: [L][chunks][M][d] partial gZ, [L][tiles][chunks][d] partial gls, [L][tiles][chunks] partial gvar
struct MMGramWs { size_t gz, gl, gv, total; };
static inline MMGramWs mmg_workspace(int L, int M, int N, int d) {
  const size_t nch = (size_t)mmg_chunks(N), nrt = (size_t)mmg_tiles(M);
  MMGramWs w;
  w.gz = 0;
  w.gl = w.gz + (size_t)L * nch * M * d;
  w.gv = w.gl + (size_t)L * nrt * nch * d;
  w.total = w.gv + (size_t)L * nrt * nch;
  return w;
}
