// Device helpers and the tape layout of the pathwise policy rollout and its reverse sweep (mm_pathwise_policy.hip, 1 .. 4
// actions).  Encoder, cost, the policy's predictive mean, the fixed-order wave sum.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "mm_common.h"
#include "mm_compose.h"

int mm_pathwise_launch(int S, int L, int M, int K, int d, int dtype, const void* x, const void* omega_t, const void* phase,
                       const void* zs_t, const void* hz, const double* x_scale, const double* prior_scale, const double* variance,
                       const double* mean_c, const void* wb, void* f_out, void* jac, hipStream_t s, int kernel = 0);
// the same outputs from the MEAN of the drift (shared weights beta [L,M] f64 in place of the stream; mm_pathwise_mean.hip, d <= 16)
int mm_pathwise_mean_launch(int S, int L, int M, int d, int dtype, const void* x, const void* zs_t, const void* hz,
                            const double* x_scale, const double* variance, const double* mean_c, const double* beta, void* f_out,
                            void* jac, hipStream_t s, int kernel);

#define MMP_NE 24            // largest encoded dimension (2 na + nb, na <= 8, nx <= 16)
#define MMP_POLICY_MMAX 256

struct MMPwTapeLayout {
  size_t x;      // [H + 1][S][nx] T   states
  size_t din;    // [H][S][nd] T       drift inputs (e_h, u_h)
  size_t f;      // [S][nx] T          the current step's drift sample (scratch)
  size_t jac;    // [H][S][nx][nd] T   d f / d d per step (0 bytes when not differentiating)
  size_t total;
};
// Lf: the number of drift samples a step keeps -- nx, or the Lg latents of a coregionalised drift (the _mixed entries: the f
// slot is [S][Lg] and the Jacobian block [H][S][Lg][nd])
static inline MMPwTapeLayout mm_pw_tape_layout_latent(int S, int H, int nx, int na, int nu, int Lf, int dtype, int with_jac) {
  MMPwTapeLayout o;
  const size_t es = mm_elem_size(dtype), A = 256;
  const int nd = nx + na + nu;
  size_t off = 0;
  o.x = off;   off = mm_align_up(off + (size_t)(H + 1) * S * nx * es, A);
  o.din = off; off = mm_align_up(off + (size_t)H * S * nd * es, A);
  o.f = off;   off = mm_align_up(off + (size_t)S * Lf * es, A);
  o.jac = off; off = mm_align_up(off + (with_jac ? (size_t)H * S * Lf * nd * es : 0), A);
  o.total = off;
  return o;
}
// nd = nx + na + nu (nu = 1: the one-action tape)
static inline MMPwTapeLayout mm_pw_tape_layout(int S, int H, int nx, int na, int nu, int dtype, int with_jac) {
  return mm_pw_tape_layout_latent(S, H, nx, na, nu, nx, dtype, with_jac);
}

__device__ __forceinline__ void mmp_encode(const MMComposeDims& D, const double* x, double* e) {
  for (int i = 0; i < D.na; ++i) { double sn, cs; sincos(x[D.active[i]], &sn, &cs); e[i] = sn; e[D.na + i] = cs; }
  for (int i = 0; i < D.nb; ++i) e[2 * D.na + i] = x[D.inactive[i]];
}
// adjoint of the encoder: ge [ne] -> gx [nx] (ACCUMULATED)
__device__ __forceinline__ void mmp_encode_bwd(const MMComposeDims& D, const double* x, const double* ge, double* gx) {
  for (int i = 0; i < D.na; ++i) {
    double sn, cs;
    sincos(x[D.active[i]], &sn, &cs);
    gx[D.active[i]] += cs * ge[i] - sn * ge[D.na + i];
  }
  for (int i = 0; i < D.nb; ++i) gx[D.inactive[i]] += ge[2 * D.na + i];
}
// cost = -exp(-err^T W err / 2) of an encoded state; gq != NULL: also d cost / d e (W need not be symmetric)
__device__ __forceinline__ double mmp_cost(int ne, const double* e, const double* target, const double* precis, double* gq) {
  double err[MMP_NE], q = 0.0;
  for (int i = 0; i < ne; ++i) err[i] = e[i] - target[i];
  for (int i = 0; i < ne; ++i) {
    double r = 0.0;
    for (int j = 0; j < ne; ++j) r = fma(precis[i * ne + j], err[j], r);
    q = fma(err[i], r, q);
  }
  const double c = -exp(-0.5 * q);
  if (gq) {
    for (int i = 0; i < ne; ++i) {
      double r = 0.0;
      for (int j = 0; j < ne; ++j) r = fma(precis[i * ne + j] + precis[j * ne + i], err[j], r);
      gq[i] = -0.5 * c * r;                                  // d c = -c/2 dq,  dq = err^T (W + W^T) de
    }
  }
  return c;
}

// policy block in LDS: Z [M][ne] | beta [M] | 1 / ls2 [ne]; var, mean in registers
struct MMPwPolicy { const double* Z; const double* beta; const double* ils2; double var, mean; int M; };

__device__ __forceinline__ double mmp_policy_mean(int ne, const MMPwPolicy& P, const double* e) {
  double f = P.mean;
  for (int m = 0; m < P.M; ++m) {
    double r2 = 0.0;
    for (int k = 0; k < ne; ++k) { const double t = e[k] - P.Z[m * ne + k]; r2 = fma(t * t, P.ils2[k], r2); }
    f = fma(P.beta[m], P.var * exp(-0.5 * r2), f);
  }
  return f;
}
__device__ __forceinline__ double mmp_ndtr(double x) { return 0.5 * erfc(-x * 0.7071067811865476); }

template <typename T>
__device__ __forceinline__ void mmp_stage_policy(const double* Zg, const double* bg, const double* ls2g, int M, int ne, double* sm) {
  for (int i = threadIdx.x; i < M * ne; i += blockDim.x) sm[i] = Zg[i];
  for (int i = threadIdx.x; i < M; i += blockDim.x) sm[M * ne + i] = bg[i];
  for (int i = threadIdx.x; i < ne; i += blockDim.x) sm[M * ne + M + i] = 1.0 / ls2g[i];
  __syncthreads();
}

__device__ __forceinline__ double mmp_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
