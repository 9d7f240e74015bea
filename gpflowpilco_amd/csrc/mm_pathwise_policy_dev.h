// Device helpers and the tape layout of the pathwise policy rollout and its reverse sweep (mm_pathwise_policy.hip, 1 .. 4
// actions).  Encoder, cost, the policy's predictive mean, the fixed-order wave sum; and what its entries hand their drivers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "mm_common.h"
#include "mm_compose.h"

#include "mm_pathwise_drift.h"

#define MMP_NE 24            // largest encoded dimension (2 na + nb, na <= 8, nx <= 16)
#define MMP_POLICY_MMAX 256

// What an entry of mm_pathwise_policy.hip knows about its rollout, by name: the forward and the reverse driver take this and
// their per-call buffers.  The entries differ in which fields they set and in the four at the end of the list.
struct MMPwRollout {
  // S, M, K, dtype, kernel and the operands (a reverse sweep: S and dtype alone); L and d are the driver's (the latents a step
  // keeps, nd drift inputs)
  MMPwDrift drift;
  int nx = 0, na = 0, nu = 0;
  const int32_t* active_dims = nullptr;
  const void* policy_packed = nullptr;                  // an mm_pack_model pack with L = nu: its f64 blocks are read
  size_t policy_bytes = 0;
  int policy_M = 0;
  const double *head_scale = nullptr, *head_shift = nullptr;    // [nu]
  const void *target = nullptr, *precis = nullptr;
  int Lg = 0;                                           // mixed: f = mix_W g + mix_c, mix_W [nx][Lg], mix_c [nx] or NULL
  const double *mix_W = nullptr, *mix_c = nullptr;
  int H = 0;
  double dt = 0.0;
  void* stream = nullptr;
  int nd_max = 8;              // 8: the one-action and _nd entries; 16: _wide, _mixed, _kern, _mean
  bool mixed = false;          // a coregionalised drift (the _mixed entries; _kern and _mean with Lg or mix_W set)
  bool one_action = false;     // the one-action entries: na > 0 without active_dims is MM_E_DIM, not MM_E_ARG
  bool seeded_entry = false;   // reverse sweeps: either seed may be NULL, not both (else g_cost is required)
};

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
