// The MEAN of a pathwise drift on gfx950 -- SURVEY.md row f-3: what the rollout's drift(eu) is when the reference builds its
// dynamics with model_uncertainty=False (build_dynamics, gpflow_pilco/loops/pilco.py:45-79: the drift wrapped in a
// KernelRegressor, models/core.py:60-62).  Every sample evaluates the SAME function
//
//   f[s,a]   = var_a sum_m beta[a,m] e_m + mean_a                                 (e_m, g_m) = pw_kern<KF>(zs_t[a,:,m] . xs - hz[a,m] - hx)
//   J[s,a,k] = ln2 var_a sum_m beta[a,m] g_m (zs_t[a,k,m] xscale_a,k - xscale_a,k^2 x_s,k)
//
// -- the update half of the weight stream (mm_pathwise.hip) with the per-sample v[s,a,m] replaced by the shared beta[a,m] =
// (Kuu^-1 u)_m.  Nothing of size S M exists: the operands of a latent (d + 2 values per centre, ~100 KB for the C5 drift) are
// staged through LDS in chunks of PWM_MC centres and every sample of the workgroup reads them from there, so the pass is bound
// by the S L M basis values (2^x, and the d FMAs on either side of it), not by HBM.
//
// grid (ceil(S / SB), L), 64 NW threads (NW = 8 waves for DK = 8, 4 for DK = 16: the reduction buffer below stays under 64 KB).
// A workgroup owns SB samples of one latent; its 64 NW threads are SB samples x NSL = 64 NW / SB slices of the centres: thread
// (sample sl, slice q) keeps x_s in registers and walks the centres q, q + NSL, ... of every chunk -- the lanes of one slice read
// one LDS address (a broadcast), no cross-lane step inside the loop.  SB is chosen by the host, 64 down to 8, so that a small
// batch still spreads over the chip (S = 128, L = 4: 64 workgroups of 64 slices, 32 centres per thread at M = 2000).
// The NSL partial sums of a sample meet in LDS and are added in slice order by one thread per output: no atomics, bitwise
// reproducible.  Values accumulate in f64 whatever T (the stream pass: T per lane, f64 across lanes), the Jacobian sums in T
// as the stream pass keeps them; beta is f64 in both modes.  Centres with beta = 0 (padding) add exactly 0: their basis value
// is finite (zs = hz = 0: e = 2^-hx <= 1).
#include "mm_pathwise_drift.h"
#include "mm_pathwise_kern.h"

#define PWM_MC 256      // centres per LDS chunk (f64, DK = 16: 38 KB)

template <typename T, int DK>
struct PwMean {
  static constexpr int NW = DK > 8 ? 4 : 8;                      // waves per workgroup
  static constexpr int NT = 64 * NW;
  static constexpr int ROW = DK + (sizeof(T) == 4 ? 4 : 2);      // zs_t[DK] | hz | padding to 16 bytes
  static size_t lds_bytes(bool jac) {
    const size_t op = (size_t)PWM_MC * (ROW * sizeof(T) + sizeof(double)), red = (size_t)NT * (jac ? DK + 2 : 1) * sizeof(double);
    return op > red ? op : red;
  }
};

template <typename T, int DK, int KF, bool JAC>
__global__ __launch_bounds__((PwMean<T, DK>::NT)) void k_pw_mean(int S, int L, int M, int d, int SB,
                                                               const T* __restrict__ x,            // [S,d]
                                                               const T* __restrict__ zs,           // [L,d,M] scaled, k-major
                                                               const T* __restrict__ hz,           // [L,M]
                                                               const double* __restrict__ xscale,  // [L,d]
                                                               const double* __restrict__ var,     // [L]
                                                               const double* __restrict__ meanc,   // [L] or null
                                                               const double* __restrict__ beta,    // [L,M]
                                                               T* __restrict__ out,                // [S,L]
                                                               T* __restrict__ jac) {              // JAC: [S,L,d]
  constexpr int NT = PwMean<T, DK>::NT, ROW = PwMean<T, DK>::ROW, MC = PWM_MC;
  constexpr int NQ = JAC ? DK + 2 : 1;                           // per thread: sum beta e | sum beta g | sum beta g zs_k
  extern __shared__ __attribute__((aligned(16))) char pwm_smem[];
  T* op = reinterpret_cast<T*>(pwm_smem);                        // [MC][ROW]
  double* sb = reinterpret_cast<double*>(pwm_smem + (size_t)MC * ROW * sizeof(T));   // [MC] beta
  double* red = reinterpret_cast<double*>(pwm_smem);             // [NT][NQ], after the last chunk
  const int tid = threadIdx.x, a = blockIdx.y;
  const int sl = tid & (SB - 1), slice = tid / SB, NSL = NT / SB;   // SB: a power of two <= 64
  const int s = blockIdx.x * SB + sl, row = s < S ? s : S - 1;   // (ragged tail: the last sample again, not stored)
  T xs[DK], hx = (T)0;
#pragma unroll
  for (int k = 0; k < DK; ++k) {
    const T v = x[(size_t)row * d + (k < d ? k : 0)];
    const T sc = (T)xscale[a * d + (k < d ? k : 0)];
    xs[k] = (k < d) ? v * sc : (T)0;
    hx += xs[k] * xs[k];
  }
  hx *= (T)0.5;
  double accf = 0.0;
  T accg = (T)0, accJ[JAC ? DK : 1];
#pragma unroll
  for (int k = 0; k < (JAC ? DK : 1); ++k) accJ[k] = (T)0;

  for (int m0 = 0; m0 < M; m0 += MC) {
    const int mc = M - m0 < MC ? M - m0 : MC;
    __syncthreads();                                             // the previous chunk is consumed
    for (int idx = tid; idx < (DK + 1) * mc; idx += NT) {        // rows 0..d-1 of zs_t (d..DK-1: zero), row DK: hz
      const int k = idx / mc, m = idx - k * mc;
      T v = (T)0;
      if (k < d) v = zs[((size_t)a * d + k) * M + m0 + m];
      else if (k == DK) v = hz[(size_t)a * M + m0 + m];
      op[m * ROW + k] = v;
    }
    for (int m = tid; m < mc; m += NT) sb[m] = beta[(size_t)a * M + m0 + m];
    __syncthreads();
    for (int m = slice; m < mc; m += NSL) {
      const T* c = op + m * ROW;
      T arg = -c[DK] - hx;
#pragma unroll
      for (int k = 0; k < DK; ++k) arg += c[k] * xs[k];
      T e, g;
      pw_kern<KF>(arg, e, g);
      const double b = sb[m];
      accf = fma(b, (double)e, accf);
      if constexpr (JAC) {
        const T tj = (T)b * g;
        accg += tj;
#pragma unroll
        for (int k = 0; k < DK; ++k) accJ[k] += tj * c[k];
      }
    }
  }
  __syncthreads();                                               // the operands are dead: their LDS takes the partial sums
  red[tid * NQ] = accf;                                          // tid = slice SB + sl
  if constexpr (JAC) {
    red[tid * NQ + 1] = (double)accg;
#pragma unroll
    for (int k = 0; k < DK; ++k) red[tid * NQ + 2 + k] = (double)accJ[k];
  }
  __syncthreads();
  for (int t = tid; t < SB * NQ; t += NT) {                      // slice order: the same sum on every run
    const int r = t / NQ, j = t - r * NQ;
    double acc = 0.0;
    for (int q = 0; q < NSL; ++q) acc += red[(q * SB + r) * NQ + j];
    red[r * NQ + j] = acc;                                       // (slice 0's slot: read by this thread alone)
  }
  __syncthreads();
  const int NO = JAC ? 1 + d : 1;
  for (int t = tid; t < SB * NO; t += NT) {
    const int r = t / NO, j = t - r * NO, so = blockIdx.x * SB + r;
    if (so >= S) continue;
    const double vr = var[a];
    if (j == 0) {
      out[(size_t)so * L + a] = (T)(vr * red[r * NQ] + (meanc ? meanc[a] : 0.0));
    } else if constexpr (JAC) {
      // arg = zs . xs - hz - hx with xs = x xscale: d arg / d x_k = xscale_k (zs_k - xs_k)
      const int k = j - 1;
      const T sc = (T)xscale[a * d + k];
      const double xk = (double)(x[(size_t)so * d + k] * sc);    // the loop's xs_k
      jac[((size_t)so * L + a) * d + k] = (T)(0.6931471805599453 * vr * (double)sc * (red[r * NQ + 2 + k] - xk * red[r * NQ + 1]));
    }
  }
}

int pwm_check(int S, int L, int M, int d, int dtype, int kern) {
  if (kern < 0 || kern >= MM_PW_KERNELS) return MM_E_ARG;     // 0 SquaredExponential, 1 Matern-3/2, 2 Matern-5/2
  if (S <= 0 || L <= 0 || M <= 0 || d <= 0) return MM_E_ARG;
  if (d > 16) return MM_E_DIM;                                // DK = 8 | 16: what the policy rollouts take
  if (dtype != MM_F32 && dtype != MM_F64) return MM_E_DTYPE;
  return 0;
}

// one evaluation f [S,L] (and, jac != NULL, d f / d x [S,L,d]); reached through mm_pw_drift_eval (mm_pathwise.hip)
template <typename T>
int pwm_launch(const MMPwDrift& D, const T* x, T* out, T* jac, hipStream_t s) {
  const int S = D.S, L = D.L, M = D.M, d = D.d, kern = D.kernel;
  const T *zs = (const T*)D.zs_t, *hz = (const T*)D.hz;
  const double *xscale = D.x_scale, *var = D.variance, *meanc = D.mean_c, *beta = D.beta;
  // samples per workgroup: the largest of 64 .. 8 that still gives the chip a workgroup per CU
  int SB = 64;
  while (SB > 8 && (size_t)((S + SB - 1) / SB) * L < 256) SB >>= 1;
  const dim3 grid((S + SB - 1) / SB, L);
#define PWM_LAUNCH_K(DK_, KF_, JAC_)                                                                                  \
  do {                                                                                                                \
    typedef PwMean<T, DK_> P_;                                                                                        \
    hipLaunchKernelGGL((k_pw_mean<T, DK_, KF_, JAC_>), grid, dim3(P_::NT), P_::lds_bytes(JAC_), s, S, L, M, d, SB, x, zs, hz,  \
                       xscale, var, meanc, beta, out, jac);                                                           \
  } while (0)
#define PWM_LAUNCH_(DK_, JAC_) do { if (kern == 0) PWM_LAUNCH_K(DK_, 0, JAC_); else if (kern == 1) PWM_LAUNCH_K(DK_, 1, JAC_); else PWM_LAUNCH_K(DK_, 2, JAC_); } while (0)
#define PWM_LAUNCH(DK_) do { if (jac) PWM_LAUNCH_(DK_, true); else PWM_LAUNCH_(DK_, false); } while (0)
  if (d <= 8) PWM_LAUNCH(8); else PWM_LAUNCH(16);
#undef PWM_LAUNCH
#undef PWM_LAUNCH_
#undef PWM_LAUNCH_K
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
template int pwm_launch<double>(const MMPwDrift&, const double*, double*, double*, hipStream_t);
template int pwm_launch<float>(const MMPwDrift&, const float*, float*, float*, hipStream_t);

extern "C" int mm_pathwise_mean_eval(int S, int L, int M, int d, int dtype, const void* x, const void* zs_t, const void* hz,
                                     const double* x_scale, const double* variance, const double* mean_c, const double* beta,
                                     void* f_out, void* jac_out, void* stream, int kernel) {
  const int rc = pwm_check(S, L, M, d, dtype, kernel);
  if (rc) return rc;
  if (!x || !zs_t || !hz || !x_scale || !variance || !beta || !f_out) return MM_E_ARG;
  MMPwDrift D;
  D.S = S; D.L = L; D.M = M; D.d = d; D.dtype = dtype; D.kernel = kernel;
  D.zs_t = zs_t; D.hz = hz; D.x_scale = x_scale; D.variance = variance; D.mean_c = mean_c; D.beta = beta;
  MMPwOut o; o.f = f_out; o.jac = jac_out;
  return mm_pw_drift_eval(D, x, o, (hipStream_t)stream);
}
