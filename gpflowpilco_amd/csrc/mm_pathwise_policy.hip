// Pathwise POLICY rollout and its reverse sweep on gfx950, for policies with nu = 1 .. 4 actions -- SURVEY.md row f-3 (the
// cartpole's wiring: nx 4, one angle, one force; the double pendulum's: nx 4, two angles, two torques).
//
// What the reference's only caller of sample paths runs and differentiates (PathwisePILCO._policy_loss_closure,
// gpflow_pilco/loops/pilco.py:263-298; the tensor branch of forward_sde, dynamics/forward_sde.py:23-31; Euler.step,
// dynamics/solvers.py:50-65; the mean over samples and the gradient tape: examples/cartpole_swingup/train_utils.py:108-135).
// On sample paths the policy is evaluated pointwise, so the head has no cross moments: per sample path s and step h
//     e   = encoder(x_h)                  TrigonometricEncoder on tensors: [sin a, cos a, x_inactive]   (components.py:44-75)
//     u_a = scale_a (Phi(f_a(e)) + shift_a),  a < nu,   f_a(e) = sum_m beta_am k_a(e, z_am) + c_a       (models/core.py:60-71: the
//                                          KernelRegressor's predictive MEAN through Chain[Scale, Shift, NormalCDF])
//     x_{h+1} = x_h + dt f_s([e, u_0 .. u_{nu-1}])   f_s: the s-th drift sample path (mm_pathwise.hip: a weight stream, HBM-bound);
//                                          nd = ne + nu drift inputs, actions in latent order (as forward_sde appends them)
//     cost[h][s] = -exp(-(enc(x_{h+1}) - t)^T W (enc(x_{h+1}) - t) / 2)                                  (components.py:39-41)
// Forward: per step one small kernel (k_pw_head_nd: Euler update of the previous step, cost, encoder, policy -> the drift's
// input) and one stream pass (mm_pw_drift_eval, d <= 16, as it is); the taped forward makes the stream pass also emit
// d f_s / d d_s [S][nx][nd] (its JAC variant).
// Backward: samples are independent, so the WHOLE reverse sweep is one kernel (k_pw_policy_bwd_nd: thread = sample, loop over
// the steps backwards, the state's adjoint in registers) that reads the tape -- states, drift inputs, Jacobians: no second
// pass over the weight stream -- and accumulates the packed policy's gradient per wave (fixed-order wave sums -> per-wave
// slabs -> k_pw_grad_sum: deterministic).  All small algebra in f64 whatever the paths' element type.  The policy is an ordinary
// mm_pack_model pack with L = nu; only its f64 blocks are read (Z64 [L][M][ne], beta64 [L][M], ls2 [L][ne], var [L], meanc [L]).
//
// Every set of entries is ONE implementation (mmp_nd_rollout, mmp_nd_backward): the one-action entries (scalar head constants,
// nu = 1, nd <= 8), the _nd entries (nd <= 8), the _wide entries (same signatures, nd <= 16 -- the cart-double-pendulum: nx 6,
// two angles, one force: nd 9; a three-link arm: nd 13), the _kern entry (a drift of any kernel family), and
// the _mixed entries (nd <= 16), which take a COREGIONALISED drift f = W g + c: the stream pass runs with the Lg <= nx
// latents into a latent-sized tape (sample slot [S][Lg], Jacobians [H][S][Lg][nd]) and both kernels mix in place of a launch of
// its own (bool MIXED: the head steps x += dt (c + W g), the sweep takes g d = dt J_g^T (W^T g x)).  The _mean entry is the same
// function with the per-step stream pass replaced by the shared-weight mean pass (mm_pathwise_mean.hip): the drift of every
// sample is the posterior mean, nothing is streamed; tape and sweeps do not know the difference.
//
// Both kernels are templates in the action count: the loops over the latents unroll and the per-latent constants sit in
// registers.
//
// LDS of the reverse sweep (doubles per workgroup of four waves): the nu policy blocks nu (M ne + M + ne), target and W
// (ne + ne^2, + 8 spare), and one gradient slab per wave 4 nu (M ne + M + ne + 2).  The kernel takes a shape when
//     8 (nu (M ne + M + ne) + ne + ne^2 + 8 + 4 nu (M ne + M + ne + 2))  <=  160 KiB        (MMP_ND_LDS_MAX)
// -- every shape with M <= 64 and ne + nu <= 16 (tightest: nu 4, ne 12, which stops at M = 77); within ne + nu <= 8 at M = 256: nu (ne + 1) <= 15, i.e. nu = 1
// (any ne <= 7), nu = 2 (ne <= 6: the double pendulum, 144 KB), nu = 3 with ne <= 4; not nu = 3 with ne = 5 (M <= 226 fits) and
// not nu = 4 with ne = 4 (M <= 203 fits).  mm_pathwise_backward_scratch_bytes_nd / _wide return 0 and the entries MM_E_DIM beyond it.
// (The one-action entries never meet it: nu = 1, ne <= 7, M <= 256 is at most 83032 bytes.)
#include "mm_pathwise_policy_dev.h"

#define MMP_ND_LDS_MAX ((size_t)160 * 1024)


// k_pw_head_nd: grid ceil(S / 256), thread = sample.  h in [0, H]:
//   h > 0: x_h = x_{h-1} + dt f_{h-1} -> tape; cost[h-1][s] of its encoding;    h < H: the drift input (e_h, u_h[nu]) -> tape.
// LDS: the NU policy blocks one after the other (each Z [M][ne] | beta [M] | 1 / ls2 [ne]), target [ne], W [ne][ne].
// MIXED (the _mixed entries: a coregionalised drift): f is the LATENT sample g [S][Lg] and the step is
//   x_{h+1,i} = x_{h,i} + dt (c_i + sum_l mixW[i][l] g_l),   mixW [nx][Lg], mixc [nx] or NULL: f64 in global memory, read at
// wave-uniform addresses (scalar loads; nothing of it in LDS).  MIXED = false: Lg, mixW, mixc are not read.
template <typename T, int NU, bool MIXED>
__global__ __launch_bounds__(256) void k_pw_head_nd(MMComposeDims D, int S, int h, int H, double dt, const T* __restrict__ xprev,
                                                    const T* __restrict__ f, T* __restrict__ xcur, T* __restrict__ din,
                                                    T* __restrict__ cost, const T* __restrict__ target,
                                                    const T* __restrict__ precis, const double* __restrict__ pZ,
                                                    const double* __restrict__ pbeta, const double* __restrict__ pls2,
                                                    const double* __restrict__ pvar, const double* __restrict__ pmean, int pM,
                                                    MMHeadND hd, int Lg, const double* __restrict__ mixW,
                                                    const double* __restrict__ mixc) {
  extern __shared__ double sm[];
  const int nx = D.nx, ne = D.ne, nd = D.nd, blk = pM * ne + pM + ne;
  double* pol = sm;                                        // [NU][M ne + M + ne]
  double* tg = pol + NU * blk;                             // [ne]
  double* W = tg + ne;                                     // [ne][ne]
  for (int i = threadIdx.x; i < ne; i += 256) tg[i] = (double)target[i];
  for (int i = threadIdx.x; i < ne * ne; i += 256) W[i] = (double)precis[i];
#pragma unroll
  for (int a = 0; a < NU; ++a)
    mmp_stage_policy<T>(pZ + (size_t)a * pM * ne, pbeta + (size_t)a * pM, pls2 + (size_t)a * ne, pM, ne, pol + a * blk);
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  double x[MMC_NX], e[MMP_NE];
  if (h > 0) {
    if (MIXED) {
      double g[MMC_NX];
      for (int l = 0; l < Lg; ++l) g[l] = (double)f[(size_t)s * Lg + l];
      for (int i = 0; i < nx; ++i) {
        double fi = mixc ? mixc[i] : 0.0;                    // the constant is added after the mixing; latent order
        for (int l = 0; l < Lg; ++l) fi = fma(mixW[i * Lg + l], g[l], fi);
        x[i] = (double)xprev[(size_t)s * nx + i] + dt * fi;
        xcur[(size_t)s * nx + i] = (T)x[i];
      }
    } else {
      for (int i = 0; i < nx; ++i) {
        x[i] = (double)xprev[(size_t)s * nx + i] + dt * (double)f[(size_t)s * nx + i];   // Euler.step, solvers.py:50-65
        xcur[(size_t)s * nx + i] = (T)x[i];
      }
    }
  } else {
    for (int i = 0; i < nx; ++i) x[i] = (double)xcur[(size_t)s * nx + i];
  }
  // (the state every later step reads is the STORED one: rounded to T once)
  for (int i = 0; i < nx; ++i) x[i] = (double)(T)x[i];
  mmp_encode(D, x, e);
  if (h > 0) cost[(size_t)(h - 1) * S + s] = (T)mmp_cost(ne, e, tg, W, nullptr);
  if (h < H) {
    for (int i = 0; i < ne; ++i) din[(size_t)s * nd + i] = (T)e[i];
#pragma unroll
    for (int a = 0; a < NU; ++a) {
      const double* pa = pol + a * blk;
      const MMPwPolicy P{pa, pa + pM * ne, pa + pM * ne + pM, pvar[a], pmean[a], pM};
      const double u = hd.scale[a] * (mmp_ndtr(mmp_policy_mean(ne, P, e)) + hd.shift[a]);
      din[(size_t)s * nd + ne + a] = (T)u;
    }
  }
}

// k_pw_policy_bwd_nd: grid ceil(S / 256), thread = sample, all H steps backwards.  gpart [nwaves][NU][npar1] (ASSIGNED): per
// wave the sum over its 64 samples and all steps of the packed policy's gradient, per latent dZ [M][ne], dbeta [M], dls2 [ne],
// dvar, dmean (npar1 = M ne + M + ne + 2);  g_x0 [S][nx] (optional).  g_cost [H][S] f64.
// SEEDED (the _seeded entries with a seed on the states, or without the built-in cost): g_x [H][S][nx] f64, block h = d loss /
// d x_{h+1} (NULL: none); g_cost NULL: the built-in cost's term is skipped.  SEEDED = false: the built-in cost alone.
// MIXED: jacs is the LATENT Jacobian tape [H][S][Lg][nd] and g d = dt J_g^T (mixW^T g x_{h+1}) in two steps (mixW as in the head
// kernel: global memory, wave-uniform addresses); everything else is the unmixed sweep.
template <typename T, int NU, bool SEEDED, bool MIXED>
__global__ __launch_bounds__(256) void k_pw_policy_bwd_nd(MMComposeDims D, int S, int H, double dt, const T* __restrict__ xs,
                                                          const T* __restrict__ dins, const T* __restrict__ jacs,
                                                          const double* __restrict__ g_cost, const double* __restrict__ g_x,
                                                          const T* __restrict__ target, const T* __restrict__ precis,
                                                          const double* __restrict__ pZ, const double* __restrict__ pbeta,
                                                          const double* __restrict__ pls2, const double* __restrict__ pvar,
                                                          const double* __restrict__ pmean, int pM, MMHeadND hd,
                                                          double* __restrict__ gpart,
                                                          double* __restrict__ g_x0, int Lg,
                                                          const double* __restrict__ mixW) {
  extern __shared__ double sm[];
  const int nx = D.nx, ne = D.ne, nd = D.nd, blk = pM * ne + pM + ne, npar1 = blk + 2, npar = NU * npar1;
  double* pol = sm;
  double* tg = pol + NU * blk;
  double* W = tg + ne;
  double* acc = W + ne * ne;                               // [4 waves][NU][npar1]
  for (int i = threadIdx.x; i < ne; i += 256) tg[i] = (double)target[i];
  for (int i = threadIdx.x; i < ne * ne; i += 256) W[i] = (double)precis[i];
  for (int i = threadIdx.x; i < 4 * npar; i += 256) acc[i] = 0.0;
#pragma unroll
  for (int a = 0; a < NU; ++a)
    mmp_stage_policy<T>(pZ + (size_t)a * pM * ne, pbeta + (size_t)a * pM, pls2 + (size_t)a * ne, pM, ne, pol + a * blk);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s = blockIdx.x * 256 + threadIdx.x;
  const bool live = s < S;
  const int sr = live ? s : S - 1;                         // (idle lanes recompute the last sample with zero adjoints)
  double var[NU], mean[NU];
#pragma unroll
  for (int a = 0; a < NU; ++a) { var[a] = pvar[a]; mean[a] = pmean[a]; }
  double gx[MMC_NX];
  for (int i = 0; i < nx; ++i) gx[i] = 0.0;
  for (int h = H - 1; h >= 0; --h) {
    double x1[MMC_NX], e1[MMP_NE], ge[MMP_NE];
    // adjoint of x_{h+1}: what later steps left in gx, plus this step's cost of its encoding
    for (int i = 0; i < nx; ++i) x1[i] = (double)xs[((size_t)(h + 1) * S + sr) * nx + i];
    if (SEEDED && g_x) {                                     // seed block h belongs to x_{h+1}; idle lanes read a zero seed
      const double* sx = g_x + ((size_t)h * S + sr) * nx;
      for (int i = 0; i < nx; ++i) gx[i] += live ? sx[i] : 0.0;
    }
    if (!SEEDED || g_cost) {
      mmp_encode(D, x1, e1);
      mmp_cost(ne, e1, tg, W, ge);
      const double gc = live ? g_cost[(size_t)h * S + sr] : 0.0;
      for (int i = 0; i < ne; ++i) ge[i] *= gc;
      mmp_encode_bwd(D, x1, ge, gx);
    }
    // x_{h+1} = x_h + dt f(d_h):  g d = dt J^T g x_{h+1}
    double gd[MMP_NE + MMC_NU], e[MMP_NE];
    if (MIXED) {
      double gg[MMC_NX];                                     // adjoint of the latent sample: gg = mixW^T g x_{h+1}
      for (int l = 0; l < Lg; ++l) {
        double r = 0.0;
        for (int i = 0; i < nx; ++i) r = fma(mixW[i * Lg + l], gx[i], r);
        gg[l] = r;
      }
      const T* J = jacs + ((size_t)h * S + sr) * (size_t)Lg * nd;
      for (int k = 0; k < nd; ++k) {
        double r = 0.0;
        for (int l = 0; l < Lg; ++l) r = fma((double)J[l * nd + k], gg[l], r);
        gd[k] = dt * r;
      }
    } else {
      const T* J = jacs + ((size_t)h * S + sr) * (size_t)nx * nd;
      for (int k = 0; k < nd; ++k) {
        double r = 0.0;
        for (int i = 0; i < nx; ++i) r = fma((double)J[i * nd + k], gx[i], r);
        gd[k] = dt * r;
      }
    }
    const T* dn = dins + ((size_t)h * S + sr) * nd;
    for (int i = 0; i < ne; ++i) e[i] = (double)dn[i];
    for (int k = 0; k < ne; ++k) ge[k] = gd[k];
#pragma unroll
    for (int a = 0; a < NU; ++a) {
      const double* pa = pol + a * blk;
      const MMPwPolicy P{pa, pa + pM * ne, pa + pM * ne + pM, var[a], mean[a], pM};
      double* wacc = acc + (wv * NU + a) * npar1;
      // policy head: u_a = scale_a (Phi(fp) + shift_a);  g fp = g u_a scale_a phi(fp)
      const double fp = mmp_policy_mean(ne, P, e);
      const double gfp = gd[ne + a] * hd.scale[a] * 0.3989422804014327 * exp(-0.5 * fp * fp);
      // policy mean fp = sum_m beta_m var exp(-sum_k (e_k - z_mk)^2 / (2 ls2_k)) + c: parameters (wave sums) and input
      double gvar = 0.0, gls2[MMP_NE];
      for (int k = 0; k < ne; ++k) gls2[k] = 0.0;
      for (int m = 0; m < pM; ++m) {
        double r2 = 0.0, df[MMP_NE];
        for (int k = 0; k < ne; ++k) { df[k] = e[k] - P.Z[m * ne + k]; r2 = fma(df[k] * df[k], P.ils2[k], r2); }
        const double km = exp(-0.5 * r2);                    // k_m / var
        const double t = gfp * P.beta[m] * P.var * km;       // g fp * beta_m k_m
        gvar = fma(gfp * P.beta[m], km, gvar);
        const double sb = mmp_wave_sum(gfp * P.var * km);    // d / d beta_m
        if (lane == 0) wacc[pM * ne + m] += sb;
        for (int k = 0; k < ne; ++k) {
          const double tz = t * df[k] * P.ils2[k];           // d k_m / d z_mk = k_m (e_k - z_mk) / ls2_k = - d k_m / d e_k
          ge[k] -= tz;
          gls2[k] = fma(0.5 * tz * df[k], P.ils2[k], gls2[k]);   // d k_m / d ls2_k = k_m (e_k - z_mk)^2 / (2 ls2_k^2)
          const double sz = mmp_wave_sum(tz);
          if (lane == 0) wacc[m * ne + k] += sz;
        }
      }
      for (int k = 0; k < ne; ++k) {
        const double sl = mmp_wave_sum(gls2[k]);
        if (lane == 0) wacc[pM * ne + pM + k] += sl;
      }
      {
        const double sv = mmp_wave_sum(gvar), sc = mmp_wave_sum(gfp);
        if (lane == 0) { wacc[pM * ne + pM + ne] += sv; wacc[pM * ne + pM + ne + 1] += sc; }
      }
    }
    // d_h = (enc(x_h), u): adjoint of x_h = that of x_{h+1} (identity part of the Euler step) + the encoder's
    double x0[MMC_NX];
    for (int i = 0; i < nx; ++i) x0[i] = (double)xs[((size_t)h * S + sr) * nx + i];
    mmp_encode_bwd(D, x0, ge, gx);
  }
  if (g_x0 && live) for (int i = 0; i < nx; ++i) g_x0[(size_t)s * nx + i] = gx[i];
  __syncthreads();
  double* o = gpart + ((size_t)blockIdx.x * 4) * npar;
  for (int i = threadIdx.x; i < 4 * npar; i += 256) o[i] = acc[i];
}

// fixed-order sum of the per-wave slabs -> g_policy [npar]
static __global__ __launch_bounds__(256) void k_pw_grad_sum(const double* __restrict__ gpart, int nslab, int npar,
                                                            double* __restrict__ g_policy) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= npar) return;
  double sacc = 0.0;
  for (int w = 0; w < nslab; ++w) sacc += gpart[(size_t)w * npar + p];
  g_policy[p] = sacc;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
static inline size_t mmp_nd_head_lds(int pM, int ne, int nu) {
  return ((size_t)nu * (pM * ne + pM + ne) + ne + ne * ne + 8) * sizeof(double);
}
static inline size_t mmp_nd_bwd_lds(int pM, int ne, int nu) {
  return mmp_nd_head_lds(pM, ne, nu) + (size_t)4 * nu * (pM * ne + pM + ne + 2) * sizeof(double);
}

// everything that can be refused without a HIP call, in the order sizes -> dtype -> dimensions (forward: the drift's M and K
// are sizes too).  one_action: the one-action entries, whose contract differs in one answer -- na > 0 without active_dims is
// MM_E_DIM from mm_compose_dims (after sizes and dtype), where every other entry says MM_E_ARG first
static int mmp_nd_check(const MMPwRollout& P, bool forward, MMComposeDims& D) {
  const MMPwDrift& F = P.drift;
  if (F.S <= 0 || (forward && (F.M <= 0 || (!F.beta && F.K <= 0))) || P.H <= 0 || P.policy_M <= 0 ||
      (!P.one_action && P.na > 0 && !P.active_dims)) return MM_E_ARG;
  if (F.dtype != MM_F32 && F.dtype != MM_F64) return MM_E_DTYPE;
  const int rc = mm_compose_dims_nd(P.nx, P.na, P.nu, P.active_dims, D);
  if (rc) return rc;
  // nd_max: 8 for the _nd entries (the Jacobian pass over whole sample groups), 16 for the _wide ones (+ its half-group form)
  if (D.nd > P.nd_max || P.policy_M > MMP_POLICY_MMAX) return MM_E_DIM;
  return 0;
}

// the shapes the tape queries answer for (0 otherwise)
static bool mmp_tape_shape_ok(int S, int H, int nx, int na, int nu) {
  return S > 0 && H > 0 && nx > 0 && nx <= MMC_NX && na >= 0 && na <= MMC_NA && na <= nx && nu >= 1 && nu <= MMC_NU;
}
extern "C" size_t mm_pathwise_tape_bytes_nd(int S, int H, int nx, int na, int nu, int dtype, int with_jacobians) {
  if (!mmp_tape_shape_ok(S, H, nx, na, nu)) return 0;
  return mm_pw_tape_layout(S, H, nx, na, nu, dtype, with_jacobians).total;
}
extern "C" size_t mm_pathwise_tape_bytes(int S, int H, int nx, int na, int dtype, int with_jacobians) {
  return mm_pathwise_tape_bytes_nd(S, H, nx, na, 1, dtype, with_jacobians);
}
// the _mixed tape: the f slot [S][Lg] and the Jacobian block [H][S][Lg][nd] hold the LATENT sample and its Jacobian
extern "C" size_t mm_pathwise_tape_bytes_mixed(int S, int H, int nx, int na, int nu, int Lg, int dtype, int with_jacobians) {
  if (!mmp_tape_shape_ok(S, H, nx, na, nu) || Lg < 1 || Lg > nx) return 0;
  return mm_pw_tape_layout_latent(S, H, nx, na, nu, Lg, dtype, with_jacobians).total;
}

#define MMP_ND_DISPATCH(nu_, M_)                                                       \
  switch (nu_) {                                                                       \
    case 1: M_(1); break;                                                              \
    case 2: M_(2); break;                                                              \
    case 3: M_(3); break;                                                              \
    default: M_(4); break;                                                             \
  }

// the head's per-action constants as the kernels take them (by value; zero beyond nu)
static MMHeadND mmp_head_constants(int nu, const double* head_scale, const double* head_shift) {
  MMHeadND hd;
  for (int a = 0; a < MMC_NU; ++a) { hd.scale[a] = a < nu ? head_scale[a] : 0.0; hd.shift[a] = a < nu ? head_shift[a] : 0.0; }
  return hd;
}

template <typename T>
static int mmp_nd_rollout_t(const MMPwRollout& P, const MMComposeDims& D, const MMModelLayout& pl, const MMPwTapeLayout& tl,
                            const T* x0, T* cost, char* tape) {
  // drift.beta != NULL: the _mean entry -- the drift is its posterior MEAN, one shared weight vector per latent in place of the
  // stream (mm_pathwise_mean.hip: same f and Jacobian slots)
  // Lg > 0: the _mixed entries -- the stream pass runs with Lg latents and no latent mean straight into the tape's (latent-sized)
  // f and Jacobian slots, the head kernel mixes
  const int nx = D.nx, ne = D.ne, nd = D.nd, nu = P.nu, S = P.drift.S, H = P.H, policy_M = P.policy_M;
  const int Lg = P.mixed ? P.Lg : 0, Lf = Lg > 0 ? Lg : nx;           // (Lg = 0: what the launches take for "no mixing")
  const double dt = P.dt, *mix_W = P.mix_W, *mix_c = P.mix_c;
  const T *target = (const T*)P.target, *precis = (const T*)P.precis;
  const char* pp = (const char*)P.policy_packed;
  const MMHeadND hd = mmp_head_constants(nu, P.head_scale, P.head_shift);
  hipStream_t s = (hipStream_t)P.stream;
  MMPwDrift drift = P.drift;                                            // one step's pass: Lf latents on the nd drift inputs
  drift.L = Lf; drift.d = nd;
  if (Lg > 0) drift.mean_c = nullptr;
  T* xs = (T*)(tape + tl.x); T* dins = (T*)(tape + tl.din); T* f = (T*)(tape + tl.f);
  T* jac = tl.jac != tl.total ? (T*)(tape + tl.jac) : nullptr;
  hipError_t e = hipMemcpyAsync(xs, x0, (size_t)S * nx * sizeof(T), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return (int)e;
  const size_t lds = mmp_nd_head_lds(policy_M, ne, nu);
  const dim3 grid((S + 255) / 256);
  for (int h = 0; h <= H; ++h) {
#define MMP_HEAD_(NU_, MIXED_)                                                                                                   \
    if (h == 0 && lds > 64 * 1024) {   /* nu >= 3 policies on wide encodings: up to 108 KB at M = 256 */                          \
      hipError_t ea = hipFuncSetAttribute((const void*)k_pw_head_nd<T, NU_, MIXED_>,                                             \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                 \
      if (ea != hipSuccess) return (int)ea;                                                                                      \
    }                                                                                                                            \
    hipLaunchKernelGGL((k_pw_head_nd<T, NU_, MIXED_>), grid, dim3(256), lds, s, D, S, h, H, dt,                                  \
                       h > 0 ? xs + (size_t)(h - 1) * S * nx : (const T*)nullptr, (const T*)f, xs + (size_t)h * S * nx,          \
                       h < H ? dins + (size_t)h * S * nd : (T*)nullptr, cost, target, precis, (const double*)(pp + pl.Z64),      \
                       (const double*)(pp + pl.beta64), (const double*)(pp + pl.ls2), (const double*)(pp + pl.var),              \
                       (const double*)(pp + pl.meanc), policy_M, hd, Lg, mix_W, mix_c)
#define MMP_HEAD(NU_) if (Lg > 0) { MMP_HEAD_(NU_, true); } else { MMP_HEAD_(NU_, false); }
    MMP_ND_DISPATCH(nu, MMP_HEAD)
#undef MMP_HEAD
#undef MMP_HEAD_
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (h == H) break;
    MMPwOut o; o.f = f; o.jac = jac ? jac + (size_t)h * S * Lf * nd : nullptr;
    const int rc = mm_pw_drift_eval(drift, dins + (size_t)h * S * nd, o, s);
    if (rc) return rc;
  }
  return 0;
}

// the forward entries: one action (nd_max = 8, nu = 1, one_action), _nd (nd_max = 8), _wide (nd_max = 16), _mixed (nd_max = 16,
// mixed: Lg, mix_W, mix_c), _kern (drift.kernel: the drift's family) and _mean (drift.beta) are this function
static int mmp_nd_rollout(const MMPwRollout& P, const void* x0, void* cost, void* tape, size_t tape_bytes, int with_jacobians) {
  const MMPwDrift& F = P.drift;
  if (F.kernel < 0 || F.kernel >= MM_PW_KERNELS) return MM_E_ARG;         // the drift's kernel family (mm_pathwise_eval_kern)
  MMComposeDims D;
  int rc = mmp_nd_check(P, true, D);
  if (rc) return rc;
  if (P.mixed && (P.Lg < 1 || P.Lg > P.nx)) return MM_E_DIM;
  if ((!F.beta && (!F.omega_t || !F.phase || !F.prior_scale || !F.wb)) || !F.zs_t || !F.hz || !F.x_scale || !F.variance ||
      !P.policy_packed || !P.head_scale || !P.head_shift || !P.target || !P.precis || !x0 || !cost || !tape ||
      (P.mixed && !P.mix_W)) return MM_E_ARG;
  const MMPwTapeLayout tl = mm_pw_tape_layout_latent(F.S, P.H, P.nx, P.na, P.nu, P.mixed ? P.Lg : P.nx, F.dtype, with_jacobians);
  if (tape_bytes < tl.total) return MM_E_WORKSPACE;
  const MMModelLayout pl = mm_model_layout(P.nu, P.policy_M, D.ne, MM_F64, 1);   // the f64 blocks precede the T blocks in every pack
  if (P.policy_bytes < pl.Zc64) return MM_E_WORKSPACE;
  if (F.dtype == MM_F64) return mmp_nd_rollout_t<double>(P, D, pl, tl, (const double*)x0, (double*)cost, (char*)tape);
  return mmp_nd_rollout_t<float>(P, D, pl, tl, (const float*)x0, (float*)cost, (char*)tape);
}

// What the entries' argument lists name alike, into the fields of the same names (nothing here goes by position).
// MMP_ROLLOUT_FIELDS: every entry; MMP_STREAM_FIELDS: the forward entries of a sampled drift.
#define MMP_ROLLOUT_FIELDS(P_)                                                                                                   \
  MMPwRollout P_;                                                                                                                \
  P_.drift.S = S; P_.drift.dtype = dtype; P_.H = H; P_.dt = dt; P_.nx = nx; P_.na = na; P_.active_dims = active_dims;            \
  P_.policy_packed = policy_packed; P_.policy_bytes = policy_bytes; P_.policy_M = policy_M; P_.target = target;                  \
  P_.precis = precis; P_.stream = stream
#define MMP_STREAM_FIELDS(P_)                                                                                                    \
  P_.drift.M = M; P_.drift.K = K; P_.drift.omega_t = omega_t; P_.drift.phase = phase; P_.drift.zs_t = zs_t; P_.drift.hz = hz;    \
  P_.drift.x_scale = x_scale; P_.drift.prior_scale = prior_scale; P_.drift.variance = variance; P_.drift.mean_c = mean_c;        \
  P_.drift.wb = wb
#define MMP_HEAD_FIELDS(P_) P_.nu = nu; P_.head_scale = head_scale; P_.head_shift = head_shift

#define MMP_ROLLOUT_ENTRY(name_, nd_max_)                                                                                          \
  extern "C" int name_(int S, int M, int K, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims, int nu,      \
                       const void* omega_t, const void* phase, const void* zs_t, const void* hz, const double* x_scale,          \
                       const double* prior_scale, const double* variance, const double* mean_c, const void* wb,                  \
                       const void* policy_packed, size_t policy_bytes, int policy_M, const double* head_scale,                   \
                       const double* head_shift, const void* target, const void* precis, const void* x0, void* cost, void* tape, \
                       size_t tape_bytes, int with_jacobians, void* stream) {                                                    \
    MMP_ROLLOUT_FIELDS(P); MMP_STREAM_FIELDS(P); MMP_HEAD_FIELDS(P);                                                             \
    P.nd_max = nd_max_;                                                                                                          \
    return mmp_nd_rollout(P, x0, cost, tape, tape_bytes, with_jacobians);                                                        \
  }
MMP_ROLLOUT_ENTRY(mm_pathwise_policy_rollout_nd, 8)
MMP_ROLLOUT_ENTRY(mm_pathwise_policy_rollout_wide, 16)
#undef MMP_ROLLOUT_ENTRY

// one action: the _nd entry with nu = 1 and the head constants by value (g_policy [npar] is the _nd one's [1][npar])
extern "C" int mm_pathwise_policy_rollout(int S, int M, int K, int dtype, int H, double dt, int nx, int na,
                                          const int32_t* active_dims, const void* omega_t, const void* phase, const void* zs_t,
                                          const void* hz, const double* x_scale, const double* prior_scale,
                                          const double* variance, const double* mean_c, const void* wb,
                                          const void* policy_packed, size_t policy_bytes, int policy_M, double head_scale,
                                          double head_shift, const void* target, const void* precis, const void* x0, void* cost,
                                          void* tape, size_t tape_bytes, int with_jacobians, void* stream) {
  MMP_ROLLOUT_FIELDS(P); MMP_STREAM_FIELDS(P);
  P.nu = 1; P.head_scale = &head_scale; P.head_shift = &head_shift; P.one_action = true;       // (nd_max: 8)
  return mmp_nd_rollout(P, x0, cost, tape, tape_bytes, with_jacobians);
}

// a coregionalised drift: the paths' operands are those of Lg latents, mean_c is not read (the constant is mix_c)
extern "C" int mm_pathwise_policy_rollout_mixed(int S, int M, int K, int dtype, int H, double dt, int nx, int na,
                                                const int32_t* active_dims, int nu, const void* omega_t, const void* phase,
                                                const void* zs_t, const void* hz, const double* x_scale, const double* prior_scale,
                                                const double* variance, const double* mean_c, const void* wb,
                                                const void* policy_packed, size_t policy_bytes, int policy_M,
                                                const double* head_scale, const double* head_shift, const void* target,
                                                const void* precis, const void* x0, void* cost, void* tape, size_t tape_bytes,
                                                int with_jacobians, void* stream, int Lg, const double* mix_W,
                                                const double* mix_c) {
  MMP_ROLLOUT_FIELDS(P); MMP_STREAM_FIELDS(P); MMP_HEAD_FIELDS(P);
  P.nd_max = 16; P.mixed = true; P.Lg = Lg; P.mix_W = mix_W; P.mix_c = mix_c;
  return mmp_nd_rollout(P, x0, cost, tape, tape_bytes, with_jacobians);
}

// the one forward entry for a drift of any kernel family (kernel: 0 SquaredExponential, 1 Matern-3/2, 2 Matern-5/2): the argument
// list of the _mixed entry plus kernel; Lg = 0 / mix_W = NULL: no mixing (then the _wide entry: nd <= 16, 1 .. 4 actions).  The
// tape layout does not depend on the family, so the reverse sweeps below are used as they are.
extern "C" int mm_pathwise_policy_rollout_kern(int S, int M, int K, int dtype, int H, double dt, int nx, int na,
                                               const int32_t* active_dims, int nu, const void* omega_t, const void* phase,
                                               const void* zs_t, const void* hz, const double* x_scale, const double* prior_scale,
                                               const double* variance, const double* mean_c, const void* wb,
                                               const void* policy_packed, size_t policy_bytes, int policy_M,
                                               const double* head_scale, const double* head_shift, const void* target,
                                               const void* precis, const void* x0, void* cost, void* tape, size_t tape_bytes,
                                               int with_jacobians, void* stream, int Lg, const double* mix_W,
                                               const double* mix_c, int kernel) {
  if (kernel < 0 || kernel >= MM_PW_KERNELS) return MM_E_ARG;
  MMP_ROLLOUT_FIELDS(P); MMP_STREAM_FIELDS(P); MMP_HEAD_FIELDS(P);
  P.drift.kernel = kernel;
  P.nd_max = 16; P.mixed = Lg != 0 || mix_W != nullptr; P.Lg = Lg; P.mix_W = mix_W; P.mix_c = P.mixed ? mix_c : nullptr;
  return mmp_nd_rollout(P, x0, cost, tape, tape_bytes, with_jacobians);
}

// the MEAN of the drift in place of its sample paths (the reference's model_uncertainty=False: the drift in a KernelRegressor):
// the _kern entry's argument list without (K, omega_t, phase, prior_scale, wb) and with beta [L][M] f64 = Kuu^-1 u after mean_c
// (L = nx, or Lg with mixing).  Same tape, same reverse sweeps; M needs no padding.
extern "C" int mm_pathwise_policy_rollout_mean(int S, int M, int dtype, int H, double dt, int nx, int na,
                                               const int32_t* active_dims, int nu, const void* zs_t, const void* hz,
                                               const double* x_scale, const double* variance, const double* mean_c,
                                               const double* beta, const void* policy_packed, size_t policy_bytes, int policy_M,
                                               const double* head_scale, const double* head_shift, const void* target,
                                               const void* precis, const void* x0, void* cost, void* tape, size_t tape_bytes,
                                               int with_jacobians, void* stream, int Lg, const double* mix_W,
                                               const double* mix_c, int kernel) {
  if (kernel < 0 || kernel >= MM_PW_KERNELS || !beta) return MM_E_ARG;
  MMP_ROLLOUT_FIELDS(P); MMP_HEAD_FIELDS(P);
  P.drift.M = M; P.drift.zs_t = zs_t; P.drift.hz = hz; P.drift.x_scale = x_scale; P.drift.variance = variance;
  P.drift.mean_c = mean_c; P.drift.beta = beta; P.drift.kernel = kernel;
  P.nd_max = 16; P.mixed = Lg != 0 || mix_W != nullptr; P.Lg = Lg; P.mix_W = mix_W; P.mix_c = P.mixed ? mix_c : nullptr;
  return mmp_nd_rollout(P, x0, cost, tape, tape_bytes, with_jacobians);
}
#undef MMP_STREAM_FIELDS

// 0: a shape the reverse sweep does not take (see the LDS bound at the top of this file)
static size_t mmp_nd_scratch_bytes(int nd_max, int S, int policy_M, int ne, int nu) {
  if (S <= 0 || policy_M <= 0 || policy_M > MMP_POLICY_MMAX || ne <= 0 || nu < 1 || nu > MMC_NU || ne + nu > nd_max) return 0;
  if (mmp_nd_bwd_lds(policy_M, ne, nu) > MMP_ND_LDS_MAX) return 0;
  return (size_t)((S + 255) / 256) * 4 * (size_t)nu * (size_t)(policy_M * ne + policy_M + ne + 2) * sizeof(double);
}
// (the one-action query has no upper bounds: it answers for shapes the entries refuse)
extern "C" size_t mm_pathwise_backward_scratch_bytes(int S, int policy_M, int ne) {
  if (S <= 0 || policy_M <= 0 || ne <= 0) return 0;
  return (size_t)((S + 255) / 256) * 4 * (size_t)(policy_M * ne + policy_M + ne + 2) * sizeof(double);
}
extern "C" size_t mm_pathwise_backward_scratch_bytes_nd(int S, int policy_M, int ne, int nu) {
  return mmp_nd_scratch_bytes(8, S, policy_M, ne, nu);
}
extern "C" size_t mm_pathwise_backward_scratch_bytes_wide(int S, int policy_M, int ne, int nu) {
  return mmp_nd_scratch_bytes(16, S, policy_M, ne, nu);
}

// the backward entries: one action (nd_max = 8, nu = 1, one_action), _nd (nd_max = 8) and _wide (nd_max = 16), unseeded (g_cost
// required, g_x = nullptr) and _seeded (seeded_entry: either seed may be NULL, not both), are this function; so is _mixed
// (nd_max = 16, seeded_entry, mixed: Lg and mix_W)
static int mmp_nd_backward(const MMPwRollout& P, const void* tape, size_t tape_bytes, const void* g_cost, const void* g_x,
                           void* g_policy, void* g_x0, void* scratch, size_t scratch_bytes) {
  const int S = P.drift.S, dtype = P.drift.dtype, H = P.H, nu = P.nu, policy_M = P.policy_M, Lg = P.Lg;
  const bool mixed = P.mixed;
  const double dt = P.dt, *mix_W = P.mix_W;
  const void *target = P.target, *precis = P.precis;
  MMComposeDims D;
  int rc = mmp_nd_check(P, false, D);
  if (rc) return rc;
  if (mixed && (Lg < 1 || Lg > P.nx)) return MM_E_DIM;
  if (!P.policy_packed || !P.head_scale || !P.head_shift || !target || !precis || !tape ||
      (P.seeded_entry ? (!g_cost && !g_x) : !g_cost) || !g_policy || !scratch || (mixed && !mix_W))
    return MM_E_ARG;
  const int ne = D.ne, npar = nu * (policy_M * ne + policy_M + ne + 2);
  const size_t lds = mmp_nd_bwd_lds(policy_M, ne, nu);
  if (lds > MMP_ND_LDS_MAX) return MM_E_DIM;
  const MMPwTapeLayout tl = mm_pw_tape_layout_latent(S, H, P.nx, P.na, nu, mixed ? Lg : P.nx, dtype, 1);
  if (tape_bytes < tl.total) return MM_E_WORKSPACE;
  if (scratch_bytes < mmp_nd_scratch_bytes(P.nd_max, S, policy_M, ne, nu)) return MM_E_WORKSPACE;
  const MMModelLayout pl = mm_model_layout(nu, policy_M, ne, MM_F64, 1);
  if (P.policy_bytes < pl.Zc64) return MM_E_WORKSPACE;
  const MMHeadND hd = mmp_head_constants(nu, P.head_scale, P.head_shift);
  const char* pp = (const char*)P.policy_packed; const char* tp = (const char*)tape;
  hipStream_t s = (hipStream_t)P.stream;
  const dim3 grid((S + 255) / 256);
  // (the built-in cost alone: the unseeded instantiation, whichever entry was called -- same arithmetic, bit-equal outputs)
  const bool seeded = g_x != nullptr || g_cost == nullptr;
#define MMP_BWD(T_, NU_, SEEDED_, MIXED_)                                                                                         \
  do {                                                                                                                          \
    if (lds > 64 * 1024) {                                                                                                      \
      hipError_t ea = hipFuncSetAttribute((const void*)k_pw_policy_bwd_nd<T_, NU_, SEEDED_, MIXED_>,                             \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                \
      if (ea != hipSuccess) return (int)ea;                                                                                     \
    }                                                                                                                           \
    hipLaunchKernelGGL((k_pw_policy_bwd_nd<T_, NU_, SEEDED_, MIXED_>), grid, dim3(256), lds, s, D, S, H, dt,                     \
                       (const T_*)(tp + tl.x), (const T_*)(tp + tl.din), (const T_*)(tp + tl.jac), (const double*)g_cost,       \
                       (const double*)g_x, (const T_*)target, (const T_*)precis, (const double*)(pp + pl.Z64),                  \
                       (const double*)(pp + pl.beta64), (const double*)(pp + pl.ls2), (const double*)(pp + pl.var),             \
                       (const double*)(pp + pl.meanc), policy_M, hd, (double*)scratch, (double*)g_x0, Lg, mix_W);               \
  } while (0)
#define MMP_BWD_T(T_, NU_)                                                                                                       \
  if (mixed) { if (seeded) MMP_BWD(T_, NU_, true, true); else MMP_BWD(T_, NU_, false, true); }                                   \
  else { if (seeded) MMP_BWD(T_, NU_, true, false); else MMP_BWD(T_, NU_, false, false); }
#define MMP_BWD_F64(NU_) MMP_BWD_T(double, NU_)
#define MMP_BWD_F32(NU_) MMP_BWD_T(float, NU_)
  if (dtype == MM_F64) { MMP_ND_DISPATCH(nu, MMP_BWD_F64) } else { MMP_ND_DISPATCH(nu, MMP_BWD_F32) }
#undef MMP_BWD_F64
#undef MMP_BWD_F32
#undef MMP_BWD_T
#undef MMP_BWD
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_pw_grad_sum, dim3((npar + 255) / 256), dim3(256), 0, s, (const double*)scratch, (int)grid.x * 4, npar,
                     (double*)g_policy);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

#define MMP_BACKWARD_ENTRY(name_, nd_max_)                                                                                         \
  extern "C" int name_(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims, int nu,                    \
                       const void* policy_packed, size_t policy_bytes, int policy_M, const double* head_scale,                   \
                       const double* head_shift, const void* target, const void* precis, const void* tape, size_t tape_bytes,    \
                       const void* g_cost, void* g_policy, void* g_x0, void* scratch, size_t scratch_bytes, void* stream) {      \
    MMP_ROLLOUT_FIELDS(P); MMP_HEAD_FIELDS(P);                                                                                   \
    P.nd_max = nd_max_;                                                                                                          \
    return mmp_nd_backward(P, tape, tape_bytes, g_cost, nullptr, g_policy, g_x0, scratch, scratch_bytes);                        \
  }                                                                                                                             \
  extern "C" int name_##_seeded(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims, int nu,          \
                                const void* policy_packed, size_t policy_bytes, int policy_M, const double* head_scale,          \
                                const double* head_shift, const void* target, const void* precis, const void* tape,              \
                                size_t tape_bytes, const void* g_cost, const void* g_x, void* g_policy, void* g_x0,              \
                                void* scratch, size_t scratch_bytes, void* stream) {                                            \
    MMP_ROLLOUT_FIELDS(P); MMP_HEAD_FIELDS(P);                                                                                   \
    P.nd_max = nd_max_; P.seeded_entry = true;                                                                                   \
    return mmp_nd_backward(P, tape, tape_bytes, g_cost, g_x, g_policy, g_x0, scratch, scratch_bytes);                            \
  }
MMP_BACKWARD_ENTRY(mm_pathwise_policy_rollout_backward_nd, 8)
MMP_BACKWARD_ENTRY(mm_pathwise_policy_rollout_backward_wide, 16)
#undef MMP_BACKWARD_ENTRY

// one action: the _nd entries with nu = 1 and the head constants by value
extern "C" int mm_pathwise_policy_rollout_backward(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                                   const void* policy_packed, size_t policy_bytes, int policy_M,
                                                   double head_scale, double head_shift, const void* target, const void* precis,
                                                   const void* tape, size_t tape_bytes, const void* g_cost, void* g_policy,
                                                   void* g_x0, void* scratch, size_t scratch_bytes, void* stream) {
  MMP_ROLLOUT_FIELDS(P);
  P.nu = 1; P.head_scale = &head_scale; P.head_shift = &head_shift; P.one_action = true;       // (nd_max: 8)
  return mmp_nd_backward(P, tape, tape_bytes, g_cost, nullptr, g_policy, g_x0, scratch, scratch_bytes);
}
extern "C" int mm_pathwise_policy_rollout_backward_seeded(int S, int dtype, int H, double dt, int nx, int na,
                                                          const int32_t* active_dims, const void* policy_packed,
                                                          size_t policy_bytes, int policy_M, double head_scale, double head_shift,
                                                          const void* target, const void* precis, const void* tape,
                                                          size_t tape_bytes, const void* g_cost, const void* g_x, void* g_policy,
                                                          void* g_x0, void* scratch, size_t scratch_bytes, void* stream) {
  MMP_ROLLOUT_FIELDS(P);
  P.nu = 1; P.head_scale = &head_scale; P.head_shift = &head_shift; P.one_action = true; P.seeded_entry = true;
  return mmp_nd_backward(P, tape, tape_bytes, g_cost, g_x, g_policy, g_x0, scratch, scratch_bytes);
}

// the reverse sweep of the _mixed rollout: the _seeded signature (either of g_cost and g_x may be NULL, not both) + the mixing
extern "C" int mm_pathwise_policy_rollout_backward_mixed(int S, int dtype, int H, double dt, int nx, int na,
                                                         const int32_t* active_dims, int nu, const void* policy_packed,
                                                         size_t policy_bytes, int policy_M, const double* head_scale,
                                                         const double* head_shift, const void* target, const void* precis,
                                                         const void* tape, size_t tape_bytes, const void* g_cost, const void* g_x,
                                                         void* g_policy, void* g_x0, void* scratch, size_t scratch_bytes,
                                                         void* stream, int Lg, const double* mix_W) {
  MMP_ROLLOUT_FIELDS(P); MMP_HEAD_FIELDS(P);
  P.nd_max = 16; P.seeded_entry = true; P.mixed = true; P.Lg = Lg; P.mix_W = mix_W;
  return mmp_nd_backward(P, tape, tape_bytes, g_cost, g_x, g_policy, g_x0, scratch, scratch_bytes);
}
#undef MMP_HEAD_FIELDS
#undef MMP_ROLLOUT_FIELDS
