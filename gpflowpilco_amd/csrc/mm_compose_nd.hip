// The composed rollout (mm_compose.hip) for policies with SEVERAL actions (gfx950): nu policy latents, u_j = scale_j (Phi(f_j(e)) +
// shift_j), d = joint(e, u) with nd = ne + nu (the double pendulum's two torques, envs/double_pendulum.py:40).
//
// What changes against the one-action step is the NormalCDF head (gpflow_pilco/moment_matching/bijectors.py:48-69, n-D branch):
// E[Phi(f_i) Phi(f_j)] = Phi2(z_i, z_j; rho_ij) is a bivariate normal CDF for i != j.  Here it is Plackett's integral
//     Phi2(h, k; rho) = Phi(h) Phi(k) + 1/(2 pi) int_0^{asin rho} exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)) dt
// by Gauss-Legendre on four equal 48-point panels -- the quadrature of gpflowpilco_amd/special.py:bvn_cdf, lanes over nodes -- and the
// diagonal keeps Owen's T (the one-action head's quadrature).  Per step:
//   mm_moment_match(policy, L = nu, full output covariance, no model uncertainty: a KernelRegressor has none)
//   k_compose_head_nd : the nu + nu (nu - 1) / 2 quadratures, Scale / Shift, the chain rule (gaussian.py:66-83) and
//                       GaussianMatch.joint (gaussian.py:53-63), one workgroup per batch element, f64 in LDS
//   mm_moment_match(drift)
//   k_compose_tail_nd : forward_sde.py:105-131 with nu policy columns + solvers.py:110-135, then the shared encoding and
//                       expected-cost bodies (mm_compose_dev.h, mm_cost.h), one launch
// mm_rollout_composed_taped_nd is the same rollout writing into a tape (mm_tape_layout_nd) that the reverse sweep of
// mm_compose_bwd_nd.hip reads: step h works in tape slot h, the states x_0 .. x_H go to the state block, and -- by the rules of
// mm_tape_layout_slots (mm_compose.h), as for one action -- the drift match runs in the tape's own workspace of the step where H of
// them fit, and leaves the sums of its backward sweeps there too (mm_moment_match_with_sums_impl) where those fit as well.
// The policy match's workspace is not kept: the reverse sweep recomputes the policy from (me, See).
// The _mixed entries at the end of the file run the same rollout for a COREGIONALISED drift (Lg <= nx latents, f = W g + c): the
// drift's match with L = Lg writes to a staging block and k_compose_mix_nd (mm_mix.h), one more launch per step, fills the slot's
// df1 / dSff / dcross; everything else is shared, and without mixing operands nothing differs from before.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mm_common.h"
#include "mm_cost.h"
#include "mm_compose.h"
#include "mm_compose_dev.h"
#include "mm_mix.h"

#define MMC_BVN_PANELS 4

template <typename T>
__global__ __launch_bounds__(64) void k_compose_encode_nd(MMComposeDims D, const T* __restrict__ mx, const T* __restrict__ Sxx,
                                                          T* __restrict__ me, T* __restrict__ See, double* __restrict__ Sxe) {
  mmc_encode_body<T>(D, mx, Sxx, me, See, Sxe, (int)blockIdx.x, (int)threadIdx.x);
}

// ---------------------------------------------------------------------------------------------
// k_compose_head_nd: policy GP output (f1 [nu], Sff [nu][nu], pre-inverted cross [ne][nu]) -> moments of u and of d = (e, u)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_compose_head_nd(MMComposeDims D, MMHeadND hd, const T* __restrict__ me,
                                                         const T* __restrict__ See, const T* __restrict__ pf1,
                                                         const T* __restrict__ pSff, const T* __restrict__ pcross,
                                                         T* __restrict__ md, T* __restrict__ Sdd, double* __restrict__ cpol) {
  const int b = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int ne = D.ne, nd = D.nd, nu = nd - ne;
  __shared__ double Sf[MMC_NU * MMC_NU], y2[MMC_NU * MMC_NU];
  __shared__ double zf[MMC_NU], vf[MMC_NU], isq[MMC_NU], y1[MMC_NU], hpre[MMC_NU], muu[MMC_NU];
  __shared__ double cp[MMC_ND * MMC_NU], Seu[MMC_ND * MMC_NU];
  if (tid < nu * nu) Sf[tid] = (double)pSff[(size_t)b * nu * nu + tid];
  __syncthreads();
  if (tid < nu) {                              // bijectors.py:48-56
    double v = Sf[tid * nu + tid];
    v = v > 0.0 ? v : 0.0;                     // variance of the regressor's mean under x ~ N: >= 0 up to rounding
    const double is = rsqrt(v + 1.0), z = is * (double)pf1[(size_t)b * nu + tid];
    vf[tid] = v; isq[tid] = is; zf[tid] = z;
    y1[tid] = 0.5 * erfc(-z * 0.70710678118654752440);
    hpre[tid] = is * 0.39894228040143267794 * exp(-0.5 * z * z) * hd.scale[tid];      // Var(f_j)^-1 Cov(f_j, u_j)
  }
  __syncthreads();
  // the second moments E[Phi(f_i) Phi(f_j)], one quadrature per wave and turn: items 0 .. nu - 1 the diagonal (Owen's T),
  // then the pairs i < j (Plackett)
  const int nit = nu + nu * (nu - 1) / 2;
  for (int it = wv; it < nit; it += 4) {
    if (it < nu) {
      const double z = zf[it], aa = rsqrt(1.0 + 2.0 * vf[it]);          // T(z, a), a in (0, 1]
      double part = 0.0;
      if (lane < 48) {
        const double t = 0.5 * aa * (MM_GL48_X[lane] + 1.0);
        part = MM_GL48_W[lane] * exp(-0.5 * z * z * (1.0 + t * t)) / (1.0 + t * t);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
      const double owen = 0.5 * aa * part * 0.15915494309189533577;     // / (2 pi)
      if (lane == 0) y2[it * nu + it] = y1[it] - 2.0 * owen;
    } else {
      int i = 0, r = it - nu;
      while (r >= nu - 1 - i) { r -= nu - 1 - i; ++i; }
      const int j = i + 1 + r;
      double rho = Sf[i * nu + j] * isq[i] * isq[j];
      rho = fmin(fmax(rho, -1.0), 1.0);
      const double a = asin(rho), h = zf[i], k = zf[j], hk2 = h * h + k * k, hk = 2.0 * h * k;
      double part = 0.0;
      if (lane < 48) {
        const double x01 = 0.5 * (MM_GL48_X[lane] + 1.0);
#pragma unroll
        for (int p = 0; p < MMC_BVN_PANELS; ++p) {
          double st, ct;
          sincos(a * ((p + x01) * (1.0 / MMC_BVN_PANELS)), &st, &ct);
          part += exp(-(hk2 - hk * st) / (2.0 * ct * ct));
        }
        part *= MM_GL48_W[lane];
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
      double v = y1[i] * y1[j] + a * (0.5 / MMC_BVN_PANELS) * part * 0.15915494309189533577;
      // Frechet bounds of a joint probability with these marginals (special.py does the same)
      v = fmin(fmax(v, fmax(y1[i] + y1[j] - 1.0, 0.0)), fmin(y1[i], y1[j]));
      if (lane == 0) { y2[i * nu + j] = v; y2[j * nu + i] = v; }
    }
  }
  if (tid < nu) muu[tid] = hd.scale[tid] * (y1[tid] + hd.shift[tid]);
  // chain rule (gaussian.py:66-83): Cov(e,e)^-1 Cov(e, u_j) = cross_pre(GP)[:, j] * hpre_j
  for (int idx = tid; idx < ne * nu; idx += 256) {
    const int j = idx % nu;
    const double v = (double)pcross[(size_t)b * ne * nu + idx] * hpre[j];
    cp[idx] = v;
    cpol[(size_t)b * ne * nu + idx] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < ne * nu; idx += 256) {
    const int k = idx / nu, j = idx - k * nu;
    double s = 0.0;
    for (int l = 0; l < ne; ++l) s = fma((double)See[((size_t)b * ne + k) * ne + l], cp[l * nu + j], s);
    Seu[idx] = s;
  }
  __syncthreads();
  T* mdb = md + (size_t)b * nd;
  T* Sdb = Sdd + (size_t)b * nd * nd;
  for (int k = tid; k < nd; k += 256) mdb[k] = k < ne ? me[(size_t)b * ne + k] : (T)muu[k - ne];
  for (int idx = tid; idx < nd * nd; idx += 256) {           // gaussian.py:53-63
    const int i = idx / nd, j = idx - i * nd;
    double v;
    if (i < ne && j < ne) v = (double)See[((size_t)b * ne + i) * ne + j];
    else if (i < ne) v = Seu[i * nu + (j - ne)];
    else if (j < ne) v = Seu[j * nu + (i - ne)];
    else {
      const int p = i - ne, q = j - ne;
      v = hd.scale[p] * hd.scale[q] * (y2[p * nu + q] - y1[p] * y1[q]);
    }
    Sdb[idx] = (T)v;
  }
}

// ---------------------------------------------------------------------------------------------
// mmc_step_body_nd: mmc_step_body (mm_compose.hip) with nu policy columns -- Cov(a, u) = Cov(a, e) cpol [ne][nu]
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void mmc_step_body_nd(const MMComposeDims& D, double dt, const double* Sxe, const double* cpol,
                                                 const T* Sdd, const T* df1, const T* dSff, const T* dcross, T* mx, T* Sxx,
                                                 T* traj_mu, T* traj_S, int b, int lane) {
  const int nx = D.nx, na = D.na, ne = D.ne, nd = D.nd, n2 = 2 * na, nu = nd - ne;
  __shared__ double Sxd[MMC_NX * MMC_ND], Sxf[MMC_NX * MMC_NX];
  const double* Sxeb = Sxe + (size_t)b * nx * ne;
  const double* cp = cpol + (size_t)b * ne * nu;
  const T* Sdb = Sdd + (size_t)b * nd * nd;
  // Cov(x, d): rows of the encoded dims = [Sae, Sae cpol], rows of the other dims = the corresponding rows of Cov(d, d)
  // (forward_sde.py:118-127: Sbd = Sdd[nd - nb - nu : nd - nu])
  for (int idx = lane; idx < nx * nd; idx += 64) {
    const int r = idx / nd, k = idx - r * nd;
    const int sl = D.slot[r];
    double v;
    if (sl < na) {
      if (k < ne) v = Sxeb[r * ne + k];
      else {
        double s = 0.0;
        for (int l = 0; l < ne; ++l) s = fma(Sxeb[r * ne + l], cp[l * nu + (k - ne)], s);
        v = s;
      }
    } else {
      v = (double)Sdb[(n2 + (sl - na)) * nd + k];
    }
    Sxd[idx] = v;
  }
  __syncthreads();
  const T* dc = dcross + (size_t)b * nd * nx;
  for (int idx = lane; idx < nx * nx; idx += 64) {           // Cov(x, f) = Cov(x, d) Cov(d,d)^-1 Cov(d, f)
    const int r = idx / nx, c = idx - r * nx;
    double s = 0.0;
    for (int k = 0; k < nd; ++k) s = fma(Sxd[r * nd + k], (double)dc[k * nx + c], s);
    Sxf[idx] = s;
  }
  __syncthreads();
  for (int idx = lane; idx < nx * nx; idx += 64) {           // solvers.py:110-135
    const int r = idx / nx, c = idx - r * nx;
    const double v = (double)Sxx[(size_t)b * nx * nx + idx] + dt * (Sxf[r * nx + c] + Sxf[c * nx + r])
                   + dt * dt * (double)dSff[(size_t)b * nx * nx + idx];
    Sxx[(size_t)b * nx * nx + idx] = (T)v;
    if (traj_S) traj_S[(size_t)b * nx * nx + idx] = (T)v;
  }
  if (lane < nx) {
    const double v = (double)mx[(size_t)b * nx + lane] + dt * (double)df1[(size_t)b * nx + lane];
    mx[(size_t)b * nx + lane] = (T)v;
    if (traj_mu) traj_mu[(size_t)b * nx + lane] = (T)v;
  }
}

// the end of a step in one launch, as k_compose_tail: Euler update, the new state's encoding, its expected cost.  One wave per
// batch element; the stages communicate through the wave's own global writes (visible after the workgroup barrier).
// Sxe_in: Cov(x, e) of the state the step starts from; (me, See, Sxe): the encoding of the new state (untaped: Sxe_in == Sxe, the one
// workspace; taped: the next slot)
template <typename T>
__global__ __launch_bounds__(64) void k_compose_tail_nd(MMComposeDims D, double dt, const double* cpol, const T* Sdd,
                                                        const T* df1, const T* dSff, const T* dcross, const double* Sxe_in,
                                                        T* mx, T* Sxx, T* traj_mu, T* traj_S, T* me, T* See, double* Sxe,
                                                        const T* target, const T* precis, T* cost) {
  extern __shared__ double csm[];
  const int b = blockIdx.x, lane = threadIdx.x;
  mmc_step_body_nd<T>(D, dt, Sxe_in, cpol, Sdd, df1, dSff, dcross, mx, Sxx, traj_mu, traj_S, b, lane);
  __syncthreads();
  mmc_encode_body<T>(D, mx, Sxx, me, See, Sxe, b, lane);
  if (cost) {
    __syncthreads();
    mm_expected_cost_body<T>(D.ne, me, See, target, precis, cost, b, lane, csm);
  }
}

// the mixing of a coregionalised drift (mm_mix.h): staged latent moments of the drift's match -> the slot's df1 / dSff / dcross, which
// the tail then reads as those of an ordinary drift with nx outputs.  One workgroup per batch element, a launch of its own.
template <typename T>
__global__ __launch_bounds__(64) void k_compose_mix_nd(int nx, int Lg, int nd, const double* __restrict__ W,
                                                       const double* __restrict__ mc, const T* __restrict__ g1,
                                                       const T* __restrict__ Sgg, const T* __restrict__ cg, T* __restrict__ df1,
                                                       T* __restrict__ dSff, T* __restrict__ dcross) {
  __shared__ double sm[MMC_NX * MMC_NX];
  const size_t b = blockIdx.x;
  mma_mix_fwd<MMADevCtx, T>(MMADevCtx(), nx, Lg, nd, W, mc, g1 + b * Lg, Sgg + b * Lg * Lg, cg + b * nd * Lg, df1 + b * nx,
                            dSff + b * nx * nx, dcross + b * nd * nx, sm);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
extern "C" size_t mm_compose_nd_workspace_bytes(int B, int nx, int na, int nu, int dtype) {
  if (B <= 0 || nx <= 0 || nx > MMC_NX || na < 0 || na > MMC_NA || na > nx || nu < 1 || nu > MMC_NU) return 0;
  if (2 * na + (nx - na) + nu > MMC_ND) return 0;
  if (dtype != MM_F32 && dtype != MM_F64) return 0;
  return mm_compose_layout_nd(B, nx, na, nu, dtype).total;
}

// tape == nullptr: every step reuses the one compose workspace `w`; else step h works in tape slot h (see the header comment)
// mixW != nullptr (the _mixed entries): the drift has Lg <= nx latents; its match writes to the staging block `stage`
// (mm_mix_stage) and k_compose_mix_nd fills df1 / dSff / dcross.  mixW == nullptr: Lg == nx, no staging, as ever.
template <typename T>
static int mm_rollout_composed_nd_t(const void* drift, size_t drift_bytes, int Md, const void* policy, size_t policy_bytes,
                                    int Mpol, int dtype, int B, int H, double dt, const MMComposeDims& D, const MMHeadND& hd,
                                    const T* target, const T* precis, T* mx, T* Sxx, T* cost, T* traj_mu, T* traj_S,
                                    void* ws_drift, size_t ws_drift_bytes, void* ws_policy, size_t ws_policy_bytes,
                                    char* w, const MMComposeLayout& cl, char* tape, const MMTapeLayout& tl, int32_t* status,
                                    hipStream_t s, int Lg, const double* mixW = nullptr, const double* mixc = nullptr,
                                    char* stage = nullptr, char* gp_scratch = nullptr, size_t gp_scratch_bytes = 0) {
  const int nx = D.nx, ne = D.ne, nd = D.nd, nu = nd - ne;
  const MMMixStage ms = mm_mix_stage(B, Lg, nd, sizeof(T));
  auto slot = [&](int h) { return tape ? tape + (size_t)h * tl.slot_bytes : w; };
  T* xm = tape ? (T*)(tape + tl.xm) : nullptr;
  T* xS = tape ? (T*)(tape + tl.xS) : nullptr;
#define MMC_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)
  if (tape) {
    hipError_t e1 = hipMemcpyAsync(xm, mx, (size_t)B * nx * sizeof(T), hipMemcpyDeviceToDevice, s);
    hipError_t e2 = hipMemcpyAsync(xS, Sxx, (size_t)B * nx * nx * sizeof(T), hipMemcpyDeviceToDevice, s);
    if (e1 != hipSuccess) return (int)e1;
    if (e2 != hipSuccess) return (int)e2;
  }
  {
    char* c0 = slot(0);
    hipLaunchKernelGGL((k_compose_encode_nd<T>), dim3(B), dim3(64), 0, s, D, (const T*)mx, (const T*)Sxx, (T*)(c0 + cl.me),
                       (T*)(c0 + cl.See), (double*)(c0 + cl.Sxe));
    MMC_CHECK();
  }
  for (int h = 0; h < H; ++h) {
    char* c = slot(h); char* n = slot(h + 1);
    T *me = (T*)(c + cl.me), *See = (T*)(c + cl.See), *pf1 = (T*)(c + cl.pf1), *pSff = (T*)(c + cl.pSff);
    T *pcross = (T*)(c + cl.pcross), *md = (T*)(c + cl.md), *Sdd = (T*)(c + cl.Sdd), *df1 = (T*)(c + cl.df1);
    T *dSff = (T*)(c + cl.dSff), *dcross = (T*)(c + cl.dcross);
    // where the drift's match writes: the slot itself, or the staging block of the mixing
    T *mf1 = mixW ? (T*)(stage + ms.g1) : df1, *mSff = mixW ? (T*)(stage + ms.Sgg) : dSff, *mcross = mixW ? (T*)(stage + ms.cg) : dcross;
    double *Sxe = (double*)(c + cl.Sxe), *cpol = (double*)(c + cl.cpol);
    // policy: mean-only regressor (models.py:34-41: model_uncertainty = False), nu latents, full covariance between them
    int rc = mm_moment_match(policy, policy_bytes, nu, Mpol, ne, dtype, B, me, See, MM_FULL_OUTPUT_COV, 0.0, pf1, pSff, pcross,
                             ws_policy, ws_policy_bytes, status, (void*)s);
    if (rc) return rc;
    hipLaunchKernelGGL((k_compose_head_nd<T>), dim3(B), dim3(256), 0, s, D, hd, (const T*)me, (const T*)See, (const T*)pf1,
                       (const T*)pSff, (const T*)pcross, md, Sdd, cpol);
    MMC_CHECK();
    // (taped, small enough: the match runs in the tape's own workspace slot of this step, which the reverse sweep reads)
    void* wsd = (tape && tl.ws_stride) ? (void*)(tape + tl.ws + (size_t)h * tl.ws_stride) : ws_drift;
    const size_t wsd_bytes = (tape && tl.ws_stride) ? tl.ws_stride : ws_drift_bytes;
    if (tape && tl.gp_stride)     // the sums of the backward's sweeps stay on the tape and give this step's value too (mm_compose.h)
      rc = mm_moment_match_with_sums_impl(drift, drift_bytes, Lg, Md, nd, dtype, B, md, Sdd, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY,
                                          0.0, mf1, mSff, mcross, wsd, wsd_bytes, tape + tl.gp + (size_t)h * tl.gp_stride,
                                          tl.gp_stride, status, (void*)s, false);
    else if (tape && gp_scratch)  // (mixed: the same routine on one scratch buffer, so that the value is that of the kept regime)
      rc = mm_moment_match_with_sums_impl(drift, drift_bytes, Lg, Md, nd, dtype, B, md, Sdd, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY,
                                          0.0, mf1, mSff, mcross, wsd, wsd_bytes, gp_scratch, gp_scratch_bytes, status, (void*)s,
                                          false);
    else
      rc = mm_moment_match(drift, drift_bytes, Lg, Md, nd, dtype, B, md, Sdd, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY, 0.0,
                           mf1, mSff, mcross, wsd, wsd_bytes, status, (void*)s);
    if (rc) return rc;
    if (mixW) {
      hipLaunchKernelGGL((k_compose_mix_nd<T>), dim3(B), dim3(64), 0, s, nx, Lg, nd, mixW, mixc, (const T*)mf1, (const T*)mSff,
                         (const T*)mcross, df1, dSff, dcross);
      MMC_CHECK();
    }
    T* tm = tape ? xm + (size_t)(h + 1) * B * nx : (traj_mu ? traj_mu + (size_t)h * B * nx : (T*)nullptr);
    T* tS = tape ? xS + (size_t)(h + 1) * B * nx * nx : (traj_S ? traj_S + (size_t)h * B * nx * nx : (T*)nullptr);
    hipLaunchKernelGGL((k_compose_tail_nd<T>), dim3(B), dim3(64), mm_cost_lds_bytes(ne), s, D, dt, (const double*)cpol,
                       (const T*)Sdd, (const T*)df1, (const T*)dSff, (const T*)dcross, (const double*)Sxe, mx, Sxx, tm, tS, (T*)(n + cl.me),
                       (T*)(n + cl.See), (double*)(n + cl.Sxe), target, precis, cost ? cost + (size_t)h * B : (T*)nullptr);
    MMC_CHECK();
  }
#undef MMC_CHECK
  return 0;
}

extern "C" int mm_rollout_composed_nd(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                      const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                      int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                      int nu, const double* head_scale, const double* head_shift,
                                      const void* target, const void* precis,
                                      void* mx, void* Sxx, void* cost, void* traj_mu, void* traj_Sigma,
                                      void* ws_drift, size_t ws_drift_bytes, void* ws_policy, size_t ws_policy_bytes,
                                      void* ws_compose, size_t ws_compose_bytes, int32_t* status, void* stream) {
  if (!drift_packed || !policy_packed || !mx || !Sxx || !head_scale || !head_shift) return MM_E_ARG;
  if (!ws_drift || !ws_policy || !ws_compose) return MM_E_ARG;
  if (B <= 0 || H <= 0 || drift_M <= 0 || policy_M <= 0) return MM_E_ARG;
  if (dtype != MM_F32 && dtype != MM_F64) return MM_E_DTYPE;
  if (cost && (!target || !precis)) return MM_E_ARG;
  MMComposeDims D;
  int rc = mm_compose_dims_nd(nx, na, nu, active_dims, D);
  if (rc) return rc;
  if (drift_L != nx || drift_d != D.nd || policy_d != D.ne) return MM_E_STATE;
  const MMComposeLayout cl = mm_compose_layout_nd(B, nx, na, nu, dtype);
  if (ws_compose_bytes < cl.total) return MM_E_WORKSPACE;
  // (the two matches check their packs and workspaces again; here so that nothing is enqueued before a refusal)
  if (ws_policy_bytes < mm_workspace_bytes(B, nu, policy_M, D.ne, dtype, MM_FULL_OUTPUT_COV)) return MM_E_WORKSPACE;
  if (ws_drift_bytes < mm_workspace_bytes(B, nx, drift_M, D.nd, dtype, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)) return MM_E_WORKSPACE;
  if (policy_bytes < mm_packed_model_bytes(nu, policy_M, D.ne, dtype, 0)) return MM_E_WORKSPACE;
  if (drift_bytes < mm_packed_model_bytes(nx, drift_M, D.nd, dtype, 1)) return MM_E_WORKSPACE;
  MMHeadND hd = {};
  for (int j = 0; j < nu; ++j) { hd.scale[j] = head_scale[j]; hd.shift[j] = head_shift[j]; }
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_F64)
    return mm_rollout_composed_nd_t<double>(drift_packed, drift_bytes, drift_M, policy_packed, policy_bytes, policy_M, dtype, B, H,
                                            dt, D, hd, (const double*)target, (const double*)precis, (double*)mx, (double*)Sxx,
                                            (double*)cost, (double*)traj_mu, (double*)traj_Sigma, ws_drift, ws_drift_bytes,
                                            ws_policy, ws_policy_bytes, (char*)ws_compose, cl, nullptr, MMTapeLayout(), status, s, nx);
  return mm_rollout_composed_nd_t<float>(drift_packed, drift_bytes, drift_M, policy_packed, policy_bytes, policy_M, dtype, B, H,
                                         dt, D, hd, (const float*)target, (const float*)precis, (float*)mx, (float*)Sxx,
                                         (float*)cost, (float*)traj_mu, (float*)traj_Sigma, ws_drift, ws_drift_bytes,
                                         ws_policy, ws_policy_bytes, (char*)ws_compose, cl, nullptr, MMTapeLayout(), status, s, nx);
}

// ---- the same rollout, recorded (f64 only, as the reverse sweep) -------------------------------------------------------------
// 0: dims out of range or a dtype other than MM_F64
extern "C" size_t mm_compose_tape_bytes_nd(int B, int H, int nx, int na, int nu, int drift_M, int dtype) {
  if (B <= 0 || H <= 0 || nx <= 0 || nx > MMC_NX || na < 0 || na > MMC_NA || na > nx || drift_M <= 0) return 0;
  if (nu < 1 || nu > MMC_NU || 2 * na + (nx - na) + nu > MMC_ND) return 0;
  if (dtype != MM_F64) return 0;
  return mm_tape_layout_nd(B, H, nx, na, nu, drift_M, dtype).total;
}

extern "C" int mm_rollout_composed_taped_nd(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                            const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                            int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                            int nu, const double* head_scale, const double* head_shift,
                                            const void* target, const void* precis, void* mx, void* Sxx, void* cost,
                                            void* ws_drift, size_t ws_drift_bytes, void* ws_policy, size_t ws_policy_bytes,
                                            void* tape, size_t tape_bytes, int32_t* status, void* stream) {
  if (!drift_packed || !policy_packed || !mx || !Sxx || !head_scale || !head_shift) return MM_E_ARG;
  if (!ws_drift || !ws_policy || !tape) return MM_E_ARG;
  if (B <= 0 || H <= 0 || drift_M <= 0 || policy_M <= 0) return MM_E_ARG;
  if (dtype != MM_F64) return MM_E_DTYPE;
  if (cost && (!target || !precis)) return MM_E_ARG;
  MMComposeDims D;
  int rc = mm_compose_dims_nd(nx, na, nu, active_dims, D);
  if (rc) return rc;
  if (drift_L != nx || drift_d != D.nd || policy_d != D.ne) return MM_E_STATE;
  const MMTapeLayout tl = mm_tape_layout_nd(B, H, nx, na, nu, drift_M, dtype);
  if (tape_bytes < tl.total) return MM_E_WORKSPACE;
  if (ws_policy_bytes < mm_workspace_bytes(B, nu, policy_M, D.ne, dtype, MM_FULL_OUTPUT_COV)) return MM_E_WORKSPACE;
  if (ws_drift_bytes < mm_workspace_bytes(B, nx, drift_M, D.nd, dtype, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)) return MM_E_WORKSPACE;
  if (policy_bytes < mm_packed_model_bytes(nu, policy_M, D.ne, dtype, 0)) return MM_E_WORKSPACE;
  if (drift_bytes < mm_packed_model_bytes(nx, drift_M, D.nd, dtype, 1)) return MM_E_WORKSPACE;
  MMHeadND hd = {};
  for (int j = 0; j < nu; ++j) { hd.scale[j] = head_scale[j]; hd.shift[j] = head_shift[j]; }
  const MMComposeLayout cl = mm_compose_layout_nd(B, nx, na, nu, dtype);
  return mm_rollout_composed_nd_t<double>(drift_packed, drift_bytes, drift_M, policy_packed, policy_bytes, policy_M, dtype, B, H, dt,
                                          D, hd, (const double*)target, (const double*)precis, (double*)mx, (double*)Sxx,
                                          (double*)cost, nullptr, nullptr, ws_drift, ws_drift_bytes, ws_policy, ws_policy_bytes, nullptr, cl,
                                          (char*)tape, tl, status, (hipStream_t)stream, nx);
}

// ---- a coregionalised drift: Lg = drift_L <= nx latents, f = W g + c (mm_mix.h) ------------------------------------------------
// mix_W [nx][drift_L] row-major, mix_c [nx] or NULL, both f64 on the device.  Everything else as the entries above with drift_L in
// place of nx for the drift's own pack and workspace.
static inline bool mm_mixed_dims_ok(int B, int nx, int na, int nu, int Lg) {
  if (B <= 0 || nx <= 0 || nx > MMC_NX || na < 0 || na > MMC_NA || na > nx || nu < 1 || nu > MMC_NU) return false;
  if (2 * na + (nx - na) + nu > MMC_ND) return false;
  return Lg >= 1 && Lg <= nx;
}

// the compose workspace of mm_rollout_composed_nd_mixed: that of mm_rollout_composed_nd, then the staging block.  0: out of range
extern "C" size_t mm_compose_nd_mixed_workspace_bytes(int B, int nx, int na, int nu, int drift_L, int dtype) {
  if (!mm_mixed_dims_ok(B, nx, na, nu, drift_L)) return 0;
  if (dtype != MM_F32 && dtype != MM_F64) return 0;
  return mm_compose_layout_nd(B, nx, na, nu, dtype).total + mm_mix_stage(B, drift_L, nx + na + nu, mm_elem_size(dtype)).total;
}

extern "C" int mm_rollout_composed_nd_mixed(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                            const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                            int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                            int nu, const double* head_scale, const double* head_shift,
                                            const void* target, const void* precis,
                                            void* mx, void* Sxx, void* cost, void* traj_mu, void* traj_Sigma,
                                            void* ws_drift, size_t ws_drift_bytes, void* ws_policy, size_t ws_policy_bytes,
                                            void* ws_compose, size_t ws_compose_bytes, int32_t* status, void* stream,
                                            const double* mix_W, const double* mix_c) {
  if (!drift_packed || !policy_packed || !mx || !Sxx || !head_scale || !head_shift || !mix_W) return MM_E_ARG;
  if (!ws_drift || !ws_policy || !ws_compose) return MM_E_ARG;
  if (B <= 0 || H <= 0 || drift_M <= 0 || policy_M <= 0) return MM_E_ARG;
  if (dtype != MM_F32 && dtype != MM_F64) return MM_E_DTYPE;
  if (cost && (!target || !precis)) return MM_E_ARG;
  MMComposeDims D;
  int rc = mm_compose_dims_nd(nx, na, nu, active_dims, D);
  if (rc) return rc;
  if (drift_L < 1 || drift_L > nx) return MM_E_DIM;
  if (drift_d != D.nd || policy_d != D.ne) return MM_E_STATE;
  const MMComposeLayout cl = mm_compose_layout_nd(B, nx, na, nu, dtype);
  if (ws_compose_bytes < cl.total + mm_mix_stage(B, drift_L, D.nd, mm_elem_size(dtype)).total) return MM_E_WORKSPACE;
  if (ws_policy_bytes < mm_workspace_bytes(B, nu, policy_M, D.ne, dtype, MM_FULL_OUTPUT_COV)) return MM_E_WORKSPACE;
  if (ws_drift_bytes < mm_workspace_bytes(B, drift_L, drift_M, D.nd, dtype, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)) return MM_E_WORKSPACE;
  if (policy_bytes < mm_packed_model_bytes(nu, policy_M, D.ne, dtype, 0)) return MM_E_WORKSPACE;
  if (drift_bytes < mm_packed_model_bytes(drift_L, drift_M, D.nd, dtype, 1)) return MM_E_WORKSPACE;
  MMHeadND hd = {};
  for (int j = 0; j < nu; ++j) { hd.scale[j] = head_scale[j]; hd.shift[j] = head_shift[j]; }
  hipStream_t s = (hipStream_t)stream;
  char* stage = (char*)ws_compose + cl.total;
  if (dtype == MM_F64)
    return mm_rollout_composed_nd_t<double>(drift_packed, drift_bytes, drift_M, policy_packed, policy_bytes, policy_M, dtype, B, H,
                                            dt, D, hd, (const double*)target, (const double*)precis, (double*)mx, (double*)Sxx,
                                            (double*)cost, (double*)traj_mu, (double*)traj_Sigma, ws_drift, ws_drift_bytes,
                                            ws_policy, ws_policy_bytes, (char*)ws_compose, cl, nullptr, MMTapeLayout(), status, s,
                                            drift_L, mix_W, mix_c, stage);
  return mm_rollout_composed_nd_t<float>(drift_packed, drift_bytes, drift_M, policy_packed, policy_bytes, policy_M, dtype, B, H,
                                         dt, D, hd, (const float*)target, (const float*)precis, (float*)mx, (float*)Sxx,
                                         (float*)cost, (float*)traj_mu, (float*)traj_Sigma, ws_drift, ws_drift_bytes,
                                         ws_policy, ws_policy_bytes, (char*)ws_compose, cl, nullptr, MMTapeLayout(), status, s,
                                         drift_L, mix_W, mix_c, stage);
}

// 0: dims out of range (drift_L outside 1 .. nx included) or a dtype other than MM_F64
extern "C" size_t mm_compose_tape_bytes_nd_mixed(int B, int H, int nx, int na, int nu, int drift_L, int drift_M, int dtype) {
  if (H <= 0 || drift_M <= 0 || !mm_mixed_dims_ok(B, nx, na, nu, drift_L)) return 0;
  if (dtype != MM_F64) return 0;
  const MMTapeLayout tl = mm_tape_layout_nd_mixed(B, H, nx, na, nu, drift_L, drift_M, dtype);
  return tl.total + mm_mix_stage(B, drift_L, nx + na + nu, mm_elem_size(dtype)).total
         + mm_tape_nd_mixed_scratch(tl, B, drift_L, drift_M, nx + na + nu, dtype);
}

extern "C" int mm_rollout_composed_taped_nd_mixed(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M,
                                                  int drift_d, const void* policy_packed, size_t policy_bytes, int policy_M,
                                                  int policy_d, int dtype, int B, int H, double dt, int nx, int na,
                                                  const int32_t* active_dims, int nu, const double* head_scale,
                                                  const double* head_shift, const void* target, const void* precis, void* mx,
                                                  void* Sxx, void* cost, void* ws_drift, size_t ws_drift_bytes, void* ws_policy,
                                                  size_t ws_policy_bytes, void* tape, size_t tape_bytes, int32_t* status,
                                                  void* stream, const double* mix_W, const double* mix_c) {
  if (!drift_packed || !policy_packed || !mx || !Sxx || !head_scale || !head_shift || !mix_W) return MM_E_ARG;
  if (!ws_drift || !ws_policy || !tape) return MM_E_ARG;
  if (B <= 0 || H <= 0 || drift_M <= 0 || policy_M <= 0) return MM_E_ARG;
  if (dtype != MM_F64) return MM_E_DTYPE;
  if (cost && (!target || !precis)) return MM_E_ARG;
  MMComposeDims D;
  int rc = mm_compose_dims_nd(nx, na, nu, active_dims, D);
  if (rc) return rc;
  if (drift_L < 1 || drift_L > nx) return MM_E_DIM;
  if (drift_d != D.nd || policy_d != D.ne) return MM_E_STATE;
  const MMTapeLayout tl = mm_tape_layout_nd_mixed(B, H, nx, na, nu, drift_L, drift_M, dtype);
  const size_t stage_bytes = mm_mix_stage(B, drift_L, D.nd, mm_elem_size(dtype)).total;
  const size_t scratch_bytes = mm_tape_nd_mixed_scratch(tl, B, drift_L, drift_M, D.nd, dtype);
  if (tape_bytes < tl.total + stage_bytes + scratch_bytes) return MM_E_WORKSPACE;
  if (ws_policy_bytes < mm_workspace_bytes(B, nu, policy_M, D.ne, dtype, MM_FULL_OUTPUT_COV)) return MM_E_WORKSPACE;
  if (ws_drift_bytes < mm_workspace_bytes(B, drift_L, drift_M, D.nd, dtype, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)) return MM_E_WORKSPACE;
  if (policy_bytes < mm_packed_model_bytes(nu, policy_M, D.ne, dtype, 0)) return MM_E_WORKSPACE;
  if (drift_bytes < mm_packed_model_bytes(drift_L, drift_M, D.nd, dtype, 1)) return MM_E_WORKSPACE;
  MMHeadND hd = {};
  for (int j = 0; j < nu; ++j) { hd.scale[j] = head_scale[j]; hd.shift[j] = head_shift[j]; }
  const MMComposeLayout cl = mm_compose_layout_nd(B, nx, na, nu, dtype);
  return mm_rollout_composed_nd_t<double>(drift_packed, drift_bytes, drift_M, policy_packed, policy_bytes, policy_M, dtype, B, H, dt,
                                          D, hd, (const double*)target, (const double*)precis, (double*)mx, (double*)Sxx,
                                          (double*)cost, nullptr, nullptr, ws_drift, ws_drift_bytes, ws_policy, ws_policy_bytes, nullptr, cl,
                                          (char*)tape, tl, status, (hipStream_t)stream, drift_L, mix_W, mix_c, (char*)tape + tl.total,
                                          scratch_bytes ? (char*)tape + tl.total + stage_bytes : nullptr, scratch_bytes);
}
