// Reverse sweep of the moment-matched policy rollout for policies with SEVERAL actions (gfx950): mm_compose_bwd.hip's sweep over the
// tape of mm_rollout_composed_taped_nd (mm_compose_nd.hip), with the arithmetic of csrc/mm_adjoint_nd.h.  Per step, in reverse:
//   k_compose_tail_bwd_nd  : cost + encoding adjoint at x_{h+1} (the shared bodies mma_cost_bwd, mma_encode_bwd), then the adjoint of
//                            the bookkeeping with nu policy columns + Euler (mma_step_bwd_nd)
//   mm_moment_match_backward_impl (mm_compose_bwd.hip, general in d): the drift's adjoint -- the chain rule alone on the sums the
//                            tape kept, or with its sweeps (and the q stage) first where the tape did not keep them, exactly as the
//                            one-action sweep selects
//   k_policy_head_bwd_nd   : sums the drift's items, then the n-D NormalCDF head adjoint (mma_head_bwd_nd) and the adjoint of the policy
//                            match with L = nu latents w.r.t. its input moments AND every latent's packed parameters
//                            (mma_policy_nd_bwd: nu latent items + nu (nu - 1) / 2 pair items)
// and k_compose_encode_bwd0 (mm_compose_bwd.hip) at x_0.  All adjoints are f64; f64 packs only.
// mm_rollout_composed_backward_nd_mixed (a coregionalised drift, mm_mix.h): k_compose_mix_bwd_nd, the adjoint of the output mixing,
// runs between k_compose_tail_bwd_nd and the drift's adjoint, which then has L = Lg latents and Lg + Lg (Lg + 1) / 2 items.
//
// Work split: ONE 256-thread workgroup per batch element runs the nu + nu (nu - 1) / 2 policy items in turn and adds them in that
// fixed order -- no floating-point atomics, two sweeps over one tape are bit-equal.
//
// LDS bound: the workgroup holds one item's M-sized vectors at a time -- mm_policy_bwd_nd_lds(M, ne, nu) bytes, dominated by a
// pair item's 11 [M][ne] + 14 [M] doubles: 88 KB at M = 64, ne = 8, nu = 4 (the kernel's dynamic-LDS limit is raised above 64 KB as the
// one-action entry does).  Shapes with policy M <= 256 (the pack keeps the caller's order of the centres), ne <= 8 and
// mm_policy_bwd_nd_lds <= 160 KB are taken (M <= 166 at ne = 8, <= 219 at ne = 6, 256 at ne <= 4); beyond, mm_compose_backward_workspace_bytes_nd returns 0 and the
// entry MM_E_DIM.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mm_common.h"
#include "mm_compose.h"
#include "mm_adjoint_nd.h"
#include "mm_adjoint_lds.h"
#include "mm_mix.h"

#define MMB_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)
#define MMB_ND_LDS_MAX ((size_t)160 * 1024)

// mm_compose_bwd.hip
__global__ void k_compose_encode_bwd0(MMComposeDims D, const double* __restrict__ x0m, const double* __restrict__ x0S,
                                      const double* __restrict__ cm, const double* __restrict__ cS, const double* __restrict__ cme,
                                      const double* __restrict__ cSee, const double* __restrict__ cSxe, double* __restrict__ g_mx0,
                                      double* __restrict__ g_Sxx0);
__global__ void k_zero_f64(double* p, size_t n);

// carry of adjoints between the kernels of the reverse sweep: MMCarryLayout (mm_compose_bwd.hip) with ccp [B][ne][nu], nd = ne + nu
struct MMCarryLayoutND {
  size_t cm, cS, cme, cSee, cSxe, ccp, cSdd, cmd, cdf1, cdSff, cdcross, total;
};
static inline MMCarryLayoutND mm_carry_layout_nd(int B, int nx, int na, int nu) {
  MMCarryLayoutND o;
  const size_t A = 256;
  const int ne = nx + na, nd = ne + nu;
  size_t off = 0;
  o.cm = off;      off = mm_align_up(off + (size_t)B * nx * 8, A);
  o.cS = off;      off = mm_align_up(off + (size_t)B * nx * nx * 8, A);
  o.cme = off;     off = mm_align_up(off + (size_t)B * ne * 8, A);
  o.cSee = off;    off = mm_align_up(off + (size_t)B * ne * ne * 8, A);
  o.cSxe = off;    off = mm_align_up(off + (size_t)B * nx * ne * 8, A);
  o.ccp = off;     off = mm_align_up(off + (size_t)B * ne * nu * 8, A);
  o.cSdd = off;    off = mm_align_up(off + (size_t)B * nd * nd * 8, A);
  o.cmd = off;     off = mm_align_up(off + (size_t)B * nd * 8, A);
  o.cdf1 = off;    off = mm_align_up(off + (size_t)B * nx * 8, A);
  o.cdSff = off;   off = mm_align_up(off + (size_t)B * nx * nx * 8, A);
  o.cdcross = off; off = mm_align_up(off + (size_t)B * nd * nx * 8, A);
  o.total = off;
  return o;
}

// k_compose_tail_bwd_nd: grid B, 64 threads; k_compose_tail_bwd with nu policy columns (cp, ccp [B][ne][nu]).
// Ctx: MMADevCtx (the _nd entries) or MMAWideCtx (the _wide entries: the dense paths for 8 < n <= 16 of mm_adjoint.h).
template <class Ctx>
__global__ __launch_bounds__(64) void k_compose_tail_bwd_nd(MMComposeDims D, double dt, int first, const double* __restrict__ x1m,
                                                            const double* __restrict__ x1S, const double* __restrict__ me1,
                                                            const double* __restrict__ See1, const double* __restrict__ target,
                                                            const double* __restrict__ precis, const double* __restrict__ gcost,
                                                            const double* __restrict__ Sxe, const double* __restrict__ cp,
                                                            const double* __restrict__ Sdd, const double* __restrict__ dcross,
                                                            double* cm, double* cS, double* cme, double* cSee, double* cSxe,
                                                            double* ccp, double* cSdd, double* cdf1, double* cdSff, double* cdcross,
                                                              const double* __restrict__ sxm, const double* __restrict__ sxS) {
  extern __shared__ double sm[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nx = D.nx, ne = D.ne, nd = D.nd, nu = nd - ne;
  Ctx c;
  double* gme = sm; double* gSee = gme + ne; double* gSxe = gSee + ne * ne; double* gm1 = gSxe + nx * ne; double* gS1 = gm1 + nx;
  double* wk = gS1 + nx * nx;
  cm += (size_t)b * nx; cS += (size_t)b * nx * nx; cme += (size_t)b * ne; cSee += (size_t)b * ne * ne; cSxe += (size_t)b * nx * ne;
  for (int i = lane; i < ne; i += 64) gme[i] = first ? 0.0 : cme[i];
  for (int i = lane; i < ne * ne; i += 64) gSee[i] = first ? 0.0 : cSee[i];
  for (int i = lane; i < nx * ne; i += 64) gSxe[i] = first ? 0.0 : cSxe[i];
  for (int i = lane; i < nx; i += 64) gm1[i] = first ? 0.0 : cm[i];
  for (int i = lane; i < nx * nx; i += 64) gS1[i] = first ? 0.0 : cS[i];
  // the caller's own seeds d loss / d (m_{h+1}, S_{h+1}) (the seeded entries; the same lanes wrote the carry above)
  if (sxm) {
    for (int i = lane; i < nx; i += 64) gm1[i] += sxm[(size_t)b * nx + i];
    for (int i = lane; i < nx * nx; i += 64) gS1[i] += sxS[(size_t)b * nx * nx + i];
  }
  __syncthreads();
  mma_cost_bwd(c, ne, me1 + (size_t)b * ne, See1 + (size_t)b * ne * ne, target, precis, gcost[b], gme, gSee, wk);
  mma_encode_bwd(c, D, x1m + (size_t)b * nx, x1S + (size_t)b * nx * nx, gme, gSee, gSxe, gm1, gS1, wk);
  mma_step_bwd_nd(c, D, dt, Sxe + (size_t)b * nx * ne, cp + (size_t)b * ne * nu, Sdd + (size_t)b * nd * nd,
                  dcross + (size_t)b * nd * nx, gm1, gS1, cSxe, ccp + (size_t)b * ne * nu, cSdd + (size_t)b * nd * nd,
                  cdf1 + (size_t)b * nx, cdSff + (size_t)b * nx * nx, cdcross + (size_t)b * nd * nx, wk);
  for (int i = lane; i < nx; i += 64) cm[i] = gm1[i];
  for (int i = lane; i < nx * nx; i += 64) cS[i] = gS1[i];
}
// (its LDS: mm_tail_bwd_nd_lds, mm_adjoint_lds.h)

// k_policy_head_bwd_nd: grid B, 256 threads.  Sums the drift match's (latent | pair) items [B][nitems][nd^2 + nd] onto the
// bookkeeping's part cSdd; writes cme, cSee (the adjoint of the encoding of x_h through the policy and the joint); accumulates the
// packed policy's gradient into gpar [B][nu][mm_policy_grad_len(M, ne)], latent by latent.
template <class Ctx>
__global__ __launch_bounds__(256) void k_policy_head_bwd_nd(int M, int ne, int nu, MMHeadND hd, const double* __restrict__ Z,
                                                            const double* __restrict__ beta, const double* __restrict__ ls2,
                                                            const double* __restrict__ var, const double* __restrict__ me,
                                                            const double* __restrict__ See, const double* __restrict__ pf1,
                                                            const double* __restrict__ pSff, const double* __restrict__ pcross,
                                                            const double* __restrict__ cSdd, const double* __restrict__ ccp,
                                                            double* __restrict__ cme, double* __restrict__ cSee,
                                                            double* __restrict__ gpar, int32_t* status,
                                                            const double* __restrict__ items, int nitems) {
  extern __shared__ double sm[];
  const int b = blockIdx.x, nd = ne + nu;
  Ctx c;
  double* gme = sm; double* gSee = gme + ne; double* gpc = gSee + ne * ne; double* gmu = gpc + ne * nu; double* gSig = gmu + ne;
  double* gpf1 = gSig + ne * ne; double* gpS = gpf1 + nu; double* hsc = gpS + nu * nu;      // head constants: scale, shift [nu] each
  double* hw = hsc + 2 * nu;                                                               // head scratch
  double* dmd = hw + mma_head_bwd_nd_scratch(ne, nu);
  double* dSd = dmd + nd;
  double* wk = dSd + nd * nd;
  {
    const int st = nd * nd + nd;
    const double* it = items + (size_t)b * nitems * st;
    for (int idx = threadIdx.x; idx < nd * nd; idx += 256) {
      const int i = idx / nd, j = idx - i * nd;
      double sv = 0.0;
      for (int t = 0; t < nitems; ++t) sv += 0.5 * (it[(size_t)t * st + i * nd + j] + it[(size_t)t * st + j * nd + i]);
      dSd[idx] = cSdd[(size_t)b * nd * nd + idx] + sv;
    }
    for (int k = threadIdx.x; k < nd; k += 256) {
      double sv = 0.0;
      for (int t = 0; t < nitems; ++t) sv += it[(size_t)t * st + nd * nd + k];
      dmd[k] = sv;
    }
    if (threadIdx.x < nu) { hsc[threadIdx.x] = hd.scale[threadIdx.x]; hsc[nu + threadIdx.x] = hd.shift[threadIdx.x]; }
  }
  __syncthreads();
  const double* meb = me + (size_t)b * ne;
  const double* Seb = See + (size_t)b * ne * ne;
  mma_head_bwd_nd(c, ne, nu, hsc, hsc + nu, pf1 + (size_t)b * nu, pSff + (size_t)b * nu * nu, pcross + (size_t)b * ne * nu, Seb, dmd,
                  dSd, ccp + (size_t)b * ne * nu, gme, gSee, gpc, gpf1, gpS, hw);
  bool ok = true;
  mma_policy_nd_bwd<Ctx, 8>(c, nu, M, ne, Z, beta, ls2, var, meb, Seb, gpf1, gpS, gpc, gmu, gSig,
                                  gpar + (size_t)b * nu * ((size_t)M * ne + M + ne + 2), wk, &ok);
  __syncthreads();
  for (int k = threadIdx.x; k < ne; k += 256) cme[(size_t)b * ne + k] = gme[k] + gmu[k];
  for (int idx = threadIdx.x; idx < ne * ne; idx += 256) cSee[(size_t)b * ne * ne + idx] = gSee[idx] + gSig[idx];
  if (!ok && threadIdx.x == 0 && status) { atomicMax(status, (int)gridDim.x - b); status[1] = 0; }
}
// (its LDS: mm_policy_bwd_nd_lds, and mm_policy_bwd_wide_lds for the _wide entries: mm_adjoint_lds.h)

// shapes the sweep takes (see the header comment): ne <= ne_max = 8 (the _nd entries) or 16 (the _wide entries)
#define MMB_ND_NE 8
#define MMB_WIDE_NE 16
static inline bool mm_compose_bwd_nd_takes(int nx, int na, int nu, int policy_M, int ne_max = MMB_ND_NE) {
  if (nx <= 0 || nx > MMC_NX || na < 0 || na > MMC_NA || na > nx || nu < 1 || nu > MMC_NU || policy_M <= 0) return false;
  const int ne = nx + na;
  if (ne + nu > MMC_ND || ne > ne_max || policy_M > MM_SORT_MIN_M) return false;
  if (ne_max <= MMB_ND_NE) return mm_policy_bwd_nd_lds(policy_M, ne, nu) <= MMB_ND_LDS_MAX;
  // (the number of sub-sweeps max(1, 256 / M) drops as M grows, so the size is not monotone in M: a policy is taken when every
  // smaller one fits too, which makes "M <= M*" the whole rule at given (ne, nu))
  for (int m = 1; m <= policy_M; ++m)
    if (mm_policy_bwd_wide_lds(m, ne, nu) > MMB_ND_LDS_MAX) return false;
  return true;
}

// the carry, then the drift match's backward buffer (used where the tape did not keep the sums of the step)
struct MMComposeBwdLayoutND { size_t carry, gp, gp_bytes, total; };
static inline MMComposeBwdLayoutND mm_compose_bwd_layout_nd(int B, int nx, int na, int nu, int Md) {
  MMComposeBwdLayoutND o;
  o.carry = 0;
  o.gp = mm_align_up(mm_carry_layout_nd(B, nx, na, nu).total, 256);
  o.gp_bytes = mm_moment_match_backward_bytes_dtype(B, nx, Md, nx + na + nu, MM_F64, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY);
  o.total = o.gp + o.gp_bytes;
  return o;
}

// a coregionalised drift (mm_mix.h, the _mixed entries): the adjoints of the latent moments (mm_mix_stage, f64) sit between the carry
// and the drift match's backward buffer, which is sized by the Lg latents
struct MMComposeBwdLayoutNDMixed { size_t carry, stage, gp, gp_bytes, total; };
static inline MMComposeBwdLayoutNDMixed mm_compose_bwd_layout_nd_mixed(int B, int nx, int na, int nu, int Lg, int Md) {
  MMComposeBwdLayoutNDMixed o;
  o.carry = 0;
  o.stage = mm_align_up(mm_carry_layout_nd(B, nx, na, nu).total, 256);
  o.gp = o.stage + mm_mix_stage(B, Lg, nx + na + nu, 8).total;
  o.gp_bytes = mm_moment_match_backward_bytes_dtype(B, Lg, Md, nx + na + nu, MM_F64, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY);
  o.total = o.gp + o.gp_bytes;
  return o;
}

// the adjoint of the mixing, between k_compose_tail_bwd_nd and the drift match's adjoint: grid B, 64 threads
__global__ __launch_bounds__(64) void k_compose_mix_bwd_nd(int nx, int Lg, int nd, const double* __restrict__ W,
                                                           const double* __restrict__ cdf1, const double* __restrict__ cdSff,
                                                           const double* __restrict__ cdcross, double* __restrict__ cg1,
                                                           double* __restrict__ cSgg, double* __restrict__ ccg) {
  __shared__ double sm[MMC_NX * MMC_NX];
  const size_t b = blockIdx.x;
  mma_mix_bwd(MMADevCtx(), nx, Lg, nd, W, cdf1 + b * nx, cdSff + b * nx * nx, cdcross + b * nd * nx, cg1 + b * Lg,
              cSgg + b * Lg * Lg, ccg + b * nd * Lg, sm);
}

// which dense code the _wide entries run (0: the fast paths of mm_adjoint.h for 8 < n <= 16; 1: the generic code)
static int g_wide_generic = 0;

extern "C" size_t mm_compose_backward_workspace_bytes_nd(int B, int nx, int na, int nu, int drift_M, int policy_M) {
  if (B <= 0 || drift_M <= 0 || !mm_compose_bwd_nd_takes(nx, na, nu, policy_M)) return 0;
  return mm_compose_bwd_layout_nd(B, nx, na, nu, drift_M).total;
}

extern "C" size_t mm_policy_grad_bytes_nd(int B, int nu, int policy_M, int policy_d) {
  if (B <= 0 || nu < 1 || nu > MMC_NU || policy_M <= 0 || policy_d <= 0) return 0;
  return (size_t)B * nu * mm_policy_grad_len(policy_M, policy_d) * sizeof(double);
}

// Reverse sweep over the tape of mm_rollout_composed_taped_nd (same models, shapes and constants).  f64 only.
//   g_cost   [H][B]: d loss / d cost[h][b]
//   g_policy [B][nu][M d + M + d + 2] (out, overwritten): per batch element and latent, in latent order, the gradient w.r.t. the
//            PACKED policy -- Z [M][d], beta [M], ls2 = lengthscales^2 [d], variance, mean_c
//   g_mx0 [B][nx], g_Sxx0 [B][nx][nx] (out, optional): gradient w.r.t. the initial state (symmetric)
// g_xm [H][B][nx], g_xS [H][B][nx][nx] (both or neither): the caller's seeds on the trajectory, as in mm_compose_bwd.hip
// mixed (the _mixed entry): the drift has drift_L <= nx latents mixed by mix_W; else drift_L == nx and mix_W is not read
static int mm_rollout_composed_backward_nd_impl(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                                const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                                int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                                int nu, const double* head_scale, const double* head_shift,
                                                const void* target, const void* precis, const void* tape, size_t tape_bytes,
                                                const void* g_cost, const void* g_xm, const void* g_xS,
                                                void* g_policy, void* g_mx0, void* g_Sxx0,
                                                void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                                int32_t* status, void* stream, bool mixed = false,
                                                const double* mix_W = nullptr, bool wide = false) {
  if ((g_xm == nullptr) != (g_xS == nullptr)) return MM_E_ARG;
  if (mixed && !mix_W) return MM_E_ARG;
  if (!drift_packed || !policy_packed || !tape || !g_cost || !g_policy || !ws_drift || !ws_bwd || !target || !precis) return MM_E_ARG;
  if (!head_scale || !head_shift) return MM_E_ARG;
  if (B <= 0 || H <= 0 || drift_M <= 0 || policy_M <= 0) return MM_E_ARG;
  if (dtype != MM_F64) return MM_E_DTYPE;
  if ((g_mx0 == nullptr) != (g_Sxx0 == nullptr)) return MM_E_ARG;
  MMComposeDims D;
  int rc = mm_compose_dims_nd(nx, na, nu, active_dims, D);
  if (rc) return rc;
  const int ne = D.ne, nd = D.nd;
  if (mixed && (drift_L < 1 || drift_L > nx)) return MM_E_DIM;
  if ((!mixed && drift_L != nx) || drift_d != nd || policy_d != ne) return MM_E_STATE;
  if (!mm_compose_bwd_nd_takes(nx, na, nu, policy_M, wide ? MMB_WIDE_NE : MMB_ND_NE)) return MM_E_DIM;
  const int Lg = drift_L;
  const MMMixStage ms = mm_mix_stage(B, Lg, nd, 8);
  const MMTapeLayout tl = mixed ? mm_tape_layout_nd_mixed(B, H, nx, na, nu, Lg, drift_M, dtype)
                                : mm_tape_layout_nd(B, H, nx, na, nu, drift_M, dtype);
  if (tape_bytes < tl.total + (mixed ? ms.total + mm_tape_nd_mixed_scratch(tl, B, Lg, drift_M, nd, dtype) : 0)) return MM_E_WORKSPACE;
  const MMCarryLayoutND kl = mm_carry_layout_nd(B, nx, na, nu);
  MMComposeBwdLayoutND bl = mm_compose_bwd_layout_nd(B, nx, na, nu, drift_M);
  size_t stage_off = 0;
  if (mixed) {
    const MMComposeBwdLayoutNDMixed blm = mm_compose_bwd_layout_nd_mixed(B, nx, na, nu, Lg, drift_M);
    bl.carry = blm.carry; bl.gp = blm.gp; bl.gp_bytes = blm.gp_bytes; bl.total = blm.total;
    stage_off = blm.stage;
  }
  if (ws_bwd_bytes < bl.total) return MM_E_WORKSPACE;
  if (ws_drift_bytes < mm_workspace_bytes(B, Lg, drift_M, nd, dtype, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)) return MM_E_WORKSPACE;
  const MMModelLayout pl = mm_model_layout(nu, policy_M, ne, dtype, 1);
  if (policy_bytes < pl.Cm) return MM_E_WORKSPACE;
  if (drift_bytes < mm_packed_model_bytes(Lg, drift_M, nd, dtype, 1)) return MM_E_WORKSPACE;
  MMHeadND hd = {};
  for (int j = 0; j < nu; ++j) { hd.scale[j] = head_scale[j]; hd.shift[j] = head_shift[j]; }
  const MMComposeLayout cl = mm_compose_layout_nd(B, nx, na, nu, dtype);
  hipStream_t s = (hipStream_t)stream;
  char* cw = (char*)ws_bwd + bl.carry; char* gw = (char*)ws_bwd + bl.gp;
  const char* tp = (const char*)tape; const char* pp = (const char*)policy_packed;
  auto cr = [&](size_t off) { return (double*)(cw + off); };
  const double* xm = (const double*)(tp + tl.xm); const double* xS = (const double*)(tp + tl.xS);
  const size_t lds_tail = mm_tail_bwd_nd_lds(nx, ne, nd);
  const size_t lds_pol = wide ? mm_policy_bwd_wide_lds(policy_M, ne, nu) : mm_policy_bwd_nd_lds(policy_M, ne, nu);
  // the kernels of this entry's family (the wide ones on the dense fast paths, or -- mm_compose_wide_dense_path -- the generic code)
  auto k_tail = k_compose_tail_bwd_nd<MMADevCtx>;
  auto k_policy = k_policy_head_bwd_nd<MMADevCtx>;
  if (wide && g_wide_generic) { k_tail = k_compose_tail_bwd_nd<MMAWideCtx<false>>; k_policy = k_policy_head_bwd_nd<MMAWideCtx<false>>; }
  else if (wide) { k_tail = k_compose_tail_bwd_nd<MMAWideCtx<true>>; k_policy = k_policy_head_bwd_nd<MMAWideCtx<true>>; }
  if (lds_pol > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_policy, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_pol);
    if (e != hipSuccess) return (int)e;
  }
  const size_t npar = (size_t)B * nu * mm_policy_grad_len(policy_M, ne);
  hipLaunchKernelGGL(k_zero_f64, dim3((unsigned)((npar + 255) / 256)), dim3(256), 0, s, (double*)g_policy, npar);
  MMB_CHECK();
  const int dflags = MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY;
  const size_t items_off = mm_gp_bwd_items_offset(B, Lg, drift_M, nd, MM_F64, dflags);
  // the adjoints the drift match's backward reads: the carry's own, or (mixed) those of the latent moments
  char* sg = (char*)ws_bwd + stage_off;
  const double* gdf1 = mixed ? (const double*)(sg + ms.g1) : cr(kl.cdf1);
  const double* gdSff = mixed ? (const double*)(sg + ms.Sgg) : cr(kl.cdSff);
  const double* gdcross = mixed ? (const double*)(sg + ms.cg) : cr(kl.cdcross);
  for (int h = H - 1; h >= 0; --h) {
    const char* sl = tp + (size_t)h * tl.slot_bytes; const char* sn = tp + (size_t)(h + 1) * tl.slot_bytes;
    hipLaunchKernelGGL(k_tail, dim3(B), dim3(64), lds_tail, s, D, dt, h == H - 1 ? 1 : 0,
                       xm + (size_t)(h + 1) * B * nx, xS + (size_t)(h + 1) * B * nx * nx, (const double*)(sn + cl.me),
                       (const double*)(sn + cl.See), (const double*)target, (const double*)precis,
                       (const double*)g_cost + (size_t)h * B, (const double*)(sl + cl.Sxe), (const double*)(sl + cl.cpol),
                       (const double*)(sl + cl.Sdd), (const double*)(sl + cl.dcross), cr(kl.cm), cr(kl.cS), cr(kl.cme),
                       cr(kl.cSee), cr(kl.cSxe), cr(kl.ccp), cr(kl.cSdd), cr(kl.cdf1), cr(kl.cdSff), cr(kl.cdcross),
                       g_xm ? (const double*)g_xm + (size_t)h * B * nx : (const double*)nullptr,
                       g_xS ? (const double*)g_xS + (size_t)h * B * nx * nx : (const double*)nullptr);
    MMB_CHECK();
    if (mixed) {
      hipLaunchKernelGGL(k_compose_mix_bwd_nd, dim3(B), dim3(64), 0, s, nx, Lg, nd, mix_W, (const double*)cr(kl.cdf1),
                         (const double*)cr(kl.cdSff), (const double*)cr(kl.cdcross), (double*)(sg + ms.g1), (double*)(sg + ms.Sgg),
                         (double*)(sg + ms.cg));
      MMB_CHECK();
    }
    // the drift's match (its items are summed by the next kernel), as the one-action sweep runs it
    const bool kept = tl.ws_stride != 0;                   // the tape holds this step's q-stage workspace
    const bool sums = tl.gp_stride != 0;                   // ... and the sums of its backward sweeps: chain rule alone
    void* wsd = kept ? (void*)(const_cast<char*>(tp) + tl.ws + (size_t)h * tl.ws_stride) : ws_drift;
    char* gslot = sums ? const_cast<char*>(tp) + tl.gp + (size_t)h * tl.gp_stride : gw;
    rc = mm_moment_match_backward_impl(drift_packed, drift_bytes, Lg, drift_M, nd, dtype, B, sl + cl.md, sl + cl.Sdd, dflags,
                                       gdf1, gdSff, gdcross, cr(kl.cmd), cr(kl.cSdd), 1, wsd,
                                       kept ? tl.ws_stride : ws_drift_bytes, gslot, sums ? tl.gp_stride : bl.gp_bytes, status, stream,
                                       kept, true, sums ? MMB_MODE_CHAIN : MMB_MODE_ALL, false /* the tape is this rollout's own */,
                                       wide && !g_wide_generic);
    if (rc) return rc;
    hipLaunchKernelGGL(k_policy, dim3(B), dim3(256), lds_pol, s, policy_M, ne, nu, hd, (const double*)(pp + pl.Z64),
                       (const double*)(pp + pl.beta64), (const double*)(pp + pl.ls2), (const double*)(pp + pl.var),
                       (const double*)(sl + cl.me), (const double*)(sl + cl.See), (const double*)(sl + cl.pf1),
                       (const double*)(sl + cl.pSff), (const double*)(sl + cl.pcross), (const double*)cr(kl.cSdd),
                       (const double*)cr(kl.ccp), cr(kl.cme), cr(kl.cSee), (double*)g_policy, status,
                       (const double*)(gslot + items_off), Lg + Lg * (Lg + 1) / 2);
    MMB_CHECK();
  }
  if (g_mx0) {
    const size_t lds0 = (size_t)(nx + nx * nx + mma_encode_bwd_scratch(nx, na) + 8) * sizeof(double);
    hipLaunchKernelGGL(k_compose_encode_bwd0, dim3(B), dim3(64), lds0, s, D, xm, xS, (const double*)cr(kl.cm), (const double*)cr(kl.cS),
                       (const double*)cr(kl.cme), (const double*)cr(kl.cSee), (const double*)cr(kl.cSxe), (double*)g_mx0, (double*)g_Sxx0);
    MMB_CHECK();
  }
  return 0;
}

extern "C" int mm_rollout_composed_backward_nd(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                               const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                               int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                               int nu, const double* head_scale, const double* head_shift,
                                               const void* target, const void* precis, const void* tape, size_t tape_bytes,
                                               const void* g_cost, void* g_policy, void* g_mx0, void* g_Sxx0,
                                               void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                               int32_t* status, void* stream) {
  return mm_rollout_composed_backward_nd_impl(drift_packed, drift_bytes, drift_L, drift_M, drift_d, policy_packed, policy_bytes,
                                              policy_M, policy_d, dtype, B, H, dt, nx, na, active_dims, nu, head_scale, head_shift,
                                              target, precis, tape, tape_bytes, g_cost, nullptr, nullptr, g_policy, g_mx0, g_Sxx0,
                                              ws_drift, ws_drift_bytes, ws_bwd, ws_bwd_bytes, status, stream);
}

// ... with per-step seeds d loss / d (m_{h+1}, S_{h+1}) on the trajectory (mm_rollout_composed_backward_seeded for 1 to 4 actions)
extern "C" int mm_rollout_composed_backward_nd_seeded(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M,
                                                      int drift_d, const void* policy_packed, size_t policy_bytes, int policy_M,
                                                      int policy_d, int dtype, int B, int H, double dt, int nx, int na,
                                                      const int32_t* active_dims, int nu, const double* head_scale,
                                                      const double* head_shift, const void* target, const void* precis,
                                                      const void* tape, size_t tape_bytes, const void* g_cost,
                                                      const void* g_xm, const void* g_xS,
                                                      void* g_policy, void* g_mx0, void* g_Sxx0,
                                                      void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                                      int32_t* status, void* stream) {
  return mm_rollout_composed_backward_nd_impl(drift_packed, drift_bytes, drift_L, drift_M, drift_d, policy_packed, policy_bytes,
                                              policy_M, policy_d, dtype, B, H, dt, nx, na, active_dims, nu, head_scale, head_shift,
                                              target, precis, tape, tape_bytes, g_cost, g_xm, g_xS, g_policy, g_mx0, g_Sxx0,
                                              ws_drift, ws_drift_bytes, ws_bwd, ws_bwd_bytes, status, stream);
}

// ---- a coregionalised drift: the sweep over the tape of mm_rollout_composed_taped_nd_mixed (mm_compose_nd.hip) -----------------
// 0: the shapes mm_compose_backward_workspace_bytes_nd refuses, or drift_L outside 1 .. nx
extern "C" size_t mm_compose_backward_workspace_bytes_nd_mixed(int B, int nx, int na, int nu, int drift_L, int drift_M,
                                                               int policy_M) {
  if (B <= 0 || drift_M <= 0 || !mm_compose_bwd_nd_takes(nx, na, nu, policy_M) || drift_L < 1 || drift_L > nx) return 0;
  return mm_compose_bwd_layout_nd_mixed(B, nx, na, nu, drift_L, drift_M).total;
}

// mm_rollout_composed_backward_nd_seeded with the adjoint of the mixing in front of the drift's adjoint (g_xm / g_xS NULL: the plain
// sweep).  mix_W [nx][drift_L] as the forward's; no gradient w.r.t. W, c or the drift.
extern "C" int mm_rollout_composed_backward_nd_mixed(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M,
                                                     int drift_d, const void* policy_packed, size_t policy_bytes, int policy_M,
                                                     int policy_d, int dtype, int B, int H, double dt, int nx, int na,
                                                     const int32_t* active_dims, int nu, const double* head_scale,
                                                     const double* head_shift, const void* target, const void* precis,
                                                     const void* tape, size_t tape_bytes, const void* g_cost,
                                                     const void* g_xm, const void* g_xS,
                                                     void* g_policy, void* g_mx0, void* g_Sxx0,
                                                     void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                                     int32_t* status, void* stream, const double* mix_W) {
  return mm_rollout_composed_backward_nd_impl(drift_packed, drift_bytes, drift_L, drift_M, drift_d, policy_packed, policy_bytes,
                                              policy_M, policy_d, dtype, B, H, dt, nx, na, active_dims, nu, head_scale, head_shift,
                                              target, precis, tape, tape_bytes, g_cost, g_xm, g_xS, g_policy, g_mx0, g_Sxx0,
                                              ws_drift, ws_drift_bytes, ws_bwd, ws_bwd_bytes, status, stream, true, mix_W);
}

// ---- 8 < ne <= 16 encoded dims: the _wide entries ------------------------------------------------------------------------------
// The same sweep over the same tapes (mm_rollout_composed_taped_nd / _nd_mixed take every ne the compose layer allows) with
// MMAWideCtx kernels: ne <= 16 (ne <= 8 included, so that the two families can be compared), 1 <= nu <= 4, policy M <= 256 and
// mm_policy_bwd_nd_lds(M, ne, nu) <= 160 KB -- the same LDS size function as the _nd entries, dominated by a pair item's
// 11 [M][ne] + 14 [M] doubles plus the sub-sweeps' [ns][M][ne + 2] partial sums, ns = max(1, 256 / M); with one action no pair
// item runs and its scratch is left out (mm_policy_bwd_wide_lds: the one-action item's 5 [M][ne] + 8 [M] doubles).  A policy is
// taken when it and every smaller one fit: M <= 121 with one action and M <= 50 with 2 to 4 at ne = 16, M <= 229 and M <= 106 at
// ne = 11, every M <= 256 with one action and M <= 146 with several at ne = 9.  The per-centre arrays
// stay [M][d] (a lane-per-centre stride of 128 bytes at d = 16: a bank conflict a padded row would avoid): the bodies of
// mm_adjoint.h / mm_adjoint_nd.h index them, are shared with the _nd kernels, whose code must not change, and a stride argument
// would change it.  The drift's adjoint (mm_moment_match_backward_impl) launches its items kernel with the wide context too
// (the pair items' inverse at d = nd <= 16).
extern "C" size_t mm_compose_backward_workspace_bytes_wide(int B, int nx, int na, int nu, int drift_M, int policy_M) {
  if (B <= 0 || drift_M <= 0 || !mm_compose_bwd_nd_takes(nx, na, nu, policy_M, MMB_WIDE_NE)) return 0;
  return mm_compose_bwd_layout_nd(B, nx, na, nu, drift_M).total;
}

extern "C" size_t mm_compose_backward_workspace_bytes_wide_mixed(int B, int nx, int na, int nu, int drift_L, int drift_M,
                                                                 int policy_M) {
  if (B <= 0 || drift_M <= 0 || !mm_compose_bwd_nd_takes(nx, na, nu, policy_M, MMB_WIDE_NE) || drift_L < 1 || drift_L > nx) return 0;
  return mm_compose_bwd_layout_nd_mixed(B, nx, na, nu, drift_L, drift_M).total;
}

// generic != 0: the _wide entries run the generic dense code from now on (0: the fast paths, the default).  Returns the previous
// setting.  For measuring one against the other in one process (tools/bench_compose_wide.py); not thread-safe.
extern "C" int mm_compose_wide_dense_path(int generic) {
  const int was = g_wide_generic;
  g_wide_generic = generic ? 1 : 0;
  return was;
}

extern "C" int mm_compose_wide_backward(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                                 const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                                 int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                                 int nu, const double* head_scale, const double* head_shift,
                                                 const void* target, const void* precis, const void* tape, size_t tape_bytes,
                                                 const void* g_cost, void* g_policy, void* g_mx0, void* g_Sxx0,
                                                 void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                                 int32_t* status, void* stream) {
  return mm_rollout_composed_backward_nd_impl(drift_packed, drift_bytes, drift_L, drift_M, drift_d, policy_packed, policy_bytes,
                                              policy_M, policy_d, dtype, B, H, dt, nx, na, active_dims, nu, head_scale, head_shift,
                                              target, precis, tape, tape_bytes, g_cost, nullptr, nullptr, g_policy, g_mx0, g_Sxx0,
                                              ws_drift, ws_drift_bytes, ws_bwd, ws_bwd_bytes, status, stream, false, nullptr, true);
}

extern "C" int mm_compose_wide_backward_seeded(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M,
                                                        int drift_d, const void* policy_packed, size_t policy_bytes, int policy_M,
                                                        int policy_d, int dtype, int B, int H, double dt, int nx, int na,
                                                        const int32_t* active_dims, int nu, const double* head_scale,
                                                        const double* head_shift, const void* target, const void* precis,
                                                        const void* tape, size_t tape_bytes, const void* g_cost,
                                                        const void* g_xm, const void* g_xS,
                                                        void* g_policy, void* g_mx0, void* g_Sxx0,
                                                        void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                                        int32_t* status, void* stream) {
  return mm_rollout_composed_backward_nd_impl(drift_packed, drift_bytes, drift_L, drift_M, drift_d, policy_packed, policy_bytes,
                                              policy_M, policy_d, dtype, B, H, dt, nx, na, active_dims, nu, head_scale, head_shift,
                                              target, precis, tape, tape_bytes, g_cost, g_xm, g_xS, g_policy, g_mx0, g_Sxx0,
                                              ws_drift, ws_drift_bytes, ws_bwd, ws_bwd_bytes, status, stream, false, nullptr, true);
}

// a coregionalised drift (the tape of mm_rollout_composed_taped_nd_mixed): mix_W as mm_rollout_composed_backward_nd_mixed
extern "C" int mm_compose_wide_backward_mixed(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M,
                                                       int drift_d, const void* policy_packed, size_t policy_bytes, int policy_M,
                                                       int policy_d, int dtype, int B, int H, double dt, int nx, int na,
                                                       const int32_t* active_dims, int nu, const double* head_scale,
                                                       const double* head_shift, const void* target, const void* precis,
                                                       const void* tape, size_t tape_bytes, const void* g_cost,
                                                       void* g_policy, void* g_mx0, void* g_Sxx0,
                                                       void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                                       int32_t* status, void* stream, const double* mix_W) {
  return mm_rollout_composed_backward_nd_impl(drift_packed, drift_bytes, drift_L, drift_M, drift_d, policy_packed, policy_bytes,
                                              policy_M, policy_d, dtype, B, H, dt, nx, na, active_dims, nu, head_scale, head_shift,
                                              target, precis, tape, tape_bytes, g_cost, nullptr, nullptr, g_policy, g_mx0, g_Sxx0,
                                              ws_drift, ws_drift_bytes, ws_bwd, ws_bwd_bytes, status, stream, true, mix_W, true);
}

extern "C" int mm_compose_wide_backward_mixed_seeded(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M,
                                                              int drift_d, const void* policy_packed, size_t policy_bytes,
                                                              int policy_M, int policy_d, int dtype, int B, int H, double dt, int nx,
                                                              int na, const int32_t* active_dims, int nu, const double* head_scale,
                                                              const double* head_shift, const void* target, const void* precis,
                                                              const void* tape, size_t tape_bytes, const void* g_cost,
                                                              const void* g_xm, const void* g_xS,
                                                              void* g_policy, void* g_mx0, void* g_Sxx0,
                                                              void* ws_drift, size_t ws_drift_bytes, void* ws_bwd,
                                                              size_t ws_bwd_bytes, int32_t* status, void* stream,
                                                              const double* mix_W) {
  return mm_rollout_composed_backward_nd_impl(drift_packed, drift_bytes, drift_L, drift_M, drift_d, policy_packed, policy_bytes,
                                              policy_M, policy_d, dtype, B, H, dt, nx, na, active_dims, nu, head_scale, head_shift,
                                              target, precis, tape, tape_bytes, g_cost, g_xm, g_xS, g_policy, g_mx0, g_Sxx0,
                                              ws_drift, ws_drift_bytes, ws_bwd, ws_bwd_bytes, status, stream, true, mix_W, true);
}
