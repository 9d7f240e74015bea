// Reverse-mode (adjoint) arithmetic of the composed rollout step for policies with SEVERAL actions (mm_compose_nd.hip): what
// mm_adjoint.h holds for one action, with nu policy latents and nd = ne + nu.
//   mma_step_bwd_nd      adjoint of mmc_step_body_nd: mma_step_bwd with cp [ne][nu] -- the action columns of Cov(x, d) are
//                        Sxe . cp[:, a]
//   mma_head_bwd_nd      adjoint of k_compose_head_nd (moment_matching/bijectors.py:39-69, n-D branch): the diagonal as
//                        mma_head_bwd (Owen's T), the pairs i < j through Phi2(z_i, z_j; rho_ij) with the closed-form partials
//                        special._BvnCdf.backward uses -- phi(h) Phi((k - rho h) / sqrt(1 - rho^2)), the same in k, the bivariate
//                        density in rho -- not the derivative of the quadrature; the Frechet clamp and the clip of rho are
//                        ignored in the derivative, as there
//   mma_policy_pair_bwd  adjoint of one off-diagonal entry Sff_aa' = sum_ij w^a_i w^a'_j expm1(delta_ij) of the mean-only
//                        policy match with L = nu latents (moment_matching/models.py:200-299, MM_FULL_OUTPUT_COV, no model
//                        uncertainty) w.r.t. the input moments AND both latents' packed parameters
//   mma_policy_nd_bwd    the whole match: mma_policy_small_bwd per latent (f1_a, Sff_aa, cross[:, a]) + the nu (nu - 1) / 2 pairs
// All in f64, written for an execution context `Ctx` exactly as mm_adjoint.h (tests/hostcheck/mm_adjoint_nd_host.hip is the CPU
// build that tests/test_adjoint_nd_host.py checks against autograd).
#pragma once
#include "mm_adjoint.h"

// ---------------------------------------------------------------------------------------------------------------------
// mma_step_bwd_nd: adjoint of mmc_step_body_nd
//   Sxd = rows [Sxe_r, Sxe_r . cp] (encoded dims; cp [ne][nu]) | rows of Sdd (the other dims);  Sxf = Sxd dcross;
//   m' = m + dt df1;  S' = S + dt (Sxf + Sxf^T) + dt^2 dSff.
// in : gm1 [nx], gS1 [nx, nx]
// out: gSxe [nx, ne], gcp [ne, nu], gSdd [nd, nd], gdf1 [nx], gdSff [nx, nx], gdcross [nd, nx]  (all ASSIGNED);
//      the adjoint of (m, S) through the direct terms is (gm1, gS1) itself.
// sm: mma_step_bwd_scratch(nx, nd) doubles.
// ---------------------------------------------------------------------------------------------------------------------
MMA_FN void mma_step_bwd_nd(Ctx c, const MMComposeDims& D, double dt, const double* Sxe, const double* cp, const double* Sdd,
                            const double* dcross, const double* gm1, const double* gS1, double* gSxe, double* gcp, double* gSdd,
                            double* gdf1, double* gdSff, double* gdcross, double* sm) {
  const int lane = c.lane(), nl = c.nl();
  const int nx = D.nx, na = D.na, ne = D.ne, nd = D.nd, n2 = 2 * na, nu = nd - ne;
  double* Sxd = sm; double* gSxd = Sxd + nx * nd; double* gSxf = gSxd + nx * nd;
  for (int idx = lane; idx < nx * nd; idx += nl) {
    const int r = idx / nd, k = idx - r * nd;
    const int sl = D.slot[r];
    double v;
    if (sl < na) {
      if (k < ne) v = Sxe[r * ne + k];
      else { double s = 0.0; for (int l = 0; l < ne; ++l) s = fma(Sxe[r * ne + l], cp[l * nu + (k - ne)], s); v = s; }
    } else {
      v = Sdd[(n2 + (sl - na)) * nd + k];
    }
    Sxd[idx] = v;
  }
  for (int idx = lane; idx < nx * nx; idx += nl) {
    const int r = idx / nx, cc = idx - r * nx;
    gSxf[idx] = dt * (gS1[idx] + gS1[cc * nx + r]);
    gdSff[idx] = dt * dt * gS1[idx];
  }
  for (int i = lane; i < nx; i += nl) gdf1[i] = dt * gm1[i];
  c.sync();
  for (int idx = lane; idx < nx * nd; idx += nl) {        // gSxd = gSxf dcross^T
    const int r = idx / nd, k = idx - r * nd;
    double s = 0.0;
    for (int cc = 0; cc < nx; ++cc) s = fma(gSxf[r * nx + cc], dcross[k * nx + cc], s);
    gSxd[idx] = s;
  }
  for (int idx = lane; idx < nd * nx; idx += nl) {        // gdcross = Sxd^T gSxf
    const int k = idx / nx, cc = idx - k * nx;
    double s = 0.0;
    for (int r = 0; r < nx; ++r) s = fma(Sxd[r * nd + k], gSxf[r * nx + cc], s);
    gdcross[idx] = s;
  }
  c.sync();
  for (int idx = lane; idx < nx * ne; idx += nl) {
    const int r = idx / ne, k = idx - r * ne;
    double v = 0.0;
    if (D.slot[r] < na) {
      v = gSxd[r * nd + k];
      for (int a = 0; a < nu; ++a) v = fma(gSxd[r * nd + ne + a], cp[k * nu + a], v);
    }
    gSxe[idx] = v;
  }
  for (int idx = lane; idx < ne * nu; idx += nl) {
    const int l = idx / nu, a = idx - l * nu;
    double s = 0.0;
    for (int i = 0; i < na; ++i) { const int r = D.active[i]; s = fma(gSxd[r * nd + ne + a], Sxe[r * ne + l], s); }
    gcp[idx] = s;
  }
  for (int idx = lane; idx < nd * nd; idx += nl) {
    const int i = idx / nd, k = idx - i * nd;
    gSdd[idx] = (i >= n2 && i < ne) ? gSxd[D.inactive[i - n2] * nd + k] : 0.0;
  }
  c.sync();
}

// ---------------------------------------------------------------------------------------------------------------------
// mma_head_bwd_nd: adjoint of k_compose_head_nd.  Per action i:
//   v_i = max(pSff_ii, 0), isq_i = 1 / sqrt(v_i + 1), z_i = isq_i pf1_i, y1_i = Phi(z_i), y2_ii = y1_i - 2 T(z_i, 1 / sqrt(1 + 2 v_i)),
//   hpre_i = isq_i phi(z_i) scale_i, mu_u_i = scale_i (y1_i + shift_i), cp[:, i] = pcross[:, i] hpre_i;
// per pair i < j:  rho_ij = pSff_ij isq_i isq_j (the UPPER entry is the one read), y2_ij = y2_ji = Phi2(z_i, z_j; rho_ij);
//   Suu_ij = scale_i scale_j (y2_ij - y1_i y1_j), Seu = See cp, md = [me, mu_u], Sdd = [[See, Seu], [Seu^T, Suu]].
// in : gmd [nd], gSdd [nd, nd], gcp [ne, nu]  (adjoints of md, Sdd and of cp's use in the step's bookkeeping)
// out: gme [ne], gSee [ne, ne], gpcross [ne, nu], gpf1 [nu], gpSff [nu, nu] (lower triangle zero), all ASSIGNED.
// sm: mma_head_bwd_nd_scratch(ne, nu) doubles.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int mma_head_bwd_nd_scratch(int ne, int nu) { return 2 * ne * nu + 2 * nu; }

MMA_FN void mma_head_bwd_nd(Ctx c, int ne, int nu, const double* scale, const double* shift, const double* pf1, const double* pSff,
                            const double* pcross, const double* See, const double* gmd, const double* gSdd, const double* gcp,
                            double* gme, double* gSee, double* gpcross, double* gpf1, double* gpSff, double* sm) {
  const int lane = c.lane(), nl = c.nl(), nd = ne + nu;
  double* gct = sm;                 // [ne][nu] total adjoint of cp
  double* gsu = gct + ne * nu;      // [ne][nu] adjoint of Seu
  double* hpre = gsu + ne * nu;     // [nu]
  double* ghp = hpre + nu;          // [nu]
  for (int idx = lane; idx < ne * nu; idx += nl) {
    const int k = idx / nu, j = idx - k * nu;
    gsu[idx] = gSdd[k * nd + ne + j] + gSdd[(ne + j) * nd + k];
  }
  for (int j = lane; j < nu; j += nl) {
    const double v = pSff[j * nu + j] > 0.0 ? pSff[j * nu + j] : 0.0;
    const double is = 1.0 / sqrt(v + 1.0), z = is * pf1[j];
    hpre[j] = is * MMA_INV_SQRT_2PI * exp(-0.5 * z * z) * scale[j];
  }
  c.sync();
  for (int idx = lane; idx < ne * nu; idx += nl) {         // direct + through Seu = See cp
    const int l = idx / nu, j = idx - l * nu;
    double s = gcp[idx];
    for (int k = 0; k < ne; ++k) s = fma(See[k * ne + l], gsu[k * nu + j], s);
    gct[idx] = s;
  }
  c.sync();
  for (int k = lane; k < ne; k += nl) gme[k] = gmd[k];
  for (int idx = lane; idx < ne * nu; idx += nl) gpcross[idx] = gct[idx] * hpre[idx % nu];
  for (int idx = lane; idx < ne * ne; idx += nl) {
    const int k = idx / ne, l = idx - k * ne;
    double s = gSdd[k * nd + l];
    for (int j = 0; j < nu; ++j) s = fma(gsu[k * nu + j], pcross[l * nu + j] * hpre[j], s);
    gSee[idx] = s;
  }
  for (int j = lane; j < nu; j += nl) {
    double s = 0.0;
    for (int k = 0; k < ne; ++k) s = fma(gct[k * nu + j], pcross[k * nu + j], s);
    ghp[j] = s;
  }
  c.sync();
  if (lane == 0) {                                         // nu <= 4: the scalar chain of every action and pair
    double z[MMC_NU], isq[MMC_NU], y1[MMC_NU], phi[MMC_NU], gz[MMC_NU], gisq[MMC_NU];
    for (int i = 0; i < nu; ++i) {
      const double v = pSff[i * nu + i] > 0.0 ? pSff[i * nu + i] : 0.0;
      isq[i] = 1.0 / sqrt(v + 1.0); z[i] = isq[i] * pf1[i];
      phi[i] = MMA_INV_SQRT_2PI * exp(-0.5 * z[i] * z[i]);
      y1[i] = 0.5 * erfc(-z[i] * 0.70710678118654752440);
      for (int j = 0; j < nu; ++j) gpSff[i * nu + j] = 0.0;
    }
    for (int i = 0; i < nu; ++i) {                         // y1, the diagonal's Owen's T, hpre: as mma_head_bwd
      double gy1 = scale[i] * gmd[ne + i];
      for (int q = 0; q < nu; ++q)
        gy1 -= scale[i] * scale[q] * y1[q] * (gSdd[(ne + i) * nd + ne + q] + gSdd[(ne + q) * nd + ne + i]);
      const double gy2 = scale[i] * scale[i] * gSdd[(ne + i) * nd + ne + i];
      gy1 += gy2;
      const double gT = -2.0 * gy2;
      const double v = pSff[i * nu + i] > 0.0 ? pSff[i * nu + i] : 0.0;
      const double aa = 1.0 / sqrt(1.0 + 2.0 * v);
      const double PhiAz = 0.5 * erfc(-aa * z[i] * 0.70710678118654752440);
      gz[i] = gy1 * phi[i] - gT * phi[i] * (PhiAz - 0.5) - ghp[i] * z[i] * hpre[i];
      const double gaa = gT * exp(-0.5 * z[i] * z[i] * (1.0 + aa * aa)) * MMA_INV_2PI / (1.0 + aa * aa);
      gisq[i] = ghp[i] * scale[i] * phi[i];
      gpf1[i] = -gaa * aa * aa * aa;                        // (parked: the aa part of the adjoint of v_i)
    }
    for (int i = 0; i < nu; ++i) {
      for (int j = i + 1; j < nu; ++j) {                   // Phi2(h, k; rho), closed-form partials
        const double g = scale[i] * scale[j] * (gSdd[(ne + i) * nd + ne + j] + gSdd[(ne + j) * nd + ne + i]);
        const double sij = pSff[i * nu + j];
        const double rho = sij * isq[i] * isq[j], h = z[i], k = z[j];
        const double s2 = 1.0 - rho * rho, s = sqrt(s2);
        gz[i] += g * phi[i] * 0.5 * erfc(-((k - rho * h) / s) * 0.70710678118654752440);
        gz[j] += g * phi[j] * 0.5 * erfc(-((h - rho * k) / s) * 0.70710678118654752440);
        const double grho = g * exp(-(h * h - 2.0 * rho * h * k + k * k) / (2.0 * s2)) * MMA_INV_2PI / s;
        gpSff[i * nu + j] = grho * isq[i] * isq[j];
        gisq[i] += grho * sij * isq[j];
        gisq[j] += grho * sij * isq[i];
      }
    }
    for (int i = 0; i < nu; ++i) {
      const double gi = gisq[i] + gz[i] * pf1[i];
      const double gvx = -0.5 * gi * isq[i] * isq[i] * isq[i] + gpf1[i];
      gpSff[i * nu + i] = pSff[i * nu + i] > 0.0 ? gvx : 0.0;
      gpf1[i] = gz[i] * isq[i];
    }
  }
  (void)shift;
  c.sync();
}

// ---------------------------------------------------------------------------------------------------------------------
// mma_policy_pair_bwd: adjoint of Sff_ab = sum_ij w^a_i w^b_j expm1(delta_ij) for two DIFFERENT latents a, b of the mean-only match
// (autodiff.small_algebra is the d x d algebra, autodiff.moment_match_torch the evaluation):
//   A = Lambda_a, B = Lambda_b (diagonal), Pa = (Sigma + A)^-1, Pb = (Sigma + B)^-1, V = A B (A + B)^-1, W = (Sigma + V)^-1,
//   T = V - V W V, G = A^-1 T B^-1, Dr = A^-1 - Pa - A^-1 T A^-1, Dc = B^-1 - Pb - B^-1 T B^-1,
//   const = -1/2 log|Sigma + V| + 1/2 log|V| - 1/2 log|A| - 1/2 log|B| + 1/2 log|Sigma + A| + 1/2 log|Sigma + B|,
//   zeta_i = z^a_i - mu, zeta'_j = z^b_j - mu, w^a_i = beta^a_i var_a |A|^1/2 |Sigma + A|^-1/2 exp(-zeta_i^T Pa zeta_i / 2),
//   delta_ij = const - zeta_i^T Dr zeta_i / 2 - zeta'_j^T Dc zeta'_j / 2 + zeta_i^T G zeta'_j.
// The latents' means do not enter a centred pair.  The lengthscale chain runs through A, B in Pa, Pb, V, T, G, Dr, Dc, the
// log-normalisers and const.
// in : g = gSff[a][b] + gSff[b][a].   gmu [d], gSig [d, d] (symmetric part) ACCUMULATED;  gpa, gpb (mm_policy_grad_len each, the
// two latents' slabs) ACCUMULATED.  Sigma: the lower triangle is read.  sm: mma_policy_pair_bwd_scratch(M, d, nl) doubles.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int mma_policy_pair_bwd_scratch(int M, int d, int nl) {
  const int dp = d + 1, ns = mma_policy_nsub(M, nl);
  return 18 * d * dp + M * (11 * d + 14) + ns * M * (d + 2) + 4 * d + 16;
}

MMA_FN void mma_policy_pair_bwd(Ctx c, int M, int d, const double* Za, const double* betaa, const double* la2, double vara,
                                const double* Zb, const double* betab, const double* lb2, double varb, const double* mu,
                                const double* Sigma, double g, double* gmu, double* gSig, double* gpa, double* gpb, double* sm,
                                bool* ok) {
  const int lane = c.lane(), nl = c.nl(), dp = d + 1, msz = d * dp, ns = mma_policy_nsub(M, nl), Md = M * d;
  double* Sg = sm;           double* Pa = Sg + msz;    double* Pb = Pa + msz;    double* Wv = Pb + msz;   double* Yw = Wv + msz;
  double* Tm = Yw + msz;     double* Gm = Tm + msz;    double* Dr = Gm + msz;    double* Dc = Dr + msz;
  double* PaB = Dc + msz;    double* PbB = PaB + msz;  double* R2 = PbB + msz;   double* K2 = R2 + msz;   double* Xm = K2 + msz;
  double* TB = Xm + msz;     double* W1 = TB + msz;    double* W2 = W1 + msz;    double* SvB = W2 + msz;
  double* za = SvB + msz;    double* zb = za + Md;     double* Pza = zb + Md;    double* Pzb = Pza + Md;
  double* Dza = Pzb + Md;    double* Dzb = Dza + Md;   double* Gzb = Dzb + Md;   double* Ua = Gzb + Md;   double* Ub = Ua + Md;
  double* zba = Ub + Md;     double* zbb = zba + Md;
  double* wa = zbb + Md;     double* qa = wa + M;      double* rhoa = qa + M;    double* wb = rhoa + M;   double* qb = wb + M;
  double* gamb = qb + M;     double* ra = gamb + M;    double* Ra = ra + M;      double* cb = Ra + M;     double* Kb = cb + M;
  double* mba = Kb + M;      double* mbb = mba + M;    double* wba = mbb + M;    double* wbb = wba + M;
  double* part = wbb + M;                  // [ns][M][d + 2]
  double* Vv = part + ns * M * (d + 2);    // [d] V
  double* Vb = Vv + d;                     // [d] adjoint of V
  double* Lab = Vb + d;                    // [d] adjoint of A
  double* Lbb = Lab + d;                   // [d] adjoint of B
  double* sc = Lbb + d;                    // scalars [16]

  for (int idx = lane; idx < d * d; idx += nl) {
    const int i = idx / d, j = idx - i * d;
    const double s = i >= j ? Sigma[i * d + j] : Sigma[j * d + i];
    const double v = la2[i] * lb2[i] / (la2[i] + lb2[i]);
    Sg[i * dp + j] = s;
    Pa[i * dp + j] = s + (i == j ? la2[i] : 0.0);
    Pb[i * dp + j] = s + (i == j ? lb2[i] : 0.0);
    Wv[i * dp + j] = s + (i == j ? v : 0.0);
    if (i == j) Vv[i] = v;
  }
  c.sync();
  const double lda = mma_spd_inverse(c, Pa, Yw, d, dp, ok);
  const double ldb = mma_spd_inverse(c, Pb, Yw, d, dp, ok);
  const double ldv = mma_spd_inverse(c, Wv, Yw, d, dp, ok);
  double sla = 0.0, slb = 0.0, slv = 0.0;
  for (int k = 0; k < d; ++k) { sla += log(la2[k]); slb += log(lb2[k]); slv += log(Vv[k]); }
  const double lna = log(vara) + 0.5 * sla - 0.5 * lda, lnb = log(varb) + 0.5 * slb - 0.5 * ldb;
  const double cst = -0.5 * ldv + 0.5 * slv - 0.5 * sla - 0.5 * slb + 0.5 * lda + 0.5 * ldb;
  for (int idx = lane; idx < d * d; idx += nl) {
    const int i = idx / d, j = idx - i * d;
    const double t = (i == j ? Vv[i] : 0.0) - Vv[i] * Wv[i * dp + j] * Vv[j];
    Tm[i * dp + j] = t;
    Gm[i * dp + j] = t / (la2[i] * lb2[j]);
    Dr[i * dp + j] = (i == j ? 1.0 / la2[i] : 0.0) - Pa[i * dp + j] - t / (la2[i] * la2[j]);
    Dc[i * dp + j] = (i == j ? 1.0 / lb2[i] : 0.0) - Pb[i * dp + j] - t / (lb2[i] * lb2[j]);
  }
  c.sync();
  // ---- per centre of either latent: forward quantities -------------------------------------------------------------
  for (int idx = lane; idx < 2 * M; idx += nl) {
    const bool second = idx >= M;
    const int m = second ? idx - M : idx;
    const double* Z = second ? Zb : Za;
    const double* Pm = second ? Pb : Pa;
    const double* Dm = second ? Dc : Dr;
    double* zs = second ? zb : za; double* Pz = second ? Pzb : Pza; double* Dz = second ? Dzb : Dza;
    for (int k = 0; k < d; ++k) zs[m * d + k] = Z[m * d + k] - mu[k];
    double maha = 0.0, r1 = 0.0;
    for (int i = 0; i < d; ++i) {
      double tp = 0.0, te = 0.0, tg = 0.0;
      for (int k = 0; k < d; ++k) {
        const double zk = zs[m * d + k];
        tp = fma(Pm[i * dp + k], zk, tp); te = fma(Dm[i * dp + k], zk, te); tg = fma(Gm[i * dp + k], zk, tg);
      }
      Pz[m * d + i] = tp; Dz[m * d + i] = te;
      if (second) Gzb[m * d + i] = tg;
      maha = fma(zs[m * d + i], tp, maha);
      r1 = fma(zs[m * d + i], te, r1);
    }
    if (second) { qb[m] = exp(lnb - 0.5 * maha); wb[m] = betab[m] * qb[m]; gamb[m] = -0.5 * r1; }
    else { qa[m] = exp(lna - 0.5 * maha); wa[m] = betaa[m] * qa[m]; rhoa[m] = -0.5 * r1; }
  }
  c.sync();
  // ---- M x M sweep, rows: r_i = sum_j E_ij w'_j, R_i = sum_j Omega_ij, U_i = sum_j Omega_ij zeta'_j ----------------------
  for (int idx = lane; idx < ns * M; idx += nl) {
    const int i = idx % M, sub = idx / M;
    double ri = 0.0, Ri = 0.0;
    double* pu = part + (size_t)idx * (d + 2);
    for (int k = 0; k < d; ++k) pu[k] = 0.0;
    for (int j = sub; j < M; j += ns) {
      double delta = rhoa[i] + gamb[j] + cst;
      for (int k = 0; k < d; ++k) delta = fma(za[i * d + k], Gzb[j * d + k], delta);
      const double Ex = expm1(fmin(delta, MM_EXP_CAP_F64));
      const double om = wa[i] * wb[j] * (Ex + 1.0);
      ri = fma(Ex, wb[j], ri); Ri += om;
      for (int k = 0; k < d; ++k) pu[k] = fma(om, zb[j * d + k], pu[k]);
    }
    pu[d] = ri; pu[d + 1] = Ri;
  }
  c.sync();
  for (int idx = lane; idx < M * (d + 2); idx += nl) {
    const int i = idx / (d + 2), k = idx - i * (d + 2);
    double v = 0.0;
    for (int sub = 0; sub < ns; ++sub) v += part[(size_t)(sub * M + i) * (d + 2) + k];
    if (k < d) Ua[i * d + k] = v; else if (k == d) ra[i] = v; else Ra[i] = v;
  }
  c.sync();
  // ---- the same sweep, columns: c_j = sum_i w_i E_ij, K_j = sum_i Omega_ij, U'_j = sum_i Omega_ij zeta_i ------------------
  for (int idx = lane; idx < ns * M; idx += nl) {
    const int j = idx % M, sub = idx / M;
    double cj = 0.0, Kj = 0.0;
    double* pu = part + (size_t)idx * (d + 2);
    for (int k = 0; k < d; ++k) pu[k] = 0.0;
    for (int i = sub; i < M; i += ns) {
      double delta = rhoa[i] + gamb[j] + cst;
      for (int k = 0; k < d; ++k) delta = fma(za[i * d + k], Gzb[j * d + k], delta);
      const double Ex = expm1(fmin(delta, MM_EXP_CAP_F64));
      const double om = wa[i] * wb[j] * (Ex + 1.0);
      cj = fma(Ex, wa[i], cj); Kj += om;
      for (int k = 0; k < d; ++k) pu[k] = fma(om, za[i * d + k], pu[k]);
    }
    pu[d] = cj; pu[d + 1] = Kj;
  }
  c.sync();
  for (int idx = lane; idx < M * (d + 2); idx += nl) {
    const int j = idx / (d + 2), k = idx - j * (d + 2);
    double v = 0.0;
    for (int sub = 0; sub < ns; ++sub) v += part[(size_t)(sub * M + j) * (d + 2) + k];
    if (k < d) Ub[j * d + k] = v; else if (k == d) cb[j] = v; else Kb[j] = v;
  }
  c.sync();
  // ---- per-centre adjoints ------------------------------------------------------------------------------------------------
  for (int i = lane; i < M; i += nl) {
    wba[i] = g * ra[i]; mba[i] = -0.5 * wba[i] * wa[i];
    wbb[i] = g * cb[i]; mbb[i] = -0.5 * wbb[i] * wb[i];
  }
  c.sync();
  for (int idx = lane; idx < Md; idx += nl) {
    const int i = idx / d, k = idx - i * d;
    double ga = 0.0, gb = 0.0;
    for (int l = 0; l < d; ++l) { ga = fma(Gm[k * dp + l], Ua[i * d + l], ga); gb = fma(Gm[l * dp + k], Ub[i * d + l], gb); }
    zba[idx] = g * (ga - Ra[i] * Dza[idx]) + 2.0 * mba[i] * Pza[idx];
    zbb[idx] = g * (gb - Kb[i] * Dzb[idx]) + 2.0 * mbb[i] * Pzb[idx];
  }
  c.sync();
  // ---- sums over the centres ----------------------------------------------------------------------------------------------
  for (int idx = lane; idx < d * d; idx += nl) {
    const int a = idx / d, b = idx - a * d;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
    for (int i = 0; i < M; ++i) {
      const double zza = za[i * d + a] * za[i * d + b], zzb = zb[i * d + a] * zb[i * d + b];
      v0 = fma(mba[i], zza, v0); v1 = fma(mbb[i], zzb, v1);
      v2 = fma(Ra[i], zza, v2); v3 = fma(Kb[i], zzb, v3);
      v4 = fma(za[i * d + a], Ua[i * d + b], v4);
    }
    // adjoints of Dr, Dc, G:  DrB = -g R2 / 2, DcB = -g K2 / 2, GB = g X;  Pa's adjoint takes -DrB, Pb's -DcB
    R2[a * dp + b] = -0.5 * g * v2; K2[a * dp + b] = -0.5 * g * v3; Xm[a * dp + b] = g * v4;
    PaB[a * dp + b] = v0 + 0.5 * g * v2; PbB[a * dp + b] = v1 + 0.5 * g * v3;
  }
  for (int k = lane; k < d; k += nl) {
    double s = 0.0;
    for (int i = 0; i < M; ++i) s += zba[i * d + k] + zbb[i * d + k];
    gmu[k] -= s;
  }
  if (lane == 0) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < M; ++i) { s0 = fma(wba[i], wa[i], s0); s1 = fma(wbb[i], wb[i], s1); s2 += Ra[i]; }
    sc[0] = s0; sc[1] = s1; sc[2] = g * s2;              // adjoints of lognorm_a, lognorm_b, const
  }
  c.sync();
  const double lnab = sc[0], lnbb = sc[1], cbar = sc[2];
  const double ldab = 0.5 * cbar - 0.5 * lnab, ldbb = 0.5 * cbar - 0.5 * lnbb;
  // ---- the d x d algebra, in reverse ----------------------------------------------------------------------------------------
  for (int idx = lane; idx < d * d; idx += nl) {           // adjoint of T (symmetrised: T is symmetric by construction)
    const int a = idx / d, b = idx - a * d;
    const double tab = -R2[a * dp + b] / (la2[a] * la2[b]) - K2[a * dp + b] / (lb2[a] * lb2[b]);
    TB[a * dp + b] = tab + 0.5 * (Xm[a * dp + b] / (la2[a] * lb2[b]) + Xm[b * dp + a] / (la2[b] * lb2[a]));
  }
  mma_mm(c, d, d, d, PaB, dp, Pa, dp, Yw, dp);
  c.sync();
  mma_mm(c, d, d, d, Pa, dp, Yw, dp, W1, dp);              // W1 = Pa PaB Pa
  c.sync();
  mma_mm(c, d, d, d, PbB, dp, Pb, dp, Yw, dp);
  c.sync();
  mma_mm(c, d, d, d, Pb, dp, Yw, dp, W2, dp);              // W2 = Pb PbB Pb
  c.sync();
  for (int idx = lane; idx < d * d; idx += nl) {
    const int a = idx / d, b = idx - a * d;
    Yw[a * dp + b] = Vv[a] * TB[a * dp + b] * Vv[b];
  }
  c.sync();
  mma_mm(c, d, d, d, Yw, dp, Wv, dp, SvB, dp);
  c.sync();
  mma_mm(c, d, d, d, Wv, dp, SvB, dp, Yw, dp);             // Yw = W (V TB V) W
  c.sync();
  for (int idx = lane; idx < d * d; idx += nl) {
    const int a = idx / d, b = idx - a * d;
    const double sv = 0.5 * (Yw[a * dp + b] + Yw[b * dp + a]) - 0.5 * cbar * Wv[a * dp + b];
    SvB[a * dp + b] = sv;
    const double ab = -0.5 * (W1[a * dp + b] + W1[b * dp + a]) + ldab * Pa[a * dp + b];
    const double bb = -0.5 * (W2[a * dp + b] + W2[b * dp + a]) + ldbb * Pb[a * dp + b];
    PaB[a * dp + b] = ab; PbB[a * dp + b] = bb;            // adjoints of Sigma + A, Sigma + B (PaB, PbB are spent)
  }
  c.sync();
  for (int idx = lane; idx < d * d; idx += nl) {
    const int a = idx / d, b = idx - a * d;
    gSig[a * d + b] += PaB[a * dp + b] + PbB[a * dp + b] + SvB[a * dp + b];
  }
  for (int k = lane; k < d; k += nl) {
    double swt = 0.0, sdr = 0.0, sdc = 0.0, sga = 0.0, sgb = 0.0;
    for (int l = 0; l < d; ++l) {
      swt = fma(Wv[k * dp + l] * Vv[l], TB[l * dp + k], swt);
      sdr = fma(R2[k * dp + l], Tm[k * dp + l] / la2[l], sdr);
      sdc = fma(K2[k * dp + l], Tm[k * dp + l] / lb2[l], sdc);
      sga = fma(Xm[k * dp + l], Gm[k * dp + l], sga);
      sgb = fma(Xm[l * dp + k], Gm[l * dp + k], sgb);
    }
    const double vbar = TB[k * dp + k] - 2.0 * swt + 0.5 * cbar / Vv[k] + SvB[k * dp + k];
    const double ia = 1.0 / la2[k], ib = 1.0 / lb2[k];
    Lab[k] = -R2[k * dp + k] * ia * ia + 2.0 * sdr * ia * ia - sga * ia - 0.5 * cbar * ia + 0.5 * lnab * ia
           + PaB[k * dp + k] + vbar * (Vv[k] * ia) * (Vv[k] * ia);
    Lbb[k] = -K2[k * dp + k] * ib * ib + 2.0 * sdc * ib * ib - sgb * ib - 0.5 * cbar * ib + 0.5 * lnbb * ib
           + PbB[k * dp + k] + vbar * (Vv[k] * ib) * (Vv[k] * ib);
    Vb[k] = vbar;
  }
  c.sync();
  // ---- the two latents' packed gradients (accumulated) ------------------------------------------------------------------------
  for (int idx = lane; idx < Md; idx += nl) { gpa[idx] += zba[idx]; gpb[idx] += zbb[idx]; }
  for (int i = lane; i < M; i += nl) { gpa[Md + i] += wba[i] * qa[i]; gpb[Md + i] += wbb[i] * qb[i]; }
  for (int k = lane; k < d; k += nl) { gpa[Md + M + k] += Lab[k]; gpb[Md + M + k] += Lbb[k]; }
  if (lane == 0) { gpa[Md + M + d] += lnab / vara; gpb[Md + M + d] += lnbb / varb; }
  c.sync();
}

// ---------------------------------------------------------------------------------------------------------------------
// mma_policy_nd_bwd: adjoint of the policy match with L = nu latents (mean-only, full output covariance, no model uncertainty).
//   Z [nu][M][d], beta [nu][M], ls2 [nu][d], var [nu] in the caller's order (M <= 256: the pack does not permute the centres).
// in : gf1 [nu], gSff [nu][nu] (need not be symmetric), gcross [d][nu].
// out: gmu [d], gSig [d, d] (symmetric) ASSIGNED;  gpar [nu][mm_policy_grad_len(M, d)] ACCUMULATED.
// The nu latent items and the nu (nu - 1) / 2 pair items run in turn and are summed in that fixed order.
// sm: mma_policy_nd_bwd_scratch(M, d, nl) doubles.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int mma_policy_nd_bwd_scratch(int M, int d, int nl) {
  const int a = mma_policy_small_bwd_scratch(M, d, nl), b = mma_policy_pair_bwd_scratch(M, d, nl);
  return (a > b ? a : b) + d * d + 2 * d;
}

template <class Ctx, int DK>
__host__ __device__ inline void mma_policy_nd_bwd(Ctx c, int nu, int M, int d, const double* Z, const double* beta, const double* ls2,
                                                  const double* var, const double* mu, const double* Sigma, const double* gf1,
                                                  const double* gSff, const double* gcross, double* gmu, double* gSig,
                                                  double* gpar, double* sm, bool* ok) {
  const int lane = c.lane(), nl = c.nl();
  const size_t glen = (size_t)M * d + M + d + 2;            // mm_policy_grad_len (mm_compose.h; host only)
  double* tS = sm; double* tm = tS + d * d; double* gc = tm + d; double* rest = gc + d;
  for (int idx = lane; idx < d * d; idx += nl) gSig[idx] = 0.0;
  for (int k = lane; k < d; k += nl) gmu[k] = 0.0;
  c.sync();
  for (int a = 0; a < nu; ++a) {
    for (int k = lane; k < d; k += nl) gc[k] = gcross[k * nu + a];
    c.sync();
    mma_policy_small_bwd<Ctx, DK>(c, M, d, Z + (size_t)a * M * d, beta + (size_t)a * M, ls2 + (size_t)a * d, var[a], mu, Sigma,
                                  gf1[a], gSff[a * nu + a], gc, tm, tS, gpar + a * glen, rest, ok);
    c.sync();
    for (int idx = lane; idx < d * d; idx += nl) gSig[idx] += tS[idx];
    for (int k = lane; k < d; k += nl) gmu[k] += tm[k];
    c.sync();
  }
  for (int a = 0; a < nu; ++a) {
    for (int b = a + 1; b < nu; ++b) {
      mma_policy_pair_bwd(c, M, d, Z + (size_t)a * M * d, beta + (size_t)a * M, ls2 + (size_t)a * d, var[a],
                          Z + (size_t)b * M * d, beta + (size_t)b * M, ls2 + (size_t)b * d, var[b], mu, Sigma,
                          gSff[a * nu + b] + gSff[b * nu + a], gmu, gSig, gpar + a * glen, gpar + b * glen, rest, ok);
      c.sync();
    }
  }
}
