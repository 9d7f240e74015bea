/*
 * gpflowpilco_mm.h -- C ABI of the MI355X (gfx950) moment-matched GP propagation.
 *
 * Drop-in boundary for the per-step hot path of j-wilson/GPflowPILCO:
 *   moment_matching(GaussianMoments, SVGP|GPR)            gpflow_pilco/moment_matching/models.py:44-299
 *   kernel_expectation  <K_xZ>, <K_Zx K_xZ'>              gpflow_pilco/utils/kernel_expectation.py:72-288
 *   MomentMatchingEuler.step                              gpflow_pilco/dynamics/solvers.py:108-135
 *
 * The reference has no FFI of its own (pure Python/TF); these entry points are what a
 * maintainer would bind from the handlers above.  Conventions:
 *   - every pointer is a DEVICE pointer unless it says "host"; row-major contiguous; the batch
 *     axis B is the leading axis, so a B-shard is a pointer offset;
 *   - the caller owns every buffer including the workspace (size from *_bytes queries);
 *   - calls only enqueue work (no allocation, no synchronisation; graph-capturable) in the order of `stream` (a hipStream_t
 *     passed as void*): when `stream` reaches the end of a call's work, everything the call enqueued is complete.  Some calls
 *     (mm_moment_match, the rollouts, mm_moment_match_with_sums / _backward) run independent latency-bound kernel chains on a
 *     library-owned side stream beside a long sweep and join it to `stream` before they return (fork / join by events; under
 *     stream capture the side stream joins the capture).  That side stream and its two events belong to the CALLER'S stream: one
 *     triple per (device, caller stream), created on first use and kept for the process -- calls on different streams share
 *     nothing and may run concurrently, one of them under HIP-graph capture (ABI users: one enqueuing thread per stream at a time,
 *     as for any stream-ordered API).  The stage API (mm_q_forward, mm_Q_reduce_forward) never leaves work on a side stream;
 *   - return value: 0 ok, <0 bad argument (MM_E_*), >0 a hipError_t;
 *   - `status` (device int32[4], zeroed by the caller, may be NULL): [0] = B - b for the smallest
 *     batch index b whose (Sigma + V) Cholesky was not positive definite (0 = all fine; outputs
 *     of that b are NaN), [1] = an item code.  The reference raises InvalidArgumentError there
 *     (kernel_expectation.py:125-126, models.py:271).  [2] / [3] (MM_F32 packs; ABI version 2): running counts of the
 *     (batch element, off-diagonal pair) items the forward / the backward re-reduced in f64 because the f32 sweep's own
 *     rounding-error estimate exceeded MM_ROUTE_TOL (3e-4) of the batch element's off-diagonal covariance scale
 *     (csrc/mm_route.hip): the f32 pack's accuracy contract -- what stays in f32 is within ~4e-5 of
 *     that scale (rounding; plus <= ~1e-5 systematic), the rest has f64 accuracy.  The reference computes these terms in float64 throughout
 *     (kernel_expectation.py:158-165).
 *   - `packed` / `packed_bytes`: the buffer filled by mm_pack_model and its size (whether C is
 *     present is inferred from the size).
 *
 * dtype selects the element type T of the state (mu, Sigma), outputs and the streaming
 * workspace.  All d x d algebra, log-normalisers, first moments and cross terms are done in
 * f64 regardless; T only governs the M x M inner reduction and storage.
 */
#ifndef GPFLOWPILCO_MM_H
#define GPFLOWPILCO_MM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_F32 0
#define MM_F64 1

#define MM_DMAX 32          /* largest supported GP input dimension d            */
#define MM_M_ALIGN 128      /* inducing-point axis is zero-padded to this multiple */

/* flags */
#define MM_FULL_OUTPUT_COV   1   /* models.py full_output_cov=True: Sff is [B,L,L]; else [B,L]     */
#define MM_MODEL_UNCERTAINTY 2   /* models.py model_uncertainty=True: adds E[Var f] (needs C)      */
#define MM_FORCE_GENERIC     4   /* use the portable VALU reduce kernel even where an MFMA one exists */
/* mm_Q_reduce_forward only: run a subset of its launches (none of the three bits = all three);
 * lets a caller bracket each kernel with its own events (bench.py does). */
#define MM_STAGE_DIAG        8   /* f64 reduce of the diagonal pairs a == a' (incl. the C-weighted term) */
#define MM_STAGE_OFFDIAG    16   /* T reduce of the off-diagonal pairs a < a'                          */
#define MM_STAGE_FINALIZE   32   /* partial slabs -> Sff                                               */
/* measurement aid: every tile of the reduce kernels takes its most expensive range tier (f32 reduce: all three
 * split-product stages + the exp2 branch; f64 reduce: the k ln2 + r form) whatever the data.  The tiers are all
 * valid on the whole range, so results are unchanged up to rounding; bench.py --recipe worst times it. */
#define MM_FORCE_WORST_TIER 64
/* mm_moment_match_backward only: `workspace` still holds the q stage of exactly this (mu, Sigma, flags) -- the forward of the
 * same match was the last call on it, on the same stream -- so the q stage is not run again.  The caller's promise; the
 * device checks the part it can see (the q stage stamps the mean it read into the workspace) and reports a stale workspace
 * as status = {B - b, -1}. */
#define MM_WORKSPACE_CURRENT 128
/* MM_F32 packs, test / measurement aids of the accuracy contract (csrc/mm_route.hip): MM_FORCE_ROUTE sends EVERY off-diagonal
 * (b, pair) item through the f64 re-reduce whatever its error estimate says (forward and backward); MM_NO_ROUTE none (the f32
 * sweep's result as it is: what rounds 1-3 returned). */
#define MM_FORCE_ROUTE 256
#define MM_NO_ROUTE 512
/* mm_moment_match_backward only: `bwd_ws` holds the sums mm_moment_match_with_sums left for exactly this (mu, Sigma, flags):
 * the M x M sweeps are not run again, the call is the chain rule alone.  Combine with MM_WORKSPACE_CURRENT when `workspace`
 * is untouched as well; without it the q stage (only) is re-run.  The sums are stamped with the mean they were swept for and
 * the device verifies it: sums of another state are reported as status = {B - b, -2}. */
#define MM_SUMS_CURRENT 1024

/* error codes */
#define MM_E_ARG      (-1)  /* NULL pointer / non-positive size                  */
#define MM_E_DIM      (-2)  /* d > MM_DMAX or unsupported shape                  */
#define MM_E_DTYPE    (-3)
#define MM_E_WORKSPACE (-4) /* workspace too small                               */
#define MM_E_NO_C     (-5)  /* MM_MODEL_UNCERTAINTY asked for but model packed without C */
#define MM_E_STATE    (-6)  /* euler/rollout needs d == L                         */

int mm_abi_version(void);

/* ---- model packing (once per model; replaces the per-call Kuu Cholesky + triangular
 *      solves of models.py:216-235 by the precomputed beta = Kuu^-1 u and
 *      C = Kuu^-1 S Kuu^-1 - Kuu^-1) ------------------------------------ */
size_t mm_packed_model_bytes(int L, int M, int d, int dtype, int with_C);

int mm_pack_model(void* packed, size_t packed_bytes,
                  int L, int M, int d, int dtype,
                  const double* Z,            /* [L,M,d] inducing inputs (kernel-sliced)   */
                  const double* lengthscales, /* [L,d]                                     */
                  const double* variance,     /* [L]                                       */
                  const double* beta,         /* [L,M]   Kuu^-1 u                          */
                  const double* C,            /* [L,M,M] or NULL                           */
                  const double* mean_c,       /* [L] Constant mean, or NULL (Zero)         */
                  void* stream);

/* Order of the inducing points inside the pack.  The outputs of the path are sums over a latent's inducing points, so the pack
 * is free to store them in an order of its own: packs of M > 256 points are sorted per latent by |(z - mean z) / lengthscale|
 * (tiles of the M x M reduces then hold points of similar norm: lower per-tile range tiers); smaller packs -- in particular
 * every policy pack of the composed rollout, whose g_policy is per packed centre -- keep the caller's order.
 * perm [L][M] (device, int32): the caller's index of the point at packed position m.  q_out (mm_q_forward) is written in the
 * CALLER's order; the per-point sums of mm_backward_sums are in PACKED order. */
int mm_pack_perm(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int32_t* perm, void* stream);

/* ---- one moment match: (mu, Sigma) -> (f1, Sff, Sigma^-1 Cov(x,f)) --------------------
 * Replaces _mm_gauss_svgp_mo / _so / _mm_gauss_gpr up to (not including) the
 * LinearCoregionalization mixing (models.py:279-286), which stays on the host. */
size_t mm_workspace_bytes(int B, int L, int M, int d, int dtype, int flags);

int mm_moment_match(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype,
                    int B,
                    const void* mu,        /* [B,d]   T */
                    const void* Sigma,     /* [B,d,d] T (symmetric; lower triangle is read) */
                    int flags, double jitter,
                    void* f1,              /* [B,L]   T  (includes the Constant mean)       */
                    void* Sff,             /* [B,L,L] T, or [B,L] without MM_FULL_OUTPUT_COV */
                    void* cross_pre,       /* [B,d,L] T  Sigma^-1 Cov(x,f) (preinv=True)    */
                    void* workspace, size_t workspace_bytes,
                    int32_t* status, void* stream);

/* ---- stage-level entry points; mm_moment_match = q then Q ------- */
/* <K_xZ> terms (kernel_expectation.py:200-214 + gpflow <k(x,Z)>): fills the workspace and
 * writes f1, cross_pre; q_out (optional, [B,L,M] T) receives eKfu[b,m,a] transposed. */
int mm_q_forward(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B,
                 const void* mu, const void* Sigma, int flags,
                 void* f1, void* cross_pre, void* q_out,
                 void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

/* fused <K_Zx K_xZ'> reduce (kernel_expectation.py:72-247 + models.py:219-261) -> Sff.
 * Must follow mm_q_forward on the same workspace/stream. */
int mm_Q_reduce_forward(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B,
                        int flags, double jitter, void* Sff,
                        void* workspace, size_t workspace_bytes, void* stream);

/* MomentMatchingEuler.step (solvers.py:110-135), requires d == L:
 *   mu' = mu + dt f1;  Sigma' = Sigma + dt (Sxf + Sxf^T) + dt^2 Sff,  Sxf = Sigma cross_pre */
int mm_euler_update(int B, int d, int dtype, double dt,
                    const void* mu, const void* Sigma,
                    const void* f1, const void* Sff, const void* cross_pre,
                    void* mu_out, void* Sigma_out, void* stream);

/* Drift-only closed rollout (Euler.__call__ fold, solvers.py:67-105, with
 * forward_sde(x, drift, None, None, None), forward_sde.py:34-46): H steps enqueued
 * back-to-back.  mu/Sigma are updated in place; traj_mu [H,B,d] / traj_Sigma [H,B,d,d]
 * (optional) receive the state after every step. */
int mm_rollout_closed(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B, int H,
                      double dt, int flags, double jitter,
                      void* mu, void* Sigma, void* traj_mu, void* traj_Sigma,
                      void* workspace, size_t workspace_bytes,
                      int32_t* status, void* stream);

/* Closed-form expected saturating cost E[-exp(-0.5 (x - x*)^T W (x - x*))], x ~ N(mean, cov)
 * (GaussianObjective.__call__ on GaussianMoments, gpflow_pilco/components.py:26-37): the
 * per-step statistic the rollout accumulates (loops/pilco.py:199-205).
 * mean [N,d], cov [N,d,d], target [d], precis [d,d] -> cost [N]  (all T). */
int mm_expected_cost(int N, int d, int dtype, const void* mean, const void* cov,
                     const void* target, const void* precis, void* cost, void* stream);

/* Diagnostic: after mm_q_forward (f32 model, d <= 8), how many (batch element, off-diagonal pair) items take the
 * moment collapse of csrc/mm_moments.hip / mm_moments6.hip (the degree-3..6 polynomial p6 of the remainder from weight
 * moments, wave tiles with max |b| <= 1/4 skipped: Cauchy-Schwarz bound <= 1/2), and for how many of those the bound alone puts
 * every |b| <= 1/4 (no tile work at all).  The collapse is decided per GROUP OF 64 ROWS of an item (the pack's norm order puts the
 * rows of large |A_i| last): out: device int32[6] = {collapsed in every row group, total, wholly inside, routed, partly collapsed
 * (some row groups), collapsed row groups over all items (of total * ceil(M / 128) * 2)}; zeros where the collapse does not
 * apply; routed = the items the last mm_moment_match / mm_Q_reduce_forward on this workspace re-reduced in f64
 * (csrc/mm_route.hip; meaningful only after such a call on an MM_F32 pack). */
int mm_offdiag_stats(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B, int flags,
                     const void* workspace, size_t workspace_bytes, int32_t* out, void* stream);

/* Diagnostic: the number of (batch element, off-diagonal pair) items the last mm_moment_match / mm_Q_reduce_forward on this
 * workspace put on the work list of the persistent f32 off-diagonal sweep (csrc/mm_mfma.hip: the items with a tile to visit; MM_F32
 * packs with d <= 8 and M <= 2048, else 0).  out: device int32[1]. */
int mm_offdiag_worklist_len(int L, int M, int d, int dtype, int B, int flags, const void* workspace, size_t workspace_bytes,
                            int32_t* out, void* stream);

/* Diagnostic: the two factors of the lengthscale-scaled bound by which the f32 off-diagonal sweep skips column tiles
 * (csrc/mm_mfma.hip; MM_F32 packs with d <= 8, else MM_E_DIM), copied out device to device: zt2s_out [L][Mp/32] f32 from the pack
 * (per 32-point tile of the packed order max_m sum_k (z_mk - zbar_k)^2 / lengthscale_k^2, rounded up; Mp = M rounded up to
 * MM_M_ALIGN) and gmax2s_out [B][P-L][Mp/64] f32 from the last mm_q_forward / mm_moment_match on this workspace (per 64-row group
 * max_i sum_k (A_ik lengthscale_a',k)^2, rounded up). */
int mm_offdiag_skip_bounds(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B, int flags,
                           const void* workspace, size_t workspace_bytes, float* zt2s_out, float* gmax2s_out, void* stream);

/* Diagnostic of the f32 pack's accuracy contract (csrc/mm_route.hip): after mm_moment_match / mm_Q_reduce_forward (or the
 * backward) on an MM_F32 pack, out [B][P-L][2] f64 = per (batch element, off-diagonal pair) {the sweep's estimate of its own
 * rounding error, the scale it is compared with}: an item is re-reduced in f64 when est > MM_ROUTE_TOL (3e-4) x scale. */
int mm_route_estimates(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B, int flags,
                       const void* workspace, size_t workspace_bytes, double* out, void* stream);

/* ---- composed policy rollout: SURVEY.md row f-2 -------------------------------------------------------
 * The rollout harness of MomentMatchingPILCO (gpflow_pilco/loops/pilco.py:192-220) for the cartpole-shaped system
 *   x (nx) -> TrigonometricEncoder on `active_dims` (components.py:73-75, moment_matching/components.py:19-57,
 *             maths.py:143-176) -> e = [sin a, cos a, x_inactive]  (ne = nx + na)
 *          -> policy = InverseLinkWrapper(KernelRegressor(SVGP, one latent), Chain[Scale, Shift, NormalCDF])
 *             (models/core.py:60-71, moment_matching/models.py:27-41, bijectors.py:21-69): u = scale (Phi(f(e)) + shift)
 *          -> drift SVGP on d = joint(e, u) (nd = ne + 1) with the cross-covariance bookkeeping of
 *             dynamics/forward_sde.py:95-137 -> MomentMatchingEuler.step (solvers.py:110-135)
 *          -> expected Gaussian cost of the encoded new state (components.py:26-37), per step.
 * H steps are enqueued back to back: per step two mm_moment_match calls and four small kernels
 * (csrc/mm_compose.hip).  drift: packed with C (model uncertainty on), drift_L == nx, drift_d == nd;
 * policy: one latent, policy_d == ne, evaluated without model uncertainty (a KernelRegressor has none).
 * mx [B,nx] / Sxx [B,nx,nx] are updated in place; cost [H,B] (optional, needs target [ne], precis [ne,ne]) receives
 * the per-step statistic (the loss of pilco.py:199-205 is its sum over H); traj_* [H,B,..] optional.
 * active_dims: HOST array of na distinct state indices.  One action (Owen's T branch, bijectors.py:57-58); several
 * actions: mm_rollout_composed_nd below.
 * na == 0 (a system without a periodic coordinate, forward_sde.py:49-68: mountain car) is taken by every rollout entry and
 * size query of this header -- moment-matched and pathwise, one action, _nd and _wide: the encoding is the identity (e = x,
 * ne = nx, nd = nx + nu, Cov(x, e) = Sxx), active_dims may be NULL, target / precis are those of the raw state, and every
 * other bound stays as stated.  na < 0 is MM_E_DIM (0 from a size query). */
size_t mm_compose_workspace_bytes(int B, int nx, int na, int dtype);
int mm_rollout_composed(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                        const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                        int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                        double head_scale, double head_shift, const void* target, const void* precis,
                        void* mx, void* Sxx, void* cost, void* traj_mu, void* traj_Sigma,
                        void* ws_drift, size_t ws_drift_bytes, void* ws_policy, size_t ws_policy_bytes,
                        void* ws_compose, size_t ws_compose_bytes, int32_t* status, void* stream);

/* The same rollout for a policy with nu actions (1 <= nu <= 4, ne + nu <= 32, else MM_E_DIM): policy = InverseLinkWrapper(
 * KernelRegressor(SVGP with nu latents), Chain[Scale, Shift, NormalCDF]), u_j = head_scale[j] (Phi(f_j(e)) + head_shift[j]),
 * drift on d = joint(e, u) with nd = ne + nu (csrc/mm_compose_nd.hip).  The head is the n-D branch of bijectors.py:48-69:
 * E[Phi(f_i) Phi(f_j)] is a bivariate normal CDF, evaluated by Plackett's integral on 4 x 48 Gauss-Legendre nodes (the diagonal
 * keeps Owen's T).  policy: packed with L = nu latents, policy_d == ne; drift_d == nd; head_scale / head_shift: HOST arrays of
 * nu doubles.  Everything else as mm_rollout_composed; nu == 1 computes what mm_rollout_composed computes (through the general
 * policy match).  Its tape and reverse sweep are mm_rollout_composed_taped_nd / mm_rollout_composed_backward_nd further down. */
size_t mm_compose_nd_workspace_bytes(int B, int nx, int na, int nu, int dtype);
int mm_rollout_composed_nd(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                           const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                           int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                           int nu, const double* head_scale, const double* head_shift,
                           const void* target, const void* precis,
                           void* mx, void* Sxx, void* cost, void* traj_mu, void* traj_Sigma,
                           void* ws_drift, size_t ws_drift_bytes, void* ws_policy, size_t ws_policy_bytes,
                           void* ws_compose, size_t ws_compose_bytes, int32_t* status, void* stream);

/* The same rollout, RECORDED for differentiation: every per-step intermediate and the states x_0 .. x_H are written into
 * `tape` (mm_compose_tape_bytes) instead of a reused workspace; mx / Sxx / cost as above.  Where H copies of the drift's
 * workspace fit in 512 MB the tape also keeps the drift match's q stage of every step (the reverse sweep then does not
 * re-run it). */
size_t mm_compose_tape_bytes(int B, int H, int nx, int na, int drift_M, int dtype);
int mm_rollout_composed_taped(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                              const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                              int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                              double head_scale, double head_shift, const void* target, const void* precis,
                              void* mx, void* Sxx, void* cost, void* ws_drift, size_t ws_drift_bytes,
                              void* ws_policy, size_t ws_policy_bytes, void* tape, size_t tape_bytes,
                              int32_t* status, void* stream);

/* ---- gradient of the composed rollout: SURVEY.md rows f-1 x f-2 -----------------------------------------------
 * What the only real caller needs: update_policy differentiates the whole closure with tf.GradientTape
 * (gpflow_pilco/utils/optimizers.py:51-56, examples/cartpole_swingup/train_utils.py:91-105, loops/pilco.py:192-220).
 * mm_rollout_composed_backward is the reverse sweep over the tape (f64 only; policy M <= 256 centres on ne <= 8 encoded dims,
 * else MM_E_DIM; B >= 1):
 *   g_cost   [H][B]  (in)  d loss / d cost[h][b]  (all ones for the loss of pilco.py:199-205)
 *   g_policy [B][M d + M + d + 2] (out, overwritten): per batch element the gradient w.r.t. the PACKED policy --
 *            Z [M][d], beta = Kuu^-1 u [M], ls2 = lengthscales^2 [d], variance, mean_c; sum over B and chain through
 *            beta(q_mu, Z, lengthscales, variance) on the host (a 30 x 30 precompute)
 *   g_mx0 [B][nx], g_Sxx0 [B][nx][nx] (out, both or neither): gradient w.r.t. the initial state (symmetric)
 * ws_bwd: mm_compose_backward_workspace_bytes; ws_drift: the drift's mm_workspace_bytes (full covariance + uncertainty). */
size_t mm_compose_backward_workspace_bytes(int B, int nx, int na, int drift_M);
size_t mm_policy_grad_bytes(int B, int policy_M, int policy_d);
int mm_rollout_composed_backward(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                 const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                 int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                 double head_scale, double head_shift, const void* target, const void* precis,
                                 const void* tape, size_t tape_bytes, const void* g_cost,
                                 void* g_policy, void* g_mx0, void* g_Sxx0,
                                 void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                 int32_t* status, void* stream);

/* The same reverse sweep SEEDED on the trajectory: g_xm [H][B][nx] = d loss / d m_{h+1} and g_xS [H][B][nx][nx] =
 * d loss / d S_{h+1} (both or neither, else MM_E_ARG; f64) are added to the carried adjoint of x_{h+1} in step h, before the
 * built-in cost's adjoint, so g_cost keeps working beside them (all zeros: the seeds alone).  The taped states x_1 .. x_H thereby
 * become differentiable outputs and any objective evaluated on them by the caller sits on the native chain.  Only the symmetric
 * part of a seed on the symmetric S is determined: pass (G + G^T) / 2.  With null seeds the result is bit-equal to
 * mm_rollout_composed_backward (one sweep serves both entries). */
int mm_rollout_composed_backward_seeded(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                        const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                        int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                        double head_scale, double head_shift, const void* target, const void* precis,
                                        const void* tape, size_t tape_bytes, const void* g_cost,
                                        const void* g_xm, const void* g_xS,
                                        void* g_policy, void* g_mx0, void* g_Sxx0,
                                        void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                        int32_t* status, void* stream);

/* ---- the same for a policy with nu actions (csrc/mm_compose_nd.hip, csrc/mm_compose_bwd_nd.hip; f64 only, else MM_E_DTYPE) ----
 * mm_rollout_composed_taped_nd is mm_rollout_composed_nd writing into a tape: H + 1 slots of the multi-action compose workspace,
 * the states x_0 .. x_H, and -- where H of them fit in 512 MB, by the rules of mm_compose_tape_bytes -- per step the drift match's
 * q-stage workspace and the sums of its backward sweeps (the reverse sweep re-runs what the tape did not keep).  The policy
 * match's workspace is not kept: the reverse sweep recomputes the policy from the taped (me, See).
 * mm_rollout_composed_backward_nd is the reverse sweep:
 *   g_cost   [H][B]  (in)
 *   g_policy [B][nu][M d + M + d + 2] (out, overwritten; mm_policy_grad_bytes_nd): per batch element and latent, in latent
 *            order, the gradient w.r.t. the packed policy -- Z [M][d], beta [M], ls2 [d], variance, mean_c; the centres in the
 *            caller's order (M <= 256: the pack does not permute them)
 *   g_mx0 [B][nx], g_Sxx0 [B][nx][nx] (out, both or neither)
 * One workgroup per batch element runs the nu latent and nu (nu - 1) / 2 pair adjoints of the policy match in turn, from LDS;
 * no floating-point atomics: two sweeps over one tape are bit-equal.  Shapes taken: policy M <= 256, ne <= 8, nu <= 4 and the
 * workgroup's LDS (88 KB at M = 64, ne = 8, nu = 4) <= 160 KB, i.e. M <= 166 at ne = 8 -- every policy with M <= 64; beyond,
 * mm_compose_backward_workspace_bytes_nd returns 0 and mm_rollout_composed_backward_nd MM_E_DIM.  A non-PD state is reported
 * through `status` as by mm_rollout_composed_backward.  nu == 1 computes what the one-action entries compute. */
size_t mm_compose_tape_bytes_nd(int B, int H, int nx, int na, int nu, int drift_M, int dtype);
int mm_rollout_composed_taped_nd(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                 const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                 int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                 int nu, const double* head_scale, const double* head_shift,
                                 const void* target, const void* precis, void* mx, void* Sxx, void* cost,
                                 void* ws_drift, size_t ws_drift_bytes, void* ws_policy, size_t ws_policy_bytes,
                                 void* tape, size_t tape_bytes, int32_t* status, void* stream);
size_t mm_compose_backward_workspace_bytes_nd(int B, int nx, int na, int nu, int drift_M, int policy_M);
size_t mm_policy_grad_bytes_nd(int B, int nu, int policy_M, int policy_d);
int mm_rollout_composed_backward_nd(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                    const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                    int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                    int nu, const double* head_scale, const double* head_shift,
                                    const void* target, const void* precis, const void* tape, size_t tape_bytes,
                                    const void* g_cost, void* g_policy, void* g_mx0, void* g_Sxx0,
                                    void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                    int32_t* status, void* stream);
/* ... seeded on the trajectory exactly as mm_rollout_composed_backward_seeded (g_xm [H][B][nx], g_xS [H][B][nx][nx]) */
int mm_rollout_composed_backward_nd_seeded(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                           const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                           int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                           int nu, const double* head_scale, const double* head_shift,
                                           const void* target, const void* precis, const void* tape, size_t tape_bytes,
                                           const void* g_cost, const void* g_xm, const void* g_xS,
                                           void* g_policy, void* g_mx0, void* g_Sxx0,
                                           void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                           int32_t* status, void* stream);

/* ---- the _nd rollouts with a COREGIONALISED drift (gpflow's LinearCoregionalization; csrc/mm_mix.h) -----------------------------
 * The drift pack has drift_L = Lg latents on drift_d = nd inputs (packed with C, no mean of its own), 1 <= Lg <= nx, and its nx
 * outputs are f = W g + c:
 *   mix_W  device, f64, row-major [nx][drift_L]          (NULL: MM_E_ARG)
 *   mix_c  device, f64, [nx], or NULL for no output mean
 * Per step the drift's match runs with L = Lg, full output covariance and model uncertainty (added in latent space, as
 * moment_matching/models.py:254-286), into a staging block; then ONE launch per step (one workgroup per batch element) writes
 *   f1 = W g1 + c,   Sff = W Sgg W^T (i <= j computed and mirrored: exactly symmetric),   cross = cross_g W^T  [nd][nx]
 * in f64 whatever the state type, rounded on store.  Tail, encoder, head and cost see an ordinary drift with nx outputs.  (The packed
 * [B][Lg] blocks of neighbouring batch elements overlap the [B][nx] ones, so the mixing is not done in place: hence the staging
 * block and mm_compose_nd_mixed_workspace_bytes.)  The tape stores the mixed moments; its kept drift workspace and kept backward
 * sums are sized with Lg.  Where the tape does not keep the sums per step, the taped forward still computes the drift's value with
 * the routine of mm_moment_match_with_sums, into one scratch buffer at the end of the tape: the value of a taped rollout, and its
 * gradient, are the same in every regime of the tape (element b of a large batch reproduces that element of a small one bit for
 * bit), at the price of the backward's sweeps in place of the forward's in that taped forward.  The reverse sweep runs the adjoint g g1 = W^T g f1, g Sgg = W^T (g Sff) W, g cross_g = (g cross) W
 * between the tail's adjoint and the drift match's adjoint with L = Lg.  No gradient w.r.t. W, c or the drift; no floating-point
 * atomics (two sweeps over one tape are bit-equal).
 * drift_L < 1 or > nx: MM_E_DIM, and the size queries return 0.  Every other check is that of the _nd entry of the same name with
 * drift_L in place of nx for the drift's pack and workspace (mm_workspace_bytes(B, drift_L, ...), mm_packed_model_bytes(drift_L, ...)).
 * The argument lists are those of mm_rollout_composed_nd / _taped_nd / _backward_nd_seeded (null seeds: the plain sweep) with the
 * mixing operands appended. */
size_t mm_compose_nd_mixed_workspace_bytes(int B, int nx, int na, int nu, int drift_L, int dtype);
int mm_rollout_composed_nd_mixed(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                 const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                 int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                 int nu, const double* head_scale, const double* head_shift,
                                 const void* target, const void* precis,
                                 void* mx, void* Sxx, void* cost, void* traj_mu, void* traj_Sigma,
                                 void* ws_drift, size_t ws_drift_bytes, void* ws_policy, size_t ws_policy_bytes,
                                 void* ws_compose, size_t ws_compose_bytes, int32_t* status, void* stream,
                                 const double* mix_W, const double* mix_c);
size_t mm_compose_tape_bytes_nd_mixed(int B, int H, int nx, int na, int nu, int drift_L, int drift_M, int dtype);
int mm_rollout_composed_taped_nd_mixed(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                       const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                       int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                       int nu, const double* head_scale, const double* head_shift,
                                       const void* target, const void* precis, void* mx, void* Sxx, void* cost,
                                       void* ws_drift, size_t ws_drift_bytes, void* ws_policy, size_t ws_policy_bytes,
                                       void* tape, size_t tape_bytes, int32_t* status, void* stream,
                                       const double* mix_W, const double* mix_c);
size_t mm_compose_backward_workspace_bytes_nd_mixed(int B, int nx, int na, int nu, int drift_L, int drift_M, int policy_M);
int mm_rollout_composed_backward_nd_mixed(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                          const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                          int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                          int nu, const double* head_scale, const double* head_shift,
                                          const void* target, const void* precis, const void* tape, size_t tape_bytes,
                                          const void* g_cost, const void* g_xm, const void* g_xS,
                                          void* g_policy, void* g_mx0, void* g_Sxx0,
                                          void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                          int32_t* status, void* stream, const double* mix_W);

/* ---- the reverse sweep for 8 < ne <= 16 encoded dims: the _wide entries (csrc/mm_compose_bwd_nd.hip) -----------------------------
 * The sweeps of mm_rollout_composed_backward_nd[_seeded] / _nd_mixed over the same tapes (mm_rollout_composed_taped_nd and
 * _taped_nd_mixed take every ne the compose layer allows), argument for argument, for ne = nx + na <= 16 (ne <= 8 included), 1 to 4
 * actions, policy M <= 256 and the policy kernel's LDS -- the _nd entries' size function at the wider ne, without the pair item's
 * scratch when there is one action -- within 160 KB for this M and every smaller one: at ne = 16, M <= 121 with one action and
 * M <= 50 with 2 to 4; at ne = 9, 256 and 146.  Beyond, the size queries return 0 and the entries MM_E_DIM; the
 * other codes are those of the _nd entries.  The small dense algebra at 8 < n <= 16 (the SPD inverses of the policy adjoint and
 * of the drift's pair items, the pivoted solve of the cost adjoint) runs on one wave with four entries per lane; pivot choice, row exchanges and the sign of
 * the determinant are those of the generic code.  f64 only; no floating-point atomics (two sweeps over one tape are bit-equal).
 * The _wide_mixed entries take mix_W last; _wide_mixed_seeded has the argument list of mm_rollout_composed_backward_nd_mixed.
 * mm_compose_wide_dense_path(generic): which dense code the _wide entries run from now on in this process -- 0 (default) the
 * one-wave paths, non-zero the generic code of the _nd entries; returns the previous setting.  A measuring aid, not thread-safe. */
size_t mm_compose_backward_workspace_bytes_wide(int B, int nx, int na, int nu, int drift_M, int policy_M);
size_t mm_compose_backward_workspace_bytes_wide_mixed(int B, int nx, int na, int nu, int drift_L, int drift_M, int policy_M);
int mm_compose_wide_dense_path(int generic);
int mm_compose_wide_backward(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                      const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                      int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                      int nu, const double* head_scale, const double* head_shift,
                                      const void* target, const void* precis, const void* tape, size_t tape_bytes,
                                      const void* g_cost, void* g_policy, void* g_mx0, void* g_Sxx0,
                                      void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                      int32_t* status, void* stream);
int mm_compose_wide_backward_seeded(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                             const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                             int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                             int nu, const double* head_scale, const double* head_shift,
                                             const void* target, const void* precis, const void* tape, size_t tape_bytes,
                                             const void* g_cost, const void* g_xm, const void* g_xS,
                                             void* g_policy, void* g_mx0, void* g_Sxx0,
                                             void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                             int32_t* status, void* stream);
int mm_compose_wide_backward_mixed(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M, int drift_d,
                                            const void* policy_packed, size_t policy_bytes, int policy_M, int policy_d,
                                            int dtype, int B, int H, double dt, int nx, int na, const int32_t* active_dims,
                                            int nu, const double* head_scale, const double* head_shift,
                                            const void* target, const void* precis, const void* tape, size_t tape_bytes,
                                            const void* g_cost, void* g_policy, void* g_mx0, void* g_Sxx0,
                                            void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                            int32_t* status, void* stream, const double* mix_W);
int mm_compose_wide_backward_mixed_seeded(const void* drift_packed, size_t drift_bytes, int drift_L, int drift_M,
                                                   int drift_d, const void* policy_packed, size_t policy_bytes, int policy_M,
                                                   int policy_d, int dtype, int B, int H, double dt, int nx, int na,
                                                   const int32_t* active_dims, int nu, const double* head_scale,
                                                   const double* head_shift, const void* target, const void* precis,
                                                   const void* tape, size_t tape_bytes, const void* g_cost,
                                                   const void* g_xm, const void* g_xS,
                                                   void* g_policy, void* g_mx0, void* g_Sxx0,
                                                   void* ws_drift, size_t ws_drift_bytes, void* ws_bwd, size_t ws_bwd_bytes,
                                                   int32_t* status, void* stream, const double* mix_W);

/* ---- backward w.r.t. the input moments, stage A (f64 mode) ---------------------
 * The M x M part of d(f1, Sff, cross)/d(mu, Sigma) reduced to M-sized sums (see csrc/mm_backward.hip);
 * gpflowpilco_amd/autodiff.py finishes the chain rule.  Must follow mm_moment_match / mm_q_forward +
 * mm_Q_reduce_forward with the same (mu, Sigma, flags) on the same workspace.
 * out: [B][P][3+d][Mp] column sums (Ksum, csum, cC, Usum[d]) then [B][P-L][2][Mp] row sums (Rsum, rsum), the inducing points
 * in PACKED order (mm_pack_perm). */
size_t mm_backward_bytes(int B, int L, int M, int d, int flags);
int mm_backward_sums(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B,
                     const void* mu, int flags, const void* workspace, size_t workspace_bytes,
                     void* out, size_t out_bytes, void* stream);

/* ---- backward w.r.t. the input moments, complete: the vector-Jacobian product of one moment match
 *   (g_f1 [B,L], g_Sff [B,L,L] | [B,L], g_cross [B,d,L]) -> g_mu [B,d], g_Sigma [B,d,d] (symmetric; += if accumulate_Sigma)
 * for a frozen model (the reference: tf.GradientTape through moment_matching/models.py:200-299).  Gradients are f64 in and
 * out; (mu, Sigma) have the pack's type.  Re-runs the q stage for (mu, Sigma) on `workspace`, then
 *   MM_F64 packs: the M x M sweeps of mm_backward_sums for every pair,
 *   MM_F32 packs with d <= 8 (mm_bwd_f32_supported): the f64 sweep for the L diagonal pairs only; the off-diagonal pairs
 *     are reduced to 1 + 2d + 3d^2 aggregates each -- polynomial part from the degree-4 weight moments in f64, remainder
 *     by a bf16-MFMA tile sweep (csrc/mm_bwd_f32.hip); other f32 packs return MM_E_DTYPE (use an f64 pack of the model),
 * then the M-sized moments and the d x d chain rule per (latent | pair) item and their sum (csrc/mm_compose_bwd.hip,
 * mm_adjoint.h).  bwd_ws: mm_moment_match_backward_bytes (enough for either pack type).
 * flags: the forward's, optionally | MM_WORKSPACE_CURRENT, optionally | MM_STAGE_* to run only part of the backward on what
 * earlier calls left in `workspace` / `bwd_ws` (measurement): MM_STAGE_DIAG = the f64 sweep (f64 packs: of every pair),
 * MM_STAGE_OFFDIAG = the f32 remainder sweep, MM_STAGE_FINALIZE = moment GEMM, aggregates, item moments, items and their sum. */
int mm_bwd_f32_supported(int d);
size_t mm_moment_match_backward_bytes(int B, int L, int M, int d, int flags);
size_t mm_moment_match_backward_bytes_dtype(int B, int L, int M, int d, int dtype, int flags);   /* exactly what that pack type needs */
/* the off-diagonal aggregates of an MM_F32 pack alone (tests, diagnostics): runs the q stage of (mu, Sigma) on `workspace`;
 * pagg [B][P-L][1 + 2d + 3d^2] f64 = sum_ij Omega_ij (1 | zeta_i | zeta_i zeta_i^T | zeta'_j | zeta'_j zeta'_j^T | zeta_i zeta'_j^T),
 * zeta = z - mu, Omega_ij = w_i w'_j e^{delta_ij} (pairs a < a' row by row) */
size_t mm_backward_pair_aggregates_bytes(int B, int L, int M, int d, int flags);
int mm_backward_pair_aggregates(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B,
                                const void* mu, const void* Sigma, int flags, void* workspace, size_t workspace_bytes,
                                void* scratch, size_t scratch_bytes, void* pagg, size_t pagg_bytes,
                                int32_t* status, void* stream);
int mm_moment_match_backward(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B,
                             const void* mu, const void* Sigma, int flags,
                             const void* g_f1, const void* g_Sff, const void* g_cross,
                             void* g_mu, void* g_Sigma, int accumulate_Sigma,
                             void* workspace, size_t workspace_bytes, void* bwd_ws, size_t bwd_ws_bytes,
                             int32_t* status, void* stream);
/* Value AND gradient without sweeping twice (what tf.GradientTape + tape.gradient cost the reference together,
 * utils/optimizers.py:51-56).  Nothing the backward's M x M sweeps compute depends on the incoming gradient, and their sums
 * contain the forward's: Sff_aa = sum_j (w_j c_j + q_j cC_j) + var + jitter, Sff_aa' = pagg[0] - (sum w)(sum w').
 * mm_moment_match_with_sums = mm_moment_match (same outputs, same types; Sff to the backward sweeps' accuracy, which is the
 * forward's or better) computed from the q stage + the BACKWARD's sweeps, which stay on `bwd_ws`
 * (mm_moment_match_backward_bytes_dtype); the matching mm_moment_match_backward(flags | MM_SUMS_CURRENT [| MM_WORKSPACE_CURRENT])
 * on the same bwd_ws is then the chain rule alone.  MM_F32 packs need d <= 8 (MM_E_DTYPE otherwise). */
int mm_moment_match_with_sums(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B,
                              const void* mu, const void* Sigma, int flags, double jitter,
                              void* f1, void* Sff, void* cross_pre,
                              void* workspace, size_t workspace_bytes, void* bwd_ws, size_t bwd_ws_bytes,
                              int32_t* status, void* stream);

/* ---- pathwise (decoupled-sampling) rollout: SURVEY.md row f-3, BASELINE.json configs[4] ---------
 * f[s,a] = scale_a sum_k w[s,a,k] cos(2 pi (omega_t[a,:,k].x_s + phase[a,k]))
 *        + var_a   sum_m v[s,a,m] 2^(zs_t[a,:,m].(x_s * x_scale[a]) - hz[a,m] - hx) + mean_a
 * i.e. PathwiseSVGP.predict_f_samples with one input per sample path (gpflow_pilco/models/svgp.py:124-130,
 * loops/pilco.py:281-291; arithmetic in the un-vendored gpflow-sampling package -- parity unpinned).
 * Shared operands are pre-scaled and k-major: omega_t [L,d,K] = omega^T / 2pi, phase [L,K] = b / 2pi,
 * x_scale [L,d] = sqrt(log2 e) / lengthscales (f64), zs_t [L,d,M] = (Z * x_scale)^T, hz [L,M] = |zs|^2 / 2,
 * hx = |x * x_scale|^2 / 2 (computed in the kernel).
 * The per-sample weights arrive as ONE blocked stream wb[G][L][NB][4][BT]: G = ceil(S/4) sample groups,
 * BT = 256 (f32) / 128 (f64) terms per block, NB = K/BT prior blocks followed by M/BT update blocks;
 * element [g][a][tb][sl][t] is w[4g+sl][a][tb*BT+t] (or v[..][(tb-K/BT)*BT+t]).  K and M must be multiples
 * of BT and S is padded to a multiple of 4 (zero weights).  Each wave then streams one contiguous region.
 * x [S,d], f_out [S,L]: T. */
int mm_pathwise_eval(int S, int L, int M, int K, int d, int dtype,
                     const void* x, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                     const double* x_scale, const double* prior_scale, const double* variance,
                     const double* mean_c, const void* wb, void* f_out, void* stream);

/* The same evaluation that also emits, in the same pass, abs_out [S,L] T = scale_a sum_k |w cos(.)| + var_a sum_m |v 2^(.)|: the sum
 * of the ABSOLUTE terms of f[s,a].  A T-typed weight stream and T-typed basis values leave an error of at most ~2 eps_T abs_out in
 * f[s,a] (eps_f32 = 6e-8: v = Kuu^-1 (u - Phi w) cancels 1e5 .. 1e7-fold in sum_m v_m k(x, z_m) at M = 2000, so an f32 sample's
 * value can have lost its digits -- the caller sees it here instead of not at all; the f64 mode is the accurate path). */
int mm_pathwise_eval_bound(int S, int L, int M, int K, int d, int dtype,
                           const void* x, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                           const double* x_scale, const double* prior_scale, const double* variance,
                           const double* mean_c, const void* wb, void* f_out, void* abs_out, void* stream);

/* Euler.step folded H times on the sample paths (dynamics/solvers.py:50-65, no diffusion; d == L):
 * x <- x + dt f(x).  x is updated in place (x_tmp: scratch of the same size); traj [H,S,d] optional. */
int mm_pathwise_rollout(int S, int L, int M, int K, int d, int dtype, int H, double dt,
                        void* x, void* x_tmp, const void* omega_t, const void* phase, const void* zs_t,
                        const void* hz, const double* x_scale, const double* prior_scale,
                        const double* variance, const double* mean_c, const void* wb,
                        void* traj, void* stream);

/* The same evaluation that also emits the per-sample Jacobian d f[s,a] / d x[s,:]  (jac_out [S,L,d] T; d <= 16, MM_E_DIM beyond):
 * in the SAME pass over the weight stream (d more FMAs and, in the prior blocks, one more transcendental per term and sample).
 * d <= 8: a wave keeps the sums of a whole group of four samples; 8 < d <= 16: it walks the group's blocks twice, two samples at
 * a time (their weights are separate rows of every block, so nothing is read twice).  f_out is bit-equal to mm_pathwise_eval's. */
int mm_pathwise_eval_jac(int S, int L, int M, int K, int d, int dtype,
                         const void* x, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                         const double* x_scale, const double* prior_scale, const double* variance,
                         const double* mean_c, const void* wb, void* f_out, void* jac_out, void* stream);

/* ---- pathwise POLICY rollout and its gradient: row f-3 completed ---------------------------------------------------
 * PathwisePILCO._policy_loss_closure (gpflow_pilco/loops/pilco.py:263-298) for the cartpole-shaped system, per sample path s:
 *   e = TrigonometricEncoder(x) (components.py:44-75) -> u = scale (Phi(f_pol(e)) + shift), f_pol = the policy SVGP's predictive
 *   mean (models/core.py:60-71) -> x' = x + dt f_s([e, u]) (tensor branch of forward_sde, dynamics/forward_sde.py:23-31; Euler.step,
 *   solvers.py:50-65) -> cost[h][s] = -exp(-(enc(x') - target)^T precis (enc(x') - target) / 2) (components.py:39-41).
 * The drift paths are the operands of mm_pathwise_eval with L = nx latents on nd = nx + na + 1 inputs (nd <= 8); the policy is a
 * one-latent pack (mm_pack_model, M <= 256 centres on ne = nx + na inputs; only its f64 blocks are read).  x0 [S,nx], target [ne],
 * precis [ne,ne], cost [H,S]: T.  tape (mm_pathwise_tape_bytes): states x_0..x_H, the drift inputs of every step and, with
 * with_jacobians != 0, d f_s / d (e, u) of every step -- what mm_pathwise_policy_rollout_backward reads (the reference
 * differentiates the mean sample loss with a gradient tape: examples/cartpole_swingup/train_utils.py:108-135):
 *   g_cost [H][S] f64 (in; 1/S everywhere for the mean loss) -> g_policy [M ne + M + ne + 2] f64 (out: dZ, dbeta, d ls^2, dvar,
 *   dmean of the PACKED policy, summed over the samples; chain through beta(q_mu, Z, ls, var) on the host), g_x0 [S][nx] f64
 *   (optional).  The reverse sweep is ONE kernel (samples are independent) and does not touch the weight stream again. */
size_t mm_pathwise_tape_bytes(int S, int H, int nx, int na, int dtype, int with_jacobians);
int mm_pathwise_policy_rollout(int S, int M, int K, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                               const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                               const double* x_scale, const double* prior_scale, const double* variance,
                               const double* mean_c, const void* wb,
                               const void* policy_packed, size_t policy_bytes, int policy_M, double head_scale, double head_shift,
                               const void* target, const void* precis, const void* x0, void* cost,
                               void* tape, size_t tape_bytes, int with_jacobians, void* stream);
size_t mm_pathwise_backward_scratch_bytes(int S, int policy_M, int ne);
int mm_pathwise_policy_rollout_backward(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                        const void* policy_packed, size_t policy_bytes, int policy_M,
                                        double head_scale, double head_shift, const void* target, const void* precis,
                                        const void* tape, size_t tape_bytes, const void* g_cost, void* g_policy, void* g_x0,
                                        void* scratch, size_t scratch_bytes, void* stream);
/* The reverse sweep with a seed on the STATES, for a loss the caller evaluates on the taped trajectory (a caller-defined objective
 * on sample paths: loops/pilco.py:272-275 calls self.objective(x = encoder(state), t = t) per step).  The argument list of
 * mm_pathwise_policy_rollout_backward with g_x after g_cost:  g_x [H][S][nx] f64, block h = d loss / d x_{h+1} -- the state the
 * tape stores at index h + 1, the convention of g_xm in mm_rollout_composed_backward_seeded -- read in f64 whatever the tape's
 * element type.  g_x may be NULL (then the entry is the unseeded one, bit for bit); g_cost may be NULL: the built-in cost is not
 * part of the loss and its term is skipped (target / precis must still be valid device buffers of ne and ne x ne elements: the
 * kernels stage them as always, only their values are ignored).  Both NULL: MM_E_ARG.  Every other
 * refusal, the scratch size, the LDS bound and the outputs are the unseeded entry's. */
int mm_pathwise_policy_rollout_backward_seeded(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                               const void* policy_packed, size_t policy_bytes, int policy_M,
                                               double head_scale, double head_shift, const void* target, const void* precis,
                                               const void* tape, size_t tape_bytes, const void* g_cost, const void* g_x,
                                               void* g_policy, void* g_x0, void* scratch, size_t scratch_bytes, void* stream);

/* ---- the same for policies with SEVERAL actions (csrc/mm_pathwise_policy.hip): 1 <= nu <= 4 ---------------------------------
 * On sample paths the policy is evaluated pointwise, so its nu actions are nu independent heads appended to the encoding in
 * latent order: u_a = head_scale[a] (Phi(f_a(e)) + head_shift[a]), drift input d = (e, u_0 .. u_{nu-1}), nd = nx + na + nu <= 8
 * (the double pendulum: nx 4, two angles, two torques -> nd = 8).  The policy is an mm_pack_model pack with L = nu latents
 * (M <= 256 centres each on ne = nx + na inputs; only its f64 blocks are read); head_scale, head_shift: HOST arrays [nu].
 * Everything else -- operands, tape (with nd = nx + na + nu), g_cost, g_x0 -- as in the one-action entries above;
 * g_policy [nu][M ne + M + ne + 2] f64: per latent dZ, dbeta, d ls^2, dvar, dmean.  With nu = 1 the size queries return the
 * one-action sizes, and the rollout, the tape and the gradients are the one-action entries': those are these entries called
 * with nu = 1 and their by-value head constants (the same code; they differ only in answering MM_E_DIM, after the size and dtype
 * checks, where these answer MM_E_ARG for na > 0 without active_dims, and in a scratch query without upper bounds).
 * Refused before any HIP call: nu outside 1..4, nx + na + nu > 8 or policy_M > 256 (MM_E_DIM); a null pointer (MM_E_ARG); a dtype
 * other than MM_F32 / MM_F64 (MM_E_DTYPE); a short tape, policy buffer or scratch (MM_E_WORKSPACE).
 * The reverse sweep keeps the nu policy blocks and one gradient slab per wave in LDS and takes a shape when
 *   8 (nu (M ne + M + ne) + ne + ne^2 + 8 + 4 nu (M ne + M + ne + 2)) <= 160 KiB:
 * every shape with M <= 64; at M = 256 nu = 1, nu = 2 (ne <= 6: 144 KB) and nu = 3 with ne <= 4, but not nu = 3 with ne = 5
 * (M <= 226) or nu = 4 with ne = 4 (M <= 203).  Beyond it mm_pathwise_backward_scratch_bytes_nd returns 0 (as for any shape the
 * entry refuses) and mm_pathwise_policy_rollout_backward_nd MM_E_DIM; the forward entry has no such bound. */
size_t mm_pathwise_tape_bytes_nd(int S, int H, int nx, int na, int nu, int dtype, int with_jacobians);
int mm_pathwise_policy_rollout_nd(int S, int M, int K, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                  int nu, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                                  const double* x_scale, const double* prior_scale, const double* variance,
                                  const double* mean_c, const void* wb,
                                  const void* policy_packed, size_t policy_bytes, int policy_M,
                                  const double* head_scale, const double* head_shift,
                                  const void* target, const void* precis, const void* x0, void* cost,
                                  void* tape, size_t tape_bytes, int with_jacobians, void* stream);
size_t mm_pathwise_backward_scratch_bytes_nd(int S, int policy_M, int ne, int nu);
int mm_pathwise_policy_rollout_backward_nd(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                           int nu, const void* policy_packed, size_t policy_bytes, int policy_M,
                                           const double* head_scale, const double* head_shift,
                                           const void* target, const void* precis,
                                           const void* tape, size_t tape_bytes, const void* g_cost, void* g_policy, void* g_x0,
                                           void* scratch, size_t scratch_bytes, void* stream);
/* ... with a seed on the states: g_x [H][S][nx] f64 after g_cost, as in mm_pathwise_policy_rollout_backward_seeded above. */
int mm_pathwise_policy_rollout_backward_nd_seeded(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                                  int nu, const void* policy_packed, size_t policy_bytes, int policy_M,
                                                  const double* head_scale, const double* head_shift,
                                                  const void* target, const void* precis,
                                                  const void* tape, size_t tape_bytes, const void* g_cost, const void* g_x,
                                                  void* g_policy, void* g_x0, void* scratch, size_t scratch_bytes, void* stream);

/* ---- the same entries for WIDER systems: nd = nx + na + nu <= 16 (1 <= nu <= 4) ---------------------------------------------
 * Signatures, operands, tape (mm_pathwise_tape_bytes_nd: it has no bound on nd), results and error codes of the _nd entries; one
 * implementation serves both, so for nd <= 8 the results are bit-equal.  The cart-double-pendulum (nx 6, two angles, one force)
 * has nd 9, a three-link arm nd 13.  Refused with MM_E_DIM: nd > 16, nu outside 1..4, policy_M > 256, and -- the reverse sweep
 * only -- a shape outside the LDS bound above (with ne up to 15): every shape with M <= 64 fits; the tightest case, nu 4 on
 * ne 12, stops at M = 77.  mm_pathwise_backward_scratch_bytes_wide returns 0 for what the backward entry refuses. */
int mm_pathwise_policy_rollout_wide(int S, int M, int K, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                    int nu, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                                    const double* x_scale, const double* prior_scale, const double* variance,
                                    const double* mean_c, const void* wb,
                                    const void* policy_packed, size_t policy_bytes, int policy_M,
                                    const double* head_scale, const double* head_shift,
                                    const void* target, const void* precis, const void* x0, void* cost,
                                    void* tape, size_t tape_bytes, int with_jacobians, void* stream);
size_t mm_pathwise_backward_scratch_bytes_wide(int S, int policy_M, int ne, int nu);
int mm_pathwise_policy_rollout_backward_wide(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                             int nu, const void* policy_packed, size_t policy_bytes, int policy_M,
                                             const double* head_scale, const double* head_shift,
                                             const void* target, const void* precis,
                                             const void* tape, size_t tape_bytes, const void* g_cost, void* g_policy, void* g_x0,
                                             void* scratch, size_t scratch_bytes, void* stream);
int mm_pathwise_policy_rollout_backward_wide_seeded(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                                    int nu, const void* policy_packed, size_t policy_bytes, int policy_M,
                                                    const double* head_scale, const double* head_shift,
                                                    const void* target, const void* precis,
                                                    const void* tape, size_t tape_bytes, const void* g_cost, const void* g_x,
                                                    void* g_policy, void* g_x0, void* scratch, size_t scratch_bytes, void* stream);

/* ---- the same entries for a COREGIONALISED drift: f = W g + c, Lg latents mixed to nx outputs (1 <= Lg <= nx) --------------------
 * The paths' operands (omega_t .. wb) are those of mm_pathwise_eval with L = Lg latents on nd = nx + na + nu <= 16 inputs
 * (1 <= nu <= 4; the same implementation as the _nd / _wide entries, so any nd <= 16 is taken); mean_c is NOT read: the constant
 * is mix_c, added after the mixing.  mix_W [nx][Lg], mix_c [nx] (may be NULL: zero): f64 DEVICE arrays, appended after the
 * _nd arguments.  Per step  x_{h+1,i} = x_{h,i} + dt (c_i + sum_l W[i][l] g_l)  in f64, one fma per latent in latent order,
 * rounded to T on store.  The tape is latent-sized: after the states and drift inputs of the _nd tape come the sample slot
 * [S][Lg] and the Jacobian block [H][S][Lg][nd] -- the stream pass writes g and d g / d d straight into them, there is no
 * separate mixing launch -- so mm_pathwise_tape_bytes_mixed(.., Lg = nx, ..) == mm_pathwise_tape_bytes_nd(..) and a smaller Lg
 * shrinks exactly those two blocks.  states x_0 .. x_H lead the tape as before.
 * The backward has the arguments of mm_pathwise_policy_rollout_backward_nd_seeded (either of g_cost and g_x may be NULL, not
 * both) + Lg, mix_W:  g d = dt J_g^T (W^T g x_{h+1}); everything else is the unmixed sweep.  W and c are read from global memory
 * at wave-uniform addresses, not through LDS: the sweep takes every shape for which
 * mm_pathwise_backward_scratch_bytes_wide(S, policy_M, ne, nu) is non-zero, with that scratch size; g_policy as in the _nd entries.
 * Refused: Lg < 1 or Lg > nx, nd > 16, nu outside 1..4, policy_M > 256 (MM_E_DIM; mm_pathwise_tape_bytes_mixed returns 0); a NULL
 * mix_W or any other required pointer (MM_E_ARG); short buffers (MM_E_WORKSPACE). */
size_t mm_pathwise_tape_bytes_mixed(int S, int H, int nx, int na, int nu, int Lg, int dtype, int with_jacobians);
int mm_pathwise_policy_rollout_mixed(int S, int M, int K, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                     int nu, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                                     const double* x_scale, const double* prior_scale, const double* variance,
                                     const double* mean_c, const void* wb,
                                     const void* policy_packed, size_t policy_bytes, int policy_M,
                                     const double* head_scale, const double* head_shift,
                                     const void* target, const void* precis, const void* x0, void* cost,
                                     void* tape, size_t tape_bytes, int with_jacobians, void* stream,
                                     int Lg, const double* mix_W, const double* mix_c);
int mm_pathwise_policy_rollout_backward_mixed(int S, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                              int nu, const void* policy_packed, size_t policy_bytes, int policy_M,
                                              const double* head_scale, const double* head_shift,
                                              const void* target, const void* precis,
                                              const void* tape, size_t tape_bytes, const void* g_cost, const void* g_x,
                                              void* g_policy, void* g_x0, void* scratch, size_t scratch_bytes, void* stream,
                                              int Lg, const double* mix_W);

/* ---- drifts with a Matern kernel: the _kern siblings ------------------------------------------------------------------------
 * The entries above evaluate SquaredExponential latents.  Their _kern siblings take one more argument, kernel, the family of
 * EVERY latent of the paths: 0 SquaredExponential (then bit-equal to the entry without the argument, which is this call),
 * 1 Matern-3/2, 2 Matern-5/2 in gpflow's parametrisation; anything else is MM_E_ARG, refused before any HIP call.  Operands,
 * layouts, outputs and the other error codes are unchanged: the stream's argument a = zs_t.(x x_scale) - hz - hx is
 * -(log2 e / 2) r^2 for every family, and the update half's basis value 2^a becomes
 *   Matern-3/2: (1 + s) e^-s, s = sqrt3 r        Matern-5/2: (1 + s + s^2 / 3) e^-s, s = sqrt5 r        (r^2 = -2 ln2 a, clamped at 0)
 * The prior half is the same w cos(.); only the distribution the caller draws omega from differs (a multivariate Student-t with
 * 2 nu degrees of freedom: pathwise.spectral_frequencies).  abs_out of the _bound entry uses the family's basis value.
 *
 * mm_pathwise_policy_rollout_kern is the one policy-rollout entry for such a drift: the argument list of
 * mm_pathwise_policy_rollout_mixed plus kernel; Lg = 0 with mix_W = NULL means no mixing (then mm_pathwise_policy_rollout_wide:
 * nd <= 16, 1 <= nu <= 4, tape of mm_pathwise_tape_bytes_nd), otherwise the _mixed entry's rules.  The tape layout does not depend
 * on the family and the reverse sweeps read the drift only through the taped Jacobian: the backward entries are
 * mm_pathwise_policy_rollout_backward_wide[_seeded] resp. _backward_mixed, as they are. */
int mm_pathwise_eval_kern(int S, int L, int M, int K, int d, int dtype,
                          const void* x, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                          const double* x_scale, const double* prior_scale, const double* variance,
                          const double* mean_c, const void* wb, void* f_out, void* stream, int kernel);
int mm_pathwise_eval_bound_kern(int S, int L, int M, int K, int d, int dtype,
                                const void* x, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                                const double* x_scale, const double* prior_scale, const double* variance,
                                const double* mean_c, const void* wb, void* f_out, void* abs_out, void* stream, int kernel);
int mm_pathwise_rollout_kern(int S, int L, int M, int K, int d, int dtype, int H, double dt,
                             void* x, void* x_tmp, const void* omega_t, const void* phase, const void* zs_t,
                             const void* hz, const double* x_scale, const double* prior_scale,
                             const double* variance, const double* mean_c, const void* wb,
                             void* traj, void* stream, int kernel);
int mm_pathwise_eval_jac_kern(int S, int L, int M, int K, int d, int dtype,
                              const void* x, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                              const double* x_scale, const double* prior_scale, const double* variance,
                              const double* mean_c, const void* wb, void* f_out, void* jac_out, void* stream, int kernel);
int mm_pathwise_policy_rollout_kern(int S, int M, int K, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                    int nu, const void* omega_t, const void* phase, const void* zs_t, const void* hz,
                                    const double* x_scale, const double* prior_scale, const double* variance,
                                    const double* mean_c, const void* wb,
                                    const void* policy_packed, size_t policy_bytes, int policy_M,
                                    const double* head_scale, const double* head_shift,
                                    const void* target, const void* precis, const void* x0, void* cost,
                                    void* tape, size_t tape_bytes, int with_jacobians, void* stream,
                                    int Lg, const double* mix_W, const double* mix_c, int kernel);

/* ---- a MEAN-ONLY drift: shared weights instead of a stream (csrc/mm_pathwise_mean.hip) --------------------------------------
 * The reference's build_dynamics(..., model_uncertainty=False) wraps the drift in a KernelRegressor: under the Euler solver the
 * drift of EVERY sample is then the posterior mean K(x, Z) Kuu^-1 u + c, and the sample paths are never read.  That function has
 * no per-sample weights: with beta [L][M] f64 = Kuu^-1 u (zero on padded centres, which then add exactly 0),
 *   f[s][a]    = variance[a] sum_m beta[a][m] e_m + mean_c[a]                  (e_m, g_m): the family's basis value and slope at
 *   J[s][a][k] = ln2 variance[a] sum_m beta[a][m] g_m (zs_t[a][k][m] x_scale[a][k] - x_scale[a][k]^2 x[s][k])    zs_t . xs - hz - hx
 * -- the update half of mm_pathwise_eval_jac_kern with v[s][a][m] = beta[a][m] for every s.  x [S][d], zs_t [L][d][M], hz [L][M]
 * of dtype; x_scale [L][d], variance [L], mean_c [L] (or NULL), beta [L][M] f64; kernel as in the _kern entries.  M is any
 * positive number (no block size: nothing is streamed), d <= 16 (MM_E_DIM beyond).  Nothing of size S M is read or written: a
 * latent's operands go through LDS in chunks and serve every sample of the workgroup.  Values accumulate in f64 in both modes, the
 * partial sums of a sample are added in a fixed order: bitwise reproducible.
 *
 * mm_pathwise_mean_eval: f_out [S][L] and, jac_out != NULL, jac_out [S][L][d] (the layouts of mm_pathwise_eval_jac).
 * mm_pathwise_policy_rollout_mean: mm_pathwise_policy_rollout_kern with the mean in place of the paths -- its argument list without
 * (K, omega_t, phase, prior_scale, wb) and with beta after mean_c; nd <= 16, 1 <= nu <= 4, Lg / mix_W / mix_c as there (0 / NULL:
 * no mixing; beta is then [nx][M], else [Lg][M]).  The tape is that of mm_pathwise_tape_bytes_nd resp. _mixed and the gradients
 * come from mm_pathwise_policy_rollout_backward_wide[_seeded] resp. _backward_mixed, as they are.
 * Both validate before any HIP call and return the codes above (MM_E_ARG: a size <= 0, a missing pointer, an unknown kernel). */
int mm_pathwise_mean_eval(int S, int L, int M, int d, int dtype,
                          const void* x, const void* zs_t, const void* hz, const double* x_scale, const double* variance,
                          const double* mean_c, const double* beta, void* f_out, void* jac_out, void* stream, int kernel);
int mm_pathwise_policy_rollout_mean(int S, int M, int dtype, int H, double dt, int nx, int na, const int32_t* active_dims,
                                    int nu, const void* zs_t, const void* hz, const double* x_scale, const double* variance,
                                    const double* mean_c, const double* beta,
                                    const void* policy_packed, size_t policy_bytes, int policy_M,
                                    const double* head_scale, const double* head_shift,
                                    const void* target, const void* precis, const void* x0, void* cost,
                                    void* tape, size_t tape_bytes, int with_jacobians, void* stream,
                                    int Lg, const double* mix_W, const double* mix_c, int kernel);

/* ---- path GENERATION: the two reformatting steps of a draw (csrc/mm_pathwise_sample.hip) -----------------------------------
 * PathwisePILCO draws new paths on every optimiser step (loops/pilco.py:281-284).  Between the random draws, two GEMMs and two
 * triangular solves (the caller's: pathwise.PathSampler keeps them on torch's BLAS with a cached Kuu factor) a draw is
 * reformatting; these two entries do it in one launch resp. one pass each, into buffers the caller reuses across draws.
 *
 * mm_pathwise_basis: from the draws n [L,K,d] (standard normal) and b [L,K] (uniform on [0, 2 pi)), f64, and the model's
 * Z [L,M,d], ls [L,d], var [L], f64:
 *   omega_out [L,d,Kp] T = (n[l][k][j] / ls[l][j]) / 2 pi,  phase_out [L,Kp] T = b[l][k] / 2 pi   (mm_pathwise_eval's omega_t, phase;
 *                          Kp = K rounded up to BT; zero for k >= K; the division by 2 pi is a multiplication by the f64
 *                          reciprocal, as torch evaluates a division by a host scalar on the device: bit-equal to it)
 *   phiZ_out [L,M,K] f64 = sqrt(2 var_l / K) cos(sum_j Z[l][m][j] (n[l][k][j] / ls[l][j]) + b[l][k])
 * BT = 128 (MM_F64) or 256 (MM_F32).  MM_E_DIM: d > MM_DMAX or a non-positive size.
 *
 * mm_pathwise_pack_stream: the blocked weight stream of mm_pathwise_eval from the prior weights w [S,L,K] f64 and the update
 * weights v [L,M,S] f64 (sample index fastest: the layout a solve with the right-hand side [L,M,S] leaves):
 *   wb_out [G][L][NB][4][BT] T, G = ceil(S / 4), NB = (Kp + Mp) / BT:  [g][l][nb][sl][t] = (T) w[4g+sl][l][nb BT + t] for
 *   nb < Kp / BT, else (T) v[l][(nb - Kp/BT) BT + t][4g+sl]; zero where k >= K, m >= M or 4g+sl >= S.
 * Every element of wb_out is written exactly once (no memset needed between draws).  MM_E_DIM: a non-positive size. */
int mm_pathwise_basis(int L, int K, int M, int d, int dtype, const double* n, const double* b, const double* Z,
                      const double* ls, const double* var, void* omega_out, void* phase_out, double* phiZ_out, void* stream);
int mm_pathwise_pack_stream(int S, int L, int K, int M, int dtype, const double* w, const double* v, void* wb_out,
                            void* stream);

/* ---- SE-ARD Gram matrix of the SVGP ELBO and its adjoint (csrc/mm_gram.hip; everything f64, row-major) ----------------------
 * mm_gram_se: X [N,d], Z [L,M,d], ls [L,d], var [L] -> K [L,M,N],
 *   K[l][m][n] = var_l exp(-1/2 sum_k ((x_nk - z_lmk) / ls_lk)^2), the squared distance formed from differences.
 *   X == NULL is the SELF mode: K[l] = k_l(Z_l, Z_l) as [L,M,M] (N must equal M), symmetric to the bit with a diagonal of
 *   exactly var_l; the caller adds its jitter.
 * mm_gram_se_backward: G [L,M,N] and the same operands -> gZ [L,M,d], gls [L,d], gvar [L]; with t = G K (K recomputed, not read)
 *   gZ[l][m][k] = sum_n t (x_nk - z_lmk) / ls_lk^2,  gls[l][k] = sum_mn t (x_nk - z_lmk)^2 / ls_lk^3,  gvar[l] = sum_mn t / var_l.
 *   There is no gradient with respect to X.  In the self mode G is a GENERAL [L,M,M] matrix (it need not be symmetric) and the
 *   result is the full derivative through both argument slots: gZ_i = sum_j (G_ij + G_ji) K_ij (z_j - z_i) / ls^2.
 *   Per-chunk partial sums go to the workspace (mm_gram_workspace_bytes(L, M, N, d), N = M in the self mode) and a second launch
 *   adds them in a fixed order: no atomics, two calls on the same inputs are bit-equal.
 * Any L, M, N >= 1 (no padding asked of the caller), 1 <= d <= MM_DMAX; MM_E_DIM otherwise (the size query returns 0). */
size_t mm_gram_workspace_bytes(int L, int M, int N, int d);
int mm_gram_se(int L, int M, int N, int d, const double* X, const double* Z, const double* ls, const double* var, double* K,
               void* stream);
int mm_gram_se_backward(int L, int M, int N, int d, const double* G, const double* X, const double* Z, const double* ls,
                        const double* var, double* gZ, double* gls, double* gvar, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---- predictive mean and variance at deterministic points (csrc/mm_predict.hip, schedule in csrc/mm_predict.h; f64, row-major) ----
 * mm_predict_se: X [N,d], Z [L,M,d], ls [L,d], var [L], beta [L,M], C [L,M,M] SYMMETRIC (only the blocks on and below the diagonal
 *   are read), mean_c [L] or NULL ->
 *     mean[n][l] = sum_m K_l[m][n] beta_l[m] (+ mean_c[l]),   fvar[n][l] = var_l + sum_ij K_l[i][n] C_l[i][j] K_l[j][n],
 *   K_l[m][n] as mm_gram_se's.  With beta = Kuu^-1 u and C = Kuu^-1 (S - Kuu) Kuu^-1 (what a packed model is built from) these are the
 *   marginals of gpflow's predict_f per latent.  C == NULL and fvar == NULL together: the mean alone (MM_E_ARG when only one is NULL).
 *   K is formed tile by tile and never stored beyond one strip per workgroup of a capped grid: mm_predict_workspace_bytes depends
 *   on M alone (it ignores N; > 0 for every accepted shape, 0 for a rejected one).  No atomics: two calls are bit-equal.
 * Any L, M, N >= 1, 1 <= d <= MM_DMAX, M <= 2^20; MM_E_DIM otherwise; MM_E_WORKSPACE for a workspace below the query's size. */
size_t mm_predict_workspace_bytes(int L, int M, int N, int d);
int mm_predict_se(int L, int M, int N, int d, const double* X, const double* Z, const double* ls, const double* var,
                  const double* beta, const double* C, const double* mean_c, double* mean, double* fvar, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---- streamed Gram statistics of the collapsed (SGPR) bound and their adjoint (csrc/mm_gram_stats.hip, schedule in
 * csrc/mm_gram_stats.h; f64, row-major) ----
 * mm_gram_stats_se: X [N,d], R [N,Q], Z [L,M,d], ls [L,d], var [L] ->
 *     Phi[l] = K_l K_l^T [M,M] (written in full, symmetric to the bit),   Psi[l] = K_l R [M,Q],   K_l[m][n] as mm_gram_se's.
 *   Q == 0 with R == NULL and Psi == NULL: Phi alone (MM_E_ARG when the three disagree).
 * mm_gram_stats_se_backward: GPhi [L,M,M] (a GENERAL matrix: GPhi + GPhi^T is used), GPsi [L,M,Q] and the same operands ->
 *   gZ [L,M,d], gls [L,d], gvar [L]: mm_gram_se_backward's sums with G = (GPhi + GPhi^T) K + GPsi R^T, formed tile by tile.
 *   There is no gradient with respect to X or R.
 * K is never stored: nothing of a size proportional to L M N is allocated, written or read, and mm_gram_stats_workspace_bytes
 * ignores N (one buffer of that size serves both entries; 0 for a rejected shape).  No atomics: two calls are bit-equal.
 * Any L, M, N >= 1, 1 <= d <= MM_DMAX, 0 <= Q <= 33, M <= 2^15; MM_E_DIM otherwise; MM_E_WORKSPACE for a workspace below the
 * query's size. */
size_t mm_gram_stats_workspace_bytes(int L, int M, int N, int d, int Q);
int mm_gram_stats_se(int L, int M, int N, int d, int Q, const double* X, const double* R, const double* Z, const double* ls,
                     const double* var, double* Phi, double* Psi, void* workspace, size_t workspace_bytes, void* stream);
int mm_gram_stats_se_backward(int L, int M, int N, int d, int Q, const double* GPhi, const double* GPsi, const double* X,
                              const double* R, const double* Z, const double* ls, const double* var, double* gZ, double* gls,
                              double* gvar, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPFLOWPILCO_MM_H */
