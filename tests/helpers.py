"""Shared builders: the same numpy parameters go to the CPU oracle and to the GPU path."""
import numpy as np
import torch

from gpflowpilco_amd import models as gp
from gpflowpilco_amd.synthetic import SyntheticSVGP, generate_covariance, make_inputs, make_svgp
from oracle import mm_oracle as mo

F64 = torch.float64


def oracle_params(s: SyntheticSVGP) -> mo.SVGPParams:
  L, M, d = s.shape
  return mo.SVGPParams(Z=np.broadcast_to(s.Z, (L, M, d)).copy(), lengthscales=s.lengthscales,
                       variance=s.variance, q_mu=s.q_mu, q_sqrt=s.q_sqrt, whiten=s.whiten,
                       mean_c=s.mean_c)


def random_svgp_params(seed, L, M, d, whiten, ls_bounds=(0.3, 3.0), mean=True, W_rows=None,
                       separate_Z=True):
  """Reference-test style random SVGP (tests/test_moment_matching.py:199-236)."""
  rng = np.random.default_rng(seed)
  Z = rng.uniform(size=(L, M, d)) if separate_Z else np.broadcast_to(rng.uniform(size=(M, d)), (L, M, d)).copy()
  ls = np.exp(rng.uniform(np.log(ls_bounds[0]), np.log(ls_bounds[1]), size=(L, d)))
  q_mu = 0.89 * rng.standard_normal((M, L))
  q_cov = generate_covariance(rng, M, (L,), 0.89)
  W = None
  P = L
  if W_rows is not None:
    W = rng.uniform(size=(W_rows, L))
    W = W / np.linalg.norm(W, axis=-1, keepdims=True)
    P = W_rows
  mean_c = 1 + rng.standard_normal(P) if mean else None
  return mo.SVGPParams(Z=Z, lengthscales=ls, variance=np.full(L, 0.89 ** 2), q_mu=q_mu,
                       q_sqrt=np.linalg.cholesky(q_cov), whiten=whiten, mean_c=mean_c, W=W)


def gp_model_from_oracle(p: mo.SVGPParams, device) -> gp.SVGP:
  L = p.Z.shape[0]
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=device)
  kernels = [gp.SquaredExponential(variance=t(p.variance[a]), lengthscales=t(p.lengthscales[a])) for a in range(L)]
  iv = gp.SeparateIndependentInducingVariables([gp.InducingPoints(t(p.Z[a])) for a in range(L)])
  kernel = gp.LinearCoregionalization(kernels, t(p.W)) if p.W is not None else gp.SeparateIndependent(kernels)
  mean = gp.Zero() if p.mean_c is None else gp.Constant(t(p.mean_c))
  return gp.SVGP(kernel=kernel, inducing_variable=iv, q_mu=t(p.q_mu), q_sqrt=t(p.q_sqrt),
                 whiten=p.whiten, mean_function=mean, num_latent_gps=L)


def to_dev(a, device, dtype):
  return torch.tensor(np.asarray(a), dtype=dtype, device=device)


def contract_err(Sff, Sffo):
  """The f32 pack's accuracy contract (include/gpflowpilco_mm.h): per batch element the error of the
  off-diagonal block relative to that block's own scale (its largest |entry|: what MM_ROUTE_TOL is stated against) and of the
  diagonal relative to the largest variance.  Returns (worst off-diagonal, worst diagonal) over the batch."""
  got = Sff.detach().double().cpu().numpy() if isinstance(Sff, torch.Tensor) else np.asarray(Sff)
  L = got.shape[-1]
  eye = np.eye(L, dtype=bool)
  err = np.abs(got - Sffo)
  off = dia = 0.0
  for b in range(got.shape[0]):
    if L > 1:
      off = max(off, float(err[b][~eye].max() / max(np.abs(Sffo[b][~eye]).max(), 1e-300)))
    dia = max(dia, float(err[b][eye].max() / max(np.abs(Sffo[b][eye]).max(), 1e-300)))
  return off, dia


def f32_state(mu, Sigma):
  """The state as an f32 pack receives it (the oracle is evaluated there: the comparison point of an f32 tolerance)."""
  return np.asarray(mu, dtype=np.float32).astype(np.float64), np.asarray(Sigma, dtype=np.float32).astype(np.float64)


def _materialised(ops6, mu, Sigma, full, unc, g):
  """One float64 CPU evaluation of autodiff.moment_match_torch and one backward of sum(g . output)."""
  from gpflowpilco_amd import autodiff
  Z, ls, var, beta, C, mc = ops6
  mu = mu.clone().requires_grad_(True)
  Sigma = Sigma.clone().requires_grad_(True)
  f1, Sff, cross = autodiff.moment_match_torch(mu, Sigma, Z, ls, var, beta, C if unc else None, mc, full, unc)
  ((g[0] * f1).sum() + (g[1] * Sff).sum() + (g[2] * cross).sum()).backward()
  return (f1.detach(), Sff.detach(), cross.detach(), mu.grad, 0.5 * (Sigma.grad + Sigma.grad.transpose(1, 2)))


def materialised_reference(model, mu, Sigma, full_output_cov, model_uncertainty, g_f1, g_Sff, g_cross, floor_trials=2):
  """The moment match and its vector-Jacobian product without any of the kernels' M x M code: autodiff.moment_match_torch (the
  materialised [P, M, M] evaluation) and its autograd, on the CPU in float64, on the operands the pack is built from.

  ``model``: the (Z, ls, var, beta, C, mean_c) of ``SVGP.precompute`` (any device; moved to the CPU here), or a model, whose
  ``precompute("cpu")`` is taken.  Kuu never enters: beta and C are inputs.
  Returns ((f1, Sff, cross, g_mu, g_Sigma symmetrised), floors): float64 CPU tensors, and for each of the five the reference's
  own conditioning floor -- every entry of mu, Sigma, Z, beta and C multiplied by 1 +- 2^-52 with seeded random signs (Sigma
  and C re-symmetrised), the evaluation repeated, the largest change over ``floor_trials`` trials relative to the tensor's
  largest |entry|.  No computed digit below that floor means anything, whoever computes it."""
  ops6 = model.precompute("cpu") if hasattr(model, "precompute") else model
  cpu = lambda t: None if t is None else torch.as_tensor(t).detach().to("cpu", F64)
  Z, ls, var, beta, C, mc = (cpu(t) for t in ops6)
  if not model_uncertainty:
    C = None
  mu, Sigma = cpu(mu), cpu(Sigma)
  g = tuple(cpu(t) for t in (g_f1, g_Sff, g_cross))
  want = _materialised((Z, ls, var, beta, C, mc), mu, Sigma, full_output_cov, model_uncertainty, g)
  gen = torch.Generator(device="cpu").manual_seed(20240)
  ulp = 2.0 ** -52
  sym = lambda A: 0.5 * (A + A.transpose(-1, -2))
  jig = lambda t: t * (1.0 + ulp * (2.0 * torch.randint(0, 2, t.shape, generator=gen).to(F64) - 1.0))
  floors = [0.0] * 5
  for _ in range(floor_trials):
    pert = _materialised((jig(Z), ls, var, jig(beta), None if C is None else sym(jig(C)), mc), jig(mu), sym(jig(Sigma)),
                         full_output_cov, model_uncertainty, g)
    for k, (a_, b_) in enumerate(zip(pert, want)):
      floors[k] = max(floors[k], float((a_ - b_).abs().max() / b_.abs().max().clamp_min(1e-300)))
  return want, tuple(floors)


# The draws on which the f64 pack is pinned to materialised_reference (tests/test_gpu_f64_reference.py; their floors are
# asserted on the CPU in tests/test_f64_reference_host.py).  The sizes are the smallest that select each launch path of
# mm_backward_sums_impl (csrc/mm_backward.hip) and of the forward's f64 sweep.  id: (L, M, d, B, full, unc, ls_bounds, scale, stable)
_LS, _LSW = (0.7, 3.0), (2.5, 5.0)
REFERENCE_DRAWS = {
    "both_small": (2, 40, 3, 1, True, True, _LS, 0.2, True),       # Mp 128: k_bwd_mfma_both<1,1>; forward k_qred_f64_both; M < 64
    "both_overflow": (4, 100, 3, 33, True, True, _LS, 0.2, True),  # Mp 128, 1056 work items: unfactored columns + rows launch
    "diag_ks2": (2, 130, 8, 3, True, True, _LS, 0.2, True),        # Mp 256: k_bwd_diag<2,1,true,false> + split launches
    "diag_nounc": (3, 300, 5, 2, True, False, _LS, 0.2, True),     # k_bwd_diag<2,1,false,false>; M > 256: norm-sorted pack
    "diagcov": (2, 130, 16, 2, False, True, _LS, 0.2, True),       # P = L, no row launch; (KS4, NU) = (4, 2)
    "L1": (1, 200, 8, 2, True, True, _LS, 0.2, True),              # no off-diagonal pair
    "ks3": (2, 200, 12, 2, True, True, _LS, 0.2, True),            # <3,1>
    "ks4_nu1": (2, 150, 14, 2, True, True, _LS, 0.2, True),        # <4,1>
    "ks6": (2, 90, 20, 1, True, True, _LSW, 0.2, True),            # <6,2>
    "ks8": (2, 70, 31, 2, True, True, _LSW, 0.2, True),            # <8,2>
    "d32": (2, 60, 32, 1, True, True, _LSW, 0.2, True),            # k_bwd_sums<32> only
    "chunks": (5, 600, 4, 2, True, True, _LS, 0.2, True),          # two forward launches, batch chunks, ten tiles per side
    "unstable": (3, 300, 8, 2, True, True, (0.3, 3.0), 0.1, False),  # the bench recipe's kind of model
    "tiers": (3, 150, 6, 3, True, True, (0.2, 1.0), 1.0, True),    # every wave tile past the last Taylor tier: mm_exp_f64, |b| <= 3.7
    # two more, by a host count of max |b_ij| = |zeta_i G zeta_j| per 32 x 32 wave tile: over the rows above the tiles fall in
    # the tiers |b| < 1/64 ... < 1/4 and >= 1/2, none in [1/4, 1/2) and no b below -4
    "tiers_mid": (3, 150, 6, 3, True, True, (0.5, 2.0), 0.5, True),   # tiles in [1/8, 1/4) and [1/4, 1/2): the two last Taylor tiers
    "tiers_deep": (3, 150, 6, 3, True, True, (0.05, 0.3), 1.0, True),  # b from -51 to 59: e^b below 2^-53 and the exponent cap's side
}


def reference_draw(name, device="cpu", seed_g=2):
  """-> (syn, mu, Sigma, (g1, g2, g3), full, unc) of a REFERENCE_DRAWS row: numpy state, float64 CPU cotangents (g2 symmetric
  over its last two axes when ``full``: the kernels fill Sff symmetrically)."""
  L, M, d, B, full, unc, ls_bounds, scale, stable = REFERENCE_DRAWS[name]
  syn = make_svgp(L, M, d, seed=60 + L + d, device=str(device), ls_bounds=ls_bounds, mean_c=True, stable=stable)
  mu, Sigma = make_inputs(B, d, seed=9, scale=scale, lo=0.3, hi=0.7)
  g = torch.Generator(device="cpu").manual_seed(seed_g)
  g1 = torch.randn(B, L, generator=g, dtype=F64)
  g2 = torch.randn(B, L, L, generator=g, dtype=F64) if full else torch.randn(B, L, generator=g, dtype=F64)
  g3 = torch.randn(B, d, L, generator=g, dtype=F64)
  if full:
    g2 = 0.5 * (g2 + g2.transpose(1, 2))
  return syn, mu, Sigma, (g1, g2, g3), full, unc


def scale_err(got, want):
  """max |got - want| relative to max |want| (per tensor)."""
  got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
  return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
