"""Matern-3/2 and Matern-5/2 drifts on the pathwise solver: kernels, spectral draw, update weights, refusals (CPU) and every
native route -- evaluation, Jacobian, rounding bound, drift-only rollout, policy rollouts with their gradients, the path sampler
-- against the float64 numpy helper ``tests/pathwise_matern_oracle.py`` (GPU).

Bars: f64 values 1e-10 of max |f|, Jacobian 1e-8 of max |J| and within 1e-6 of central differences of
the helper; an f32 value lies inside its own ``eval_with_bound`` bound; policy rollouts f64 1e-10 / f32 5e-3 (the bars of
``tests/test_pathwise_multiaction.py``); gradients 1e-8 against a float64 torch mirror and 1e-6 against central differences; the f32 Jacobian 3e-3 of max |J| (the f32
Jacobian bar of ``tests/test_pathwise_wide.py``), against the helper and against the f64 pass on the same paths."""
import copy
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, models as gp
from gpflowpilco_amd.synthetic import make_svgp
from oracle import mm_oracle as mo
from oracle import pathwise_oracle as pw
from tests import pathwise_matern_oracle as pmat
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, scale_err

F64, F32 = torch.float64, torch.float32
FAMILIES = {"matern32": 1, "matern52": 2}
CLASSES = {"se": gp.SquaredExponential, "matern32": gp.Matern32, "matern52": gp.Matern52}
F64_VALUE_BAR, F64_JAC_BAR, FD_BAR = 1e-10, 1e-8, 1e-6
F32_JAC_BAR = 3e-3                                    # tests/test_pathwise_wide.py's bar for an f32 Jacobian
F32_BAR, F64_BAR = 5e-3, 1e-10                        # policy rollouts: tests/test_pathwise_multiaction.py
SAMPLER_BAR = 1e-9                                    # tests/test_path_sampler.py's bar for "same draws, same paths"
H6, DT = 6, 0.5


def _model(p: mo.SVGPParams, device, kernel: str, pathwise: bool = True):
  """The torch model of oracle parameters with latents of class ``kernel``."""
  from gpflowpilco_amd.pathwise import PathwiseSVGP
  L = p.Z.shape[0]
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=device)
  kernels = [CLASSES[kernel](variance=t(p.variance[a]), lengthscales=t(p.lengthscales[a])) for a in range(L)]
  iv = gp.SeparateIndependentInducingVariables([gp.InducingPoints(t(p.Z[a])) for a in range(L)])
  kern = gp.LinearCoregionalization(kernels, t(p.W)) if p.W is not None else gp.SeparateIndependent(kernels)
  mean = gp.Zero() if p.mean_c is None else gp.Constant(t(p.mean_c))
  cls = PathwiseSVGP if pathwise else gp.SVGP
  return cls(kernel=kern, inducing_variable=iv, q_mu=t(p.q_mu), q_sqrt=t(p.q_sqrt), whiten=p.whiten, mean_function=mean,
             num_latent_gps=L)


def _arrays_of(paths, K, M):
  """The explicit arrays of a ``Paths`` (float64 numpy): the inverse of ``paths_from_arrays``' packing."""
  G, L, NB, _, BT = paths.wb.shape
  allw = paths.wb.permute(0, 3, 1, 2, 4).reshape(G * 4, L, NB * BT)[:paths.num_samples].double().cpu().numpy()
  Kp = paths.omega.shape[-1]
  omega = 2.0 * math.pi * paths.omega.double().cpu().numpy().transpose(0, 2, 1)[:, :K]
  phase = 2.0 * math.pi * paths.phase.double().cpu().numpy()[:, :K]
  return pw.Paths(omega=omega, phase=phase, w=allw[..., :K], v=allw[..., Kp:Kp + M])


# ---- CPU: the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["matern32", "matern52"])
def test_kernel_matrix_is_the_closed_form(name):
  rng = np.random.default_rng(1)
  X, Y = rng.uniform(-1, 2, size=(12, 3)), rng.uniform(-1, 2, size=(7, 3))
  ls, var = np.array([0.7, 1.3, 2.1]), 0.83
  k = CLASSES[name](variance=var, lengthscales=torch.tensor(ls))
  r = np.sqrt((((X[:, None] - Y[None]) / ls) ** 2).sum(-1))
  want = var * ((1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r) if name == "matern32" else
                (1 + np.sqrt(5) * r + 5 * r * r / 3) * np.exp(-np.sqrt(5) * r))
  got = k.K(torch.tensor(X), torch.tensor(Y)).numpy()
  assert np.abs(got - want).max() < 1e-12
  assert np.abs(pmat.kernel(X, Y, ls, var, FAMILIES[name]) - want).max() < 1e-14        # (the helper states the same forms)
  # (expanded form: r^2 ~ 1e-16 on the diagonal moves k by O(r^2) for Matern-5/2 and O(r^3)-smoothly for 3/2: sqrt3 r ~ 2e-8)
  assert np.abs(np.diagonal(k.K(torch.tensor(X)).numpy()) - var).max() < 1e-7
  sliced = CLASSES[name](variance=var, lengthscales=torch.tensor(ls[:2]), active_dims=(2, 0))
  assert torch.equal(sliced.K(torch.tensor(X), torch.tensor(Y)),
                     CLASSES[name](variance=var, lengthscales=torch.tensor(ls[:2])).K(torch.tensor(X[:, [2, 0]]),
                                                                                       torch.tensor(Y[:, [2, 0]])))
  assert sliced.slice_cov(torch.eye(3, dtype=F64)).shape == (2, 2) and sliced.lengthscales_vector(2).shape == (2,)
  assert isinstance(k, gp.Kernel) and not isinstance(k, gp.SquaredExponential)


def test_family_of_a_list_of_kernels_and_the_containers():
  se, m32, m52 = gp.SquaredExponential(), gp.Matern32(), gp.Matern52()
  assert gp.kernel_family([se, se]) == 0 and gp.kernel_family([m32]) == 1 and gp.kernel_family([m52, m52, m52]) == 2
  with pytest.raises(ValueError, match=r"latent 0: Matern52.*latent 1: SquaredExponential"):
    gp.kernel_family([m52, se])
  assert gp.SharedIndependent(m52, 3).num_latent_gps == 3 and gp.SeparateIndependent([m32, m32]).num_latent_gps == 2
  assert gp.LinearCoregionalization([m52, m52], np.ones((3, 2))).W.shape == (3, 2)


@pytest.mark.parametrize("name", ["matern32", "matern52"])
def test_spectral_draw_reproduces_the_kernel(name):
  """(2 / K) sum cos(omega.x + b) cos(omega.y + b) with the frequencies ``generate_paths`` uses, K = 65536: within six standard
  deviations 6 / sqrt K of the estimator (each term is bounded by 2, variance <= 1) of k(x, y) / var on 20 pairs."""
  from gpflowpilco_amd.pathwise import spectral_frequencies
  fam, K, d = FAMILIES[name], 65536, 3
  g = torch.Generator().manual_seed(0)
  ls = torch.tensor([[0.6, 1.1, 1.9]], dtype=F64)
  n = torch.randn(1, K, d, dtype=F64, generator=g)
  b = 2.0 * math.pi * torch.rand(1, K, dtype=F64, generator=g)
  chi = torch.randn(1, K, 3 if fam == 1 else 5, dtype=F64, generator=g)
  omega = spectral_frequencies(n, ls, fam, chi)[0]
  x = 2.0 * torch.rand(20, d, dtype=F64, generator=g)
  y = x + 1.5 * (torch.rand(20, d, dtype=F64, generator=g) - 0.5)
  est = (2.0 / K) * (torch.cos(x @ omega.T + b) * torch.cos(y @ omega.T + b)).sum(-1).numpy()
  want = np.array([pmat.kernel(x[i:i + 1].numpy(), y[i:i + 1].numpy(), ls[0].numpy(), 1.0, fam)[0, 0] for i in range(20)])
  err = np.abs(est - want).max()
  print(f"spectral draw {name}: max |estimate - k| = {err:.2e} (bar {6 / math.sqrt(K):.2e})")
  assert err < 6.0 / math.sqrt(K)
  assert torch.equal(spectral_frequencies(n, ls, 0), n / ls[:, None, :])
  with pytest.raises(ValueError):
    spectral_frequencies(n, ls, fam, None)


@pytest.mark.parametrize("case", ["matern32", "matern52", "matern52-coregionalised"])
def test_update_weights_interpolate_the_inducing_values(case):
  """q_sqrt = 0, whiten=False: every path of ``generate_paths`` passes through q_mu at the inducing points up to the jitter,
  Phi w + K v = u - jitter v, so the helper's f(Z) - q_mu + jitter v vanishes (1e-9 of max |q_mu|)."""
  from gpflowpilco_amd.pathwise import generate_paths
  name = case.split("-")[0]
  fam, coreg = FAMILIES[name], case.endswith("coregionalised")
  L, M, d, S, K = 2, 24, 3, 5, 64
  p = random_svgp_params(seed=11, L=L, M=M, d=d, whiten=False, ls_bounds=(0.8, 2.0), mean=True, W_rows=3 if coreg else None,
                         separate_Z=False)
  p.q_sqrt = np.zeros_like(p.q_sqrt)
  model = _model(p, "cpu", name)
  paths = generate_paths(model, S, K, dtype=F64, device="cpu", generator=torch.Generator().manual_seed(4))
  assert paths.kernel == fam and (paths.mix_W is not None) == coreg
  arr = _arrays_of(paths, K, M)
  worst = 0.0
  for m in range(M):
    x = np.broadcast_to(p.Z[0][m], (S, d))
    want = p.q_mu[m][None, :] - p.kuu_jitter * arr.v[:, :, m]                          # [S, L]
    if coreg:
      want = want @ p.W.T
    worst = max(worst, np.abs(pmat.eval_paths(arr, p, x, fam) - np.asarray(p.mean_c)[None] - want).max())
  assert worst < 1e-9 * np.abs(p.q_mu).max(), worst


def test_se_draws_are_what_they_were():
  """A SquaredExponential model draws, from a given generator state, bit for bit what ``generate_paths`` drew before the Matern
  families existed: an in-test restatement of that draw order (n, b, w, eps and nothing after)."""
  from gpflowpilco_amd.linalg import cholesky
  from gpflowpilco_amd.pathwise import generate_paths, paths_from_arrays
  L, M, d, S, K = 2, 20, 3, 6, 40
  p = random_svgp_params(seed=12, L=L, M=M, d=d, whiten=True, ls_bounds=(0.8, 2.0), mean=True, separate_Z=True)
  model = _model(p, "cpu", "se")
  seed = lambda: torch.Generator().manual_seed(21)
  got = generate_paths(model, S, K, dtype=F64, device="cpu", generator=seed())
  g = seed()
  Z, ls, var = (torch.tensor(a, dtype=F64) for a in (p.Z, p.lengthscales, p.variance))
  rn = lambda *shape: torch.randn(*shape, dtype=F64, generator=g)
  omega = rn(L, K, d) / ls[:, None, :]
  phase = 2.0 * math.pi * torch.rand(L, K, dtype=F64, generator=g)
  w = rn(S, L, K)
  A = Z / ls[:, None, :]
  d2 = (A * A).sum(-1)[:, :, None] + (A * A).sum(-1)[:, None, :] - 2.0 * A @ A.transpose(1, 2)
  Luu = cholesky(var[:, None, None] * torch.exp(-0.5 * d2.clamp_min(0.0)) + gp.DEFAULT_JITTER * torch.eye(M, dtype=F64))
  eps = rn(S, L, M)
  u = torch.tensor(p.q_mu).T[None] + torch.einsum('slm,lnm->sln', eps, torch.tril(torch.tensor(p.q_sqrt)))
  u = torch.einsum('lnm,slm->sln', Luu, u)
  Phi_Z = torch.sqrt(2.0 * var / K)[:, None, None] * torch.cos(Z @ omega.transpose(1, 2) + phase[:, None, :])
  v = torch.cholesky_solve((u - torch.einsum('lmk,slk->slm', Phi_Z, w)).permute(1, 2, 0), Luu).permute(2, 0, 1)
  ref = paths_from_arrays(omega, phase, w, v, Z, ls, var, torch.tensor(p.mean_c), dtype=F64, device="cpu")
  assert got.kernel == 0 and ref.kernel == 0
  for name in ("omega", "phase", "zs", "hz", "wb", "lengthscales", "prior_scale", "variance", "mean_c"):
    assert torch.equal(getattr(got, name), getattr(ref, name)), name
  assert torch.equal(g.get_state(), (lambda gg: (generate_paths(model, S, K, dtype=F64, device="cpu", generator=gg), gg)[1])(seed())
                     .get_state())                                              # ... and consumes the same amount of the stream


# ---- CPU: refusals ---------------------------------------------------------------------------------------------------------------
def _cartpole(device, drift_kernel="matern52", policy_kernel="se", S=8):
  """nx 4, one angle, one action, nd 6: (system with a Euler solver, objective, x0)."""
  from gpflowpilco_amd import bijectors as tfb, dynamics
  from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=device)
  drift = _model(oracle_params(make_svgp(4, 30, 6, seed=3, ls_bounds=(0.8, 3.0))), device, drift_kernel)
  pol = _model(random_svgp_params(seed=5, L=1, M=12, d=5, whiten=True, ls_bounds=(0.8, 2.0), mean=True), device, policy_kernel,
               pathwise=False)
  head = tfb.Chain([tfb.Scale(t(2.0)), tfb.Shift(t(-0.5)), tfb.NormalCDF()])
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head)
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=TrigonometricEncoder(active_dims=(1,)),
                                    solver=dynamics.Euler())
  objective = GaussianObjective(target=t(np.zeros(5)), precis=t(np.eye(5)))
  x0 = t(np.random.default_rng(2).uniform(0.2, 0.8, size=(S, 4)))
  return system, objective, x0


def test_moment_matching_refuses_a_matern_model():
  from gpflowpilco_amd.moment_matching import GaussianMoments, moment_matching
  p = random_svgp_params(seed=13, L=2, M=10, d=2, whiten=True, mean=True)
  model = _model(p, "cpu", "matern52", pathwise=False)
  with pytest.raises(NotImplementedError, match="closed forms for SquaredExponential only"):
    model.precompute("cpu")
  with pytest.raises(NotImplementedError, match="closed forms for SquaredExponential only"):
    model.packed(F64, True, "cpu")
  x = GaussianMoments((torch.zeros(1, 2, dtype=F64), 0.1 * torch.eye(2, dtype=F64)[None]), centered=True)
  with pytest.raises(NotImplementedError, match="closed forms for SquaredExponential only"):
    moment_matching(x, model)
  mixed = _model(p, "cpu", "matern52", pathwise=False)
  mixed.kernel.kernels[1] = gp.SquaredExponential(variance=0.5, lengthscales=torch.ones(2, dtype=F64))
  with pytest.raises(ValueError, match="of one family"):
    mixed.precompute("cpu")
  with pytest.raises(ValueError, match="of one family"):
    from gpflowpilco_amd.pathwise import generate_paths
    generate_paths(mixed, 4, 16, dtype=F64, device="cpu")


@pytest.mark.parametrize("name", ["matern32", "matern52"])
def test_predict_mean_of_a_matern_model(name):
  p = random_svgp_params(seed=14, L=2, M=15, d=3, whiten=True, ls_bounds=(0.8, 2.0), mean=True)
  model = _model(p, "cpu", name, pathwise=False)
  x = np.random.default_rng(3).uniform(size=(9, 3))
  want = np.empty((9, 2))
  for a in range(2):
    Kuu = pmat.kernel(p.Z[a], p.Z[a], p.lengthscales[a], p.variance[a], FAMILIES[name]) + p.kuu_jitter * np.eye(15)
    Lu = np.linalg.cholesky(Kuu)
    want[:, a] = pmat.kernel(x, p.Z[a], p.lengthscales[a], p.variance[a], FAMILIES[name]) @ np.linalg.solve(Lu.T, p.q_mu[:, a]) \
        + p.mean_c[a]
  assert scale_err(model.predict_mean(torch.tensor(x)), want) < 1e-10


def test_closures_name_their_reason_for_a_matern_model():
  from gpflowpilco_amd import dynamics
  from gpflowpilco_amd.loops import _native_parts, pathwise_policy_loss_closure, policy_loss_closure
  system, objective, x0 = _cartpole("cpu")
  why = []
  assert _native_parts(system, objective, why, moment_solver=False) is not None and not why        # the pathwise solver takes it
  system.solver = dynamics.MomentMatchingEuler()
  assert _native_parts(system, objective, why, moment_solver=True) is None
  assert "Matern52 drift" in why[0] and "SquaredExponential only" in why[0]
  init = lambda: (x0[0], 0.01 * torch.eye(4, dtype=F64))
  with pytest.raises(ValueError, match="Matern52 drift"):
    policy_loss_closure(system, objective, init, 2, native=True)
  # a Matern policy: refused by both solvers' native routes
  for solver, moment in ((dynamics.Euler(), False), (dynamics.MomentMatchingEuler(), True)):
    sys_p, obj_p, _ = _cartpole("cpu", drift_kernel="se", policy_kernel="matern32")
    sys_p.solver = solver
    why = []
    assert _native_parts(sys_p, obj_p, why, moment_solver=moment) is None
    assert "Matern32 policy" in why[0] and "SquaredExponential policy" in why[0]
  sys_p, obj_p, _ = _cartpole("cpu", drift_kernel="se", policy_kernel="matern32")
  with pytest.raises(ValueError, match="Matern32 policy"):
    pathwise_policy_loss_closure(sys_p, obj_p, lambda: x0, 2, native=True)
  sys_p.solver = dynamics.MomentMatchingEuler()
  with pytest.raises(ValueError, match="Matern32 policy"):
    policy_loss_closure(sys_p, obj_p, init, 2, native=True)


def test_kern_entries_refuse_an_unknown_family_without_a_gpu():
  lib = _lib.lib()
  import ctypes
  buf = (ctypes.c_char * 64)()
  p = ctypes.addressof(buf)
  act = (ctypes.c_int32 * 1)(1)
  for k in (3, -1):
    assert lib.mm_pathwise_eval_kern(4, 2, 256, 256, 3, 0, *([p] * 11), None, k) == -1
    assert lib.mm_pathwise_eval_jac_kern(4, 2, 256, 256, 3, 0, *([p] * 12), None, k) == -1
    assert lib.mm_pathwise_eval_bound_kern(4, 2, 256, 256, 3, 0, *([p] * 12), None, k) == -1
    assert lib.mm_pathwise_rollout_kern(4, 3, 256, 256, 3, 0, 2, 1.0, *([p] * 12), None, k) == -1
    assert lib.mm_pathwise_policy_rollout_kern(4, 256, 256, 0, 2, 1.0, 4, 1, act, 1, *([p] * 9), p, 64, 12, p, p, p, p, p, p, p,
                                               64, 0, None, 0, None, None, k) == -1
  # a known family: the sibling's own validation, still before any launch
  assert lib.mm_pathwise_eval_kern(4, 2, 100, 256, 3, 0, *([p] * 11), None, 2) == -2          # M no multiple of the block
  assert lib.mm_pathwise_eval_kern(4, 2, 256, 256, 3, 0, None, *([p] * 10), None, 1) == -1
  assert lib.mm_pathwise_policy_rollout_kern(4, 256, 256, 0, 2, 1.0, 4, 1, act, 5, *([p] * 9), p, 64, 12, p, p, p, p, p, p, p,
                                             64, 0, None, 0, None, None, 1) == -2              # nu outside 1 .. 4


def test_paths_from_arrays_takes_the_family_by_name():
  from gpflowpilco_amd.pathwise import paths_from_arrays
  z = lambda *s: np.zeros(s)
  for name, code in (("se", 0), ("matern32", 1), ("matern52", 2)):
    P = paths_from_arrays(z(1, 4, 2), z(1, 4), z(3, 1, 4), z(3, 1, 5), z(1, 5, 2), np.ones((1, 2)), np.ones(1), dtype=F64,
                          device="cpu", kernel=name)
    assert P.kernel == code
  with pytest.raises(ValueError):
    paths_from_arrays(z(1, 4, 2), z(1, 4), z(3, 1, 4), z(3, 1, 5), z(1, 5, 2), np.ones((1, 2)), np.ones(1), dtype=F64,
                      device="cpu", kernel="matern12")


# ---- GPU: evaluation, Jacobian, rounding bound ------------------------------------------------------------------------------------
# (d, K blocks, M): S = 37 (ragged last group), L = 5 (a wave owns two latents); d 3 / 6 / 9 -> DK 4 / 8 / 16 (half-groups); one and
# three blocks of K and of M (M = 100 is padded): the ring's prefetch clamps with fewer and with more blocks than its depth.  BIG:
# operands that do not fit the LDS kernel (17 (K + M) elements > 144 KB): the global-operand kernel.
EVAL_SHAPES = [(3, 1, 100), (6, 3, 3), (9, 1, 3), (9, 3, 100), "BIG"]
S_EVAL, L_EVAL = 37, 5


@functools.lru_cache(maxsize=None)
def _eval_case(name, shape, f32):
  """numpy model, paths, inputs and the helper's f / J / central differences (computed once, shared, never modified).  A sample
  sits exactly on an inducing point of every latent's own set where the latents share Z (row 5 of latent 0's here: separate Z)."""
  fam, bt = FAMILIES[name], 256 if f32 else 128
  if shape == "BIG":
    d, K, M = 16, (1024 if f32 else 512), (1280 if f32 else 640)
  else:
    d, K, M = shape[0], shape[1] * bt, (shape[2] if shape[2] == 100 else shape[2] * bt)
  p = random_svgp_params(seed=60 + d, L=L_EVAL, M=M, d=d, whiten=True, ls_bounds=(0.8, 3.0), mean=True, separate_Z=True)
  rng = np.random.default_rng(61 + d)
  paths = pmat.draw_paths(rng, p, S_EVAL, K, fam)
  x = rng.uniform(size=(S_EVAL, d))
  x[3] = p.Z[0][5]                                                                   # on an inducing point of latent 0
  x[8] = p.Z[4][M - 1]                                                               # ... and of latent 4
  f, J = pmat.eval_paths(paths, p, x, fam), pmat.eval_jac(paths, p, x, fam)
  dirn = rng.standard_normal(x.shape)
  h = 1e-6
  fd = (pmat.eval_paths(paths, p, x + h * dirn, fam) - pmat.eval_paths(paths, p, x - h * dirn, fam)) / (2 * h)
  return dict(p=p, paths=paths, x=x, f=f, J=J, dirn=dirn, fd=fd, fam=fam, d=d, K=K, M=M)


def _device_paths(c, dtype, device, kernel=None):
  from gpflowpilco_amd.pathwise import paths_from_arrays
  p, P = c["p"], c["paths"]
  return paths_from_arrays(P.omega, P.phase, P.w, P.v, p.Z, p.lengthscales, p.variance, p.mean_c, dtype=dtype, device=device,
                           kernel=c["fam"] if kernel is None else kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=lambda s: s if isinstance(s, str) else "d{}K{}M{}".format(*s))
@pytest.mark.parametrize("name", ["matern32", "matern52"])
def test_gpu_f64_values_and_jacobian_match_the_helper(name, shape, device):
  c = _eval_case(name, shape, False)
  P = _device_paths(c, F64, device)
  x = torch.tensor(c["x"], dtype=F64, device=device)
  f = P(x)
  fj, J = P.eval_jac(x)
  fb, err = P.eval_with_bound(x)
  assert torch.equal(f, fj) and torch.equal(f, fb)
  assert torch.isfinite(f).all() and torch.isfinite(J).all() and torch.isfinite(err).all()
  ef, eJ = scale_err(f, c["f"]), scale_err(J, c["J"])
  Jd = np.einsum('sld,sd->sl', J.cpu().numpy(), c["dirn"])
  efd = float(np.abs(Jd - c["fd"]).max() / max(1.0, np.abs(c["fd"]).max()))
  on = [3, 8]
  eon = max(scale_err(f[on], c["f"][on]), scale_err(J[on], c["J"][on]) * 1e-2)
  print(f"{name} {shape} f64: values {ef:.2e} Jacobian {eJ:.2e} vs central differences {efd:.2e}; on-point rows (values, J/100) {eon:.2e}")
  assert ef < F64_VALUE_BAR and eJ < F64_JAC_BAR and efd < FD_BAR
  assert scale_err(f[on], c["f"][on]) < F64_VALUE_BAR and scale_err(J[on], c["J"][on]) < F64_JAC_BAR
  assert float((f.double().cpu() - torch.tensor(c["f"])).abs().max()) <= float(err.max())       # (the f64 bound holds too)
  xg = x.clone().requires_grad_(True)                                                            # autograd through __call__
  P(xg).sum().backward()
  assert scale_err(xg.grad, c["J"].sum(1)) < F64_JAC_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=lambda s: s if isinstance(s, str) else "d{}K{}M{}".format(*s))
@pytest.mark.parametrize("name", ["matern32", "matern52"])
def test_gpu_f32_values_lie_inside_their_rounding_bound(name, shape, device):
  """The reference is the helper evaluated on the f32-rounded operands' SOURCE (the f64 arrays): the bound covers the rounding of
  the stream, the operands and the basis values.  The worst ratio error / bound is printed.  The f32
  Jacobian -- the packed sample-pair code of the LDS kernels and the f32 ``JAC`` instantiations of the global-operand one (BIG) --
  is held to 3e-3 of max |J| against the helper AND against the f64 pass on the same arrays, over all rows and over the two rows
  that sit on an inducing point alone (relative to those rows' own max |J|)."""
  c = _eval_case(name, shape, True)
  P = _device_paths(c, F32, device)
  x32 = torch.tensor(c["x"], dtype=F32, device=device)
  f, err = P.eval_with_bound(x32)
  fj, J = P.eval_jac(x32)
  assert torch.equal(f, P(x32)) and torch.equal(f, fj)
  assert torch.isfinite(f).all() and torch.isfinite(J).all() and torch.isfinite(err).all()
  # the helper at the inputs the device received (x rounded to f32); the operands' own rounding is inside the bound's budget
  want = pmat.eval_paths(c["paths"], c["p"], x32.double().cpu().numpy(), c["fam"])
  ratio = (f.double().cpu().numpy() - want) / err.double().cpu().numpy()
  worst = float(np.abs(ratio).max())
  Jo = pmat.eval_jac(c["paths"], c["p"], x32.double().cpu().numpy(), c["fam"])
  f64v, J64 = _device_paths(c, F64, device).eval_jac(x32.double())
  J64 = J64.cpu().numpy()
  on = [3, 8]
  eJ, eJon = scale_err(J, Jo), scale_err(J[on], Jo[on])
  eJ64, eJ64on = scale_err(J, J64), scale_err(J[on], J64[on])
  e64 = scale_err(f, f64v.cpu().numpy())
  print(f"{name} {shape} f32: worst |error| / bound = {worst:.3f} (rows on an inducing point: {float(np.abs(ratio[on]).max()):.3f}); "
        f"Jacobian vs helper {eJ:.2e} (on-point rows {eJon:.2e}), vs the f64 pass {eJ64:.2e} (on-point rows {eJ64on:.2e}); "
        f"values vs the f64 pass {e64:.2e}")
  assert worst <= 1.0
  assert eJ < F32_JAC_BAR and eJon < F32_JAC_BAR and eJ64 < F32_JAC_BAR and eJ64on < F32_JAC_BAR
  assert float(np.abs(J.double().cpu().numpy()[on]).max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_gpu_kernel_zero_through_the_kern_entries_is_bit_equal(dtype, device):
  """kernel = 0 through mm_pathwise_eval_kern / _eval_jac_kern / _eval_bound_kern / _rollout_kern: the existing entries' bits."""
  from gpflowpilco_amd.ops import _dtype_code, _ptr, _stream
  lib = _lib.lib()
  for shape in ((6, 3, 3), "BIG"):
    c = _eval_case("matern52", shape, dtype == F32)
    P = _device_paths(c, dtype, device, kernel="se")
    S, L, Mp, Kp, d = P._dims()
    x = torch.tensor(c["x"], dtype=dtype, device=device)
    ops = (x.data_ptr(), P.omega.data_ptr(), P.phase.data_ptr(), P.zs.data_ptr(), P.hz.data_ptr(), P.lengthscales.data_ptr(),
           P.prior_scale.data_ptr(), P.variance.data_ptr(), _ptr(P.mean_c), P.wb.data_ptr())
    new = lambda *s: torch.zeros(*s, dtype=dtype, device=device)
    f, fj, J, fb, ab = new(S, L), new(S, L), new(S, L, d), new(S, L), new(S, L)
    code, st = _dtype_code(dtype), _stream(x.device)
    assert lib.mm_pathwise_eval_kern(S, L, Mp, Kp, d, code, *ops, f.data_ptr(), st, 0) == 0
    assert lib.mm_pathwise_eval_jac_kern(S, L, Mp, Kp, d, code, *ops, fj.data_ptr(), J.data_ptr(), st, 0) == 0
    assert lib.mm_pathwise_eval_bound_kern(S, L, Mp, Kp, d, code, *ops, fb.data_ptr(), ab.data_ptr(), st, 0) == 0
    f0 = P(x)
    f1, J1 = P.eval_jac(x)
    assert torch.equal(f, f0) and torch.equal(fj, f1) and torch.equal(J, J1) and torch.equal(fb, f0)
    assert torch.equal(ab * (8.0 * 0.5 * torch.finfo(dtype).eps), P.eval_with_bound(x)[1])
    assert float(J.abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["se", "matern32"])
def test_gpu_drift_only_rollout(name, dtype, device):
  """``Paths.rollout`` (d == L): kernel 0 through mm_pathwise_rollout_kern is bit-equal to mm_pathwise_rollout; a Matern drift
  follows the helper's Euler fold."""
  from gpflowpilco_amd.ops import _dtype_code, _ptr, _stream
  from gpflowpilco_amd.pathwise import paths_from_arrays
  fam = 0 if name == "se" else FAMILIES[name]
  S, L, H = 37, 3, 4
  p = random_svgp_params(seed=70, L=L, M=50, d=L, whiten=True, ls_bounds=(0.8, 3.0), mean=True, separate_Z=True)
  rng = np.random.default_rng(71)
  paths = pmat.draw_paths(rng, p, S, 130, fam)
  paths.w *= 0.3; paths.v *= 0.3
  x0 = rng.uniform(0.2, 0.8, size=(S, L))
  P = paths_from_arrays(paths.omega, paths.phase, paths.w, paths.v, p.Z, p.lengthscales, p.variance, p.mean_c, dtype=dtype,
                        device=device, kernel=name)
  xt = torch.tensor(x0, dtype=dtype, device=device)
  xH, traj = P.rollout(xt, H, dt=DT, keep_trajectory=True)
  if fam == 0:
    S_, L_, Mp, Kp, d = P._dims()
    x, tmp, tr = xt.clone(), torch.empty_like(xt), torch.empty(H, S, L, dtype=dtype, device=device)
    rc = _lib.lib().mm_pathwise_rollout_kern(S, L, Mp, Kp, d, _dtype_code(dtype), H, DT, x.data_ptr(), tmp.data_ptr(),
                                             P.omega.data_ptr(), P.phase.data_ptr(), P.zs.data_ptr(), P.hz.data_ptr(),
                                             P.lengthscales.data_ptr(), P.prior_scale.data_ptr(), P.variance.data_ptr(),
                                             _ptr(P.mean_c), P.wb.data_ptr(), tr.data_ptr(), _stream(xt.device), 0)
    assert rc == 0 and torch.equal(x, xH) and torch.equal(tr, traj)
    return
  x, want = x0.copy(), []
  for _ in range(H):
    x = x + DT * pmat.eval_paths(paths, p, x, fam)
    want.append(x.copy())
  e = scale_err(traj, np.stack(want))
  print(f"drift-only rollout {name} {dtype}: {e:.2e}")
  assert e < (F64_BAR if dtype == F64 else F32_BAR) and torch.equal(traj[-1], xH)


# ---- GPU: policy rollouts ---------------------------------------------------------------------------------------------------------
SCALE, SHIFT = (2.0, 1.5), (-0.5, -0.4)
SYSTEMS = {"P": dict(nx=4, active=(0, 1), nu=2, seed=40, Lg=None),       # nd 8, two actions
           "D": dict(nx=6, active=(1, 2), nu=1, seed=45, Lg=None),       # nd 9: wide, one action
           "G": dict(nx=3, active=(1,), nu=1, seed=47, Lg=2),            # coregionalised: Lg 2 -> nx 3, nd 5
           "C": dict(nx=4, active=(1,), nu=1, seed=49, Lg=None)}         # the cartpole shape: one action, nd 6, unmixed -- a Matern
                                                                         # drift makes PolicyRollout take the wide / _nd entries


@functools.lru_cache(maxsize=None)
def _system(sysname, name, S):
  c = SYSTEMS[sysname]
  fam = 0 if name == "se" else FAMILIES[name]
  nx, active, nu, seed, Lg = c["nx"], c["active"], c["nu"], c["seed"], c["Lg"]
  na = len(active); ne = nx + na; nd = ne + nu
  rng = np.random.default_rng(seed)
  if Lg is None:
    drift = oracle_params(make_svgp(nx, 50, nd, seed=seed + 1, ls_bounds=(0.8, 3.0)))
  else:
    drift = random_svgp_params(seed=seed + 1, L=Lg, M=50, d=nd, whiten=True, ls_bounds=(0.8, 3.0), mean=True, W_rows=nx,
                               separate_Z=True)
    drift.q_mu = 0.3 * drift.q_mu
    drift.mean_c = 0.1 * drift.mean_c
  drift.Z[..., ne:] = 4.0 * drift.Z[..., ne:] - 2.0                       # action axes in [-2, 2]
  pol = random_svgp_params(seed=seed + 2, L=nu, M=12, d=ne, whiten=True, ls_bounds=(0.8, 2.0), mean=True, separate_Z=True)
  pol.q_mu = 0.3 * pol.q_mu
  paths = pmat.draw_paths(rng, drift, S, 130, fam)
  paths.w *= 0.3; paths.v *= 0.3
  x0 = rng.uniform(0.2, 0.8, size=(S, nx))
  target = np.zeros(ne); target[na:2 * na] = 1.0; target[2 * na:] = 0.1
  A = rng.standard_normal((ne, ne))
  precis = 0.5 * (A @ A.T) / ne + 0.5 * np.eye(ne)
  scale, shift = np.array(SCALE[:nu]), np.array(SHIFT[:nu])
  cost_o, states_o = pmat.policy_rollout(paths, drift, fam, pol, scale, shift, active, target, precis, x0, H6, dt=DT)
  return dict(c, fam=fam, name=name, S=S, na=na, ne=ne, nd=nd, drift=drift, pol=pol, paths=paths, x0=x0, target=target,
              precis=precis, scale=scale, shift=shift, cost_o=cost_o, states_o=states_o)


def _roll_case(sy, device, dtype, kernel=None):
  from gpflowpilco_amd.pathwise import PolicyRollout, paths_from_arrays
  P, dr = sy["paths"], sy["drift"]
  mixed = dr.W is not None
  gp_paths = paths_from_arrays(P.omega, P.phase, P.w, P.v, dr.Z, dr.lengthscales, dr.variance, None if mixed else dr.mean_c,
                               dtype=dtype, device=device, mix_W=dr.W, mix_c=dr.mean_c if mixed else None,
                               kernel=sy["fam"] if kernel is None else kernel)
  pol_model = gp_model_from_oracle(sy["pol"], device)
  nu = sy["nu"]
  scale = float(sy["scale"][0]) if nu == 1 else tuple(sy["scale"])
  shift = float(sy["shift"][0]) if nu == 1 else tuple(sy["shift"])
  roll = PolicyRollout(gp_paths, pol_model.packed(F64, False, device), nx=sy["nx"], active_dims=sy["active"], head_scale=scale,
                       head_shift=shift, target=torch.tensor(sy["target"]), precis=torch.tensor(sy["precis"]),
                       wide=sy["nd"] > 8)
  return gp_paths, pol_model, roll


def _forward_errors(sysname, name, S, dtype, device):
  sy = _system(sysname, name, S)
  _, _, roll = _roll_case(sy, device, dtype)
  x0 = torch.tensor(sy["x0"], dtype=dtype, device=device)
  cost, tape = roll(x0, H6, dt=DT, with_jacobians=False)
  cost_j, tape_j = roll(x0, H6, dt=DT, with_jacobians=True)
  assert torch.equal(cost, cost_j) and torch.equal(roll.states(tape, H6), roll.states(tape_j, H6))
  return scale_err(cost, sy["cost_o"]), scale_err(roll.states(tape, H6), sy["states_o"])


@pytest.mark.gpu
@pytest.mark.parametrize("S", [37, 300])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("sysname,name", [("P", "matern32"), ("P", "matern52"), ("D", "matern32"), ("D", "matern52"),
                                          ("G", "matern52"), ("C", "matern32")])
def test_gpu_policy_rollout_matches_the_helper(sysname, name, dtype, S, device):
  ec, es = _forward_errors(sysname, name, S, dtype, device)
  if dtype == F32:
    se = max(_forward_errors(sysname, "se", S, dtype, device))
    print(f"policy rollout {sysname} {name} S={S} f32: cost {ec:.3e} states {es:.3e}; SquaredExponential, same recipe, same process: "
          f"{se:.3e}")
  else:
    print(f"policy rollout {sysname} {name} S={S} f64: cost {ec:.3e} states {es:.3e}")
  tol = F64_BAR if dtype == F64 else F32_BAR
  assert ec < tol and es < tol


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("sysname", ["P", "D", "G"])
def test_gpu_policy_rollout_kern_with_kernel_zero_is_bit_equal(sysname, dtype, device):
  """mm_pathwise_policy_rollout_kern(kernel = 0): the cost and the WHOLE tape of the existing entry (_nd for P, _wide for D,
  _mixed for G)."""
  sy = _system(sysname, "se", 37)
  P, pm, roll = _roll_case(sy, device, dtype)
  assert roll.kernel == 0
  S, L, Mp, Kp, d = P._dims()
  x0 = torch.tensor(sy["x0"], dtype=dtype, device=device)
  from gpflowpilco_amd.ops import _dtype_code, _ptr, _stream
  lib, pol = _lib.lib(), roll.policy
  for jac in (False, True):
    # (the one-action system D runs the _wide entry here: nd_entries follows wide)
    cost, tape = roll(x0, H6, dt=DT, with_jacobians=jac)
    cost2, tape2 = torch.full_like(cost, 7.0), torch.zeros_like(tape)
    tape.zero_()
    cost, tape_ref = roll(x0, H6, dt=DT, with_jacobians=jac)
    # the padding between the tape's blocks is never written: compare two zero-initialised buffers
    tape_a = torch.zeros_like(tape_ref)
    import ctypes
    nu = sy["nu"]
    sc, sh = (ctypes.c_double * nu)(*sy["scale"]), (ctypes.c_double * nu)(*sy["shift"])
    act = (ctypes.c_int32 * sy["na"])(*sy["active"])
    mixing = (roll.Lg, roll._mix_W.data_ptr(), _ptr(roll._mix_c)) if roll.mixed else (0, None, None)
    common = (S, Mp, Kp, _dtype_code(dtype), H6, DT, sy["nx"], sy["na"], act, nu, P.omega.data_ptr(), P.phase.data_ptr(),
              P.zs.data_ptr(), P.hz.data_ptr(), P.lengthscales.data_ptr(), P.prior_scale.data_ptr(), P.variance.data_ptr(),
              _ptr(P.mean_c), P.wb.data_ptr(), pol.buf.data_ptr(), pol.nbytes, pol.M, sc, sh, roll.target.data_ptr(),
              roll.precis.data_ptr(), x0.data_ptr())
    rc = lib.mm_pathwise_policy_rollout_kern(*common, cost2.data_ptr(), tape2.data_ptr(), tape2.numel(), int(jac),
                                             _stream(x0.device), *mixing, 0)
    assert rc == 0
    entry = "mm_pathwise_policy_rollout_" + ("mixed" if roll.mixed else "wide" if roll.wide else "nd")
    cost_a = torch.full_like(cost, 3.0)
    rc = getattr(lib, entry)(*common, cost_a.data_ptr(), tape_a.data_ptr(), tape_a.numel(), int(jac), _stream(x0.device),
                             *(mixing if roll.mixed else ()))
    assert rc == 0
    assert torch.equal(cost2, cost_a) and torch.equal(tape2, tape_a) and float(cost2.abs().max()) > 0.0


# ---- GPU: gradients through the closure -------------------------------------------------------------------------------------------
class _TorchPaths:
  """A differentiable float64 torch mirror of Matern sample paths (difference form), in place of ``pathwise.Paths``."""

  def __init__(self, sy, device):
    t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=device)
    P, dr = sy["paths"], sy["drift"]
    self.om, self.ph, self.w, self.v = t(P.omega), t(P.phase), t(P.w), t(P.v)
    self.Z, self.ls, self.var = t(dr.Z), t(dr.lengthscales), t(dr.variance)
    self.W = None if dr.W is None else t(dr.W)
    self.mean = None if dr.mean_c is None else t(dr.mean_c)
    self.fam = sy["fam"]

  def __call__(self, x):
    f = []
    for a in range(self.Z.shape[0]):
      phi = torch.sqrt(2.0 * self.var[a] / self.om.shape[1]) * torch.cos(x @ self.om[a].T + self.ph[a][None])
      r2 = (((x[:, None, :] - self.Z[a][None]) / self.ls[a]) ** 2).sum(-1)
      f.append((self.w[:, a] * phi).sum(-1) + (self.v[:, a] * self.var[a] * gp.stationary_profile(r2, self.fam)).sum(-1))
    f = torch.stack(f, dim=-1)
    if self.W is not None:
      f = f @ self.W.T
    return f if self.mean is None else f + self.mean[None]


def _torch_system(sy, device):
  from gpflowpilco_amd import bijectors as tfb, dynamics
  from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=device)
  drift = _model(sy["drift"], device, sy["name"])
  pol_model = gp_model_from_oracle(sy["pol"], device)
  head = tfb.Chain([tfb.Scale(t(sy["scale"])), tfb.Shift(t(sy["shift"])), tfb.NormalCDF()])
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol_model), invlink=head)
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=TrigonometricEncoder(active_dims=sy["active"]),
                                    solver=dynamics.Euler())
  return system, GaussianObjective(target=t(sy["target"]), precis=t(sy["precis"])), pol_model


def _policy_params(pm, nu):
  ks, ivs = pm.kernel.kernels, pm.inducing_variable.inducing_variables
  return {"q_mu": [pm.q_mu], "Z": [ivs[a].Z for a in range(nu)], "lengthscales": [ks[a].lengthscales for a in range(nu)],
          "variance": [ks[a].variance for a in range(nu)]}


FLAGS = dict(native_actions=4, native_inputs=16, native_coregionalized=True)


@pytest.mark.gpu
@pytest.mark.parametrize("sysname,name", [("P", "matern52"), ("D", "matern32"), ("G", "matern52"), ("C", "matern32")])
def test_gpu_gradient_of_the_mean_sample_loss_through_the_closure(sysname, name, device):
  """d mean_s sum_h cost / d (q_mu, Z, lengthscales, variance of the policy, x0), f64, H = 5, S = 37, through
  ``pathwise_policy_loss_closure``: (i) torch autograd of the closure's torch composition on a float64 torch MIRROR of the paths
  (difference-form kernels, no native code), 1e-8 relative per tensor; (ii) central differences (h = 1e-6) of the numpy helper
  along one random direction per group and for x0, 1e-6 max(1, |fd|); (iii) the closure with native=False on the SAME device
  paths, 1e-9 in loss and gradients; (iv) two backward calls on one tape are bit-equal."""
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _system(sysname, name, 37)
  S, H, nu = 37, 5, sy["nu"]
  system, objective, pm = _torch_system(sy, device)
  groups = _policy_params(pm, nu)
  params = [t for ts in groups.values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)
  paths, _, roll = _roll_case(sy, device, F64)
  assert roll.supports_backward() and paths.kernel == sy["fam"]
  assert roll.wide and roll.nd_entries                       # (system C: forced by the family, not by the shape)

  def run(pth, **kw):
    for t in params + [x0]:
      t.grad = None
    loss = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=pth, **kw)()
    loss.mean().backward()
    return loss.detach(), [t.grad.detach().clone() for t in params + [x0]]
  with warnings.catch_warnings():
    warnings.simplefilter("error")                                                   # (no fallback: the native route ran)
    ln, gn = run(paths, native=True, **({} if sysname == "C" else FLAGS))           # (C: the closure's default arguments)
    lt, gt = run(paths, native=False)
    lm, gm = run(_TorchPaths(sy, device), native=False)
  want = sy["cost_o"][:H].sum(0)
  assert scale_err(ln, want) < F64_BAR and scale_err(lm, want) < F64_BAR
  el = float((ln - lt).abs().max())
  assert el < 1e-9, el
  names = [f"{k}[{a}]" for k, ts in groups.items() for a in range(len(ts))] + ["x0"]
  for nm, a_, b_, c_ in zip(names, gn, gm, gt):
    em = float((a_ - b_).abs().max()) / max(1e-14, float(b_.abs().max()))
    et = float((a_ - c_).abs().max()) / max(1e-14, float(c_.abs().max()))
    print(f"gradient {sysname} {name} {nm}: native vs torch mirror {em:.2e}, vs torch composition on the device paths {et:.2e}")
    assert em < 1e-8 and et < 1e-9, (nm, em, et)

  rng = np.random.default_rng(5)

  def oracle_loss(pol, x_init):
    return pmat.policy_rollout(sy["paths"], sy["drift"], sy["fam"], pol, sy["scale"], sy["shift"], sy["active"], sy["target"],
                               sy["precis"], x_init, H, dt=DT)[0].sum(0).mean()
  h, gi = 1e-6, 0
  for field in ("q_mu", "Z", "lengthscales", "variance"):
    base = np.asarray(getattr(sy["pol"], field), dtype=np.float64)
    dirn = rng.standard_normal(base.shape)
    vals = []
    for sgn in (1.0, -1.0):
      pol2 = copy.deepcopy(sy["pol"])
      setattr(pol2, field, base + sgn * h * dirn)
      vals.append(oracle_loss(pol2, sy["x0"]))
    fd = (vals[0] - vals[1]) / (2 * h)
    n = len(groups[field])
    got = gn[gi].cpu().numpy() if field == "q_mu" else np.stack([t.cpu().numpy().reshape(base.shape[1:]) for t in gn[gi:gi + n]])
    gi += n
    an = float((got.reshape(base.shape) * dirn).sum())
    print(f"gradient {sysname} {name} {field}: native {an:+.8e} fd {fd:+.8e}")
    assert abs(fd - an) < 1e-6 * max(1.0, abs(fd)), (field, fd, an)
  dirx = rng.standard_normal(sy["x0"].shape)
  fd = (oracle_loss(sy["pol"], sy["x0"] + h * dirx) - oracle_loss(sy["pol"], sy["x0"] - h * dirx)) / (2 * h)
  an = float((gn[-1].cpu().numpy() * dirx).sum())
  assert abs(fd - an) < 1e-6 * max(1.0, abs(fd)), ("x0", fd, an)

  with torch.no_grad():
    _, tape = roll(x0.detach(), H, dt=DT, with_jacobians=True)
    g_cost = torch.full((H, S), 1.0 / S, dtype=F64, device=device)
    a1, b1 = roll.backward(tape, g_cost, H, dt=DT, want_state_grad=True)
    a2, b2 = roll.backward(tape, g_cost, H, dt=DT, want_state_grad=True)
  assert torch.equal(a1, a2) and torch.equal(b1, b2) and float(a1.abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["native_objective", "native_no_encoder", "native_sampler"])
def test_gpu_closure_options_compose_with_a_matern_drift(option, device):
  """One run each: native vs the torch composition of the same closure, 1e-9 in loss and gradients."""
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _system("P", "matern52", 37)
  S, H = 37, 5
  system, objective, pm = _torch_system(sy, device)
  params = [t for ts in _policy_params(pm, 2).values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)
  kw, paths = dict(FLAGS), _roll_case(sy, device, F64)[0]
  if option == "native_objective":
    tgt = objective.target.clone()
    objective = lambda x, t=None: -torch.exp(-0.5 * ((x - tgt) ** 2).sum(-1)) * (1.0 + 0.1 * float(t))     # a caller's own objective
    kw["native_objective"] = True
  elif option == "native_no_encoder":
    # the same drift read as a system without an encoder: nx 6 states + 2 actions on the nd 8 inputs
    system.encoder = None
    kw["native_no_encoder"] = True
    pol6 = random_svgp_params(seed=44, L=2, M=12, d=6, whiten=True, ls_bounds=(0.8, 2.0), mean=True, separate_Z=True)
    pm = gp_model_from_oracle(pol6, device)
    system.policy = gp.InverseLinkWrapper(gp.KernelRegressor(pm), invlink=system.policy.invlink)
    params = [t for ts in _policy_params(pm, 2).values() for t in ts]
    for t in params:
      t.requires_grad_(True)
    from gpflowpilco_amd.components import GaussianObjective
    objective = GaussianObjective(target=torch.full((6,), 0.3, dtype=F64, device=device), precis=torch.eye(6, dtype=F64, device=device))
    dr6 = random_svgp_params(seed=43, L=6, M=50, d=8, whiten=True, ls_bounds=(0.8, 3.0), mean=True, separate_Z=True)
    dr6.q_mu = 0.1 * dr6.q_mu; dr6.mean_c = 0.05 * dr6.mean_c
    system.drift = _model(dr6, device, "matern52")
    x0 = torch.tensor(np.random.default_rng(8).uniform(0.2, 0.8, size=(S, 6)), dtype=F64, device=device, requires_grad=True)
    paths = system.drift.generate_paths(S, 256, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(3))
  else:
    kw["native_sampler"] = True
    paths = None

  def run(**k):
    for t in params + [x0]:
      t.grad = None
    torch.manual_seed(17)                                           # native_sampler: both runs draw the same paths
    loss = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, num_bases=256, **k)()
    loss.mean().backward()
    return loss.detach(), [t.grad.detach().clone() for t in params + [x0]]
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    ln, gn = run(native=True, **kw)
  lt, gt = run(native=False, native_sampler=(option == "native_sampler"))
  el = float((ln - lt).abs().max()) / max(1e-14, float(lt.abs().max()))
  eg = max(float((a_ - b_).abs().max()) / max(1e-14, float(b_.abs().max())) for a_, b_ in zip(gn, gt))
  print(f"closure {option} matern52: native vs torch composition, loss {el:.2e} gradients {eg:.2e}")
  assert torch.isfinite(ln).all() and el < 1e-9 and eg < 1e-9


@pytest.mark.gpu
def test_gpu_moment_closure_falls_back_once_for_a_matern_drift_and_names_it(device):
  """``policy_loss_closure``: a Matern drift is named in the one fallback warning; the torch composition then meets
  ``moment_matching``'s own refusal (no SquaredExponential numbers for a Matern model)."""
  from gpflowpilco_amd import dynamics
  from gpflowpilco_amd.loops import policy_loss_closure
  system, objective, x0 = _cartpole(device)
  system.solver = dynamics.MomentMatchingEuler()
  init = lambda: (x0, 0.01 * torch.eye(4, dtype=F64, device=device).expand(x0.shape[0], 4, 4).contiguous())
  closure = policy_loss_closure(system, objective, init, 2)
  with torch.no_grad():
    with pytest.warns(RuntimeWarning, match=r"Matern52 drift.*SquaredExponential only"):
      with pytest.raises(NotImplementedError, match="closed forms for SquaredExponential only"):
        closure()
    with warnings.catch_warnings():
      warnings.simplefilter("error")                                                 # said once
      with pytest.raises(NotImplementedError):
        closure()


# ---- GPU: the sampler -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("coreg", [False, True], ids=["separate", "coregionalised"])
@pytest.mark.parametrize("name", ["matern32", "matern52"])
def test_gpu_sampler_draw_is_generate_paths(name, coreg, device):
  from gpflowpilco_amd.pathwise import generate_paths
  L, M, d, K, S = 3, 100, 6, 256, 37
  p = random_svgp_params(seed=80, L=L, M=M, d=d, whiten=True, ls_bounds=(0.8, 3.0), mean=True, W_rows=4 if coreg else None,
                         separate_Z=True)
  model = _model(p, device, name)
  seed = lambda: torch.Generator(device=device).manual_seed(9)
  x = torch.rand(S, d, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(10))
  for dtype in (F64, F32):
    ref = generate_paths(model, S, K, dtype=dtype, device=device, generator=seed())
    sampler = model.path_sampler(S, K, dtype=dtype, device=device)
    got = sampler.draw(seed())
    assert got.kernel == ref.kernel == FAMILIES[name]
    for nm in ("zs", "hz", "omega", "phase", "lengthscales", "prior_scale", "variance"):
      assert torch.equal(getattr(got, nm), getattr(ref, nm)), nm
    nbK = got.omega.shape[-1] // got.wb.shape[-1]
    assert torch.equal(got.wb[:, :, :nbK], ref.wb[:, :, :nbK])
    if dtype == F64:
      f_ref, f_got = ref(x), got(x)
      err = float((f_got - f_ref).abs().max() / f_ref.abs().max())
      print(f"sampler {name} coreg={coreg}: |df| / max|f| = {err:.2e}")
      assert err <= SAMPLER_BAR
      vmax = float(ref.wb[:, :, nbK:].abs().max())
    else:
      ulp = 2.0 ** (math.floor(math.log2(vmax)) - 23)
      assert float((got.wb[:, :, nbK:].double() - ref.wb[:, :, nbK:].double()).abs().max()) <= ulp
  copy_ = sampler.draw(seed(), clone=True)                                      # an independent copy keeps the family
  assert copy_.kernel == FAMILIES[name] and copy_.wb.data_ptr() != sampler.buffers["wb"].data_ptr() and torch.equal(copy_.wb, got.wb)
  # the SE model of the same numbers: another cache key, no chi buffers
  se_sampler = _model(p, device, "se").path_sampler(S, K, dtype=F64, device=device)
  assert se_sampler.draw(seed()).kernel == 0
  assert "chi" in sampler.buffers and "chi" not in se_sampler.buffers and "tscale" not in se_sampler.buffers


@pytest.mark.gpu
def test_gpu_graphed_closure_with_the_native_sampler_draws_new_matern_paths(device):
  from gpflowpilco_amd.loops import GraphedPolicyLoss, pathwise_policy_loss_closure
  sy = _system("P", "matern52", 37)
  system, objective, pm = _torch_system(sy, device)
  params = [t for ts in _policy_params(pm, 2).values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device)
  closure = pathwise_policy_loss_closure(system, objective, lambda: x0, 4, dt=DT, num_bases=256, native=True, native_sampler=True,
                                         **FLAGS)
  graphed = GraphedPolicyLoss(lambda: closure().mean(), params)
  l1, g1 = graphed.loss_and_grad()
  l1, g1 = l1.clone(), [g.clone() for g in g1]
  l2, g2 = graphed.loss_and_grad()
  assert torch.isfinite(l1).all() and torch.isfinite(l2).all() and not torch.equal(l1, l2)
  assert all(torch.isfinite(g).all() for g in g1 + list(g2)) and any(not torch.equal(a, b) for a, b in zip(g1, g2))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["matern32", "matern52"])
def test_gpu_prior_paths_have_the_kernel_as_their_covariance(name, device):
  """S = 4096 paths of a prior-only model (q_mu = 0, q_sqrt = I, whitened, M = 16, K = 1024) at one fixed pair (x, y): the sample
  covariance of f(x), f(y) lies within 6 . 2 var / sqrt S (six standard deviations of a sample covariance of two Gaussians of
  variance <= var: sd <= sqrt(2) var / sqrt S) plus the K = 1024 feature error 6 var / sqrt K of k(x, y)."""
  from gpflowpilco_amd.pathwise import generate_paths
  fam, S, M, K, d = FAMILIES[name], 4096, 16, 1024, 3
  rng = np.random.default_rng(90)
  var = 0.7
  p = mo.SVGPParams(Z=rng.uniform(size=(1, M, d)), lengthscales=np.array([[0.6, 0.9, 1.4]]), variance=np.array([var]),
                    q_mu=np.zeros((M, 1)), q_sqrt=np.eye(M)[None], whiten=True, mean_c=None)
  model = _model(p, device, name)
  paths = generate_paths(model, S, K, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(1))
  x, y = np.array([0.3, 0.5, 0.4]), np.array([0.55, 0.2, 0.7])
  ev = lambda pt: paths(torch.tensor(np.broadcast_to(pt, (S, d)).copy(), dtype=F64, device=device))[:, 0].cpu().numpy()
  fx, fy = ev(x), ev(y)
  cov = np.cov(np.stack([fx, fy]))
  bar = 6.0 * 2.0 * var / math.sqrt(S) + 6.0 * var / math.sqrt(K)
  want = np.array([[var, pmat.kernel(x[None], y[None], p.lengthscales[0], var, fam)[0, 0]]])
  print(f"prior paths {name}: var {cov[0, 0]:.4f} / {cov[1, 1]:.4f} (k = {var}), cov {cov[0, 1]:.4f} (k = {want[0, 1]:.4f}), bar {bar:.3f}")
  assert abs(cov[0, 1] - want[0, 1]) < bar and abs(cov[0, 0] - var) < bar and abs(cov[1, 1] - var) < bar
