"""numpy restatement of pathwise sample paths with Matern-3/2 / Matern-5/2 latents (TEST INFRASTRUCTURE ONLY).

Everything is evaluated in float64 straight from ``(omega, phase, w, v, Z, lengthscales, variance, mean)``, with the kernels in
DIFFERENCE form (r from x - z, not from the expanded squares the device uses): gpflow's parametrisation,

  r^2 = sum_k ((x_k - z_k) / l_k)^2
  Matern-3/2: k = var (1 + sqrt3 r) exp(-sqrt3 r),              g := -k'(r) / (var r) = 3 exp(-sqrt3 r)
  Matern-5/2: k = var (1 + sqrt5 r + 5 r^2 / 3) exp(-sqrt5 r),  g = 5/3 (1 + sqrt5 r) exp(-sqrt5 r)
  d k / d x_k = -var g (x_k - z_k) / l_k^2

``family``: 0 SquaredExponential (g = k / var), 1 Matern-3/2, 2 Matern-5/2 -- the codes of the C ABI's ``kernel`` argument.  The
path container, the random-Fourier features, the encoder, the cost and the policy head are those of ``oracle.pathwise_oracle``
and ``tests.pathwise_multiaction_oracle`` (the policy is SquaredExponential in every native rollout)."""
import numpy as np
from scipy.linalg import cho_solve, cholesky

from oracle import pathwise_oracle as pw
from tests import pathwise_multiaction_oracle as pmo

NU2 = {1: 3, 2: 5}           # 2 nu: the degrees of freedom of the spectral Student-t


def profile(r, family):
  """(k / var, g) as functions of r >= 0."""
  if family == 0:
    e = np.exp(-0.5 * r * r)
    return e, e
  s = np.sqrt(float(NU2[family])) * r
  if family == 1:
    return (1.0 + s) * np.exp(-s), 3.0 * np.exp(-s)
  return (1.0 + s + s * s / 3.0) * np.exp(-s), (5.0 / 3.0) * (1.0 + s) * np.exp(-s)


def kernel(x, z, ls, var, family):
  """x [n, d], z [m, d] -> k [n, m] (difference form)."""
  diff = (x[:, None, :] - z[None, :, :]) / ls
  return var * profile(np.sqrt((diff * diff).sum(-1)), family)[0]


def kernel_grad(x, z, ls, var, family):
  """-> d k(x_i, z_j) / d x_i [n, m, d]."""
  diff = x[:, None, :] - z[None, :, :]
  r = np.sqrt(((diff / ls) ** 2).sum(-1))
  return -var * profile(r, family)[1][..., None] * diff / (ls * ls)


def spectral_frequencies(rng, ls, K, family):
  """omega [L, K, d]: n / ls (SquaredExponential) or (n / ls) sqrt(2 nu / chi2_{2 nu}), one chi2 per (latent, basis function)."""
  L, d = ls.shape
  omega = rng.standard_normal((L, K, d)) / ls[:, None, :]
  if family:
    chi2 = (rng.standard_normal((L, K, NU2[family])) ** 2).sum(-1)
    omega = omega * np.sqrt(NU2[family] / chi2)[:, :, None]
  return omega


def draw_paths(rng, model, num_samples, num_bases, family) -> pw.Paths:
  """``pw.draw_paths`` with the family's frequencies and Gram matrix."""
  L, M, d = model.Z.shape
  S, K = num_samples, num_bases
  omega = spectral_frequencies(rng, model.lengthscales, K, family)
  phase = rng.uniform(0.0, 2.0 * np.pi, size=(L, K))
  w = rng.standard_normal((S, L, K))
  v = np.empty((S, L, M))
  for a in range(L):
    Kuu = kernel(model.Z[a], model.Z[a], model.lengthscales[a], model.variance[a], family) + model.kuu_jitter * np.eye(M)
    Lu = cholesky(Kuu, lower=True)
    eps = rng.standard_normal((S, M))
    u = model.q_mu[:, a][None, :] + eps @ np.tril(model.q_sqrt[a]).T
    if model.whiten:
      u = u @ Lu.T
    resid = u - w[:, a, :] @ pw.features(omega[a], phase[a], model.variance[a], model.Z[a]).T
    v[:, a, :] = cho_solve((Lu, True), resid.T).T
  return pw.Paths(omega=omega, phase=phase, w=w, v=v)


def eval_latents(paths, model, x, family):
  """g_s(x_s): x [S, d] -> [S, L], without any mean."""
  S, L, K = paths.w.shape
  out = np.empty((S, L))
  for a in range(L):
    phi = pw.features(paths.omega[a], paths.phase[a], model.variance[a], x)
    diff = (x[:, None, :] - model.Z[a][None]) / model.lengthscales[a]
    kxz = model.variance[a] * profile(np.sqrt((diff * diff).sum(-1)), family)[0]
    out[:, a] = np.sum(paths.w[:, a, :] * phi, -1) + np.sum(paths.v[:, a, :] * kxz, -1)
  return out


def eval_paths(paths, model, x, family):
  """f_s(x_s) [S, L] (a coregionalised model, ``model.W`` [nx, L]: W g + c [S, nx])."""
  g = eval_latents(paths, model, x, family)
  if model.W is not None:
    g = g @ np.asarray(model.W).T
  return g if model.mean_c is None else g + np.asarray(model.mean_c)[None]


def eval_jac(paths, model, x, family):
  """d f_s / d x_s [S, L, d] (coregionalised: [S, nx, d])."""
  S, L, K = paths.w.shape
  d = x.shape[-1]
  J = np.empty((S, L, d))
  for a in range(L):
    arg = x @ paths.omega[a].T + paths.phase[a][None, :]
    t = -np.sqrt(2.0 * model.variance[a] / K) * paths.w[:, a, :] * np.sin(arg)                 # [S, K]
    diff = x[:, None, :] - model.Z[a][None]                                                   # [S, M, d]
    r = np.sqrt(((diff / model.lengthscales[a]) ** 2).sum(-1))
    dk = -model.variance[a] * profile(r, family)[1][..., None] * diff / model.lengthscales[a] ** 2
    J[:, a, :] = t @ paths.omega[a] + np.einsum('sm,smk->sk', paths.v[:, a, :], dk)
  return J if model.W is None else np.einsum('il,sld->sid', np.asarray(model.W), J)


def policy_rollout(paths, drift, family, policy, scales, shifts, active_dims, target, precis, x0, num_steps, dt=1.0):
  """The fold of ``pmo.policy_rollout_costs_nd`` with this module's drift: -> (cost [H, S], states [H + 1, S, nx])."""
  scales, shifts = np.atleast_1d(np.asarray(scales, dtype=np.float64)), np.atleast_1d(np.asarray(shifts, dtype=np.float64))
  x = np.array(x0, dtype=np.float64, copy=True)
  costs, states = [], [x.copy()]
  for _ in range(num_steps):
    e = pw.encode(x, active_dims)
    u = pmo.actions(policy, scales, shifts, e)
    x = x + dt * eval_paths(paths, drift, np.concatenate([e, u], axis=-1), family)
    costs.append(pw.tensor_cost(pw.encode(x, active_dims), target, precis))
    states.append(x.copy())
  return np.stack(costs), np.stack(states)
