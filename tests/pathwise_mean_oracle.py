"""numpy restatement of a MEAN-ONLY pathwise drift and its policy rollout (TEST INFRASTRUCTURE ONLY).

What the reference's ``build_dynamics(..., model_uncertainty=False)`` gives under the Euler solver: the drift wrapped in a
``KernelRegressor`` (models/core.py:60-62), so every sample steps with the posterior mean of each latent at (e, u),

  f_a(x) = sum_m beta_am k_a(x, z_am) + c_a,     beta_a = (Kuu_a + jitter I)^-1 u_a      (u = Luu q_mu when whitened)

A fold of existing functions: ``oracle.pathwise_oracle``'s ``encode`` / ``policy_mean`` / ``tensor_cost``,
``tests.pathwise_multiaction_oracle``'s ``actions`` / ``latent_slice`` and ``tests.pathwise_matern_oracle``'s ``kernel`` /
``kernel_grad`` (difference form, every family).  ``family``: 0 SquaredExponential, 1 Matern-3/2, 2 Matern-5/2."""
import numpy as np
from scipy.linalg import cho_solve, cholesky

from oracle.pathwise_oracle import encode, policy_mean, tensor_cost  # noqa: F401  (policy_mean: through ``actions``)
from tests.pathwise_matern_oracle import kernel, kernel_grad
from tests.pathwise_multiaction_oracle import actions, latent_slice


def mean_weights(model, family):
  """beta [L, M] = Kuu^-1 u per latent."""
  L, M, _ = model.Z.shape
  beta = np.empty((L, M))
  for a in range(L):
    p = latent_slice(model, a)
    Lu = cholesky(kernel(p.Z[0], p.Z[0], p.lengthscales[0], p.variance[0], family) + model.kuu_jitter * np.eye(M), lower=True)
    u = p.q_mu[:, 0]
    beta[a] = cho_solve((Lu, True), Lu @ u if model.whiten else u)
  return beta


def latent_values(model, family, x, beta):
  """-> (g [S, L], var sum_m |beta_m k_m / var| [S, L]) of the latents, without any mean: the value and the sum of its absolute
  terms (what the project's rounding bound ``BOUND_ULPS u sum |terms|`` is stated against)."""
  S, L = x.shape[0], model.Z.shape[0]
  g, ab = np.empty((S, L)), np.empty((S, L))
  for a in range(L):
    k = kernel(x, model.Z[a], model.lengthscales[a], model.variance[a], family)                 # [S, M]
    g[:, a], ab[:, a] = k @ beta[a], np.abs(k * beta[a][None]).sum(-1)
  return g, ab


def mean_values(model, family, x, beta=None):
  """The drift's mean f [S, L] (a coregionalised model, ``model.W`` [nx, L]: W g + c [S, nx])."""
  g = latent_values(model, family, x, mean_weights(model, family) if beta is None else beta)[0]
  if model.W is not None:
    g = g @ np.asarray(model.W).T
  return g if model.mean_c is None else g + np.asarray(model.mean_c)[None]


def mean_jac(model, family, x, beta=None):
  """d f / d x [S, L, d] (coregionalised: [S, nx, d])."""
  beta = mean_weights(model, family) if beta is None else beta
  J = np.stack([np.einsum('m,smk->sk', beta[a], kernel_grad(x, model.Z[a], model.lengthscales[a], model.variance[a], family))
                for a in range(model.Z.shape[0])], axis=1)
  return J if model.W is None else np.einsum('il,sld->sid', np.asarray(model.W), J)


def policy_rollout(drift, family, policy, scales, shifts, active_dims, target, precis, x0, num_steps, dt=1.0, beta=None):
  """loops/pilco.py:263-298 with the mean as the drift of every sample: -> (cost [H, S], states [H + 1, S, nx])."""
  scales, shifts = np.atleast_1d(np.asarray(scales, dtype=np.float64)), np.atleast_1d(np.asarray(shifts, dtype=np.float64))
  beta = mean_weights(drift, family) if beta is None else beta
  x = np.array(x0, dtype=np.float64, copy=True)
  costs, states = [], [x.copy()]
  for _ in range(num_steps):
    e = encode(x, active_dims)
    u = actions(policy, scales, shifts, e)
    x = x + dt * mean_values(drift, family, np.concatenate([e, u], axis=-1), beta)
    costs.append(tensor_cost(encode(x, active_dims), target, precis))
    states.append(x.copy())
  return np.stack(costs), np.stack(states)
