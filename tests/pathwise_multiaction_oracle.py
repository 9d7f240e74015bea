"""numpy restatement of the pathwise policy rollout for policies with SEVERAL actions (TEST INFRASTRUCTURE ONLY).

A fold of ``oracle.pathwise_oracle``'s own functions -- ``encode``, ``policy_mean`` (called on each latent's slice of the
``SVGPParams``), ``eval_paths``, ``tensor_cost`` -- with the head applied per action and the actions appended to the encoding
in latent order: u = stack_a scale_a (Phi(f_a(e)) + shift_a), d = (e, u), what the tensor branch of ``forward_sde``
(dynamics/forward_sde.py:23-31) builds from a policy with nu outputs.  With nu = 1 it is ``pw.policy_rollout_costs``.

Two knobs exist only for the tests' guards (a wrong wiring must be far outside the f32 tolerance): ``feed_order`` permutes the
actions before they reach the drift, ``latent_of`` picks the latent whose parameters each action is evaluated from."""
import copy

import numpy as np
from scipy.special import ndtr

from oracle import pathwise_oracle as pw


def latent_slice(policy, a):
  """The one-latent SVGPParams of latent a."""
  p = copy.copy(policy)
  p.Z, p.lengthscales, p.variance = policy.Z[a:a + 1], policy.lengthscales[a:a + 1], policy.variance[a:a + 1]
  p.q_mu, p.q_sqrt = policy.q_mu[:, a:a + 1], policy.q_sqrt[a:a + 1]
  p.mean_c = None if policy.mean_c is None else np.asarray(policy.mean_c).reshape(-1)[a:a + 1]
  return p


def actions(policy, scales, shifts, e, latent_of=None):
  """e [S, ne] -> u [S, nu]."""
  nu = policy.Z.shape[0]
  lat = range(nu) if latent_of is None else latent_of
  return np.stack([scales[a] * (ndtr(pw.policy_mean(latent_slice(policy, lat[a]), e)) + shifts[a]) for a in range(nu)], axis=-1)


def policy_rollout_costs_nd(paths, drift, policy, scales, shifts, active_dims, target, precis, x0, num_steps, dt=1.0,
                            keep=False, feed_order=None, latent_of=None):
  """-> cost [H, S] (keep: also the states [H + 1, S, nx])."""
  scales, shifts = np.atleast_1d(np.asarray(scales, dtype=np.float64)), np.atleast_1d(np.asarray(shifts, dtype=np.float64))
  x = np.array(x0, dtype=np.float64, copy=True)
  costs, states = [], [x.copy()]
  for _ in range(num_steps):
    e = pw.encode(x, active_dims)
    u = actions(policy, scales, shifts, e, latent_of)
    if feed_order is not None:
      u = u[:, list(feed_order)]
    x = x + dt * pw.eval_paths(paths, drift, np.concatenate([e, u], axis=-1))
    costs.append(pw.tensor_cost(pw.encode(x, active_dims), target, precis))
    states.append(x.copy())
  return (np.stack(costs), np.stack(states)) if keep else np.stack(costs)
