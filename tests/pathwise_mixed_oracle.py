"""numpy restatement of the pathwise policy rollout on a COREGIONALISED drift (TEST INFRASTRUCTURE ONLY).

A fold of ``oracle.pathwise_oracle`` (``encode``, ``eval_paths``, ``tensor_cost``) and ``tests/pathwise_multiaction_oracle.py``
(``actions``: the head per action, appended to the encoding in latent order) with the drift sample

    f = eval_paths(latent paths)(d) @ W.T + c,        W [nx, Lg], c [nx] or None

-- Lg latent paths without a mean of their own, mixed to nx outputs, the constant added after the mixing: what gpflow's
``LinearCoregionalization`` posterior does to the latent samples (``SVGP.initialize`` builds such a model whenever
``num_latent_gps`` differs from the number of outputs).

``wiring`` exists only for the tests' guards (a wrong wiring must be far outside the f32 tolerance):
  "no_c"     the constant is dropped;
  "stride"   W's buffer is read with the other stride (as if it were stored [Lg, nx]);
  "rotated"  the latents reach W in rotated order (latent l + 1 in place of latent l)."""
import numpy as np

from oracle import pathwise_oracle as pw
from tests import pathwise_multiaction_oracle as pmo


def mixed_eval(paths, drift, W, c, d, wiring=None):
  """d [S, nd] -> f [S, nx] = g W^T + c, g = the Lg latent paths' values (``drift``: the latent SVGPParams, no mean)."""
  assert drift.mean_c is None
  W = np.asarray(W, dtype=np.float64)
  g = pw.eval_paths(paths, drift, d)                                     # [S, Lg]
  if wiring == "rotated":
    g = np.roll(g, -1, axis=1)
  if wiring == "stride":
    W = W.reshape(-1).reshape(W.shape[1], W.shape[0]).T
  f = g @ W.T
  return f if (c is None or wiring == "no_c") else f + np.asarray(c, dtype=np.float64)[None]


def policy_rollout_costs_mixed(paths, drift, W, c, policy, scales, shifts, active_dims, target, precis, x0, num_steps, dt=1.0,
                               keep=False, wiring=None):
  """-> cost [H, S] (keep: also the states [H + 1, S, nx])."""
  scales, shifts = np.atleast_1d(np.asarray(scales, dtype=np.float64)), np.atleast_1d(np.asarray(shifts, dtype=np.float64))
  x = np.array(x0, dtype=np.float64, copy=True)
  costs, states = [], [x.copy()]
  for _ in range(num_steps):
    e = pw.encode(x, active_dims)
    u = pmo.actions(policy, scales, shifts, e)
    x = x + dt * mixed_eval(paths, drift, W, c, np.concatenate([e, u], axis=-1), wiring)
    costs.append(pw.tensor_cost(pw.encode(x, active_dims), target, precis))
    states.append(x.copy())
  return (np.stack(costs), np.stack(states)) if keep else np.stack(costs)
