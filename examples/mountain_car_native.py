"""A mountain-car-shaped system -- two state dims, one action, NO encoder (dynamics/forward_sde.py:49-68) -- on the native
moment-matched rollout (needs the built library and a GPU).

  python examples/mountain_car_native.py [--steps 30]

Three things the default routing sends to the torch composition run natively when asked for:
  native_no_encoder=True   the rollout entries with na = 0: loss (mm_rollout_composed) and gradient (taped rollout + reverse sweep);
  native_objective=True    any objective of the state: here a time-weighted quadratic cost with a trainable weight matrix, evaluated
                           in torch on the trajectory the native rollout returns (autodiff.ComposedTrajectoryFunction; the seeded
                           reverse sweep carries its gradient back to the policy).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp                      # noqa: E402
from gpflowpilco_amd.components import GaussianObjective                                # noqa: E402
from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure            # noqa: E402
from gpflowpilco_amd.synthetic import make_policy, make_svgp                                   # noqa: E402

F64 = torch.float64


class TimeWeightedQuadratic:
  """(1 + 0.1 t) [(m - tau)^T W (m - tau) + tr(W S)]: the expectation of a quadratic cost under x ~ N(m, S)."""

  def __init__(self, W, tau):
    self.W, self.tau = W, tau

  def __call__(self, x, t=None):
    e = x.mean() - self.tau
    return (1.0 + 0.1 * t) * ((e * (e @ self.W)).sum(-1) + (self.W * x.covariance(dense=True)).sum((-1, -2)))


def build(dev, seed=7):
  """(system, trainable policy parameters): position and velocity, one force in [-1, 1], drift M = 40, policy M = 12."""
  drift_s = make_svgp(2, 40, 3, seed=seed, device=str(dev), ls_bounds=(0.8, 3.0))
  drift_s.Z = drift_s.Z * np.array([1, 1, 2.0]) - np.array([0, 0, 1.0])       # the action axis covers u = 2 (Phi(f) - 1/2)
  drift, pol = drift_s.to_model(dev), make_policy(12, 2, seed + 1).to_model(dev)
  kern = pol.latent_kernels[0]
  params = [pol.q_mu, kern.lengthscales, kern.variance]
  for p in params:
    p.requires_grad_(True)
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=tfb.Chain([tfb.Scale(2.0), tfb.Shift(-0.5), tfb.NormalCDF()]))
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=None, solver=dynamics.MomentMatchingEuler())
  return system, params


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=30)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("this example needs a GPU (the package has no CPU fallback)")
  dev = torch.device("cuda", 0)
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=dev)
  system, params = build(dev)
  init = get_state_initializer(t([[0.4, 0.3]]), t(0.02 * np.eye(2))[None])
  # 1. the reference's saturating cost of the raw state: target [nx]
  goal = GaussianObjective(target=t([0.6, 0.0]), precis=t(np.diag([4.0, 1.0])))
  closure = policy_loss_closure(system, goal, init, args.steps, native=True, native_no_encoder=True)
  with torch.no_grad():
    print(f"native loss, no encoder:            {float(closure().sum()):+.6f}")
  loss = closure().sum()
  loss.backward()
  print(f"native gradient, |d loss / d q_mu|: {float(params[0].grad.norm()):.3e}")
  # 2. an objective of the caller's own, with a parameter that is trained with the policy
  W = t(np.diag([2.0, 0.5])).requires_grad_(True)
  custom = policy_loss_closure(system, TimeWeightedQuadratic(W, t([0.6, 0.0])), init, args.steps, native=True,
                               native_no_encoder=True, native_objective=True)
  for p in params:
    p.grad = None
  loss = custom().sum()
  loss.backward()
  print(f"custom objective on the native rollout: {float(loss):+.6f}, |d / d q_mu| {float(params[0].grad.norm()):.3e}, "
        f"|d / d W| {float(W.grad.norm()):.3e}")


if __name__ == "__main__":
  main()
