"""A pathwise (sample-path) policy update on a mountain-car-shaped system -- two state dims, one action, NO encoder -- with a cost
of the caller's own on the native rollout (needs the built library and a GPU).

  python examples/mountain_car_pathwise.py [--steps 30] [--samples 512] [--updates 5]

On sample paths an objective is just a function of a tensor of states (loops/pilco.py:272-275 calls ``objective(x=encoder(state),
t=t)`` per step).  With ``native_objective=True`` the rollout stays in the native kernels and returns its states as a differentiable
output (``pathwise.PolicyTrajectoryFunction``); the objective -- here a time-weighted quadratic cost with a trainable weight matrix --
is accumulated over them in torch, and the seeded reverse sweep carries its gradient back to the policy.  ``native_no_encoder=True``
takes the system without an encoder; ``native_sampler=True`` draws new paths on every call from a cached sampler.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp                      # noqa: E402
from gpflowpilco_amd.loops import pathwise_policy_loss_closure                          # noqa: E402
from gpflowpilco_amd.pathwise import PathwiseSVGP                                       # noqa: E402
from gpflowpilco_amd.synthetic import make_policy, make_svgp                            # noqa: E402

F64 = torch.float64


class TimeWeightedQuadratic:
  """(1 + 0.1 t) (x - tau)^T W (x - tau) of a tensor of states [..., nx]."""

  def __init__(self, W, tau):
    self.W, self.tau = W, tau

  def __call__(self, x, t=None):
    e = x - self.tau
    return (1.0 + 0.1 * t) * (e * (e @ self.W)).sum(-1)


def build(dev, seed=7):
  """(system, trainable policy parameters): position and velocity, one force in [-1, 1], drift M = 40, policy M = 12."""
  drift_s = make_svgp(2, 40, 3, seed=seed, device=str(dev), ls_bounds=(0.8, 3.0))
  drift_s.Z = drift_s.Z * np.array([1, 1, 2.0]) - np.array([0, 0, 1.0])       # the action axis covers u = 2 (Phi(f) - 1/2)
  base, pol = drift_s.to_model(dev), make_policy(12, 2, seed + 1).to_model(dev)
  drift = PathwiseSVGP(kernel=base.kernel, inducing_variable=base.inducing_variable, q_mu=base.q_mu, q_sqrt=base.q_sqrt, whiten=True,
                       num_latent_gps=2)
  kern = pol.latent_kernels[0]
  params = [pol.q_mu, kern.lengthscales, kern.variance]
  for p in params:
    p.requires_grad_(True)
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=tfb.Chain([tfb.Scale(2.0), tfb.Shift(-0.5), tfb.NormalCDF()]))
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=None, solver=dynamics.Euler())
  return system, params


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=30)
  ap.add_argument("--samples", type=int, default=512)
  ap.add_argument("--updates", type=int, default=5)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("this example needs a GPU (the package has no CPU fallback)")
  dev = torch.device("cuda", 0)
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=dev)
  system, params = build(dev)
  gen = torch.Generator(device=dev).manual_seed(1)
  x0 = t([0.4, 0.3]) + 0.1 * torch.randn(args.samples, 2, dtype=F64, device=dev, generator=gen)
  W = t(np.diag([2.0, 0.5])).requires_grad_(True)
  closure = pathwise_policy_loss_closure(system, TimeWeightedQuadratic(W, t([0.6, 0.0])), lambda: x0, args.steps, dt=0.1,
                                         num_bases=256, native=True, native_no_encoder=True, native_objective=True,
                                         native_sampler=True)
  opt = torch.optim.Adam(params, lr=0.02)
  for it in range(args.updates):
    opt.zero_grad()
    W.grad = None
    loss = closure().mean()                                  # new sample paths on every call
    loss.backward()
    print(f"update {it}: mean sample loss {float(loss.detach()):+.6f}, |d / d q_mu| {float(params[0].grad.norm()):.3e}, "
          f"|d / d W| {float(W.grad.norm()):.3e}")
    opt.step()


if __name__ == "__main__":
  main()
