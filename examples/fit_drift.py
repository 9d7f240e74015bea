"""The PILCO loop closed with nothing synthetic: simulate, fit the drift from the transitions, improve the policy on the fitted drift
(needs the built library and a GPU).

  python examples/fit_drift.py [--episodes 6] [--fit-iters 40] [--policy-steps 10]

1. A small two-state system (position, velocity; one force in [-1, 1]) is simulated in numpy under random forces and its
   transitions (x_t, u_t) -> x_{t+1} - x_t are collected.
2. ``SVGP.initialize`` builds the drift model from the data (median-heuristic lengthscales, k-means inducing points) and
   ``training.fit_svgp`` fits it: L-BFGS on the negative ELBO plus the signal-to-noise prior, the Gram matrices and their adjoints
   from the HIP kernel.  The fitted values are written into the model's own tensors, so the pack cache repacks them.
3. A few Adam steps of ``policy_loss_closure(..., native_no_encoder=True)``: the moment-matched rollout and its reverse sweep
   run natively on the drift that step 2 produced.
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
from gpflowpilco_amd.synthetic import make_policy                                       # noqa: E402
from gpflowpilco_amd.training import fit_svgp                                           # noqa: E402

F64 = torch.float64


def step(x, u):
  """One unit time step of a damped cart in a rippled potential."""
  p, v = x
  v = v + 0.1 * (u - 0.5 * np.sin(3.0 * p)) - 0.02 * v
  return np.array([p + 0.1 * v, v])


def collect(episodes, length, rng):
  X, Y = [], []
  for _ in range(episodes):
    x = np.array([rng.uniform(0.2, 0.6), rng.uniform(-0.2, 0.2)])
    for _ in range(length):
      u = rng.uniform(-1.0, 1.0)
      x1 = step(x, u)
      X.append(np.append(x, u)); Y.append(x1 - x + 1e-3 * rng.standard_normal(2))
      x = x1
  return np.array(X), np.array(Y)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--episodes", type=int, default=6)
  ap.add_argument("--length", type=int, default=40)
  ap.add_argument("--inducing", type=int, default=40)
  ap.add_argument("--fit-iters", type=int, default=40)
  ap.add_argument("--collapsed", action="store_true",
                  help="fit the hyper-parameters on the collapsed (SGPR) bound and set q(u) to its closed-form optimum")
  ap.add_argument("--policy-steps", type=int, default=10)
  ap.add_argument("--horizon", type=int, default=15)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("this example needs a GPU (the package has no CPU fallback)")
  dev = torch.device("cuda", 0)
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=dev)
  # 1. data
  X, Y = collect(args.episodes, args.length, np.random.default_rng(0))
  held_X, held_Y = collect(2, args.length, np.random.default_rng(1))
  # 2. the drift, from the data
  drift = gp.SVGP.initialize((torch.tensor(X), torch.tensor(Y)), args.inducing, seed=0, prior=gp.PilcoPenaltySNR(1000.0, 30.0),
                             likelihood=gp.GaussianLikelihood(1e-2))
  rmse = lambda: float(((drift.predict_mean(t(held_X)) - t(held_Y)) ** 2).mean().sqrt())

  def log_density():                                      # held-out mean log density of the transitions under predict_y
    with torch.no_grad():
      return float(drift.predict_log_density((t(held_X), t(held_Y))).mean())
  before, before_ld = rmse(), log_density()
  history = fit_svgp(drift, (t(X), t(Y)), max_iter=args.fit_iters, collapsed=args.collapsed)
  print(f"drift fit: {len(X)} transitions, {len(history) - 1} L-BFGS iterations, loss {history[0]:+.2f} -> {history[-1]:+.2f}, "
        f"held-out RMSE {before:.2e} -> {rmse():.2e}, held-out mean log density {before_ld:+.3f} -> {log_density():+.3f}")
  # 3. the policy, on the fitted drift
  pol = make_policy(12, 2, 8).to_model(dev)
  kern = pol.latent_kernels[0]
  params = [pol.q_mu, kern.lengthscales, kern.variance]
  for p in params:
    p.requires_grad_(True)
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=tfb.Chain([tfb.Scale(2.0), tfb.Shift(-0.5), tfb.NormalCDF()]))
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=None, solver=dynamics.MomentMatchingEuler())
  goal = GaussianObjective(target=t([0.8, 0.0]), precis=t(np.diag([4.0, 1.0])))
  init = get_state_initializer(t([[0.4, 0.0]]), t(1e-3 * np.eye(2))[None])
  closure = policy_loss_closure(system, goal, init, args.horizon, native=True, native_no_encoder=True)
  opt = torch.optim.Adam(params, lr=0.05)
  for it in range(args.policy_steps):
    opt.zero_grad()
    loss = closure().sum()
    loss.backward()
    opt.step()
    print(f"policy step {it:2d}: expected cost over {args.horizon} steps {float(loss.detach()):.6f}")


if __name__ == "__main__":
  main()
