#!/usr/bin/env python
"""Timings of the two opt-in native routes of ``loops.policy_loss_closure``, in the style of tools/bench_multiaction.py (device
events around back-to-back calls after warm-up, the variants of one shape in alternating windows, median and min .. max of the
windows, ms per step, f64, eager, H = 30).  Prints one JSON line.

default       system M0 of tests/test_no_encoder.py (nx 2, one action, NO encoder: nd 3, drift M 40, policy M 12) at
              B = 1 / 64 / 256: the native forward and the native loss + gradient (``native_no_encoder=True``) against the torch
              composition of the same closure (``native=False``), same process.
--objective   the cart-pole shape (nx 4, one angle, drift M 100, policy M 30; the one-action row of tools/bench_multiaction.py
              --grad) at the same batch sizes: loss + gradient of a time-weighted quadratic objective through
              ``native_objective=True`` (native trajectory op + the objective in torch), of the same objective through the torch
              composition, and of the built-in GaussianObjective through the native reverse sweep; the difference between the
              first and the last is what the torch-side objective costs per step."""
import argparse
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _here)

import torch  # noqa: E402

from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp  # noqa: E402
from gpflowpilco_amd.components import GaussianObjective  # noqa: E402
from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure  # noqa: E402
from gpflowpilco_amd.synthetic import generate_covariance, make_svgp  # noqa: E402
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, to_dev  # noqa: E402

_spec = importlib.util.spec_from_file_location("bench_multiaction", os.path.join(_here, "tools", "bench_multiaction.py"))
bm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bm)
F64 = torch.float64


class TimeWeightedQuadratic:
  def __init__(self, W, tau):
    self.W, self.tau = W, tau

  def __call__(self, x, t=None):
    e = x.mean() - self.tau
    return (1.0 + 0.1 * t) * ((e * (e @ self.W)).sum(-1) + (self.W * x.covariance(dense=True)).sum((-1, -2)))


def m0_system(B, device, seed=70):
  nx, nd = 2, 3
  drift_o = oracle_params(make_svgp(nx, 40, nd, seed=seed, ls_bounds=(0.8, 3.0)))
  drift_o.Z[..., nx:] = 4.0 * drift_o.Z[..., nx:] - 2.0
  pol_o = random_svgp_params(seed=seed + 1, L=1, M=12, d=nx, whiten=True, ls_bounds=(0.5, 1.2), mean=False, separate_Z=False)
  pol_o.q_mu = 1.5 * pol_o.q_mu
  rng = np.random.default_rng(seed + 2)
  mu0 = rng.uniform(0.2, 0.7, (B, nx)); S0 = generate_covariance(rng, nx, (B,), 0.2)
  A = rng.standard_normal((nx, nx))
  drift, pol = gp_model_from_oracle(drift_o, device), gp_model_from_oracle(pol_o, device)
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=tfb.Chain([tfb.Scale(2.0), tfb.Shift(-0.5), tfb.NormalCDF()]))
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=None, solver=dynamics.MomentMatchingEuler())
  objective = GaussianObjective(target=to_dev(np.linspace(0.3, 0.6, nx), device, F64),
                                precis=to_dev(A @ A.T / nx + 0.5 * np.eye(nx), device, F64))
  kern = pol.kernel.kernels[0]
  params = [pol.q_mu, pol.inducing_variable.inducing_variables[0].Z, kern.lengthscales, kern.variance]
  for t in params:
    t.requires_grad_(True)
  return system, objective, params, drift, get_state_initializer(to_dev(mu0, device, F64), to_dev(S0, device, F64))


def pair(closure, params):
  def forward():
    with torch.no_grad():
      return closure()

  def loss_grad():
    for t in params:
      t.grad = None
    loss = closure()
    loss.sum().backward()
    return loss
  return forward, loss_grad


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=30)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--inner", type=int, default=20)
  ap.add_argument("--batches", default="1,64,256")
  ap.add_argument("--objective", action="store_true")
  ap.add_argument("--label", default="")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_no_encoder.py needs the GPU (no CPU timing is meaningful)")
  device, H = "cuda", args.steps
  res = {"tool": "bench_no_encoder" + (" --objective" if args.objective else ""), "label": args.label, "H": H,
         "unit": "ms per step, f64, eager"}
  for B in [int(b) for b in args.batches.split(",")]:
    out = {}
    if not args.objective:
      system, objective, params, drift, init = m0_system(B, device)
      with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)        # a fall-back would be timed as native: refuse
        native = policy_loss_closure(system, objective, init, H, native=True, native_no_encoder=True)
        fn, gn = pair(native, params)
        loss_n = gn().detach().clone()
      ft, gt = pair(policy_loss_closure(system, objective, init, H, native=False), params)
      out["loss_native_vs_torch"] = float((loss_n - gt().detach()).abs().max())
      fns = {"native_forward": fn, "native_loss_and_grad": gn, "torch_forward": ft, "torch_loss_and_grad": gt}
      inners = {"native_forward": args.inner, "native_loss_and_grad": args.inner, "torch_forward": 1, "torch_loss_and_grad": 1}
    else:
      _, drift, pol, mx, Sxx, target, precis = bm.build(4, (1,), 1, 100, 10, B, device)
      from gpflowpilco_amd.components import TrigonometricEncoder
      head = tfb.Chain([tfb.Scale(bm.SCALE[0]), tfb.Shift(bm.SHIFT[0]), tfb.NormalCDF()])
      system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                        encoder=TrigonometricEncoder(active_dims=(1,)), solver=dynamics.MomentMatchingEuler())
      kern = pol.kernel.kernels[0]
      params = [pol.q_mu, pol.inducing_variable.inducing_variables[0].Z, kern.lengthscales, kern.variance]
      for t in params:
        t.requires_grad_(True)
      init = get_state_initializer(mx, Sxx)
      rng = np.random.default_rng(5)
      A = rng.standard_normal((5, 5))
      custom = TimeWeightedQuadratic(to_dev(A @ A.T / 5 + 0.5 * np.eye(5), device, F64), to_dev(rng.uniform(0.0, 0.5, 5), device, F64))
      gauss = GaussianObjective(target=to_dev(target, device, F64), precis=to_dev(precis, device, F64))
      with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        _, g_custom = pair(policy_loss_closure(system, custom, init, H, native=True, native_objective=True), params)
        _, g_gauss = pair(policy_loss_closure(system, gauss, init, H, native=True), params)
        loss_n = g_custom().detach().clone(); g_gauss()
      _, g_torch = pair(policy_loss_closure(system, custom, init, H, native=False), params)
      out["loss_native_vs_torch"] = float((loss_n - g_torch().detach()).abs().max())
      fns = {"custom_objective_native_loss_and_grad": g_custom, "gaussian_objective_native_loss_and_grad": g_gauss,
             "custom_objective_torch_loss_and_grad": g_torch}
      inners = {"custom_objective_native_loss_and_grad": args.inner, "gaussian_objective_native_loss_and_grad": args.inner,
                "custom_objective_torch_loss_and_grad": 1}
    out.update(bm.alternating(fns, H, inners, args.repeats, 2))
    try:
      drift.packed(F64, True, device).check_status(B)
    except Exception as e:                     # noqa: BLE001 -- recorded beside the numbers
      out["status"] = str(e)
    res[f"B{B}"] = out
    del fns
    torch.cuda.empty_cache()
  print(json.dumps(res))


if __name__ == "__main__":
  main()
