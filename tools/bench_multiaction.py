#!/usr/bin/env python
"""Forward time per step of the multi-action native rollout (mm_rollout_composed_nd) next to the one-action one.

  system A (tests/test_multiaction.py: nx = 4, two angles, two actions, drift M = 100, policy M = 30), f64, eager, B = 1, 64, 256
  the one-action rollout at cartpole sizes (nx = 4, one angle, drift M = 100, policy M = 30), same process, B = 1, 64, 256
  the torch composition of system A at B = 1 (policy_loss_closure(native=False), no_grad)

Device events around `inner` back-to-back rollouts of H steps, after warm-up; `repeats` windows; the median and the
min .. max spread of the windows are reported, in ms per step.  ``--one-action-only`` times only the one-action rollout: run
from the root of ANOTHER checkout (the package is imported from the current directory when it holds one) it gives that
checkout's numbers for the unchanged path.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_root = os.getcwd() if os.path.isdir(os.path.join(os.getcwd(), "gpflowpilco_amd")) else _here
sys.path.insert(0, _root)

import torch  # noqa: E402

from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp, ops  # noqa: E402
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder  # noqa: E402
from gpflowpilco_amd.synthetic import generate_covariance, make_svgp  # noqa: E402
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, to_dev  # noqa: E402

F64 = torch.float64
SCALE, SHIFT = (2.0, 1.5, 1.0), (-0.5, -0.4, -0.6)


def build(nx, active, nu, Md, seed, B, device):
  na = len(active); ne = nx + na; nd = ne + nu
  drift_o = oracle_params(make_svgp(nx, Md, nd, seed=seed, ls_bounds=(0.8, 3.0)))
  drift_o.Z[..., ne:] = 4.0 * drift_o.Z[..., ne:] - 2.0
  pol_o = random_svgp_params(seed=seed + 1, L=nu, M=30, d=ne, whiten=True, ls_bounds=(0.3, 0.8), mean=False, separate_Z=False)
  pol_o.q_mu = 2.0 * pol_o.q_mu
  rng = np.random.default_rng(seed + 2)
  mu0 = rng.uniform(0.0, 0.6, (B, nx)); S0 = generate_covariance(rng, nx, (B,), 0.3)
  A = rng.standard_normal((ne, ne)); precis = A @ A.T / ne
  target = np.zeros(ne); target[na:2 * na] = 1.0
  drift = gp_model_from_oracle(drift_o, device); pol = gp_model_from_oracle(pol_o, device)
  scale = SCALE[0] if nu == 1 else SCALE[:nu]
  shift = SHIFT[0] if nu == 1 else SHIFT[:nu]
  roll = ops.ComposedRollout(drift.packed(F64, True, device), pol.packed(F64, False, device), nx=nx, active_dims=active,
                             head_scale=scale, head_shift=shift, target=to_dev(target, device, F64),
                             precis=to_dev(precis, device, F64))
  return roll, drift, pol, to_dev(mu0, device, F64), to_dev(S0, device, F64), target, precis


def windows(fn, H, inner, repeats, warmup):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  out = []
  for _ in range(repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
      fn()
    e1.record()
    e1.synchronize()
    out.append(e0.elapsed_time(e1) / (inner * H))
  return {"median": float(np.median(out)), "min": float(min(out)), "max": float(max(out)), "windows": len(out),
          "rollouts_per_window": inner}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=30)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--inner", type=int, default=40)
  ap.add_argument("--one-action-only", action="store_true")
  ap.add_argument("--label", default="")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_multiaction.py needs the GPU (no CPU timing is meaningful)")
  device = "cuda"
  H = args.steps
  res = {"tool": "bench_multiaction", "label": args.label, "H": H, "unit": "ms per step, f64, eager",
         "one_action": {}, "system_A": {}}
  for B in (1, 64, 256):
    roll, *_, mx, Sxx, _, _ = build(4, (1,), 1, 100, 10, B, device)
    res["one_action"][f"B{B}"] = windows(lambda: roll(mx, Sxx, H), H, args.inner, args.repeats, 5)
  if not args.one_action_only:
    for B in (1, 64, 256):
      roll, drift, pol, mx, Sxx, target, precis = build(4, (0, 1), 2, 100, 20, B, device)
      res["system_A"][f"B{B}"] = windows(lambda: roll(mx, Sxx, H), H, args.inner, args.repeats, 5)
      try:                                     # a state that left the PD cone would make the timed work unrepresentative
        roll.drift.check_status(B)
      except Exception as e:                   # noqa: BLE001 -- recorded beside the number, not fatal for the others
        res["system_A"][f"B{B}"]["status"] = str(e)
      if B == 1:
        from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
        head = tfb.Chain([tfb.Scale(to_dev(SCALE[:2], device, F64)), tfb.Shift(to_dev(SHIFT[:2], device, F64)), tfb.NormalCDF()])
        system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                          encoder=TrigonometricEncoder(active_dims=(0, 1)), solver=dynamics.MomentMatchingEuler())
        objective = GaussianObjective(target=to_dev(target, device, F64), precis=to_dev(precis, device, F64))
        closure = policy_loss_closure(system, objective, get_state_initializer(mx, Sxx), H, native=False)

        def torch_path():
          with torch.no_grad():
            closure()
        res["system_A"]["B1_torch_composition"] = windows(torch_path, H, 3, max(3, args.repeats // 2), 2)
  print(json.dumps(res))


if __name__ == "__main__":
  main()
