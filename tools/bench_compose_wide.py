#!/usr/bin/env python
"""Loss + gradient per step of the moment-matched policy rollout at 8 < ne <= 16 encoded dims: the native wide path
(``policy_loss_closure(native_wide=True)``: the ``_nd`` family's tape and ``mm_compose_wide_backward*``) against the torch
composition on the same system -- what these systems got before -- in one process.

  system ne11   nx 8, three angles (ne 11 / nd 12), one action, drift M 100, policy M 30
  system ne16   nx 12, four angles (ne 16 / nd 18), two actions, drift M 100, policy M 30
f64, H = 30, at B = 1, 64 and 256, every policy parameter trainable; ms per step of
  native loss + gradient, eager and replayed from a ``GraphedPolicyLoss``;
  the torch composition's loss + gradient (``native=False``), eager;
  the wide reverse sweep alone over one tape (``ComposedRollout.backward_wide`` replayed from a captured graph), on the one-wave
    dense paths of csrc/mm_adjoint.h and -- ``mm_compose_wide_dense_path(1)`` -- on the generic code.
Device events around ``inner`` back-to-back calls; the variants of one (system, B) take turns window by window.  The criterion: at
every B the slowest native window is below the fastest torch-composition window (``criterion`` in the output; the exit status is 1
where it fails).  ``dense_paths_kept``: the slowest sweep window on the one-wave paths is below the fastest on the generic code.
Writes profiles/compose_wide_bench.json and prints it as one JSON line.  ``--native-only`` leaves the torch composition out."""
import argparse
import json
import os
import sys
import warnings

import numpy as np

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_root = os.getcwd() if os.path.isdir(os.path.join(os.getcwd(), "gpflowpilco_amd")) else _here
sys.path.insert(0, _root)

import torch  # noqa: E402

from gpflowpilco_amd import _lib, bijectors as tfb, dynamics, models as gp, ops  # noqa: E402
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder  # noqa: E402
from gpflowpilco_amd.synthetic import generate_covariance, make_svgp  # noqa: E402
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, to_dev  # noqa: E402
from tools.bench_multiaction import alternating  # noqa: E402

F64 = torch.float64
SCALE, SHIFT = (2.0, 1.5), (-0.5, -0.4)
SYSTEMS = {"ne11": dict(nx=8, active=(0, 2, 5), nu=1, seed=400), "ne16": dict(nx=12, active=(0, 3, 5, 8), nu=2, seed=410)}


def build(nx, active, nu, seed, B, device, Md=100, Mp=30):
  """The recipe of tests/test_gpu_compose_wide.py (lengthscales that grow with the width) at the bench's sizes."""
  na = len(active); ne = nx + na; nd = ne + nu
  lo = 0.5 * max(1.0, np.sqrt(nd / 4.0))
  drift_o = oracle_params(make_svgp(nx, Md, nd, seed=seed, ls_bounds=(lo, 3.0 * lo)))
  drift_o.Z[..., ne:] = 4.0 * drift_o.Z[..., ne:] - 2.0
  lp = 0.5 * max(1.0, np.sqrt(ne / 4.0))
  pol_o = random_svgp_params(seed=seed + 1, L=nu, M=Mp, d=ne, whiten=True, ls_bounds=(lp, 2.4 * lp), mean=False, separate_Z=False)
  pol_o.q_mu = 1.5 * pol_o.q_mu
  rng = np.random.default_rng(seed + 2)
  mu0 = rng.uniform(0.2, 0.7, (B, nx)); S0 = generate_covariance(rng, nx, (B,), 0.15)
  A = rng.standard_normal((ne, ne))
  precis = A @ A.T / ne ** 2 + 0.5 * np.eye(ne) / ne
  target = np.linspace(0.3, 0.6, ne)
  drift, pol = gp_model_from_oracle(drift_o, device), gp_model_from_oracle(pol_o, device)
  if nu == 1:
    head = [tfb.Scale(SCALE[0]), tfb.Shift(SHIFT[0]), tfb.NormalCDF()]
  else:
    head = [tfb.Scale(to_dev(SCALE[:nu], device, F64)), tfb.Shift(to_dev(SHIFT[:nu], device, F64)), tfb.NormalCDF()]
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=tfb.Chain(head)),
                                    encoder=TrigonometricEncoder(active_dims=active), solver=dynamics.MomentMatchingEuler())
  objective = GaussianObjective(target=to_dev(target, device, F64), precis=to_dev(precis, device, F64))
  ks = pol.kernel.kernels
  params = [pol.q_mu] + [iv.Z for iv in pol.inducing_variable.inducing_variables] + [k.lengthscales for k in ks] + [k.variance for k in ks]
  for t in params:
    t.requires_grad_(True)
  roll = ops.ComposedRollout(drift.packed(F64, True, device), pol.packed(F64, False, device), nx=nx, active_dims=active,
                             head_scale=SCALE[0] if nu == 1 else SCALE[:nu], head_shift=SHIFT[0] if nu == 1 else SHIFT[:nu],
                             target=to_dev(target, device, F64), precis=to_dev(precis, device, F64))
  return system, objective, params, roll, drift, to_dev(mu0, device, F64), to_dev(S0, device, F64)


def graphed_sweep(roll, tape, g_cost, B, H, generic):
  """The wide reverse sweep over ``tape`` captured into a graph with the dense path chosen by ``generic``: -> (replay, outputs)."""
  lib = _lib.lib()
  lib.mm_compose_wide_dense_path(int(generic))
  try:
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      for _ in range(2):
        roll.backward_wide(tape, g_cost, B, H)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      out = roll.backward_wide(tape, g_cost, B, H)
  finally:
    lib.mm_compose_wide_dense_path(0)
  return graph.replay, out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=30)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--inner", type=int, default=10)
  ap.add_argument("--batches", default="1,64,256")
  ap.add_argument("--systems", default="ne11,ne16")
  ap.add_argument("--native-only", action="store_true")
  ap.add_argument("--label", default="")
  ap.add_argument("--out", default=os.path.join(_root, "profiles", "compose_wide_bench.json"))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_compose_wide.py needs the GPU (no CPU timing is meaningful)")
  from gpflowpilco_amd.loops import GraphedPolicyLoss, get_state_initializer, policy_loss_closure
  device, H = "cuda", args.steps
  res = {"tool": "bench_compose_wide", "label": args.label, "H": H, "unit": "ms per step, f64", "criterion": True,
         "dense_paths_kept": True}
  for name in args.systems.split(","):
    sysd = SYSTEMS[name]
    res[name] = {"shape": dict(nx=sysd["nx"], na=len(sysd["active"]), nu=sysd["nu"], drift_M=100, policy_M=30)}
    for B in [int(b) for b in args.batches.split(",")]:
      system, objective, params, roll, drift, mx, Sxx = build(sysd["nx"], sysd["active"], sysd["nu"], sysd["seed"], B, device)
      init = get_state_initializer(mx, Sxx)
      kw = dict(native_wide=True, native_actions=sysd["nu"])

      def loss_grad(closure):
        def run():
          for t in params:
            t.grad = None
          loss = closure()
          loss.sum().backward()
          return loss
        return run
      with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)        # a fall-back to the torch composition would be timed as native: refuse
        native = policy_loss_closure(system, objective, init, H, **kw)
        graphed = GraphedPolicyLoss(native, params)           # (the capture first, on fresh parameters: see bench_multiaction)
        g_native = loss_grad(native)
        loss_native = g_native().detach().clone()
      g_cost = torch.ones(H, B, dtype=F64, device=device)
      _, _, _, tape = roll.taped_wide(mx, Sxx, H)
      sweep_fast, out_fast = graphed_sweep(roll, tape, g_cost, B, H, generic=False)
      sweep_generic, out_generic = graphed_sweep(roll, tape, g_cost, B, H, generic=True)
      sweep_fast(); sweep_generic()
      torch.cuda.synchronize()
      out = {"sweep_fast_vs_generic_max_rel": max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
                                                   for a, b in zip(out_fast, out_generic))}
      fns = {"native_loss_and_grad": g_native, "native_loss_and_grad_replayed": graphed.loss_and_grad,
             "sweep_one_wave_paths_replayed": sweep_fast, "sweep_generic_paths_replayed": sweep_generic}
      inners = {k: args.inner for k in fns}
      if not args.native_only:
        g_torch = loss_grad(policy_loss_closure(system, objective, init, H, native=False))
        out["loss_native_vs_torch"] = float((loss_native - g_torch().detach()).abs().max())
        fns["torch_loss_and_grad"] = g_torch
        inners["torch_loss_and_grad"] = 1
      out.update(alternating(fns, H, inners, args.repeats, 1))
      try:
        drift.packed(F64, True, device).check_status(B)
      except Exception as e:                     # noqa: BLE001 -- recorded beside the numbers
        out["status"] = str(e)
      out["loss_min_max"] = [float(loss_native.min()), float(loss_native.max())]
      kept = out["sweep_one_wave_paths_replayed"]["max"] < out["sweep_generic_paths_replayed"]["min"]
      out["dense_paths_kept"] = bool(kept)
      res["dense_paths_kept"] = res["dense_paths_kept"] and bool(kept)
      if "torch_loss_and_grad" in fns:
        t = out["torch_loss_and_grad"]
        ok = max(out["native_loss_and_grad"]["max"], out["native_loss_and_grad_replayed"]["max"]) < t["min"]
        out["criterion"] = bool(ok)
        res["criterion"] = res["criterion"] and bool(ok)
        out["torch_over_native_loss_and_grad"] = t["median"] / out["native_loss_and_grad"]["median"]
        out["torch_over_native_loss_and_grad_replayed"] = t["median"] / out["native_loss_and_grad_replayed"]["median"]
      res[name][f"B{B}"] = out
      del fns, graphed, sweep_fast, sweep_generic, out_fast, out_generic, tape
      torch.cuda.empty_cache()
  line = json.dumps(res)
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(line + "\n")
  print(line)
  return 0 if res["criterion"] else 1


if __name__ == "__main__":
  sys.exit(main())
