#!/usr/bin/env python
"""Time of a MEAN-ONLY drift on the pathwise solver (the drift in a ``KernelRegressor``: every sample steps with the posterior
mean) beside the sampled drift of the same shapes.

``loss_and_grad`` -- the 4-state, one-action system of DESIGN.md section 8 f-3 (nx 4, one angle, nd 6; drift M 2000, policy M 30,
H 30), float64 and float32 states, S = 128 / 1024 / 8192, ms per step of loss + gradient w.r.t. the policy, in one process and in
alternating windows (``bench_multiaction.alternating``):
  ``mean_native``      ``pathwise_policy_loss_closure(native=True)`` on the KernelRegressor drift (``mm_pathwise_policy_rollout_mean``)
  ``sampled_native``   the same closure on the PathwiseSVGP itself with K = 1024 bases, given paths (the weight stream)
  ``mean_torch``       the torch composition of the mean-only closure (``native=False``), ``--torch-steps`` steps, one call per window
``mean_pass`` -- ``mm_pathwise_mean_eval`` alone at S 8192, M 2000, d 8, L 8: values only and with the Jacobian, ms per call and
basis values (2^x evaluations, S L M per call) per second.
Prints one JSON line; ``--out FILE`` also writes it."""
import argparse
import json
import os
import sys
import warnings

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _here)
sys.path.insert(0, os.path.join(_here, "tools"))

import torch  # noqa: E402

from bench_multiaction import SCALE, SHIFT, alternating  # noqa: E402
from bench_pathwise_matern import drift_of  # noqa: E402
from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp  # noqa: E402
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder  # noqa: E402
from gpflowpilco_amd.loops import pathwise_policy_loss_closure  # noqa: E402
from gpflowpilco_amd.pathwise import MeanDrift  # noqa: E402
from gpflowpilco_amd.synthetic import make_policy, make_svgp  # noqa: E402

F64, F32 = torch.float64, torch.float32
MD, K = 2000, 1024
NX, ACTIVE, MP = 4, (1,), 30
NE = NX + len(ACTIVE)
ND = NE + 1
S_PASS, D_PASS, L_PASS = 8192, 8, 8


def policy_system(drift, device):
  pol = make_policy(MP, NE, seed=130).to_model(device)
  params = [pol.q_mu, pol.inducing_variable.inducing_variables[0].Z, pol.kernel.kernels[0].lengthscales, pol.kernel.kernels[0].variance]
  for t in params:
    t.requires_grad_(True)
  t64 = lambda v: torch.tensor(v, dtype=F64, device=device)
  head = tfb.Chain([tfb.Scale(t64(SCALE[0])), tfb.Shift(t64(SHIFT[0])), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=ACTIVE), solver=dynamics.Euler())
  target = torch.zeros(NE, dtype=F64, device=device); target[1] = 1.0
  return system, GaussianObjective(target=target, precis=0.25 * torch.eye(NE, dtype=F64, device=device)), params


def loss_grad_of(closure, params):
  def run():
    for t in params:
      t.grad = None
    out = closure()
    out.mean().backward()
    return out
  run()
  return run


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=30)
  ap.add_argument("--torch-steps", type=int, default=2, help="steps of the torch composition's rollout (0: skip the row)")
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--inner", type=int, default=200, help="mean passes per window")
  ap.add_argument("--inner-loss", type=int, default=5, help="loss + gradient calls per window")
  ap.add_argument("--samples", default="128,1024,8192")
  ap.add_argument("--dtypes", default="f32,f64")
  ap.add_argument("--label", default="")
  ap.add_argument("--out", default="")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_pathwise_mean.py needs the GPU (no CPU timing is meaningful)")
  device, H = "cuda", args.steps
  res = {"tool": "bench_pathwise_mean", "label": args.label,
         "shape": {"drift_M": MD, "K_sampled": K, "policy": {"nx": NX, "na": len(ACTIVE), "nu": 1, "nd": ND, "policy_M": MP, "H": H},
                   "torch_steps": args.torch_steps, "mean_pass": {"S": S_PASS, "M": MD, "d": D_PASS, "L": L_PASS}},
         "unit": "ms per step (loss_and_grad), ms per call (mean_pass); median of alternating windows"}
  syn_p = make_svgp(NX, MD, ND, seed=121, device=device, ls_bounds=(0.8, 3.0))
  syn_p.Z[:, NE:] = 4.0 * syn_p.Z[:, NE:] - 2.0
  syn_p.q_mu = 0.3 * syn_p.q_mu
  syn = make_svgp(L_PASS, MD, D_PASS, seed=120, device=device, ls_bounds=(0.8, 3.0))
  for dname in args.dtypes.split(","):
    dtype = F32 if dname == "f32" else F64
    out = {}
    for S in (int(s) for s in args.samples.split(",") if s):          # (--samples "": the mean pass alone, e.g. under a profiler)
      drift = drift_of(syn_p, "se", device)
      x0 = (0.2 + 0.6 * torch.rand(S, NX, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(9))).to(dtype)
      sys_s, objective, params = policy_system(drift, device)
      paths = drift.generate_paths(S, K, dtype=dtype, device=device, generator=torch.Generator(device=device).manual_seed(7))
      sys_m, _, params_m = policy_system(gp.KernelRegressor(drift), device)
      fns, slow = {}, {}
      with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)        # a fall-back to the torch composition would be timed as native: refuse
        fns["mean_native"] = loss_grad_of(pathwise_policy_loss_closure(sys_m, objective, lambda x0=x0: x0, H, dt=0.1, native=True),
                                          params_m)
        fns["sampled_native"] = loss_grad_of(pathwise_policy_loss_closure(sys_s, objective, lambda x0=x0: x0, H, dt=0.1, paths=paths,
                                                                          native=True), params)
      row = alternating(fns, H, args.inner_loss, args.repeats, 1)
      if args.torch_steps > 0:
        slow["mean_torch"] = loss_grad_of(pathwise_policy_loss_closure(sys_m, objective, lambda x0=x0: x0, args.torch_steps, dt=0.1,
                                                                       native=False), params_m)
        row.update(alternating(slow, args.torch_steps, 1, 2, 0))
      row["mean_over_sampled"] = row["mean_native"]["median"] / row["sampled_native"]["median"]
      row["condition_met"] = row["mean_native"]["max"] <= row["sampled_native"]["min"]
      out[f"S{S}"] = row
      del fns, slow, paths
      torch.cuda.empty_cache()
    md = MeanDrift.from_model(drift_of(syn, "se", device), dtype, device)
    x = torch.rand(S_PASS, D_PASS, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(8)).to(dtype)
    passes = alternating({"values": lambda: md._eval(x, False), "jacobian": lambda: md._eval(x, True)}, 1, args.inner, args.repeats, 2)
    for k in ("values", "jacobian"):
      passes[k]["basis_values_per_s"] = S_PASS * L_PASS * MD / (passes[k]["median"] * 1e-3)
    out["mean_pass"] = passes
    res[dname] = out
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, "w") as fh:
      fh.write(line + "\n")


if __name__ == "__main__":
  main()
