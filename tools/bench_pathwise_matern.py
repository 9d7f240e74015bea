#!/usr/bin/env python
"""Time of the pathwise weight-stream passes and of the policy loss per kernel family: SquaredExponential, Matern-3/2, Matern-5/2.

The C5-shard shape of the pathwise tools (S 8192 paths, drift M 2000, K 1024 bases, d 8 inputs, L 8 latents), float32 and float64
paths.  Per dtype, in one process and in alternating windows (``bench_multiaction.alternating``: the families take turns window by
window, median of ``--repeats`` windows), ms per call of
  ``plain``          one evaluation f_s(x_s)                      (``mm_pathwise_eval[_kern]``)
  ``jacobian``       one evaluation with its Jacobian             (``mm_pathwise_eval_jac[_kern]``)
  ``loss_and_grad``  loss + gradient of the two-action policy rollout (nx 4, angles (0, 1), nu 2: nd 8, L 4; policy M 30, H 10)
                     through ``pathwise_policy_loss_closure(native=True)``, ms per step
and each Matern row as a ratio to the SquaredExponential row of the same pass.  The paths of the three families share their numbers
(the same model arrays, the same generator state): only the kernel class differs.  ``--families se`` measures the
SquaredExponential rows alone -- what a build of another commit can run too, for a side-by-side comparison of the unchanged rows.
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
from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp  # noqa: E402
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder  # noqa: E402
from gpflowpilco_amd.loops import pathwise_policy_loss_closure  # noqa: E402
from gpflowpilco_amd.pathwise import PathwiseSVGP  # noqa: E402
from gpflowpilco_amd.synthetic import make_policy, make_svgp  # noqa: E402

F64, F32 = torch.float64, torch.float32
S, MD, K, D, L = 8192, 2000, 1024, 8, 8
NX, ACTIVE, NU, MP = 4, (0, 1), 2, 30
NE = NX + len(ACTIVE)


def drift_of(syn, family, device):
  base = syn.to_model(device) if family == "se" else syn.to_model(device, kernel=family)
  return PathwiseSVGP(kernel=base.kernel, inducing_variable=base.inducing_variable, q_mu=base.q_mu, q_sqrt=base.q_sqrt, whiten=True,
                      mean_function=None, num_latent_gps=base.num_latent_gps)


def policy_system(drift, device, dtype, seed=130):
  pols = [make_policy(MP, NE, seed=seed + a).to_model(device) for a in range(NU)]
  kernels = [p.kernel.kernels[0] for p in pols]
  ivs = [p.inducing_variable.inducing_variables[0] for p in pols]
  pol = gp.SVGP(kernel=gp.SeparateIndependent(kernels), inducing_variable=gp.SeparateIndependentInducingVariables(ivs),
                q_mu=torch.cat([p.q_mu for p in pols], dim=1), q_sqrt=torch.cat([p.q_sqrt for p in pols], dim=0), whiten=True,
                num_latent_gps=NU)
  params = [pol.q_mu] + [iv.Z for iv in ivs] + [k.lengthscales for k in kernels] + [k.variance for k in kernels]
  for t in params:
    t.requires_grad_(True)
  t64 = lambda v: torch.tensor(v, dtype=F64, device=device)
  head = tfb.Chain([tfb.Scale(t64(SCALE[:NU])), tfb.Shift(t64(SHIFT[:NU])), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=ACTIVE), solver=dynamics.Euler())
  target = torch.zeros(NE, dtype=F64, device=device); target[len(ACTIVE):2 * len(ACTIVE)] = 1.0
  objective = GaussianObjective(target=target, precis=0.25 * torch.eye(NE, dtype=F64, device=device))
  x0 = (0.2 + 0.6 * torch.rand(S, NX, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(seed + 9))).to(dtype)
  return system, objective, params, x0


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--inner", type=int, default=200, help="stream passes per window (a window then lasts 30 - 250 ms)")
  ap.add_argument("--inner-loss", type=int, default=10, help="loss + gradient calls per window")
  ap.add_argument("--families", default="se,matern32,matern52")
  ap.add_argument("--dtypes", default="f32,f64")
  ap.add_argument("--label", default="")
  ap.add_argument("--out", default="")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_pathwise_matern.py needs the GPU (no CPU timing is meaningful)")
  device, H = "cuda", args.steps
  families = args.families.split(",")
  res = {"tool": "bench_pathwise_matern", "label": args.label, "families": families,
         "shape": {"S": S, "drift_M": MD, "K": K, "d": D, "L": L, "policy": {"nx": NX, "na": len(ACTIVE), "nu": NU, "nd": NE + NU,
                                                                          "policy_M": MP, "H": H}},
         "unit": "ms per call (plain, jacobian), ms per step (loss_and_grad); median of alternating windows"}
  syn = make_svgp(L, MD, D, seed=120, device=device, ls_bounds=(0.8, 3.0))
  syn_p = make_svgp(NX, MD, NE + NU, seed=121, device=device, ls_bounds=(0.8, 3.0))
  syn_p.Z[:, NE:] = 4.0 * syn_p.Z[:, NE:] - 2.0
  syn_p.q_mu = 0.3 * syn_p.q_mu
  for dname in args.dtypes.split(","):
    dtype = F32 if dname == "f32" else F64
    stream, loss, keep = {}, {}, []
    x = torch.rand(S, D, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(8)).to(dtype)
    for fam in families:
      seed = lambda: torch.Generator(device=device).manual_seed(7)
      paths = drift_of(syn, fam, device).generate_paths(S, K, dtype=dtype, device=device, generator=seed())
      stream[f"{fam}_plain"] = lambda paths=paths: paths._latent_values(x)
      stream[f"{fam}_jacobian"] = lambda paths=paths: paths._latent_jac(x)
      drift_p = drift_of(syn_p, fam, device)
      system, objective, params, x0 = policy_system(drift_p, device, dtype)
      ppaths = drift_p.generate_paths(S, K, dtype=dtype, device=device, generator=seed())
      with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)        # a fall-back to the torch composition would be timed as native: refuse
        closure = pathwise_policy_loss_closure(system, objective, lambda x0=x0: x0, H, dt=0.1, paths=ppaths, native=True,
                                               native_actions=NU)

        def loss_grad(closure=closure, params=params):
          for t in params:
            t.grad = None
          out = closure()
          out.mean().backward()
          return out
        loss_grad()
      loss[f"{fam}_loss_and_grad"] = loss_grad
      keep.append((paths, ppaths, system))
    out = alternating(stream, 1, args.inner, args.repeats, 2)
    out.update(alternating(loss, H, args.inner_loss, args.repeats, 1))
    out["stream_bytes"] = int(keep[0][0].wb.numel() * keep[0][0].wb.element_size())
    if "se" in families:
      for fam in families:
        if fam != "se":
          for p in ("plain", "jacobian", "loss_and_grad"):
            out[f"{fam}_over_se_{p}"] = out[f"{fam}_{p}"]["median"] / out[f"se_{p}"]["median"]
    res[dname] = out
    del stream, loss, keep
    torch.cuda.empty_cache()
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, "w") as fh:
      fh.write(line + "\n")


if __name__ == "__main__":
  main()
