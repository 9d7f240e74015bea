#!/usr/bin/env python
"""Time per step of the PATHWISE policy loss with a coregionalised drift (``native_coregionalized=True``).

The README's 6-state system (nx = 6, angles (2, 4), one action: ne = 8, nd = 9), drift M = 2000, K = 1024 bases, policy M = 30,
H = 30, float64 paths, S = 1024 and S = 8192 sample paths.  Per S, in one process and in alternating windows
(``bench_multiaction.alternating``), ms per step of loss + gradient (and of the forward alone) of
  (a) ``lcm3_*`` / ``lcm6_*``   the drift as Lg = 3 / Lg = 6 latents mixed by a dense W to 6 outputs, native (the ``_mixed`` entries)
  (b) ``torch3_*`` / ``torch6_*``  the torch composition on the SAME mixed paths (``native=False``): the route (a) replaces
  (c) ``independent_*``         six independent latents through the ``_wide`` entries: what the parent of this option could run
on fixed paths (drawn once per system), and per-kernel times of the native route: the taped forward alone, the reverse sweep alone
on its tape, and H stream passes with their Jacobians alone (``mm_pathwise_eval_jac`` with the rollout's L) -- the head kernels are
the taped forward minus the stream passes.  Tape bytes per variant.  Then one ``PathSampler.draw`` at Lg = 3 against Lg = 6.
``--native-only`` leaves (b) out.  Prints one JSON line; ``--out FILE`` also writes it."""
import argparse
import json
import os
import sys
import warnings

import numpy as np

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _here)
sys.path.insert(0, os.path.join(_here, "tools"))

import torch  # noqa: E402

from bench_multiaction import SCALE, SHIFT, alternating  # noqa: E402
from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp  # noqa: E402
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder  # noqa: E402
from gpflowpilco_amd.loops import pathwise_policy_loss_closure  # noqa: E402
from gpflowpilco_amd.pathwise import PathSampler, PathwiseSVGP, PolicyRollout  # noqa: E402
from gpflowpilco_amd.synthetic import make_policy, make_svgp  # noqa: E402

F64 = torch.float64
NX, ACTIVE, MD, MP, K = 6, (2, 4), 2000, 30, 1024
NE = NX + len(ACTIVE)
ND = NE + 1


def drift_of(L, mixed, device, seed=120):
  """A PathwiseSVGP with L latents on nd inputs: mixed by a dense W [6, L] with l2-normalised rows and a small Constant mean, or
  (L = 6) independent."""
  syn = make_svgp(L, MD, ND, seed=seed, device=device, ls_bounds=(0.8, 3.0))
  syn.Z[:, NE:] = 4.0 * syn.Z[:, NE:] - 2.0                          # the action axis in [-2, 2]
  syn.q_mu = 0.3 * syn.q_mu                                         # a gentle drift: the states stay in the data's support
  base = syn.to_model(device)
  kernel, mean = base.kernel, None
  if mixed:
    rng = np.random.default_rng(seed + 1)
    W = rng.standard_normal((NX, L))
    W = W / np.linalg.norm(W, axis=-1, keepdims=True)
    kernel = gp.LinearCoregionalization(base.kernel.kernels, torch.tensor(W, dtype=F64, device=device))
    mean = gp.Constant(torch.tensor(rng.uniform(-0.03, 0.03, NX), dtype=F64, device=device))
  return PathwiseSVGP(kernel=kernel, inducing_variable=base.inducing_variable, q_mu=base.q_mu, q_sqrt=base.q_sqrt, whiten=True,
                      mean_function=mean, num_latent_gps=L)


def system_of(drift, S, device, seed=130):
  pol = make_policy(MP, NE, seed=seed).to_model(device)
  k = pol.kernel.kernels[0]
  params = [pol.q_mu, pol.inducing_variable.inducing_variables[0].Z, k.lengthscales, k.variance]
  for t in params:
    t.requires_grad_(True)
  head = tfb.Chain([tfb.Scale(SCALE[0]), tfb.Shift(SHIFT[0]), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=ACTIVE), solver=dynamics.Euler())
  target = torch.zeros(NE, dtype=F64, device=device); target[len(ACTIVE):2 * len(ACTIVE)] = 1.0
  objective = GaussianObjective(target=target, precis=0.25 * torch.eye(NE, dtype=F64, device=device))
  x0 = 0.2 + 0.6 * torch.rand(S, NX, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(seed + 2))
  return system, objective, pol, params, x0


def eager_pair(closure, params):
  def forward():
    with torch.no_grad():
      return closure()

  def loss_grad():
    for t in params:
      t.grad = None
    loss = closure()
    loss.mean().backward()
    return loss
  return forward, loss_grad


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=30)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--inner", type=int, default=3)
  ap.add_argument("--samples", default="1024,8192")
  ap.add_argument("--native-only", action="store_true")
  ap.add_argument("--label", default="")
  ap.add_argument("--out", default="")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_pathwise_coregionalized.py needs the GPU (no CPU timing is meaningful)")
  device, H = "cuda", args.steps
  res = {"tool": "bench_pathwise_coregionalized", "label": args.label, "H": H, "unit": "ms per step, f64 paths, eager",
         "shape": {"nx": NX, "na": len(ACTIVE), "nu": 1, "nd": ND, "drift_M": MD, "K": K, "policy_M": MP}}
  drifts = {"lcm3": drift_of(3, True, device), "lcm6": drift_of(6, True, device), "independent": drift_of(6, False, device)}
  on = dict(native_inputs=16, native_coregionalized=True)
  for S in [int(s) for s in args.samples.split(",")]:
    fns, inners, out, keep = {}, {}, {}, []
    for name, drift in drifts.items():
      system, objective, pol, params, x0 = system_of(drift, S, device)
      paths = drift.generate_paths(S, K, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(7))
      with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)        # a fall-back to the torch composition would be timed as native: refuse
        f, g = eager_pair(pathwise_policy_loss_closure(system, objective, lambda x0=x0: x0, H, dt=0.1, paths=paths, **on), params)
        loss_native = g().detach().clone()
      fns[f"{name}_forward"], fns[f"{name}_loss_and_grad"] = f, g
      inners[f"{name}_forward"] = inners[f"{name}_loss_and_grad"] = args.inner
      # the native route's parts: taped forward, reverse sweep on its tape, H stream passes with Jacobians
      roll = PolicyRollout(paths, pol.packed(F64, False, device), nx=NX, active_dims=ACTIVE, head_scale=SCALE[0],
                           head_shift=SHIFT[0], target=objective.target, precis=objective.precis, wide=True)
      x0d = x0.detach()
      _, tape = roll(x0d, H, dt=0.1, with_jacobians=True)
      g_cost = torch.full((H, S), 1.0 / S, dtype=F64, device=device)
      din = torch.rand(S, ND, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(8))
      fns[f"{name}_taped_forward"] = lambda roll=roll, x0d=x0d: roll(x0d, H, dt=0.1, with_jacobians=True)
      fns[f"{name}_reverse_sweep"] = lambda roll=roll, tape=tape, g_cost=g_cost: roll.backward(tape, g_cost, H, dt=0.1)

      def stream(paths=paths, din=din):
        for _ in range(H):
          paths._latent_jac(din)
      fns[f"{name}_stream_passes"] = stream
      for part in ("taped_forward", "reverse_sweep", "stream_passes"):
        inners[f"{name}_{part}"] = args.inner
      out[f"{name}_tape_bytes"] = int(tape.numel())
      out[f"{name}_stream_bytes"] = int(paths.wb.numel() * paths.wb.element_size())
      if name != "independent" and not args.native_only:
        fT, gT = eager_pair(pathwise_policy_loss_closure(system, objective, lambda x0=x0: x0, H, dt=0.1, paths=paths, native=False),
                            params)
        out[f"{name}_loss_native_vs_torch"] = float((loss_native - gT().detach()).abs().max())
        tag = name.replace("lcm", "torch")
        fns[f"{tag}_forward"], fns[f"{tag}_loss_and_grad"] = fT, gT
        inners[f"{tag}_forward"] = inners[f"{tag}_loss_and_grad"] = 1
      keep.append((paths, tape, roll))
    out.update(alternating(fns, H, inners, args.repeats, 2))
    med = lambda k: out[k]["median"]
    for name in ("lcm3", "lcm6"):
      out[f"{name}_over_independent_loss_and_grad"] = med(f"{name}_loss_and_grad") / med("independent_loss_and_grad")
      out[f"{name}_over_independent_stream_passes"] = med(f"{name}_stream_passes") / med("independent_stream_passes")
      out[f"{name}_over_independent_tape_bytes"] = out[f"{name}_tape_bytes"] / out["independent_tape_bytes"]
      tag = name.replace("lcm", "torch")
      if f"{tag}_loss_and_grad" in fns:
        out[f"{tag}_over_native_loss_and_grad"] = med(f"{tag}_loss_and_grad") / med(f"{name}_loss_and_grad")
    # a PathSampler draw: three latents against six (ms per draw: H = 1 for the per-step division)
    draws = {}
    for name in ("lcm3", "lcm6"):
      sampler = PathSampler(drifts[name], S, K, dtype=F64, device=device)
      sampler.draw()
      draws[f"{name}_draw"] = sampler.draw
    out.update({k: dict(v, unit="ms per draw") for k, v in alternating(draws, 1, args.inner, args.repeats, 2).items()})
    out["lcm3_over_lcm6_draw"] = out["lcm3_draw"]["median"] / out["lcm6_draw"]["median"]
    res[f"S{S}"] = out
    del fns, keep, draws
    torch.cuda.empty_cache()
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, "w") as fh:
      fh.write(line + "\n")


if __name__ == "__main__":
  main()
