#!/usr/bin/env python
"""Forward time per step of the multi-action native rollout (mm_rollout_composed_nd) next to the one-action one.

  system A (tests/test_multiaction.py: nx = 4, two angles, two actions, drift M = 100, policy M = 30), f64, eager, B = 1, 64, 256
  the one-action rollout at cartpole sizes (nx = 4, one angle, drift M = 100, policy M = 30), same process, B = 1, 64, 256
  the torch composition of system A at B = 1 (policy_loss_closure(native=False), no_grad)

Device events around `inner` back-to-back rollouts of H steps, after warm-up; `repeats` windows; the median and the
min .. max spread of the windows are reported, in ms per step.  ``--one-action-only`` times only the one-action rollout: run
from the root of ANOTHER checkout (the package is imported from the current directory when it holds one) it gives that
checkout's numbers for the unchanged path.  Prints one JSON line.

``--pathwise``: the pathwise (sample-path) policy loss instead -- loops.pathwise_policy_loss_closure at the C5 shard's sizes (drift
M = 2000, K = 1024 bases, policy M = 30, S = 8192 paths, H = 30), f32 and f64 paths, ms per step of
  two actions (nx = 4, two angles, nd = 8): native forward and native loss + gradient (native_actions=2), and the torch
    composition's forward and loss + gradient (native=False) on the same paths (float64 paths only: the torch composition
    evaluates the float64 policy models);
  one action (cartpole: nx = 4, one angle, nd = 6) through the existing entries, same four figures, same process: the yardstick;
  the cart-double-pendulum (nx = 6, angles (2, 4), one action, nd = 9) through ``native_inputs=16``: the wide entries and the
    Jacobian pass over half sample groups, same four figures (its torch composition differentiates through the same pass).
``--rows one_action,two_actions`` picks rows (the first two exist in earlier checkouts: run from the root of one for its numbers).
The variants of one shape are timed in alternation (window r of every variant before window r + 1 of any).  ``--samples`` /
``--drift-M`` shrink the shape for a dry run; ``--native-only`` leaves the torch composition out (the run to put under
``rocprofv3 --kernel-trace --stats``: profiles/pathwise_multiaction_kernel_stats.csv).  ``--objective custom``: the same rows with a
caller-defined objective -- the time-weighted quadratic (1 + 0.1 t / dt) (e - tau)^T W (e - tau) on tensors -- instead of the
GaussianObjective: "native" is then ``native_objective=True`` (the native rollout with its states as a differentiable output, the
objective in torch on them, the seeded reverse sweep), "torch" the torch composition with the same objective on the same paths;
``--dtypes f64`` picks the paths' element types.

``--grad``: the moment-matched policy LOSS + GRADIENT (loops.policy_loss_closure; every policy parameter trainable), f64, H = 30, ms
per step, for system A at B = 1, 64 and 256:
  native (native_actions=2: csrc/mm_compose_bwd_nd.hip), eager and replayed from a ``GraphedPolicyLoss``; the native forward, eager
    and replayed;
  the torch composition's loss + gradient (native=False), eager -- the path the native one replaces;
  the one-action native loss + gradient and forward at cartpole sizes, eager and replayed: the yardstick.
All variants of one B in the same process, in alternating windows.  ``--native-only`` leaves the torch composition out (the run for
a kernel trace: profiles/multiaction_grad_kernel_stats.csv); ``--batches 1,64`` picks the batch sizes."""
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


def alternating(fns, H, inner, repeats, warmup):
  """{name: ms-per-step stats}: device events around `inner` back-to-back calls; the variants take turns window by window.
  ``inner``: one count for every variant, or {name: count}."""
  inners = inner if isinstance(inner, dict) else {k: inner for k in fns}
  for fn in fns.values():
    for _ in range(warmup):
      fn()
  torch.cuda.synchronize()
  out = {k: [] for k in fns}
  for _ in range(repeats):
    for k, fn in fns.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(inners[k]):
        fn()
      e1.record()
      e1.synchronize()
      out[k].append(e0.elapsed_time(e1) / (inners[k] * H))
  return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "windows": len(v),
              "calls_per_window": inners[k]} for k, v in out.items()}


def grad_closures(nx, active, nu, seed, B, H, device, native_actions):
  """(native closure, torch-composition closure, trainable parameters) of the moment-matched policy loss of ``build``'s system."""
  from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
  _, drift, pol, mx, Sxx, target, precis = build(nx, active, nu, 100, seed, B, device)
  if nu == 1:
    head = tfb.Chain([tfb.Scale(SCALE[0]), tfb.Shift(SHIFT[0]), tfb.NormalCDF()])
  else:
    head = tfb.Chain([tfb.Scale(to_dev(SCALE[:nu], device, F64)), tfb.Shift(to_dev(SHIFT[:nu], device, F64)), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=active), solver=dynamics.MomentMatchingEuler())
  objective = GaussianObjective(target=to_dev(target, device, F64), precis=to_dev(precis, device, F64))
  ks = pol.kernel.kernels
  params = [pol.q_mu] + [iv.Z for iv in pol.inducing_variable.inducing_variables] + [k.lengthscales for k in ks] + [k.variance for k in ks]
  for t in params:
    t.requires_grad_(True)
  init = get_state_initializer(mx, Sxx)
  native = policy_loss_closure(system, objective, init, H, native_actions=native_actions)
  composed = policy_loss_closure(system, objective, init, H, native=False)
  return native, composed, params, drift


def main_grad(args):
  import warnings
  from gpflowpilco_amd.loops import GraphedPolicyLoss
  device, H = "cuda", args.steps
  res = {"tool": "bench_multiaction --grad", "label": args.label, "H": H, "unit": "ms per step, f64"}

  def eager_pair(closure, params):
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
  for B in [int(b) for b in args.batches.split(",")]:
    with warnings.catch_warnings():
      warnings.simplefilter("error", RuntimeWarning)          # a fall-back to the torch composition would be timed as native: refuse
      nat2, tor2, par2, drift2 = grad_closures(4, (0, 1), 2, 20, B, H, device, 2)
      nat1, _, par1, _ = grad_closures(4, (1,), 1, 10, B, H, device, 1)
      f2, g2 = eager_pair(nat2, par2)
      f1, g1 = eager_pair(nat1, par1)
      # the captures come first, on fresh parameters: a backward that ran eagerly before pins the parameters' gradient accumulation
      # to the default stream, which a later capture on another stream cannot record
      gr2, gr1 = GraphedPolicyLoss(nat2, par2), GraphedPolicyLoss(nat1, par1)
      loss_native = g2().detach().clone()
    fns = {"two_actions_forward": f2, "two_actions_loss_and_grad": g2, "two_actions_forward_replayed": gr2.loss,
           "two_actions_loss_and_grad_replayed": gr2.loss_and_grad, "one_action_forward": f1, "one_action_loss_and_grad": g1,
           "one_action_forward_replayed": gr1.loss, "one_action_loss_and_grad_replayed": gr1.loss_and_grad}
    inners = {k: args.inner for k in fns}
    out = {}
    if not args.native_only:
      _, gt = eager_pair(tor2, par2)
      loss_torch = gt().detach()
      out["loss_native_vs_torch"] = float((loss_native - loss_torch).abs().max())
      fns["two_actions_torch_loss_and_grad"] = gt
      inners["two_actions_torch_loss_and_grad"] = 1
    out.update(alternating(fns, H, inners, args.repeats, 2))
    try:
      drift2.packed(F64, True, device).check_status(B)
    except Exception as e:                     # noqa: BLE001
      out["status"] = str(e)
    med = lambda k: out[k]["median"]
    out["two_actions_loss_and_grad_over_forward"] = med("two_actions_loss_and_grad") / med("two_actions_forward")
    out["two_actions_loss_and_grad_over_forward_replayed"] = (med("two_actions_loss_and_grad_replayed")
                                                              / med("two_actions_forward_replayed"))
    out["two_over_one_action_loss_and_grad_replayed"] = (med("two_actions_loss_and_grad_replayed")
                                                         / med("one_action_loss_and_grad_replayed"))
    if "two_actions_torch_loss_and_grad" in fns:
      out["torch_over_native_loss_and_grad"] = med("two_actions_torch_loss_and_grad") / med("two_actions_loss_and_grad")
      out["torch_over_native_loss_and_grad_replayed"] = (med("two_actions_torch_loss_and_grad")
                                                         / med("two_actions_loss_and_grad_replayed"))
    res[f"B{B}"] = out
    del fns, gr2, gr1
    torch.cuda.empty_cache()
  print(json.dumps(res))


class TimeWeightedQuadratic:
  """(1 + 0.1 t / dt) (e - tau)^T W (e - tau) of a tensor of encoded states."""

  def __init__(self, W, tau, dt):
    self.W, self.tau, self.dt = W, tau, dt

  def __call__(self, x, t=None):
    e = x - self.tau
    return (1.0 + 0.1 * t / self.dt) * (e * (e @ self.W)).sum(-1)


def pathwise_shape(nx, active, nu, Md, K, S, H, dtype, seed, device, inner, repeats, with_torch=True, native_inputs=8,
                   custom=False):
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  from gpflowpilco_amd.pathwise import PathwiseSVGP
  na = len(active); ne = nx + na; nd = ne + nu
  base = make_svgp(nx, Md, nd, seed=seed, device=device, ls_bounds=(0.8, 3.0)).to_model(device)
  drift = PathwiseSVGP(kernel=base.kernel, inducing_variable=base.inducing_variable, q_mu=base.q_mu, q_sqrt=base.q_sqrt, whiten=True,
                       num_latent_gps=nx)
  pol_o = random_svgp_params(seed=seed + 1, L=nu, M=30, d=ne, whiten=True, ls_bounds=(0.8, 2.0), mean=True, separate_Z=True)
  pol_o.q_mu = 0.3 * pol_o.q_mu
  pol = gp_model_from_oracle(pol_o, device)
  if nu == 1:
    head = tfb.Chain([tfb.Scale(SCALE[0]), tfb.Shift(SHIFT[0]), tfb.NormalCDF()])
  else:
    head = tfb.Chain([tfb.Scale(to_dev(SCALE[:nu], device, F64)), tfb.Shift(to_dev(SHIFT[:nu], device, F64)), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=active), solver=dynamics.Euler())
  target = np.zeros(ne); target[na:2 * na] = 1.0
  objective = GaussianObjective(target=to_dev(target, device, dtype), precis=to_dev(np.eye(ne), device, dtype))
  extra = {}
  if custom:
    A = np.random.default_rng(seed + 3).standard_normal((ne, ne))
    objective = TimeWeightedQuadratic(to_dev(A @ A.T / ne + 0.5 * np.eye(ne), device, dtype), to_dev(target, device, dtype), 0.1)
    extra = {"native_objective": True}
  g = torch.Generator(device=device).manual_seed(seed + 2)
  x0 = 0.2 + 0.6 * torch.rand(S, nx, dtype=dtype, device=device, generator=g)
  paths = drift.generate_paths(S, K, dtype=dtype, device=device, generator=g)
  ks = pol.kernel.kernels
  params = [pol.q_mu] + [iv.Z for iv in pol.inducing_variable.inducing_variables] + [k.lengthscales for k in ks] + [k.variance for k in ks]
  for t in params:
    t.requires_grad_(True)
  wide = {"native_inputs": native_inputs} if native_inputs > 8 else {}
  native = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.1, paths=paths, native=True, native_actions=nu, **wide,
                                        **extra)
  composed = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.1, paths=paths, native=False)

  def forward(closure):
    def run():
      with torch.no_grad():
        return closure()
    return run

  def loss_grad(closure):
    def run():
      for t in params:
        t.grad = None
      loss = closure().mean()
      loss.backward()
      return loss
    return run
  fns = {"native_forward": forward(native), "native_loss_and_grad": loss_grad(native)}
  kinds = ["native"]
  if with_torch and dtype == F64:          # (the torch composition evaluates the float64 policy models: it composes with float64 paths only)
    fns.update({"torch_forward": forward(composed), "torch_loss_and_grad": loss_grad(composed)})
    kinds.append("torch")
  losses = {k: float(fns[f"{k}_loss_and_grad"]().detach()) for k in kinds}
  res = alternating(fns, H, inner, repeats, 1)
  res["mean_loss"] = losses
  res["shape"] = {"nx": nx, "na": na, "nu": nu, "nd": nd, "drift_M": Md, "K": K, "policy_M": 30, "S": S, "H": H}
  res["objective"] = "custom" if custom else "gaussian"
  for k in kinds:
    res[f"{k}_loss_and_grad_over_forward"] = res[f"{k}_loss_and_grad"]["median"] / res[f"{k}_forward"]["median"]
  if "torch" in kinds:
    res["torch_over_native_loss_and_grad"] = res["torch_loss_and_grad"]["median"] / res["native_loss_and_grad"]["median"]
    res["torch_over_native_forward"] = res["torch_forward"]["median"] / res["native_forward"]["median"]
  return res


def main_pathwise(args):
  device = "cuda"
  res = {"tool": "bench_multiaction --pathwise", "label": args.label, "unit": "ms per step, eager"}
  rows = {"two_actions": (4, (0, 1), 2, 40, 8), "one_action": (4, (1,), 1, 3, 8), "cart_double_pendulum": (6, (2, 4), 1, 70, 16)}
  res["objective"] = args.objective
  for nm, dtype in (("f32", torch.float32), ("f64", F64)):
    if nm not in args.dtypes.split(","):
      continue
    res[nm] = {}
    for row in args.rows.split(","):
      nx, active, nu, seed, native_inputs = rows[row]
      res[nm][row] = pathwise_shape(nx, active, nu, args.drift_M, 1024, args.samples, args.steps, dtype, seed, device, args.inner,
                                    args.repeats, not args.native_only, native_inputs, args.objective == "custom")
      torch.cuda.empty_cache()
  print(json.dumps(res))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=30)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--inner", type=int, default=40)
  ap.add_argument("--one-action-only", action="store_true")
  ap.add_argument("--label", default="")
  ap.add_argument("--pathwise", action="store_true")
  ap.add_argument("--native-only", action="store_true", help="--pathwise without the torch composition (for a kernel trace)")
  ap.add_argument("--rows", default="two_actions,one_action,cart_double_pendulum", help="--pathwise: which shapes")
  ap.add_argument("--objective", choices=("gaussian", "custom"), default="gaussian",
                  help="--pathwise: the GaussianObjective, or a quadratic objective through native_objective=True")
  ap.add_argument("--dtypes", default="f32,f64", help="--pathwise: the paths' element types")
  ap.add_argument("--samples", type=int, default=8192)
  ap.add_argument("--drift-M", type=int, default=2000)
  ap.add_argument("--grad", action="store_true", help="moment-matched loss + gradient, native vs torch composition (see the docstring)")
  ap.add_argument("--batches", default="1,64,256")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_multiaction.py needs the GPU (no CPU timing is meaningful)")
  if args.pathwise:
    return main_pathwise(args)
  if args.grad:
    return main_grad(args)
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
