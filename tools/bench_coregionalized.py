#!/usr/bin/env python
"""Time per step of the moment-matched policy loss with a COREGIONALISED drift (``native_coregionalized=True``).

A 6-state system (nx = 6, angles (2, 4), one action: ne = 8, nd = 9), drift M = 100, policy M = 30, H = 30, f64, B = 1, 64, 256.
Per batch size, in the same process and in alternating windows (``bench_multiaction.alternating``), ms per step of
  (a) ``lcm_*``          the drift as Lg = 3 latents mixed to 6 outputs, native: forward and loss + gradient
  (b) ``torch_*``        the torch composition of the same system (``native=False``): the path (a) replaces
  (c) ``independent_*``  a SeparateIndependent drift with 6 latents at the same sizes, native (the one-action entries): what the fewer
                         latents buy
and, for the cost of the mixing launch itself, the forward of the 6 independent latents through ``mm_rollout_composed_nd``
(``independent_nd_forward``) next to the same latents mixed with W = I through ``mm_rollout_composed_nd_mixed``
(``identity_mixed_forward``): the two differ by one mixing launch per step.  ``--native-only`` leaves (b) out.  Prints one JSON line."""
import argparse
import copy
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
from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp, ops  # noqa: E402
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder  # noqa: E402
from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure  # noqa: E402
from gpflowpilco_amd.synthetic import generate_covariance  # noqa: E402
from tests.helpers import gp_model_from_oracle, random_svgp_params, to_dev  # noqa: E402

F64 = torch.float64
NX, ACTIVE, LG, MD, MP = 6, (2, 4), 3, 100, 30


def drift_params(L, seed, coregionalized):
  ne = NX + len(ACTIVE); nd = ne + 1
  p = random_svgp_params(seed=seed, L=L, M=MD, d=nd, whiten=True, ls_bounds=(0.8, 3.0), mean=True,
                         W_rows=NX if coregionalized else None)
  p.Z[..., ne:] = 4.0 * p.Z[..., ne:] - 2.0
  p.q_mu = 0.3 * p.q_mu                                   # a gentle drift: the state stays in the PD cone for the 30 steps
  p.mean_c = 0.03 * p.mean_c
  if coregionalized:
    p.W = 0.5 * np.random.default_rng(seed + 3).standard_normal((NX, L))
  return p


def system_of(drift_o, seed, B, device):
  na = len(ACTIVE); ne = NX + na
  pol_o = random_svgp_params(seed=seed + 1, L=1, M=MP, d=ne, whiten=True, ls_bounds=(0.3, 0.8), mean=False, separate_Z=False)
  pol_o.q_mu = 2.0 * pol_o.q_mu
  rng = np.random.default_rng(seed + 2)
  mu0 = rng.uniform(0.0, 0.6, (B, NX)); S0 = generate_covariance(rng, NX, (B,), 0.1)
  A = rng.standard_normal((ne, ne)); precis = A @ A.T / ne
  target = np.zeros(ne); target[na:2 * na] = 1.0
  drift, pol = gp_model_from_oracle(drift_o, device), gp_model_from_oracle(pol_o, device)
  head = tfb.Chain([tfb.Scale(SCALE[0]), tfb.Shift(SHIFT[0]), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=ACTIVE), solver=dynamics.MomentMatchingEuler())
  objective = GaussianObjective(target=to_dev(target, device, F64), precis=to_dev(precis, device, F64))
  k = pol.kernel.kernels[0]
  params = [pol.q_mu, pol.inducing_variable.inducing_variables[0].Z, k.lengthscales, k.variance]
  for t in params:
    t.requires_grad_(True)
  return system, objective, drift, pol, params, to_dev(mu0, device, F64), to_dev(S0, device, F64)


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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=30)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--inner", type=int, default=10)
  ap.add_argument("--batches", default="1,64,256")
  ap.add_argument("--native-only", action="store_true")
  ap.add_argument("--label", default="")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_coregionalized.py needs the GPU (no CPU timing is meaningful)")
  device, H = "cuda", args.steps
  res = {"tool": "bench_coregionalized", "label": args.label, "H": H, "unit": "ms per step, f64, eager",
         "shape": {"nx": NX, "na": len(ACTIVE), "nu": 1, "Lg": LG, "drift_M": MD, "policy_M": MP}}
  lcm_o, ind_o = drift_params(LG, 90, True), drift_params(NX, 90, False)
  eye_o = copy.copy(ind_o); eye_o.W = np.eye(NX)
  for B in [int(b) for b in args.batches.split(",")]:
    sysL, objL, driftL, _, parL, mx, Sxx = system_of(lcm_o, 90, B, device)
    sysI, objI, driftI, polI, parI, _, _ = system_of(ind_o, 90, B, device)
    init = get_state_initializer(mx, Sxx)
    with warnings.catch_warnings():
      warnings.simplefilter("error", RuntimeWarning)          # a fall-back to the torch composition would be timed as native: refuse
      fL, gL = eager_pair(policy_loss_closure(sysL, objL, init, H, native_coregionalized=True), parL)
      fI, gI = eager_pair(policy_loss_closure(sysI, objI, init, H), parI)
      loss_native = gL().detach().clone(); gI()
    fns = {"lcm_forward": fL, "lcm_loss_and_grad": gL, "independent_forward": fI, "independent_loss_and_grad": gI}
    inners = {k: args.inner for k in fns}
    # the mixing launch: the same 6 latents through the nd entry, and mixed with W = I through the mixed entry
    driftE = gp_model_from_oracle(eye_o, device)
    kw = dict(nx=NX, active_dims=ACTIVE, head_scale=SCALE[0], head_shift=SHIFT[0], target=objI.target, precis=objI.precis)
    rollN = ops.ComposedRollout(driftI.packed(F64, True, device), polI.packed(F64, False, device), **kw)
    rollE = ops.ComposedRollout(driftE.packed(F64, True, device), polI.packed(F64, False, device), mix_W=to_dev(eye_o.W, device, F64),
                                mix_c=to_dev(eye_o.mean_c, device, F64), **kw)
    fns["independent_nd_forward"] = lambda: rollN.call_nd_entry(mx, Sxx, H)
    fns["identity_mixed_forward"] = lambda: rollE.call_nd_entry(mx, Sxx, H)
    inners["independent_nd_forward"] = inners["identity_mixed_forward"] = args.inner
    out = {}
    if not args.native_only:
      fT, gT = eager_pair(policy_loss_closure(sysL, objL, init, H, native=False), parL)
      out["loss_native_vs_torch"] = float((loss_native - gT().detach()).abs().max())
      fns["torch_forward"], fns["torch_loss_and_grad"] = fT, gT
      inners["torch_forward"] = inners["torch_loss_and_grad"] = 1
    out.update(alternating(fns, H, inners, args.repeats, 2))
    for nm, d in (("lcm", driftL), ("independent", driftI)):
      try:                                     # a state that left the PD cone would make the timed work unrepresentative
        d.packed(F64, True, device).check_status(B)
      except Exception as e:                   # noqa: BLE001 -- recorded beside the numbers
        out[f"status_{nm}"] = str(e)
    med = lambda k: out[k]["median"]
    out["mixing_launch_ms_per_step"] = med("identity_mixed_forward") - med("independent_nd_forward")
    out["independent_over_lcm_loss_and_grad"] = med("independent_loss_and_grad") / med("lcm_loss_and_grad")
    if "torch_loss_and_grad" in fns:
      out["torch_over_native_loss_and_grad"] = med("torch_loss_and_grad") / med("lcm_loss_and_grad")
      out["torch_over_native_forward"] = med("torch_forward") / med("lcm_forward")
    res[f"B{B}"] = out
    del fns
    torch.cuda.empty_cache()
  print(json.dumps(res))


if __name__ == "__main__":
  main()
