"""The native composed FORWARD rollouts (``mm_rollout_composed``, ``_nd``, ``_nd_mixed``) past ne = 8, against the committed oracle.

The entries take up to MMC_NX = 16 state dims, MMC_NA = 8 angles and MMC_NU = 4 actions -- 24 encoded dims, 28 drift inputs -- and
``loops.native_policy_loss`` sends every such system there for a loss without a gradient; every other GPU test of the family stays
at nx <= 6, ne <= 8, nd <= 12.  Past ne = 8 nearly every stage runs other code: the policy leaves ``k_policy_match_small`` for the
general match of a mean-only pack at d = 9 .. 24 and ``k_compose_policy``; the drift is up to 16 latents (136 pairs) on the d > 8
kernels; the tail kernel sums the reduce slabs itself only up to nd = 16 and decodes up to 152 pair indices; every
``for (idx = lane; idx < n * n; idx += 64)`` loop of the step, encode and head bodies makes a second trip; and the expected cost
leaves its register elimination for the LDS one (csrc/mm_cost.h).

Cases (B = 3, drift M = 40; the generator is ``tests/test_no_encoder.py::_system`` with lengthscales that grow with the width):
  w9     nx 7,  angles (4, 1),       1 action   ne 9 / nd 10   first shape past every <= 8 predicate; angles listed out of order
  w16    nx 12, angles (0, 3, 5, 8), 1 action   16 / 17        nd > 16: k_finalize instead of the tail's own sum
  w24    nx 16, angles 0 .. 7,       1 action   24 / 25        MMC_NX and MMC_NA together
  n13    nx 10, angle (2,),          2 actions  11 / 13        the _nd family past 8
  n28    nx 16, angles 0 .. 7,       4 actions  24 / 28        every limit at once
  mix11  nx 9,  angle (0,),          1 action, 4 latents  10 / 11   _nd_mixed past 8 (tests/test_coregionalized.py::_system)
  p1, p85, p128, p129   nx 6, angles (1, 4), policy M = 1, 85, 128, 129   ne 8 / nd 9: k_policy_match_small at d = DK = 8 with one
         centre, with an M that does not divide 256 (three threads per column, one idle), at MMS_MMAX, and one past it (general path)
  e1     nx 1, angle (0,)            2 / 3      no off-diagonal drift pair: the tail never finalizes
  b300   nx 4, angle (1,), B = 300   5 / 6      past the tail's 4096-slab bound in f64 while nd <= 16
Bars: the families' own -- f64 1e-7 of the per-quantity scale; f32 5e-4 (one action, _nd: tests/test_compose.py,
tests/test_no_encoder.py) and 2e-4 (mixed: tests/test_coregionalized.py).  Costs are compared PER STEP.  The CPU guards pin what the
parity tests rest on: the oracle rollouts are away from both ends of the cost and positive definite, the drift matches they visit
are well posed in f64 (literal oracle against the fused restatement, as tests/test_gpu_random_shapes.py), and reversing the
order of the listed angles moves the oracle by far more than any bar."""
import functools
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd import bijectors as tfb
from gpflowpilco_amd import dynamics, models as gp
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
from gpflowpilco_amd.synthetic import generate_covariance, make_svgp
from oracle import mm_compose_oracle as co
from oracle import mm_fused_ref as fr
from oracle import mm_oracle as mo
from tests import multiaction_oracle as mao
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, scale_err, to_dev

F64 = torch.float64
MD = 40
SCALE, SHIFT = (2.0, 1.5, 1.0, 1.2), (-0.5, -0.4, -0.6, -0.5)
F64_BAR = 1e-7
CASES = {
    "w9": dict(nx=7, active=(4, 1), nu=1, Mp=12, H=3, seed=200),
    "w16": dict(nx=12, active=(0, 3, 5, 8), nu=1, Mp=12, H=3, seed=210),
    "w24": dict(nx=16, active=tuple(range(8)), nu=1, Mp=12, H=2, seed=220),
    "n13": dict(nx=10, active=(2,), nu=2, Mp=12, H=3, seed=230),
    "n28": dict(nx=16, active=tuple(range(8)), nu=4, Mp=12, H=2, seed=240),
    "mix11": dict(nx=9, active=(0,), nu=1, Mp=12, H=3, seed=261, Lg=4),     # (250 .. 260 end nearer than 0.1 to the cost's zero end)
    "p1": dict(nx=6, active=(1, 4), nu=1, Mp=1, H=3, seed=260),
    "p85": dict(nx=6, active=(1, 4), nu=1, Mp=85, H=3, seed=270),
    "p128": dict(nx=6, active=(1, 4), nu=1, Mp=128, H=3, seed=280),
    "p129": dict(nx=6, active=(1, 4), nu=1, Mp=129, H=3, seed=290),
    "e1": dict(nx=1, active=(0,), nu=1, Mp=12, H=3, seed=300),
    "b300": dict(nx=4, active=(1,), nu=1, Mp=12, H=2, seed=310, B=300),
}
NAMES = tuple(CASES)


def _f32_bar(sy):
  return 2e-4 if sy["mixed"] else 5e-4


def _family(sy):
  """The entry family ``ops.ComposedRollout`` runs the case in."""
  return "nd_mixed" if sy["mixed"] else ("nd" if sy["nu"] > 1 else "one")


def _policy_fn(sy, pol_o):
  if sy["nu"] == 1 and not sy["mixed"]:
    return lambda st: co.mm_policy(st, pol_o, float(sy["scale"][0]), float(sy["shift"][0]))
  return lambda st: mao.mm_policy_nd(st, pol_o, sy["scale"], sy["shift"])


def _oracle(sy, active, H=None):
  """-> (loss [B], traj [(mu, S)] * H, step costs [H, B]) of the oracle rollout with the angles listed as ``active``."""
  H = sy["H"] if H is None else H
  loss, traj = co.policy_rollout_loss(sy["mu0"], sy["S0"], sy["drift_o"], sy["policy_fn"], active, sy["target"], sy["precis"], H,
                                      keep=True)
  steps = []
  for mu, S in traj:                                                   # pilco.py:199-205, one step at a time
    enc = co.mm_encoder((mu, S, True), active)["y"]
    steps.append(co.expected_gaussian_cost(enc[0], co.covariance(enc), sy["target"], sy["precis"]))
  steps = np.stack(steps)
  assert np.abs(steps.sum(0) - loss).max() <= 1e-13 * H
  return loss, traj, steps


@functools.lru_cache(maxsize=None)
def _system(name):
  """The numpy side of a case and its oracle rollout (computed once, shared, never modified)."""
  c = CASES[name]
  nx, active, nu, seed, B = c["nx"], c["active"], c["nu"], c["seed"], c.get("B", 3)
  na = len(active); ne = nx + na; nd = ne + nu
  mixed = "Lg" in c
  lo = 0.5 * max(1.0, np.sqrt(nd / 4.0))
  if mixed:                                                            # tests/test_coregionalized.py::_system
    drift_o = random_svgp_params(seed=seed, L=c["Lg"], M=MD, d=nd, whiten=True, ls_bounds=(lo, 3.0 * lo), mean=True, W_rows=nx)
    drift_o.W = np.random.default_rng(seed + 3).standard_normal((nx, c["Lg"]))        # signed, unnormalised
    drift_o.mean_c = 0.3 * drift_o.mean_c
  else:
    drift_o = oracle_params(make_svgp(nx, MD, nd, seed=seed, ls_bounds=(lo, 3.0 * lo)))
  drift_o.Z[..., ne:] = 4.0 * drift_o.Z[..., ne:] - 2.0                # action axes in [-2, 2]
  lp = 0.5 * max(1.0, np.sqrt(ne / 4.0))
  pol_o = random_svgp_params(seed=seed + 1, L=nu, M=c["Mp"], d=ne, whiten=True, ls_bounds=(lp, 2.4 * lp), mean=False,
                             separate_Z=False)
  pol_o.q_mu = 1.5 * pol_o.q_mu
  rng = np.random.default_rng(seed + 2)
  mu0 = rng.uniform(0.2, 0.7, (B, nx))
  S0 = generate_covariance(rng, nx, (B,), 0.15)
  A = rng.standard_normal((ne, ne))
  precis = A @ A.T / ne ** 2 + 0.5 * np.eye(ne) / ne
  target = np.linspace(0.3, 0.6, ne)
  sy = dict(c, name=name, B=B, na=na, ne=ne, nd=nd, mixed=mixed, drift_o=drift_o, pol_o=pol_o, mu0=mu0, S0=S0, target=target,
            precis=precis, scale=np.array(SCALE[:nu]), shift=np.array(SHIFT[:nu]))
  sy["policy_fn"] = _policy_fn(sy, pol_o)
  sy["loss_o"], sy["traj_o"], sy["cost_o"] = _oracle(sy, active)
  return sy


# ---- CPU guards ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_systems_are_well_posed(name):
  """The loss per step is away from both ends of the cost and every visited covariance is positive definite; at every drift input
  (m_d, S_dd) the oracle visits, the literal moment match and the algorithm-matched restatement agree on the CPU to a tenth of the
  f64 bar (in latent space, as tests/test_gpu_random_shapes.py): an f64 miss on the GPU is then the kernels', not the draw's."""
  sy = _system(name)
  H, active = sy["H"], sy["active"]
  ev = min(np.linalg.eigvalsh(S).min() for _, S in sy["traj_o"])
  print(f"wide {name}: loss per step {sy['cost_o'].min():.3f} .. {sy['cost_o'].max():.3f}, smallest trajectory eigenvalue {ev:.4f}")
  assert np.isfinite(sy["loss_o"]).all() and ev > 1e-3
  assert sy["loss_o"].max() < -0.05 * H and sy["loss_o"].min() > -0.999 * H
  assert sy["cost_o"].max() < -0.05 and sy["cost_o"].min() > -0.999
  import dataclasses
  p_lat = dataclasses.replace(sy["drift_o"], W=None, mean_c=None)
  pre = fr.precompute(p_lat)
  nb = min(sy["B"], 3)
  states = [(sy["mu0"], sy["S0"])] + list(sy["traj_o"][:-1])
  for h, (mu, S) in enumerate(states):
    enc = co.mm_encoder((mu[:nb], S[:nb], True), active)
    md, Sdd, _ = co.joint(sy["policy_fn"](enc["y"]))
    _, Slit, _ = mo.mm_gauss_svgp_mo(md, Sdd, p_lat, full_output_cov=True, model_uncertainty=True)
    _, Sfus, _ = fr.moment_match(md, Sdd, p_lat, *pre, model_uncertainty=True)
    gap = np.abs(Sfus - Slit).max() / np.abs(Slit).max()
    print(f"wide {name} step {h}: literal vs fused drift Sff {gap:.2e}")
    assert gap < 0.1 * F64_BAR, "ill-conditioned draw: fix the generator, not the tolerance"


@pytest.mark.parametrize("name", [n for n in NAMES if len(CASES[n]["active"]) >= 2])
def test_the_order_of_the_angles_matters(name):
  """Listing the active dims in reverse order moves the oracle's per-step costs, means and covariances by at least 10x the f32
  bar: a tail that confused ``active`` with sorted order, or ``slot`` with ``inactive``, cannot pass the parity test."""
  sy = _system(name)
  _, traj, cost = _oracle(sy, tuple(reversed(sy["active"])), H=2)
  assert tuple(reversed(sy["active"])) != tuple(sy["active"])
  moves = dict(cost=max(scale_err(cost[h], sy["cost_o"][h]) for h in range(2)),
               mean=max(scale_err(traj[h][0], sy["traj_o"][h][0]) for h in range(2)),
               cov=max(scale_err(traj[h][1], sy["traj_o"][h][1]) for h in range(2)))
  print(f"wide {name}: reversed angles move the oracle by {moves}")
  assert min(moves.values()) >= 10 * _f32_bar(sy), moves


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _rollout(sy, device, dtype):
  from gpflowpilco_amd import ops
  d = sy["drift_o"]
  drift = gp_model_from_oracle(d, device)
  pol_model = gp_model_from_oracle(sy["pol_o"], device)
  fam = _family(sy)
  head = dict(head_scale=float(sy["scale"][0]), head_shift=float(sy["shift"][0])) if sy["nu"] == 1 else \
      dict(head_scale=tuple(sy["scale"]), head_shift=tuple(sy["shift"]))
  mix = dict(mix_W=to_dev(d.W, device, F64), mix_c=to_dev(d.mean_c, device, F64)) if fam == "nd_mixed" else {}
  roll = ops.ComposedRollout(drift.packed(dtype, True, device), pol_model.packed(dtype, False, device), nx=sy["nx"],
                             active_dims=sy["active"], target=to_dev(sy["target"], device, dtype),
                             precis=to_dev(sy["precis"], device, dtype), **head, **mix)
  assert roll._family.name == fam and (roll.na, roll.ne, roll.nd) == (sy["na"], sy["ne"], sy["nd"])
  return roll


def _forward_errors(sy, out):
  """Worst error of the per-step costs, the trajectory means and the trajectory covariances, each step against its own scale."""
  _, _, cost, tmu, tS = out
  H = sy["H"]
  assert cost.shape == (sy["B"], H) and tmu.shape == (H, sy["B"], sy["nx"])
  return dict(cost=max(scale_err(cost[:, h], sy["cost_o"][h]) for h in range(H)),
              mean=max(scale_err(tmu[h], sy["traj_o"][h][0]) for h in range(H)),
              cov=max(scale_err(tS[h], sy["traj_o"][h][1]) for h in range(H)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_wide_forward_matches_the_oracle(name, dtype, device):
  sy = _system(name)
  roll = _rollout(sy, device, dtype)
  if sy["ne"] > 8:                                                     # forward only: the reverse sweeps keep their ne <= 8 bound
    assert not roll.supports_backward() and not roll.supports_backward_nd()
  mx, Sxx = to_dev(sy["mu0"], device, dtype), to_dev(sy["S0"], device, dtype)
  out = roll(mx, Sxx, sy["H"], keep_trajectory=True)
  roll.drift.check_status(sy["B"])
  errs = _forward_errors(sy, out)
  print(f"wide forward {name} {dtype}: cost {errs['cost']:.3e} mean {errs['mean']:.3e} cov {errs['cov']:.3e}")
  tol = F64_BAR if dtype == torch.float64 else _f32_bar(sy)
  assert max(errs.values()) < tol, errs
  m_H, S_H, _, tmu, tS = out
  assert torch.equal(m_H, tmu[-1]) and torch.equal(S_H, tS[-1])
  assert torch.equal(mx, to_dev(sy["mu0"], device, dtype))              # the inputs are not modified


def _torch_system(sy, device):
  drift = gp_model_from_oracle(sy["drift_o"], device)
  pol_model = gp_model_from_oracle(sy["pol_o"], device)
  if sy["nu"] == 1:
    head = [tfb.Scale(float(sy["scale"][0])), tfb.Shift(float(sy["shift"][0])), tfb.NormalCDF()]
  else:
    head = [tfb.Scale(to_dev(sy["scale"], device, F64)), tfb.Shift(to_dev(sy["shift"], device, F64)), tfb.NormalCDF()]
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol_model), invlink=tfb.Chain(head))
  objective = GaussianObjective(target=to_dev(sy["target"], device, F64), precis=to_dev(sy["precis"], device, F64))
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=TrigonometricEncoder(active_dims=sy["active"]),
                                    solver=dynamics.MomentMatchingEuler())
  return system, objective


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_closure_takes_the_wide_shape(name, device):
  """The public route: ``loops.policy_loss_closure(..., native=True)`` takes every case (no fall-back warning) and returns the
  oracle's loss; for w16 and n28 it is the direct rollout's loss bit for bit."""
  from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
  sy = _system(name)
  system, objective = _torch_system(sy, device)
  kw = {}
  if sy["mixed"]:
    kw["native_coregionalized"] = True
  if sy["nu"] > 1:
    kw["native_actions"] = sy["nu"]
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    loss = policy_loss_closure(system, objective, get_state_initializer(mx, Sxx), sy["H"], native=True, **kw)()
  err = scale_err(loss, sy["loss_o"])
  print(f"wide closure {name}: loss {err:.3e}")
  assert loss.shape == (sy["B"],) and err < F64_BAR
  if name in ("w16", "n28"):
    _, _, cost = _rollout(sy, device, F64)(mx, Sxx, sy["H"])
    assert torch.equal(loss, cost.sum(1))
