"""Caller-defined objectives on the native moment-matched rollout (``native_objective=True``): the seeded reverse sweeps
``mm_rollout_composed_backward_seeded`` / ``_nd_seeded`` (csrc/mm_compose_bwd.hip, csrc/mm_compose_bwd_nd.hip),
``autodiff.ComposedTrajectoryFunction`` and the routing of ``loops.policy_loss_closure``.

Systems: the cart-pole-shaped system of tests/test_gpu_backward.py (nx 4, one angle, drift M 60, policy M 30, B 2) and system A of
tests/test_multiaction_grad.py (two actions, B 3); H = 4, f64.  The objective is defined here:
    (1 + 0.1 t) [ (m - tau)^T W (m - tau) + tr(W S) ]      on the encoded state
with tensors W (symmetric positive definite) and tau, so that the mean and the covariance seeds of every step are non-zero and
differ from step to step.  The reference is the torch composition of the same closure (``native=False``); the bars are those of
tests/test_gpu_backward.py:356-359: loss 1e-9, every parameter group 1e-7 of its largest entry."""
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd.components import GaussianObjective
from tests.helpers import scale_err, to_dev

F64 = torch.float64
H4 = 4
WEIGHTS = (1.0, 0.6, 0.8)
pytestmark = pytest.mark.gpu


class QuadraticObjective:
  """(1 + 0.1 t) [(m - tau)^T W (m - tau) + tr(W S)]; ``reverse``: the time weights of steps 1 .. H in reverse order."""

  def __init__(self, W, tau, reverse=False):
    self.W, self.tau, self.reverse = W, tau, reverse

  def __call__(self, x, t=None):
    m, S = x.mean(), x.covariance(dense=True)
    e = m - self.tau
    wt = 1.0 + 0.1 * ((H4 + 1 - t) if self.reverse else t)
    return wt * ((e * (e @ self.W)).sum(-1) + (self.W * S).sum((-1, -2)))


def _case(name, device):
  """-> (system, default GaussianObjective, {group: parameter}, m0, S0, nu), every leaf requiring a gradient."""
  if name == "cartpole":
    from tests.test_gpu_backward import _cartpole_like
    system, objective, params, m0, S0, _ = _cartpole_like(device, 30)
    nu = 1
  else:
    from tests.test_multiaction import _system
    from tests.test_multiaction_grad import _setup
    system, objective, _, _, params, m0, S0 = _setup(_system("A", H4), device)
    nu = 2
  m0 = m0.detach().clone().requires_grad_(True); S0 = S0.detach().clone().requires_grad_(True)
  return system, objective, params, m0, S0, nu


def _quadratic(system, m0, device, seed=5, reverse=False):
  ne = m0.shape[-1] + len(system.encoder.active_dims)
  rng = np.random.default_rng(seed)
  A = rng.standard_normal((ne, ne))
  W = to_dev(A @ A.T / ne + 0.5 * np.eye(ne), device, F64)
  tau = to_dev(rng.uniform(0.0, 0.5, ne), device, F64)
  return QuadraticObjective(W, tau, reverse)


def _grads(system, objective, params, m0, S0, extra=(), **kw):
  from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
  leaves = list(params.values()) + [m0, S0] + list(extra)
  for t in leaves:
    t.grad = None
  loss = policy_loss_closure(system, objective, get_state_initializer(m0, S0), H4, **kw)()
  wts = torch.tensor(WEIGHTS[:loss.shape[0]], dtype=loss.dtype, device=loss.device)
  (loss * wts).sum().backward()
  out = {k: t.grad.detach().clone() for k, t in params.items()}
  out["m0"], out["S0"] = m0.grad.detach().clone(), 0.5 * (S0.grad + S0.grad.transpose(1, 2)).detach()
  for i, t in enumerate(extra):
    out[f"extra{i}"] = t.grad.detach().clone()
  return loss.detach(), out


def _group_err(got, want):
  return float((got - want).abs().max()) / max(1e-12, float(want.abs().max()))


def _compare(gn, gt, tag, bar=1e-7):
  for k in gt:
    err = _group_err(gn[k], gt[k])
    print(f"{tag} {k}: native objective route vs torch composition {err:.2e}")
    assert float(gt[k].abs().max()) > 0.0 and err < bar, (k, err)


@pytest.mark.parametrize("name", ["cartpole", "A"])
def test_custom_objective_on_the_native_rollout(name, device):
  from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
  system, _, params, m0, S0, nu = _case(name, device)
  obj = _quadratic(system, m0, device)
  kw = dict(native_objective=True, native_actions=nu)
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)                     # no fall-back
    loss_n, gn = _grads(system, obj, params, m0, S0, **kw)
    with torch.no_grad():
      loss_f = policy_loss_closure(system, obj, get_state_initializer(m0, S0), H4, **kw)()
  loss_t, gt = _grads(system, obj, params, m0, S0, native=False)
  # timing guard, on the comparator alone: with the time weights reversed its q_mu gradient moves by >= 10 x the bar, so a sweep
  # that applied a seed one step off could not pass
  _, gr = _grads(system, _quadratic(system, m0, device, reverse=True), params, m0, S0, native=False)
  moved = _group_err(gr["q_mu"], gt["q_mu"])
  print(f"timing guard {name}: reversed time weights move the comparator's q_mu gradient by {moved:.2e}")
  assert moved >= 10 * 1e-7
  assert float((loss_n - loss_t).abs().max()) < 1e-9
  _compare(gn, gt, name)
  assert float((loss_f - loss_n).abs().max()) <= 1e-12 * float(loss_n.abs().max())
  # the objective's own parameter: its gradient comes from the torch part
  obj.W.requires_grad_(True)
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)
    loss_w, gw = _grads(system, obj, params, m0, S0, extra=(obj.W,), **kw)
  loss_tw, gtw = _grads(system, obj, params, m0, S0, extra=(obj.W,), native=False)
  assert float((loss_w - loss_tw).abs().max()) < 1e-9
  _compare(gw, gtw, name + " (W trained)")
  obj.W.requires_grad_(False)
  # with the option off the closure warns once and takes the torch composition, as before
  with pytest.warns(RuntimeWarning, match="objective QuadraticObjective") as rec:
    loss_d, gd = _grads(system, obj, params, m0, S0, native_actions=nu)
  assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
  assert torch.equal(loss_d, loss_t) and all(torch.equal(gd[k], gt[k]) for k in gt)


@pytest.mark.parametrize("name", ["cartpole", "A"])
def test_gaussian_objective_with_a_trained_target_through_the_trajectory_route(name, device):
  system, objective, params, m0, S0, nu = _case(name, device)
  objective = GaussianObjective(target=objective.target.detach().clone().requires_grad_(True), precis=objective.precis)
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)
    loss_n, gn = _grads(system, objective, params, m0, S0, extra=(objective.target,), native_objective=True, native_actions=nu)
  loss_t, gt = _grads(system, objective, params, m0, S0, extra=(objective.target,), native=False)
  assert float((loss_n - loss_t).abs().max()) < 1e-9
  _compare(gn, gt, name + " (Gaussian, target trained)")
  # the option off: the pinned warning and the torch composition (tests/test_gpu_backward.py)
  with pytest.warns(RuntimeWarning, match="objective.target requires a gradient"):
    loss_d, gd = _grads(system, objective, params, m0, S0, extra=(objective.target,), native_actions=nu)
  assert torch.equal(loss_d, loss_t) and all(torch.equal(gd[k], gt[k]) for k in gt)


def _tape(name, device):
  system, objective, params, m0, S0, nu = _case(name, device)
  from gpflowpilco_amd import ops
  pm_ = system.policy.model.model
  scale, shift = system.policy.invlink.bijectors[0].scale, system.policy.invlink.bijectors[1].shift
  as_head = lambda v: (float(v) if nu == 1 else tuple(float(t) for t in v.reshape(-1).tolist()))
  roll = ops.ComposedRollout(system.drift.packed(F64, True, device), pm_.packed(F64, False, device), nx=m0.shape[-1],
                             active_dims=system.encoder.active_dims, head_scale=as_head(scale), head_shift=as_head(shift),
                             target=objective.target, precis=objective.precis)
  taped = roll.taped if nu == 1 else roll.taped_nd
  _, _, cost, tape = taped(m0.detach(), S0.detach(), H4)
  B = m0.shape[0]
  g = torch.Generator(device="cpu").manual_seed(3)
  g_cost = torch.randn(H4, B, dtype=F64, generator=g).to(device)
  g_xm = torch.randn(H4, B, roll.nx, dtype=F64, generator=g).to(device)
  g_xS = torch.randn(H4, B, roll.nx, roll.nx, dtype=F64, generator=g).to(device)
  return roll, tape, B, g_cost, g_xm, g_xS, (roll.backward if nu == 1 else roll.backward_nd)


@pytest.mark.parametrize("name", ["cartpole", "A"])
def test_seeded_entries_with_null_seeds_and_with_seeds(name, device):
  roll, tape, B, g_cost, g_xm, g_xS, sweep = _tape(name, device)
  plain = sweep(tape, g_cost, B, H4)
  null = sweep(tape, g_cost, B, H4, g_traj=(None, None))                 # the seeded entry, null seeds
  assert all(torch.equal(a, b) for a, b in zip(plain, null)) and float(plain[0].abs().max()) > 0.0
  g_xS = 0.5 * (g_xS + g_xS.transpose(-1, -2))
  seeded = sweep(tape, g_cost, B, H4, g_traj=(g_xm, g_xS))
  for b, c in zip(seeded, plain):
    assert float((b - c).abs().max()) > 1e-3 * float(c.abs().max())       # the seeds are felt
  again = sweep(tape, g_cost, B, H4, g_traj=(g_xm, g_xS))
  assert all(torch.equal(a, b) for a, b in zip(seeded, again))             # two sweeps over one tape are bit-equal
  # the sweep is linear in its seeds: (g_cost, seeds) = (g_cost, 0) + (0, seeds)
  only = sweep(tape, torch.zeros_like(g_cost), B, H4, g_traj=(g_xm, g_xS))
  for a, b, c in zip(seeded, plain, only):
    assert float((a - b - c).abs().max()) <= 1e-12 * max(float(b.abs().max()), float(c.abs().max()))
  with pytest.raises(ValueError):
    sweep(tape, g_cost, B, H4, g_traj=(g_xm, None))
  with pytest.raises(ValueError):
    sweep(tape, g_cost, B, H4, g_traj=(g_xm[:-1], g_xS[:-1]))


def test_trajectory_function_symmetrises_its_covariance_seed(device):
  """``autodiff.ComposedTrajectoryFunction``: outputs read off the tape, and an objective whose gradient w.r.t. S_t is
  unsymmetric gives the parameter gradients of its symmetric part."""
  from gpflowpilco_amd.autodiff import ComposedTrajectoryFunction
  system, objective, params, m0, S0, nu = _case("cartpole", device)
  roll, tape, B, g_cost, g_xm, g_xS, _ = _tape("cartpole", device)
  pm_ = system.policy.model.model
  tm, tS = roll(m0.detach(), S0.detach(), H4, keep_trajectory=True)[3:]

  def grads(G):
    for t in params.values():
      t.grad = None
    Zp, lsp, varp, betap, _, mcp = pm_.precompute(device)
    mcp = torch.zeros(1, dtype=F64, device=device) if mcp is None else mcp
    cost, xm, xS = ComposedTrajectoryFunction.apply(m0.detach(), S0.detach(), Zp, lsp, varp, betap, mcp, roll, H4, 1.0)
    assert cost.shape == (B, H4) and xm.shape == (B, H4, roll.nx) and xS.shape == (B, H4, roll.nx, roll.nx)
    # (taped and untaped forward sum the drift's covariance in different orders; each holds the f64 bar 1e-7 against the oracle)
    assert scale_err(xm, tm.transpose(0, 1).cpu().numpy()) < 2e-7 and scale_err(xS, tS.transpose(0, 1).cpu().numpy()) < 2e-7
    ((xm * g_xm.transpose(0, 1)).sum() + (xS * G.transpose(0, 1)).sum()).backward()
    return [t.grad.detach().clone() for t in params.values()]
  a = grads(g_xS)
  b = grads(0.5 * (g_xS + g_xS.transpose(-1, -2)))
  for u, v in zip(a, b):
    assert float(v.abs().max()) > 0.0 and float((u - v).abs().max()) <= 1e-12 * float(v.abs().max())


def test_graphed_custom_objective_replays_eager(device):
  from gpflowpilco_amd.loops import GraphedPolicyLoss, get_state_initializer, policy_loss_closure
  system, _, params, m0, S0, nu = _case("cartpole", device)
  m0, S0 = m0.detach(), S0.detach()
  obj = _quadratic(system, m0, device)
  q_mu = params["q_mu"]
  for k, t in params.items():
    t.requires_grad_(k == "q_mu")
  closure = policy_loss_closure(system, obj, get_state_initializer(m0, S0), H4, native=True, native_objective=True)
  graphed = GraphedPolicyLoss(closure, [q_mu])
  for _ in range(2):
    q_mu.grad = None
    le = closure(); le.sum().backward()
    ge = q_mu.grad.detach().clone(); le = le.detach().clone()
    lg, (gg,) = graphed.loss_and_grad()
    assert torch.allclose(lg, le, rtol=1e-12, atol=1e-14) and torch.allclose(gg, ge, rtol=1e-10, atol=1e-13)
    assert torch.allclose(graphed.loss(), le, rtol=1e-12, atol=1e-14)
    with torch.no_grad():
      q_mu.mul_(0.9)
      m0.add_(0.01)
  graphed.check()
