"""The native moment-matched policy gradient for 2 to 4 actions: the tape ``mm_rollout_composed_taped_nd`` and the reverse sweep
``mm_rollout_composed_backward_nd`` (csrc/mm_compose_nd.hip, csrc/mm_compose_bwd_nd.hip), opt-in through ``native_actions=``.

The systems are A and B of tests/test_multiaction.py (A: nx 4, angles (0, 1), two actions, drift M 100, policy M 30, B 3;
B: nx 3, one angle, three actions, drift M 60), all f64.  The references are the torch composition of the same rollout (autograd
through ``special.bvn_cdf``'s closed-form gradient) and central differences of the numpy oracle loss; the bars are those of
tests/test_gpu_backward.py::test_native_policy_gradient_at_H30_all_parameters_and_initial_state."""
import copy
import ctypes
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib
from gpflowpilco_amd import bijectors as tfb
from gpflowpilco_amd import dynamics, models as gp
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
from gpflowpilco_amd.special import ndtr
from gpflowpilco_amd.synthetic import generate_covariance, make_svgp
from oracle import mm_compose_oracle as co
from tests import multiaction_oracle as mao
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, scale_err, to_dev
from tests.test_multiaction import _rollout, _system, _torch_system

F64 = torch.float64
WEIGHTS = (1.0, 0.6, 0.8)


# ---- CPU: sizes and argument validation ----------------------------------------------------------------------------------
def test_size_functions_of_the_multi_action_gradient_entries_without_gpu():
  lib = _lib.lib()
  F64c, F32c = _lib.MM_F64, _lib.MM_F32
  assert lib.mm_abi_version() == 2
  # nu = 1: the one-action tape (one shared layout function)
  assert lib.mm_compose_tape_bytes_nd(3, 30, 4, 2, 1, 100, F64c) == lib.mm_compose_tape_bytes(3, 30, 4, 2, 100, F64c)
  tA = lib.mm_compose_tape_bytes_nd(3, 30, 4, 2, 2, 100, F64c)
  assert tA > lib.mm_compose_tape_bytes(3, 30, 4, 2, 100, F64c)
  assert lib.mm_compose_tape_bytes_nd(3, 30, 4, 2, 2, 100, F32c) == 0                   # f64 tapes only
  assert lib.mm_compose_tape_bytes_nd(3, 30, 4, 2, 0, 100, F64c) == 0 and lib.mm_compose_tape_bytes_nd(3, 30, 4, 2, 5, 100, F64c) == 0
  assert lib.mm_compose_tape_bytes_nd(3, 0, 4, 2, 2, 100, F64c) == 0 and lib.mm_compose_tape_bytes_nd(3, 30, 16, 16, 4, 100, F64c) == 0
  # the tape keeps the drift's per-step blocks by the one-action rule: both at B = 64, the workspace alone at 128, neither at 256
  per = [lib.mm_compose_tape_bytes_nd(B, 30, 4, 2, 2, 100, F64c) / B for B in (64, 128, 256)]
  assert per[0] > 1.5 * per[1] > 1.5 * 1.5 * per[2] > 0
  # the reverse sweep takes every policy with M <= 64 on ne <= 8 dims with up to 4 actions
  for nx, na in ((6, 2), (4, 4), (4, 2), (3, 1), (2, 2)):
    for nu in (1, 2, 3, 4):
      for M in (1, 30, 64):
        assert lib.mm_compose_backward_workspace_bytes_nd(3, nx, na, nu, 100, M) > 0, (nx, na, nu, M)
  w = lib.mm_compose_backward_workspace_bytes_nd
  assert w(3, 6, 2, 4, 100, 166) > 0 and w(3, 6, 2, 4, 100, 167) == 0                   # the LDS bound at ne = 8
  assert w(3, 4, 2, 2, 100, 219) > 0 and w(3, 4, 2, 2, 100, 256) == 0                   # ... at ne = 6
  assert w(3, 2, 2, 4, 100, 256) > 0 and w(3, 2, 2, 4, 100, 257) == 0                   # M <= 256: the pack keeps the centres' order
  assert w(3, 6, 3, 2, 100, 30) == 0                                                     # ne = 9
  assert w(3, 4, 2, 5, 100, 30) == 0 and w(3, 4, 2, 0, 100, 30) == 0 and w(0, 4, 2, 2, 100, 30) == 0
  assert w(6, 4, 2, 2, 100, 30) > w(3, 4, 2, 2, 100, 30)
  assert lib.mm_policy_grad_bytes_nd(2, 3, 30, 5) == 2 * 3 * (30 * 5 + 30 + 5 + 2) * 8
  assert lib.mm_policy_grad_bytes_nd(2, 1, 30, 5) == lib.mm_policy_grad_bytes(2, 30, 5)
  assert lib.mm_policy_grad_bytes_nd(2, 5, 30, 5) == 0 and lib.mm_policy_grad_bytes_nd(0, 2, 30, 5) == 0


def test_argument_validation_of_the_multi_action_gradient_entries_without_gpu():
  lib = _lib.lib()
  buf = (ctypes.c_char * 64)()
  p = ctypes.addressof(buf)
  F64c, F32c = _lib.MM_F64, _lib.MM_F32
  act = (ctypes.c_int32 * 2)(0, 1)
  sc = (ctypes.c_double * 4)(2.0, 1.5, 1.0, 1.0)
  sh = (ctypes.c_double * 4)(-0.5, -0.4, -0.6, 0.0)
  tA = lib.mm_compose_tape_bytes_nd(3, 30, 4, 2, 2, 100, F64c)
  wA = lib.mm_compose_backward_workspace_bytes_nd(3, 4, 2, 2, 100, 30)
  big = 1 << 40

  def targs(nu=2, drift_d=8, pol_d=6, dtype=F64c, drift=p, scale=sc, wd=p, wp=p, tape=p, tape_bytes=big):
    return (drift, 64, 4, 100, drift_d, p, 64, 30, pol_d, dtype, 3, 30, 1.0, 4, 2, act, nu, scale, sh, p, p,
            p, p, p, wd, 64, wp, 64, tape, tape_bytes, None, None)
  f = lib.mm_rollout_composed_taped_nd
  assert f(*targs(nu=0)) == -2 and f(*targs(nu=5)) == -2                              # MM_E_DIM
  assert f(*targs(drift=None)) == -1 and f(*targs(scale=None)) == -1                  # MM_E_ARG
  assert f(*targs(wd=None)) == -1 and f(*targs(wp=None)) == -1 and f(*targs(tape=None)) == -1
  assert f(*targs(dtype=F32c)) == -3 and f(*targs(dtype=7)) == -3                     # MM_E_DTYPE: f64 tapes only
  assert f(*targs(drift_d=7)) == -6 and f(*targs(pol_d=5)) == -6                      # MM_E_STATE
  assert f(*targs(tape_bytes=tA - 1)) == -4                                           # tape too small
  assert f(*targs(tape_bytes=tA)) == -4                                               # ... then the matches' workspaces (64 bytes)

  def bargs(nu=2, drift_d=8, pol_d=6, pol_M=30, dtype=F64c, drift=p, scale=sc, tape=p, tape_bytes=big, gpol=p, gm=None, gS=None,
            wd=p, wb=p, wb_bytes=big):
    return (drift, 64, 4, 100, drift_d, p, 64, pol_M, pol_d, dtype, 3, 30, 1.0, 4, 2, act, nu, scale, sh, p, p,
            tape, tape_bytes, p, gpol, gm, gS, wd, 64, wb, wb_bytes, None, None)
  g = lib.mm_rollout_composed_backward_nd
  assert g(*bargs(nu=0)) == -2 and g(*bargs(nu=5)) == -2                              # MM_E_DIM
  assert g(*bargs(pol_M=256)) == -2 and g(*bargs(pol_M=300)) == -2                    # ... past the LDS bound
  assert g(*bargs(drift=None)) == -1 and g(*bargs(scale=None)) == -1 and g(*bargs(tape=None)) == -1
  assert g(*bargs(gpol=None)) == -1 and g(*bargs(wd=None)) == -1 and g(*bargs(wb=None)) == -1
  assert g(*bargs(gm=p)) == -1 and g(*bargs(gS=p)) == -1                              # both state gradients or neither
  assert g(*bargs(dtype=F32c)) == -3                                                  # f64 only
  assert g(*bargs(drift_d=7)) == -6 and g(*bargs(pol_d=5)) == -6
  assert g(*bargs(tape_bytes=tA - 1)) == -4 and g(*bargs(wb_bytes=wA - 1)) == -4
  assert g(*bargs(tape_bytes=tA, wb_bytes=wA)) == -4                                  # ... then the drift's workspace / the packs


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _trainable(pol_model, nu):
  """Every policy parameter group: q_mu and each latent's inducing inputs, lengthscales and variance."""
  out = {"q_mu": pol_model.q_mu}
  for a in range(nu):
    kern = pol_model.kernel.kernels[a]
    out[f"Z{a}"] = pol_model.inducing_variable.inducing_variables[a].Z
    out[f"ls{a}"] = kern.lengthscales
    out[f"var{a}"] = kern.variance
  for t in out.values():
    t.requires_grad_(True)
  return out


def _grads(system, objective, params, m0, S0, H, **kw):
  """-> (loss [B] numpy, {group: gradient of the weighted loss}); ``kw``: native= / native_actions= of the closure."""
  from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
  leaves = list(params.values()) + [t for t in (m0, S0) if t.requires_grad]
  for t in leaves:
    t.grad = None
  loss = policy_loss_closure(system, objective, get_state_initializer(m0, S0), H, **kw)()
  wts = torch.tensor(WEIGHTS[:loss.shape[0]], dtype=loss.dtype, device=loss.device)
  (loss * wts).sum().backward()
  out = {k: t.grad.detach().clone() for k, t in params.items()}
  if m0.requires_grad:
    out["m0"], out["S0"] = m0.grad.detach().clone(), 0.5 * (S0.grad + S0.grad.transpose(1, 2)).detach()
  return loss.detach().cpu().numpy(), out


def _group_err(got, want):
  return float((got - want).abs().max()) / max(1e-12, float(want.abs().max()))


def _setup(sy, device, state_grad=True):
  system, objective, drift, pol_model = _torch_system(sy, device, F64)
  params = _trainable(pol_model, sy["nu"])
  m0 = to_dev(sy["mu0"], device, F64).requires_grad_(state_grad)
  S0 = to_dev(sy["S0"], device, F64).requires_grad_(state_grad)
  return system, objective, drift, pol_model, params, m0, S0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_gpu_taped_forward_equals_the_untaped_forward(name, device):
  sy = _system(name, 30)
  roll = _rollout(sy, device, F64)
  assert roll.supports_backward_nd() and not roll.supports_backward()
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  m_H, S_H, cost = roll(mx, Sxx, 30)
  m_t, S_t, cost_t, tape = roll.taped_nd(mx, Sxx, 30)
  roll.drift.check_status(3)
  assert cost_t.shape == (30, 3)
  errs = (scale_err(m_t, m_H.cpu().numpy()), scale_err(S_t, S_H.cpu().numpy()), scale_err(cost_t.T, cost.cpu().numpy()))
  print(f"taped vs untaped {name}: {errs}")
  assert max(errs) < 1e-12
  assert scale_err(cost_t.sum(0), sy["loss_o"]) < 1e-7
  assert torch.equal(mx, to_dev(sy["mu0"], device, F64))                          # the inputs are not modified
  with pytest.raises(NotImplementedError):
    roll.taped(mx, Sxx, 30)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_gpu_native_gradient_matches_the_torch_composition(name, device, monkeypatch):
  """H = 8, every parameter group and the initial state: native (native_actions = nu) against the torch composition; and the
  torch composition with the bivariate term replaced by Phi(h) Phi(k) is at least 1e-3 away in every group, so a sweep that
  dropped the correlation between the latents could not pass at 1e-7."""
  sy = _system(name, 8)
  nu = sy["nu"]
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")                                                # no fall-back warning
    loss_n, gn = _grads(system, objective, params, m0, S0, 8, native_actions=nu)
  loss_t, gt = _grads(system, objective, params, m0, S0, 8, native=False)
  drift.packed(F64, True, device).check_status(3)
  print(f"gradient {name}: loss err {np.abs(loss_n - loss_t).max():.2e}")
  assert np.abs(loss_n - loss_t).max() < 1e-9
  assert scale_err(loss_n, sy["loss_o"]) < 1e-7
  for k in gt:
    err = _group_err(gn[k], gt[k])
    print(f"gradient {name} {k}: native vs torch composition {err:.2e}")
    assert err < 1e-7, (k, err)
  # the default closure keeps today's routing: one "nu > 1" warning, the torch composition
  with pytest.warns(RuntimeWarning, match=r"nu > 1") as rec:
    loss_d, gd = _grads(system, objective, params, m0, S0, 8)
  assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
  assert all(torch.equal(gd[k], gt[k]) for k in gt)
  # guard: the head without the correlation
  from gpflowpilco_amd.moment_matching import bijectors as mmb
  monkeypatch.setattr(mmb, "bvn_cdf", lambda h, k, rho: ndtr(h) * ndtr(k) + 0.0 * rho)
  _, gp_ = _grads(system, objective, params, m0, S0, 8, native=False)
  monkeypatch.undo()
  for k in gt:
    far = _group_err(gp_[k], gt[k])
    print(f"guard {name} {k}: product-instead-of-BVN moves the gradient by {far:.2e}")
    assert far >= 1e-3, (k, far)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_gpu_native_gradient_matches_finite_differences_of_the_oracle(name, device):
  sy = _system(name, 3)
  nu, H = sy["nu"], 3
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    loss, g = _grads(system, objective, params, m0, S0, H, native_actions=nu)
  wts = np.array(WEIGHTS[:3])

  def oracle_loss(q_mu=None, Z=None, ls=None, mu0=None):
    pol = copy.copy(sy["pol_o"])
    if q_mu is not None: pol.q_mu = q_mu
    if Z is not None: pol.Z = Z
    if ls is not None: pol.lengthscales = ls
    fn = lambda st: mao.mm_policy_nd(st, pol, sy["scale"], sy["shift"])
    l = co.policy_rollout_loss(sy["mu0"] if mu0 is None else mu0, sy["S0"], sy["drift_o"], fn, sy["active"], sy["target"],
                               sy["precis"], H)
    return float((wts * l).sum())
  assert abs(oracle_loss() - float((wts * loss).sum())) < 1e-7 * max(1.0, abs(oracle_loss()))
  eps = 1e-5

  def fd(name_, arr, idx):
    ap, am = arr.copy(), arr.copy(); ap[idx] += eps; am[idx] -= eps
    return (oracle_loss(**{name_: ap}) - oracle_loss(**{name_: am})) / (2 * eps)
  last = nu - 1
  checks = [(f"q_mu[{m},{a}]", fd("q_mu", sy["pol_o"].q_mu, (m, a)), g["q_mu"][m, a]) for a in range(nu) for m in (0, 11, 29)]
  checks += [(f"Z{last}[7,2]", fd("Z", sy["pol_o"].Z, (last, 7, 2)), g[f"Z{last}"][7, 2]),
             (f"ls{last}[1]", fd("ls", sy["pol_o"].lengthscales, (last, 1)), g[f"ls{last}"][1]),
             ("m0[1,2]", fd("mu0", sy["mu0"], (1, 2)), g["m0"][1, 2])]
  for what, want, got in checks:
    print(f"finite differences {name} {what}: native {float(got):+.8e} fd {want:+.8e}")
    assert abs(float(got) - want) < 2e-5 * max(1.0, abs(want)), (what, float(got), want)


@pytest.mark.gpu
def test_gpu_four_actions(device):
  """nx 2, both angles (ne 4), four actions (nd 8), drift M 40, policy M 12, H 4, B 2: six pair adjoints per step."""
  s, nx, active, nu, H = 50, 2, (0, 1), 4, 4
  ne, nd = 4, 8
  drift_o = oracle_params(make_svgp(nx, 40, nd, seed=s, ls_bounds=(0.8, 3.0)))
  drift_o.Z[..., ne:] = 4.0 * drift_o.Z[..., ne:] - 2.0
  pol_o = random_svgp_params(seed=s + 1, L=nu, M=12, d=ne, whiten=True, ls_bounds=(0.3, 0.8), mean=False)
  pol_o.q_mu = 2.0 * pol_o.q_mu
  rng = np.random.default_rng(s + 2)
  mu0 = rng.uniform(0.0, 0.6, (2, nx)); S0n = generate_covariance(rng, nx, (2,), 0.3)
  A = rng.standard_normal((ne, ne))
  sy = dict(nx=nx, active=active, nu=nu, drift_o=drift_o, pol_o=pol_o, mu0=mu0, S0=S0n, target=np.array([0.0, 0.0, 1.0, 1.0]),
            precis=A @ A.T / ne, scale=np.array([2.0, 1.5, 1.0, 1.2]), shift=np.array([-0.5, -0.4, -0.6, -0.5]))
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    loss_n, gn = _grads(system, objective, params, m0, S0, H, native_actions=4)
  loss_t, gt = _grads(system, objective, params, m0, S0, H, native=False)
  drift.packed(F64, True, device).check_status(2)
  assert np.abs(loss_n - loss_t).max() < 1e-9
  for k in gt:
    err = _group_err(gn[k], gt[k])
    print(f"four actions {k}: native vs torch composition {err:.2e}")
    assert err < 1e-7, (k, err)


@pytest.mark.gpu
def test_gpu_largest_guaranteed_shape_takes_the_raised_lds_limit(device):
  """Policy M = 64 on ne = 8 encoded dims (nx 6, two angles) with four actions: the corner of the shapes the sweep always takes,
  88 KB of LDS per workgroup, i.e. past the 64 KB default (the entry raises the kernel's limit).  H 2, B 2, drift M 40 on nd = 12."""
  s, nx, active, nu, H = 60, 6, (0, 1), 4, 2
  ne, nd = 8, 12
  assert _lib.lib().mm_compose_backward_workspace_bytes_nd(2, nx, 2, nu, 40, 64) > 0
  drift_o = oracle_params(make_svgp(nx, 40, nd, seed=s, ls_bounds=(0.8, 3.0)))
  drift_o.Z[..., ne:] = 4.0 * drift_o.Z[..., ne:] - 2.0
  pol_o = random_svgp_params(seed=s + 1, L=nu, M=64, d=ne, whiten=True, ls_bounds=(0.5, 1.2), mean=False)
  rng = np.random.default_rng(s + 2)
  mu0 = rng.uniform(0.0, 0.6, (2, nx)); S0n = generate_covariance(rng, nx, (2,), 0.2)
  A = rng.standard_normal((ne, ne))
  target = np.zeros(ne); target[2:4] = 1.0
  sy = dict(nx=nx, active=active, nu=nu, drift_o=drift_o, pol_o=pol_o, mu0=mu0, S0=S0n, target=target, precis=A @ A.T / ne,
            scale=np.array([2.0, 1.5, 1.0, 1.2]), shift=np.array([-0.5, -0.4, -0.6, -0.5]))
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    loss_n, gn = _grads(system, objective, params, m0, S0, H, native_actions=4)
  loss_t, gt = _grads(system, objective, params, m0, S0, H, native=False)
  drift.packed(F64, True, device).check_status(2)
  assert np.abs(loss_n - loss_t).max() < 1e-9
  worst = max(_group_err(gn[k], gt[k]) for k in gt)
  print(f"M = 64, ne = 8, four actions: worst group, native vs torch composition {worst:.2e}")
  for k in gt:
    assert _group_err(gn[k], gt[k]) < 1e-7, (k, _group_err(gn[k], gt[k]))


@pytest.mark.gpu
def test_gpu_one_action_through_the_nd_gradient_entries(device):
  """nu = 1, the cartpole system of test_gpu_one_action_through_the_nd_entry, H = 30: tape + sweep through the nd entries against
  the one-action entries.  Not bit-equal: the nd forward takes the general policy match (the two forwards differ by <= 1e-12)."""
  from gpflowpilco_amd import ops
  drift_o = oracle_params(make_svgp(4, 100, 6, seed=10, ls_bounds=(0.8, 3.0)))
  drift_o.Z[..., 5:] = 4.0 * drift_o.Z[..., 5:] - 2.0
  pol_o = random_svgp_params(seed=11, L=1, M=30, d=5, whiten=True, ls_bounds=(0.7, 2.0), mean=False)
  pol_o.q_mu = 0.3 * pol_o.q_mu
  rng = np.random.default_rng(12)
  mu = np.array([[0.4, 0.2, 0.5, 0.3], [0.6, -0.1, 0.4, 0.5], [0.5, 0.0, 0.45, 0.4]])
  S = generate_covariance(rng, 4, (3,), 0.05)
  target = np.array([0.0, 1.0, 0, 0, 0]); precis = 4.0 * np.eye(5)
  drift = gp_model_from_oracle(drift_o, device); pol = gp_model_from_oracle(pol_o, device)
  roll = ops.ComposedRollout(drift.packed(F64, True, device), pol.packed(F64, False, device), nx=4, active_dims=(1,),
                             head_scale=2.0, head_shift=-0.5, target=to_dev(target, device, F64), precis=to_dev(precis, device, F64))
  assert roll.supports_backward() and roll.supports_backward_nd()
  mx, Sxx = to_dev(mu, device, F64), to_dev(S, device, F64)
  g_cost = to_dev(rng.uniform(0.5, 1.5, (30, 3)), device, F64)
  m1, S1, c1, tape1 = roll.taped(mx, Sxx, 30)
  gp1, gm1, gS1 = roll.backward(tape1, g_cost, 3, 30)
  m2, S2, c2, tape2 = roll.taped_nd(mx, Sxx, 30)
  gp2, gm2, gS2 = roll.backward_nd(tape2, g_cost, 3, 30)
  roll.drift.check_status(3)
  assert tape1.numel() == tape2.numel() and gp2.shape == (3, 1, gp1.shape[1])
  print("one-action tape vs nd tape, forward:", scale_err(m2, m1.cpu().numpy()), scale_err(S2, S1.cpu().numpy()),
        scale_err(c2, c1.cpu().numpy()))
  errs = (scale_err(gp2[:, 0], gp1.cpu().numpy()), scale_err(gm2, gm1.cpu().numpy()), scale_err(gS2, gS1.cpu().numpy()))
  print(f"nu = 1 through the nd gradient entries vs the one-action ones: {errs}")
  assert max(errs) < 1e-9


@pytest.mark.gpu
def test_gpu_two_sweeps_over_one_tape_are_bit_equal(device):
  sy = _system("A", 8)
  roll = _rollout(sy, device, F64)
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  _, _, _, tape = roll.taped_nd(mx, Sxx, 8)
  g_cost = torch.ones(8, 3, dtype=F64, device=device)
  a = [t.clone() for t in roll.backward_nd(tape, g_cost, 3, 8)]
  b = roll.backward_nd(tape, g_cost, 3, 8)
  assert all(torch.equal(x, y) for x, y in zip(a, b))
  assert float(a[0].abs().max()) > 0.0 and torch.isfinite(a[0]).all()
  # without the state gradient: the same policy gradient
  c = roll.backward_nd(tape, g_cost, 3, 8, want_state_grad=False)
  assert c[1] is None and c[2] is None and torch.equal(c[0], a[0])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [128, 256], ids=["workspace-kept", "nothing-kept"])
def test_gpu_tape_without_the_kept_drift_blocks(B, device):
  """System A at H = 30: the tape keeps the drift's per-step workspace and sums at B = 3, the workspace alone at B = 128 and
  neither at B = 256 (the one-action rule); the sweep then re-runs what is missing through the drift adjoint it shares with the
  one-action sweep.  Batch elements are independent: element b of the large batch must reproduce element b % 3 of the small one."""
  H = 30
  sy = _system("A", H)
  lib = _lib.lib()
  per3 = lib.mm_compose_tape_bytes_nd(3, H, 4, 2, 2, 100, _lib.MM_F64) / 3
  assert lib.mm_compose_tape_bytes_nd(B, H, 4, 2, 2, 100, _lib.MM_F64) / B < 0.7 * per3
  roll = _rollout(sy, device, F64)
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  g3 = to_dev(np.random.default_rng(0).uniform(0.5, 1.5, (H, 3)), device, F64)
  _, _, cost3, tape3 = roll.taped_nd(mx, Sxx, H)
  ref = roll.backward_nd(tape3, g3, 3, H)
  idx = torch.arange(B, device=device) % 3
  _, _, costB, tapeB = roll.taped_nd(mx[idx], Sxx[idx], H)
  got = roll.backward_nd(tapeB, g3[:, idx].contiguous(), B, H)
  roll.drift.check_status(B)
  assert scale_err(costB, cost3[:, idx].cpu().numpy()) < 1e-12
  for name, a, b in zip(("g_policy", "g_mx0", "g_Sxx0"), got, ref):
    err = scale_err(a, b[idx].cpu().numpy())
    print(f"B = {B} {name}: against the fully kept tape {err:.2e}")
    assert err < 1e-9, (name, err)


@pytest.mark.gpu
def test_gpu_captured_replay_of_the_native_gradient(device):
  from gpflowpilco_amd.loops import GraphedPolicyLoss, get_state_initializer, policy_loss_closure
  sy = _system("A", 8)
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device, state_grad=False)
  closure = policy_loss_closure(system, objective, get_state_initializer(m0, S0), 8, native_actions=2)
  plist = list(params.values())

  def eager():
    for t in plist:
      t.grad = None
    loss = closure()
    loss.sum().backward()
    return loss.detach().clone(), [t.grad.clone() for t in plist]
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)
    graphed = GraphedPolicyLoss(closure, plist)
    for trial in range(2):
      le, ge = eager()
      lg, gg = graphed.loss_and_grad()
      torch.cuda.synchronize()
      assert scale_err(lg, le.cpu().numpy()) <= 1e-12
      for a, b in zip(gg, ge):
        assert scale_err(a, b.cpu().numpy()) <= 1e-12
      assert scale_err(graphed.loss(), le.cpu().numpy()) <= 1e-12
      with torch.no_grad():                    # an in-place parameter update: the next replay follows it
        pol_model.q_mu.mul_(0.9)
  assert float((le - lg).abs().max()) < 1e-9 and float(ge[0].abs().max()) > 0.0


@pytest.mark.gpu
def test_gpu_fallbacks_name_their_reason(device):
  sy = _system("A", 3)
  H = 3

  def one_warning(match, system, objective, params, m0, S0, **kw):
    with pytest.warns(RuntimeWarning, match=match) as rec:
      out = _grads(system, objective, params, m0, S0, H, **kw)
    mine = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(mine) == 1 and "torch composition" in str(mine[0].message)
    return out

  def same(a, b):
    assert np.abs(a[0] - b[0]).max() < 1e-12
    for k in b[1]:
      assert _group_err(a[1][k], b[1][k]) < 1e-10, k
  # a policy past the LDS bound of the sweep: 256 centres on ne = 6 dims (the bound there is 219)
  big = dict(sy, pol_o=random_svgp_params(seed=77, L=2, M=256, d=6, whiten=True, ls_bounds=(0.3, 0.8), mean=False))
  system, objective, drift, pol_model, params, m0, S0 = _setup(big, device)
  params = {"q_mu": params["q_mu"]}
  got = one_warning("LDS bound", system, objective, params, m0, S0, native_actions=2)
  same(got, _grads(system, objective, params, m0, S0, H, native=False))
  # a drift that is being trained
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device)
  drift.q_mu.requires_grad_(True)
  got = one_warning("the drift is being trained", system, objective, params, m0, S0, native_actions=2)
  same(got, _grads(system, objective, params, m0, S0, H, native=False))
  drift.q_mu.requires_grad_(False)
  # a head Scale that requires a gradient
  scale_t = system.policy.invlink.bijectors[0].scale
  scale_t.requires_grad_(True)
  got = one_warning("Scale.scale requires a gradient", system, objective, dict(params, scale=scale_t), m0, S0, native_actions=2)
  assert float(got[1]["scale"].abs().max()) > 0.0
  same(got, _grads(system, objective, dict(params, scale=scale_t), m0, S0, H, native=False))
  scale_t.requires_grad_(False)
  # fewer native actions than the policy has: still a fallback
  one_warning(r"nu > 1", system, objective, params, m0, S0, native_actions=1)
  # native=True at the default native_actions: today's semantics (the forward is native, a gradient warns nu > 1)
  one_warning(r"nu > 1", system, objective, params, m0, S0, native=True)
  # a float32 state is cast up into the float64 tape, the loss cast back: no fallback
  l64, g64 = _grads(system, objective, params, m0, S0, H, native_actions=2)
  m32, S32 = m0.detach().float().requires_grad_(True), S0.detach().float().requires_grad_(True)
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)
    l32, g32 = _grads(system, objective, params, m32, S32, H, native_actions=2)
  assert l32.dtype == np.float32 and m32.grad.dtype == torch.float32
  assert np.abs(l32.astype(np.float64) - l64).max() < 1e-5
  for k in g64:
    assert _group_err(g32[k].double(), g64[k]) < 1e-4, k


@pytest.mark.gpu
def test_gpu_distributed_loss_and_grad_with_the_native_gradient(device):
  """distributed.distributed_loss_and_grad(f.with_grad, ...) in one process: the closure's mean loss and gradients."""
  from gpflowpilco_amd import distributed as D
  from gpflowpilco_amd.loops import get_state_initializer, native_policy_loss, policy_loss_closure
  sy = _system("A", 8)
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device, state_grad=False)
  plist = list(params.values())
  f = native_policy_loss(system, objective, 8, native_actions=2)
  assert f.supports_grad(m0) and not native_policy_loss(system, objective, 8).supports_grad(m0)
  loss_d, g_d = D.distributed_loss_and_grad(f.with_grad, plist, m0, S0)
  for t in plist:
    t.grad = None
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)
    lm = policy_loss_closure(system, objective, get_state_initializer(m0, S0), 8, native_actions=2)().mean()
  lm.backward()
  assert abs(float(loss_d) - float(lm)) < 1e-12 * max(1.0, abs(float(lm)))
  for t, g in zip(plist, g_d):
    assert float((t.grad - g).abs().max()) <= 1e-12 * max(1e-12, float(t.grad.abs().max()))
