"""Native rollouts of a system WITHOUT an encoder (na = 0: mountain car, dynamics/forward_sde.py:49-68), opt-in through
``native_no_encoder=``: the moment-matched entries (csrc/mm_compose*.hip, their tapes and reverse sweeps) and the pathwise
entries (csrc/mm_pathwise_policy*.hip, one action, ``_nd`` and ``_wide``).

Systems (all seeded; B = 3, S = 37, H = 4):
  M0  nx 2, one action  -> ne 2, nd 3, drift M 40, policy M 12   (mountain car's shape)
  M1  nx 3, two actions -> ne 3, nd 5, the head of tests/multiaction_oracle.py
  W   nx 9, one action  -> nd 10: the wide pathwise entries (``native_inputs=16``)
The references are the committed oracles with ``active_dims=()`` (the encoding is the identity there) and the torch composition
of the same closure (``native=False``); every bar is the bar of the existing test of the same quantity with an encoder."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib
from gpflowpilco_amd import bijectors as tfb
from gpflowpilco_amd import dynamics, models as gp
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
from gpflowpilco_amd.moment_matching import GaussianMoments, moment_matching
from gpflowpilco_amd.synthetic import generate_covariance, make_svgp
from oracle import mm_compose_oracle as co
from oracle import pathwise_oracle as pw
from tests import multiaction_oracle as mao
from tests import pathwise_multiaction_oracle as pmo
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, scale_err, to_dev
from tests.test_adjoint_host import _step_forward
from tests.test_adjoint_nd_host import _load, _step_case, _step_forward_nd, _step_nd, _STEP_NAMES

F64 = torch.float64
P = C.POINTER(C.c_double)
H4 = 4
WEIGHTS = (1.0, 0.6, 0.8)
SCALE, SHIFT = (2.0, 1.5), (-0.5, -0.4)


def _p(a):
  return a.ctypes.data_as(P)


def _ip(a):
  return a.ctypes.data_as(C.POINTER(C.c_int32))


def _c(a):
  return np.ascontiguousarray(a, dtype=np.float64)


def _t(a, grad=False):
  return torch.tensor(np.asarray(a), dtype=F64, requires_grad=grad)


def _rel(got, want):
  return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-300))


def _sym(A):
  return 0.5 * (A + np.swapaxes(A, -1, -2))


@pytest.fixture(scope="module")
def hc1():
  return _load("mm_adjoint_host", "build.sh", "mm_adjoint.h", "mm_compose.h")


@pytest.fixture(scope="module")
def hcn():
  return _load("mm_adjoint_nd_host", "build_nd.sh", "mm_adjoint_nd.h", "mm_adjoint.h", "mm_compose.h")


# ---- CPU: the adjoint bodies at na = 0 ---------------------------------------------------------------------------------------
def test_encode_adjoint_without_angles(hc1):
  """mma_encode_bwd with na = 0 against autograd of the torch encoder match without active dims (the identity: me = m,
  See = Sxx, Sxe = Sxx), bar of tests/test_adjoint_host.py::test_encode_adjoint."""
  nx = 3
  rng = np.random.default_rng(nx)
  m = rng.standard_normal(nx); S = generate_covariance(rng, nx, (), 0.4)
  gme = rng.standard_normal(nx); gSee = rng.standard_normal((nx, nx)); gSxe = rng.standard_normal((nx, nx))
  mt, St = _t(m, True), _t(S, True)
  match = moment_matching(GaussianMoments((mt[None], (0.5 * (St + St.T))[None]), centered=True), TrigonometricEncoder(()))
  assert torch.equal(match.y.mean()[0], mt)
  val = ((match.y.mean()[0] * _t(gme)).sum() + (match.y.covariance()[0] * _t(gSee)).sum()
         + (match.cross_covariance(dense=True)[0] * _t(gSxe)).sum())
  gm_w, gS_w = torch.autograd.grad(val, (mt, St))
  gm = np.zeros(nx); gS = np.zeros((nx, nx))
  hc1.hc_encode_bwd(nx, 0, None, _p(_c(m)), _p(_c(S)), _p(_c(gme)), _p(_c(gSee)), _p(_c(gSxe)), _p(gm), _p(gS))
  assert _rel(gm, gm_w.numpy()) < 1e-12 and _rel(_sym(gS), _sym(gS_w.numpy())) < 1e-12
  assert np.abs(gm).max() > 0.1 and np.abs(gS).max() > 0.1


def test_step_adjoint_without_angles(hc1):
  """mma_step_bwd with na = 0 (every row of Cov(x, d) is a row of Sdd) against autograd of ``_step_forward``: <= 1e-13."""
  rng = np.random.default_rng(6)
  nx, active, dt = 4, (), 0.7
  ne, nd = nx, nx + 1
  vals = dict(Sxe=rng.standard_normal((nx, ne)), cp=rng.standard_normal(ne), Sdd=rng.standard_normal((nd, nd)),
              df1=rng.standard_normal(nx), dSff=rng.standard_normal((nx, nx)), dcross=rng.standard_normal((nd, nx)))
  ts = {k: _t(v, True) for k, v in vals.items()}
  m, S = _t(rng.standard_normal(nx), True), _t(rng.standard_normal((nx, nx)), True)
  m1, S1 = _step_forward((nx, 0, ne, nd, active, list(range(nx))), dt, m, S, **ts)
  gm1, gS1 = rng.standard_normal(nx), rng.standard_normal((nx, nx))
  want = torch.autograd.grad((m1 * _t(gm1)).sum() + (S1 * _t(gS1)).sum(), [ts[k] for k in _STEP_NAMES] + [m, S],
                             allow_unused=True)
  out = {k: np.full_like(vals[k], np.nan) for k in _STEP_NAMES}
  hc1.hc_step_bwd(nx, 0, None, C.c_double(dt), _p(_c(vals["Sxe"])), _p(_c(vals["cp"])), _p(_c(vals["Sdd"])),
                  _p(_c(vals["dcross"])), _p(_c(gm1)), _p(_c(gS1)), _p(out["Sxe"]), _p(out["cp"]), _p(out["Sdd"]),
                  _p(out["df1"]), _p(out["dSff"]), _p(out["dcross"]))
  for k, w in zip(_STEP_NAMES, want):
    if w is None:                                   # Sxe and cp are not read without angles: their adjoints are exact zeros
      assert k in ("Sxe", "cp") and np.all(out[k] == 0.0), k
    else:
      assert _rel(out[k], w.numpy()) < 1e-13, k
  assert np.abs(out["Sdd"]).max() > 0.1


@pytest.mark.parametrize("nu", [1, 2])
def test_step_adjoint_nd_without_angles(hcn, nu):
  rng = np.random.default_rng(60 + nu)
  nx, active, dt = 4, (), 0.7
  ne, nd = nx, nx + nu
  vals, gm1, gS1 = _step_case(rng, nx, active, nu)
  ts = {k: _t(v, True) for k, v in vals.items()}
  m, S = _t(rng.standard_normal(nx), True), _t(rng.standard_normal((nx, nx)), True)
  m1, S1 = _step_forward_nd((nx, 0, ne, nd, active, list(range(nx))), dt, m, S, **ts)
  want = torch.autograd.grad((m1 * _t(gm1)).sum() + (S1 * _t(gS1)).sum(), [ts[k] for k in _STEP_NAMES] + [m, S],
                             allow_unused=True)
  out = _step_nd(hcn, nx, active, nu, dt, vals, gm1, gS1)
  for k, w in zip(_STEP_NAMES, want):
    if w is None:
      assert k in ("Sxe", "cp") and np.all(out[k] == 0.0), k
    else:
      assert _rel(out[k], w.numpy()) < 1e-13, k


# ---- CPU: sizes, argument validation, routing ----------------------------------------------------------------------------------
def test_size_queries_take_no_angles_without_gpu():
  lib = _lib.lib()
  F64c, F32c = _lib.MM_F64, _lib.MM_F32
  assert lib.mm_abi_version() == 2
  for dt_ in (F64c, F32c):
    w = lib.mm_compose_workspace_bytes(3, 2, 0, dt_)
    assert 0 < w <= lib.mm_compose_workspace_bytes(3, 2, 1, dt_) and w < lib.mm_compose_workspace_bytes(64, 2, 1, dt_)
    assert lib.mm_compose_nd_workspace_bytes(3, 2, 0, 1, dt_) == w
    assert lib.mm_compose_nd_workspace_bytes(3, 3, 0, 2, dt_) > 0
    assert lib.mm_compose_tape_bytes(3, 4, 2, 0, 40, dt_) > 4 * w
    for jac in (0, 1):
      t1 = lib.mm_pathwise_tape_bytes(37, 4, 2, 0, dt_, jac)
      assert 0 < t1 == lib.mm_pathwise_tape_bytes_nd(37, 4, 2, 0, 1, dt_, jac) < lib.mm_pathwise_tape_bytes_nd(37, 4, 3, 0, 2, dt_, jac)
  assert lib.mm_compose_tape_bytes(3, 4, 2, 0, 40, F64c) == lib.mm_compose_tape_bytes_nd(3, 4, 2, 0, 1, 40, F64c)
  assert lib.mm_compose_tape_bytes_nd(3, 4, 3, 0, 2, 40, F64c) > lib.mm_compose_tape_bytes_nd(3, 4, 3, 0, 1, 40, F64c)
  b1 = lib.mm_compose_backward_workspace_bytes(3, 2, 0, 40)
  assert 0 < b1 <= lib.mm_compose_backward_workspace_bytes(3, 2, 1, 40) and b1 < lib.mm_compose_backward_workspace_bytes(64, 2, 1, 40)
  assert lib.mm_compose_backward_workspace_bytes_nd(3, 2, 0, 1, 40, 12) > 0
  assert lib.mm_compose_backward_workspace_bytes_nd(3, 3, 0, 2, 40, 12) > 0
  assert lib.mm_compose_backward_workspace_bytes_nd(3, 9, 0, 1, 40, 12) == 0           # ne = 9: the sweeps' bound stays
  assert lib.mm_compose_workspace_bytes(3, 16, 0, F64c) > 0 and lib.mm_compose_workspace_bytes(3, 17, 0, F64c) == 0
  assert lib.mm_pathwise_backward_scratch_bytes_wide(37, 12, 9, 1) > 0
  # a negative count is still refused everywhere
  assert lib.mm_compose_workspace_bytes(3, 2, -1, F64c) == 0 and lib.mm_compose_nd_workspace_bytes(3, 2, -1, 1, F64c) == 0
  assert lib.mm_compose_tape_bytes(3, 4, 2, -1, 40, F64c) == 0 and lib.mm_compose_tape_bytes_nd(3, 4, 2, -1, 1, 40, F64c) == 0
  assert lib.mm_compose_backward_workspace_bytes(3, 2, -1, 40) == 0
  assert lib.mm_compose_backward_workspace_bytes_nd(3, 2, -1, 1, 40, 12) == 0
  assert lib.mm_pathwise_tape_bytes(37, 4, 2, -1, F64c, 1) == 0 and lib.mm_pathwise_tape_bytes_nd(37, 4, 2, -1, 1, F64c, 1) == 0


def test_entries_take_no_angles_and_refuse_a_negative_count_without_gpu():
  """Refusals happen before any HIP call: with na = 0 (and a null ``active_dims``) every entry gets past its dimension check to
  the next one (a short buffer: MM_E_WORKSPACE), with na = -1 it returns MM_E_DIM."""
  lib = _lib.lib()
  buf = (C.c_char * 64)()
  p = C.addressof(buf)
  F64c = _lib.MM_F64
  E_DIM, E_WS = -2, -4
  sc = (C.c_double * 4)(2.0, 1.5, 1.0, 1.0)
  sh = (C.c_double * 4)(-0.5, -0.4, -0.6, 0.0)
  big = 1 << 40

  def fwd1(na):
    return lib.mm_rollout_composed(p, 64, 2, 40, 2 + na + 1, p, 64, 12, 2 + na, F64c, 3, 4, 1.0, 2, na, None, 2.0, -0.5, p, p,
                                   p, p, p, None, None, p, 64, p, 64, p, 64, None, None)

  def tap1(na):
    return lib.mm_rollout_composed_taped(p, 64, 2, 40, 2 + na + 1, p, 64, 12, 2 + na, F64c, 3, 4, 1.0, 2, na, None, 2.0, -0.5,
                                         p, p, p, p, p, p, 64, p, 64, p, 64, None, None)

  def bwd1(na, f=lib.mm_rollout_composed_backward, seeds=()):
    return f(p, 64, 2, 40, 2 + na + 1, p, 64, 12, 2 + na, F64c, 3, 4, 1.0, 2, na, None, 2.0, -0.5, p, p, p, 64, p, *seeds,
             p, None, None, p, 64, p, 64, None, None)

  def fwdn(na):
    return lib.mm_rollout_composed_nd(p, 64, 3, 40, 3 + na + 2, p, 64, 12, 3 + na, F64c, 3, 4, 1.0, 3, na, None, 2, sc, sh, p, p,
                                      p, p, p, None, None, p, 64, p, 64, p, 64, None, None)

  def tapn(na):
    return lib.mm_rollout_composed_taped_nd(p, 64, 3, 40, 3 + na + 2, p, 64, 12, 3 + na, F64c, 3, 4, 1.0, 3, na, None, 2, sc, sh,
                                            p, p, p, p, p, p, 64, p, 64, p, 64, None, None)

  def bwdn(na, f=lib.mm_rollout_composed_backward_nd, seeds=()):
    return f(p, 64, 3, 40, 3 + na + 2, p, 64, 12, 3 + na, F64c, 3, 4, 1.0, 3, na, None, 2, sc, sh, p, p, p, 64, p, *seeds,
             p, None, None, p, 64, p, 64, None, None)

  def pw1(na):
    return lib.mm_pathwise_policy_rollout(37, 128, 256, F64c, 4, 0.5, 2, na, None, p, p, p, p, p, p, p, None, p, p, big, 12,
                                          2.0, -0.5, p, p, p, p, p, 64, 1, None)

  def pwb1(na):
    return lib.mm_pathwise_policy_rollout_backward(37, F64c, 4, 0.5, 2, na, None, p, big, 12, 2.0, -0.5, p, p, p, 64, p, p, None,
                                                   p, big, None)

  def pwn(na, f):
    return f(37, 128, 256, F64c, 4, 0.5, 3, na, None, 2, p, p, p, p, p, p, p, None, p, p, big, 12, sc, sh, p, p, p, p, p, 64, 1, None)

  def pwbn(na, f):
    return f(37, F64c, 4, 0.5, 3, na, None, 2, p, big, 12, sc, sh, p, p, p, 64, p, p, None, p, big, None)

  calls = [fwd1, tap1, bwd1, functools.partial(bwd1, f=lib.mm_rollout_composed_backward_seeded, seeds=(None, None)),
           fwdn, tapn, bwdn, functools.partial(bwdn, f=lib.mm_rollout_composed_backward_nd_seeded, seeds=(None, None)),
           pw1, pwb1, functools.partial(pwn, f=lib.mm_pathwise_policy_rollout_nd),
           functools.partial(pwn, f=lib.mm_pathwise_policy_rollout_wide),
           functools.partial(pwbn, f=lib.mm_pathwise_policy_rollout_backward_nd),
           functools.partial(pwbn, f=lib.mm_pathwise_policy_rollout_backward_wide)]
  for i, f in enumerate(calls):
    assert f(0) == E_WS, i
    assert f(-1) == E_DIM, i
  # the seeded entries want both seeds or neither
  assert bwd1(0, lib.mm_rollout_composed_backward_seeded, (p, None)) == -1
  assert bwdn(0, lib.mm_rollout_composed_backward_nd_seeded, (None, p)) == -1


@functools.lru_cache(maxsize=None)
def _system(name):
  """The numpy side of M0 / M1 and its oracle rollout (computed once, shared, never modified)."""
  nx, nu, seed = {"M0": (2, 1, 70), "M1": (3, 2, 80)}[name]
  ne, nd = nx, nx + nu
  drift_o = oracle_params(make_svgp(nx, 40, nd, seed=seed, ls_bounds=(0.8, 3.0)))
  drift_o.Z[..., ne:] = 4.0 * drift_o.Z[..., ne:] - 2.0                          # action axes in [-2, 2]
  pol_o = random_svgp_params(seed=seed + 1, L=nu, M=12, d=ne, whiten=True, ls_bounds=(0.5, 1.2), mean=False, separate_Z=False)
  pol_o.q_mu = 1.5 * pol_o.q_mu
  rng = np.random.default_rng(seed + 2)
  mu0 = rng.uniform(0.2, 0.7, (3, nx))
  S0 = generate_covariance(rng, nx, (3,), 0.2)
  A = rng.standard_normal((nx, nx))
  precis = A @ A.T / nx + 0.5 * np.eye(nx)
  target = np.linspace(0.3, 0.6, nx)
  if nu == 1:
    scale, shift = SCALE[0], SHIFT[0]
    policy_fn = lambda st: co.mm_policy(st, pol_o, scale, shift)
  else:
    scale, shift = np.array(SCALE[:nu]), np.array(SHIFT[:nu])
    policy_fn = lambda st: mao.mm_policy_nd(st, pol_o, scale, shift)
  loss_o, traj_o = co.policy_rollout_loss(mu0, S0, drift_o, policy_fn, (), target, precis, H4, keep=True)
  return dict(nx=nx, nu=nu, ne=ne, nd=nd, drift_o=drift_o, pol_o=pol_o, mu0=mu0, S0=S0, target=target, precis=precis,
              scale=scale, shift=shift, loss_o=loss_o, traj_o=traj_o)


def _torch_system(sy, device, dtype=F64, encoder=None, solver=None):
  drift = gp_model_from_oracle(sy["drift_o"], device)
  pol_model = gp_model_from_oracle(sy["pol_o"], device)
  if sy["nu"] == 1:
    head = [tfb.Scale(float(sy["scale"])), tfb.Shift(float(sy["shift"])), tfb.NormalCDF()]
  else:
    head = [tfb.Scale(to_dev(sy["scale"], device, dtype)), tfb.Shift(to_dev(sy["shift"], device, dtype)), tfb.NormalCDF()]
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol_model), invlink=tfb.Chain(head))
  objective = GaussianObjective(target=to_dev(sy["target"], device, dtype), precis=to_dev(sy["precis"], device, dtype))
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=encoder,
                                    solver=dynamics.MomentMatchingEuler() if solver is None else solver)
  return system, objective, drift, pol_model


def test_oracle_systems_are_well_posed():
  for name in ("M0", "M1"):
    sy = _system(name)
    ev = min(np.linalg.eigvalsh(S).min() for _, S in sy["traj_o"])
    assert ev > 1e-3 and np.isfinite(sy["loss_o"]).all()
    assert sy["loss_o"].max() < -0.05 * H4 and sy["loss_o"].min() > -0.999 * H4     # away from both ends of the cost


def test_native_parts_refuses_a_missing_encoder_unless_asked():
  from gpflowpilco_amd.loops import _native_parts, native_policy_loss, policy_loss_closure, get_state_initializer
  sy = _system("M0")
  system, objective, _, _ = _torch_system(sy, "cpu")
  why = []
  assert _native_parts(system, objective, why, True) is None
  assert why == ["encoder NoneType (the native rollout implements TrigonometricEncoder)"]
  parts = _native_parts(system, objective, [], True, no_encoder=True)
  assert parts is not None and isinstance(parts[0], TrigonometricEncoder) and parts[0].active_dims == ()
  system.encoder = TrigonometricEncoder(active_dims=())
  why = []
  assert _native_parts(system, objective, why, True) is None and "without active dims" in why[0]
  assert _native_parts(system, objective, [], True, no_encoder=True) is not None
  system.encoder = None
  assert native_policy_loss(system, objective, H4) is None
  assert native_policy_loss(system, objective, H4, native_no_encoder=True) is not None
  init = get_state_initializer(_t(sy["mu0"]), _t(sy["S0"]))
  with pytest.raises(ValueError, match="native=True"):
    policy_loss_closure(system, objective, init, H4, native=True)
  policy_loss_closure(system, objective, init, H4, native=True, native_no_encoder=True)


# ---- GPU: moment-matched -------------------------------------------------------------------------------------------------------
def _rollout(sy, device, dtype):
  from gpflowpilco_amd import ops
  drift = gp_model_from_oracle(sy["drift_o"], device)
  pol_model = gp_model_from_oracle(sy["pol_o"], device)
  scale = sy["scale"] if sy["nu"] == 1 else tuple(sy["scale"])
  shift = sy["shift"] if sy["nu"] == 1 else tuple(sy["shift"])
  return ops.ComposedRollout(drift.packed(dtype, True, device), pol_model.packed(dtype, False, device), nx=sy["nx"],
                             active_dims=(), head_scale=scale, head_shift=shift,
                             target=to_dev(sy["target"], device, dtype), precis=to_dev(sy["precis"], device, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["M0", "M1"])
def test_gpu_forward_matches_the_oracle_without_an_encoder(name, dtype, device):
  sy = _system(name)
  roll = _rollout(sy, device, dtype)
  assert roll.na == 0 and roll.ne == sy["nx"] and roll.nd == sy["nd"]
  mx, Sxx = to_dev(sy["mu0"], device, dtype), to_dev(sy["S0"], device, dtype)
  m_H, S_H, cost, tmu, tS = roll(mx, Sxx, H4, keep_trajectory=True)
  roll.drift.check_status(3)
  tol = 1e-7 if dtype == torch.float64 else 5e-4
  errs = [scale_err(cost.sum(1), sy["loss_o"])]
  for h in range(H4):
    errs += [scale_err(tmu[h], sy["traj_o"][h][0]), scale_err(tS[h], sy["traj_o"][h][1])]
  print(f"no-encoder forward {name} {dtype}: worst err {max(errs):.3e}")
  assert max(errs) < tol, errs
  assert torch.equal(m_H, tmu[-1]) and torch.equal(S_H, tS[-1])
  if dtype == torch.float64:
    # the taped forward and the states read off its tape
    taped = roll.taped if sy["nu"] == 1 else roll.taped_nd
    m_t, S_t, cost_t, tape = taped(mx, Sxx, H4)
    xm, xS = roll.tape_states(tape, 3, H4)
    # (the taped forward forms the drift's covariance from the backward's sums: another summation order, the same bar)
    assert scale_err(cost_t.sum(0), sy["loss_o"]) < tol
    for h in range(H4):
      assert scale_err(xm[h], sy["traj_o"][h][0]) < tol and scale_err(xS[h], sy["traj_o"][h][1]) < tol, h
    assert torch.equal(xm[-1], m_t) and torch.equal(xS[-1], S_t)


def _trainable(pol_model, nu):
  out = {"q_mu": pol_model.q_mu}
  for a in range(nu):
    kern = pol_model.kernel.kernels[a]
    out[f"Z{a}"] = pol_model.inducing_variable.inducing_variables[a].Z
    out[f"ls{a}"] = kern.lengthscales
    out[f"var{a}"] = kern.variance
  for t in out.values():
    t.requires_grad_(True)
  return out


def _grads(system, objective, params, m0, S0, **kw):
  from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
  leaves = list(params.values()) + [m0, S0]
  for t in leaves:
    t.grad = None
  loss = policy_loss_closure(system, objective, get_state_initializer(m0, S0), H4, **kw)()
  wts = torch.tensor(WEIGHTS[:loss.shape[0]], dtype=loss.dtype, device=loss.device)
  (loss * wts).sum().backward()
  out = {k: t.grad.detach().clone() for k, t in params.items()}
  out["m0"], out["S0"] = m0.grad.detach().clone(), 0.5 * (S0.grad + S0.grad.transpose(1, 2)).detach()
  return loss.detach(), out


def _group_err(got, want):
  return float((got - want).abs().max()) / max(1e-12, float(want.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["M0", "M1"])
def test_gpu_loss_and_gradient_without_an_encoder(name, device):
  """Every policy parameter group and (m0, S0): the native closure (no fall-back warning) against the torch composition, bars of
  tests/test_gpu_backward.py:356-359 and tests/test_multiaction_grad.py; without the option the closure falls back as before."""
  from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
  sy = _system(name)
  system, objective, drift, pol_model = _torch_system(sy, device)
  params = _trainable(pol_model, sy["nu"])
  m0 = to_dev(sy["mu0"], device, F64).requires_grad_(True)
  S0 = to_dev(sy["S0"], device, F64).requires_grad_(True)
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)
    loss_n, gn = _grads(system, objective, params, m0, S0, native_no_encoder=True, native_actions=2)
    with torch.no_grad():
      loss_f = policy_loss_closure(system, objective, get_state_initializer(m0, S0), H4, native_no_encoder=True)()
  loss_t, gt = _grads(system, objective, params, m0, S0, native=False)
  drift.packed(F64, True, device).check_status(3)
  assert float((loss_n - loss_t).abs().max()) < 1e-9 and float((loss_f - loss_t).abs().max()) < 1e-9
  assert scale_err(loss_n, sy["loss_o"]) < 1e-7
  for k in gt:
    err = _group_err(gn[k], gt[k])
    print(f"no-encoder gradient {name} {k}: native vs torch composition {err:.2e}")
    assert float(gt[k].abs().max()) > 0.0 and err < 1e-7, (k, err)
  with pytest.warns(RuntimeWarning, match="encoder NoneType"):
    loss_d, gd = _grads(system, objective, params, m0, S0, native_actions=2)
  assert all(torch.equal(gd[k], gt[k]) for k in gt)


@pytest.mark.gpu
def test_gpu_graphed_loss_without_an_encoder_replays_eager(device):
  from gpflowpilco_amd.loops import GraphedPolicyLoss, get_state_initializer, policy_loss_closure
  sy = _system("M0")
  system, objective, drift, pol_model = _torch_system(sy, device)
  pol_model.q_mu.requires_grad_(True)
  m0, S0 = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  closure = policy_loss_closure(system, objective, get_state_initializer(m0, S0), H4, native=True, native_no_encoder=True)
  graphed = GraphedPolicyLoss(closure, [pol_model.q_mu])
  for _ in range(2):
    pol_model.q_mu.grad = None
    le = closure(); le.sum().backward()
    ge = pol_model.q_mu.grad.detach().clone(); le = le.detach().clone()
    lg, (gg,) = graphed.loss_and_grad()
    assert torch.allclose(lg, le, rtol=1e-12, atol=1e-14) and torch.allclose(gg, ge, rtol=1e-10, atol=1e-13)
    assert torch.allclose(graphed.loss(), le, rtol=1e-12, atol=1e-14)
    with torch.no_grad():
      pol_model.q_mu.mul_(0.9)
      m0.add_(0.01)
  graphed.check()


@pytest.mark.gpu
def test_gpu_option_is_a_no_op_with_an_encoder(device):
  """Regression guard: the cart-pole wiring (na = 1) through the relaxed entries -- loss and gradients bit-equal with and without
  ``native_no_encoder=True``, moment-matched and pathwise."""
  from tests.test_gpu_backward import _cartpole_like
  system, objective, params, m0, S0, _ = _cartpole_like(device, 30)
  m0.requires_grad_(True); S0.requires_grad_(True)
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)
    la, ga = _grads(system, objective, params, m0, S0)
    lb, gb = _grads(system, objective, params, m0, S0, native_no_encoder=True)
  assert torch.equal(la, lb) and all(torch.equal(ga[k], gb[k]) for k in ga)
  assert float(ga["q_mu"].abs().max()) > 0.0


# ---- GPU: pathwise ---------------------------------------------------------------------------------------------------------------
DT = 0.5
PW_SYSTEMS = {"M0": dict(nx=2, nu=1, seed=90), "M1": dict(nx=3, nu=2, seed=100), "W": dict(nx=9, nu=1, seed=110)}


@functools.lru_cache(maxsize=None)
def _pw_system(name, S=37):
  """Recipe of tests/test_pathwise_multiaction.py::_system with K = 64 bases and no angles."""
  c = PW_SYSTEMS[name]
  nx, nu, seed = c["nx"], c["nu"], c["seed"]
  ne, nd = nx, nx + nu
  rng = np.random.default_rng(seed)
  drift = oracle_params(make_svgp(nx, 40, nd, seed=seed + 1, ls_bounds=(0.8, 3.0) if nd <= 8 else (1.5, 4.0)))
  drift.Z[..., ne:] = 4.0 * drift.Z[..., ne:] - 2.0
  pol = random_svgp_params(seed=seed + 2, L=nu, M=12, d=ne, whiten=True, ls_bounds=(0.8, 2.0) if ne <= 8 else (1.5, 3.0), mean=True,
                           separate_Z=True)
  pol.q_mu = 0.3 * pol.q_mu
  paths = pw.draw_paths(rng, drift, S, 64)
  paths.w *= 0.3; paths.v *= 0.3
  x0 = rng.uniform(0.2, 0.8, size=(S, nx))
  target = np.full(ne, 0.1)
  A = rng.standard_normal((ne, ne))
  precis = 0.5 * (A @ A.T) / ne + 0.5 * np.eye(ne)
  scale, shift = np.array(SCALE[:nu]), np.array(SHIFT[:nu])
  cost_o, states_o = pmo.policy_rollout_costs_nd(paths, drift, pol, scale, shift, (), target, precis, x0, H4, dt=DT, keep=True)
  if nu == 1:                                        # the helper with one action is the committed oracle itself
    c1, s1 = pw.policy_rollout_costs(paths, drift, pol, float(scale[0]), float(shift[0]), (), target, precis, x0, H4, dt=DT, keep=True)
    assert np.abs(c1 - cost_o).max() == 0.0 and np.abs(s1 - states_o).max() == 0.0
  return dict(c, S=S, ne=ne, nd=nd, drift=drift, pol=pol, paths=paths, x0=x0, target=target, precis=precis, scale=scale,
              shift=shift, cost_o=cost_o, states_o=states_o)


def _pw_device_case(sy, device, dtype):
  from gpflowpilco_amd.pathwise import PolicyRollout, paths_from_arrays
  Pp, dr = sy["paths"], sy["drift"]
  gp_paths = paths_from_arrays(Pp.omega, Pp.phase, Pp.w, Pp.v, dr.Z, dr.lengthscales, dr.variance, dr.mean_c, dtype=dtype,
                               device=device)
  pol_model = gp_model_from_oracle(sy["pol"], device)
  nu = sy["nu"]
  scale = float(sy["scale"][0]) if nu == 1 else tuple(sy["scale"])
  shift = float(sy["shift"][0]) if nu == 1 else tuple(sy["shift"])
  roll = PolicyRollout(gp_paths, pol_model.packed(F64, False, device), nx=sy["nx"], active_dims=(), head_scale=scale,
                       head_shift=shift, target=torch.tensor(sy["target"]), precis=torch.tensor(sy["precis"]), wide=sy["nd"] > 8)
  return gp_paths, pol_model, roll


def test_pathwise_oracle_systems_are_well_posed():
  for name in PW_SYSTEMS:
    sy = _pw_system(name)
    assert np.isfinite(sy["cost_o"]).all() and np.abs(sy["states_o"]).max() < 3.0
    assert sy["cost_o"].max() < -0.02 and sy["cost_o"].min() > -0.999


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["M0", "M1", "W"])
def test_gpu_pathwise_costs_and_states_without_an_encoder(name, dtype, device):
  sy = _pw_system(name)
  _, _, roll = _pw_device_case(sy, device, dtype)
  assert roll.na == 0 and roll.nd == sy["nd"]
  x0 = torch.tensor(sy["x0"], dtype=dtype, device=device)
  cost, tape = roll(x0, H4, dt=DT, with_jacobians=False)
  cost_j, tape_j = roll(x0, H4, dt=DT, with_jacobians=True)
  assert torch.equal(cost, cost_j) and torch.equal(roll.states(tape, H4), roll.states(tape_j, H4))
  ec, es = scale_err(cost, sy["cost_o"]), scale_err(roll.states(tape, H4), sy["states_o"])
  print(f"no-encoder pathwise forward {name} {dtype}: cost {ec:.3e} states {es:.3e}")
  tol = 1e-10 if dtype == torch.float64 else 5e-3
  assert ec < tol and es < tol


def _pw_torch_system(sy, device):
  from gpflowpilco_amd.pathwise import PathwiseSVGP
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=device)
  drift = gp_model_from_oracle(sy["drift"], device)
  pol_model = gp_model_from_oracle(sy["pol"], device)
  head = tfb.Chain([tfb.Scale(t(sy["scale"])), tfb.Shift(t(sy["shift"])), tfb.NormalCDF()])
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol_model), invlink=head)
  pdrift = PathwiseSVGP(kernel=drift.kernel, inducing_variable=drift.inducing_variable, q_mu=drift.q_mu, q_sqrt=drift.q_sqrt,
                        whiten=sy["drift"].whiten, mean_function=drift.mean_function, num_latent_gps=sy["nx"])
  system = dynamics.DynamicalSystem(drift=pdrift, policy=policy, encoder=None, solver=dynamics.Euler())
  objective = GaussianObjective(target=t(sy["target"]), precis=t(sy["precis"]))
  return system, objective, pol_model


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["M0", "M1", "W"])
def test_gpu_pathwise_gradient_without_an_encoder(name, device):
  """The closure with ``native_no_encoder=True`` (no fall-back warning; W through the wide entries) against the same closure with
  ``native=False`` on the same paths: 1e-8 relative per tensor; two backward calls on one tape are bit-equal."""
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _pw_system(name)
  nu = sy["nu"]
  gp_paths, _, _ = _pw_device_case(sy, device, F64)
  system, objective, pm = _pw_torch_system(sy, device)
  groups = {"q_mu": [pm.q_mu], "Z": [pm.inducing_variable.inducing_variables[a].Z for a in range(nu)],
            "lengthscales": [pm.kernel.kernels[a].lengthscales for a in range(nu)],
            "variance": [pm.kernel.kernels[a].variance for a in range(nu)]}
  flat = [t for ts in groups.values() for t in ts]
  for t in flat:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)
  kw = dict(dt=DT, paths=gp_paths, native_actions=2, native_inputs=16)

  def run(**extra):
    for t in flat + [x0]:
      t.grad = None
    loss = pathwise_policy_loss_closure(system, objective, lambda: x0, H4, **kw, **extra)()
    loss.mean().backward()
    return loss.detach(), [t.grad.detach().clone() for t in flat + [x0]]
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)
    ln, gn = run(native=True, native_no_encoder=True)
    ln2, gn2 = run(native=True, native_no_encoder=True)
  lt, gt = run(native=False)
  assert scale_err(ln, sy["cost_o"].sum(0)) < 1e-10 and scale_err(lt, sy["cost_o"].sum(0)) < 1e-10
  for a_, b_, c_ in zip(gn, gt, gn2):
    err = float((a_ - b_).abs().max()) / max(1e-300, float(b_.abs().max()))
    assert float(b_.abs().max()) > 0.0 and err < 1e-8, err
    assert torch.equal(a_, c_)
  with pytest.raises(ValueError, match="native=True"):
    pathwise_policy_loss_closure(system, objective, lambda: x0, H4, native=True, **kw)
  with pytest.warns(RuntimeWarning, match="encoder NoneType"):
    ld, _ = run()
  assert torch.equal(ld, lt)


@pytest.mark.gpu
def test_gpu_two_pathwise_sweeps_over_one_tape_are_bit_equal(device):
  sy = _pw_system("M1")
  _, _, roll = _pw_device_case(sy, device, F64)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device)
  _, tape = roll(x0, H4, dt=DT, with_jacobians=True)
  g_cost = torch.randn(H4, sy["S"], dtype=F64, generator=torch.Generator(device="cpu").manual_seed(7)).to(device)
  a = roll.backward(tape, g_cost, H4, dt=DT, want_state_grad=True)
  b = roll.backward(tape, g_cost, H4, dt=DT, want_state_grad=True)
  assert all(torch.equal(u, v) for u, v in zip(a, b)) and float(a[0].abs().max()) > 0.0
