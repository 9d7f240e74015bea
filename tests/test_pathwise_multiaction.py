"""The native pathwise policy rollout and its gradient for policies with several actions (csrc/mm_pathwise_policy.hip,
pathwise.PolicyRollout with an L = nu pack, loops.pathwise_policy_loss_closure(native_actions=...)) against the numpy
restatement tests/pathwise_multiaction_oracle.py (a fold of oracle.pathwise_oracle's own functions).

Systems (recipe of tests/test_pathwise.py::_policy_case; H = 6, dt = 0.5, S = 37: one partial wave, S = 300: two workgroups with
a partial last one):
  P  nx 4, angles (0, 1), nu 2 -> ne 6, nd 8   (the double pendulum's shape, at the Jacobian pass's limit)     seed 40
  Q  nx 3, angle (1,),    nu 3 -> ne 4, nd 7                                                                      seed 50
  C  nx 4, angle (1,),    nu 1 -> ne 5, nd 6   (cartpole: the one-action yardstick of the f32 error)             seed 3
Each latent of the policy has its own Z, lengthscales and mean, so that an action evaluated from the wrong latent or fed to
the wrong drift input moves the costs far beyond the f32 bar (test_wrong_wirings_are_far_outside_the_f32_bar).

Bars: f64 1e-10 and f32 5e-3 on costs and taped states (the one-action bars of tests/test_pathwise.py for the same quantities);
gradients 1e-8 relative per tensor against torch autograd of a torch mirror and 1e-6 max(1, |fd|) against central differences
of the numpy helper (the one-action gradient's bars)."""
import copy
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib
from gpflowpilco_amd.synthetic import make_svgp
from oracle import pathwise_oracle as pw
from tests import pathwise_multiaction_oracle as pmo
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, scale_err

F64 = torch.float64
SCALE, SHIFT = (2.0, 1.5, 1.0), (-0.5, -0.4, -0.6)
SYSTEMS = {"P": dict(nx=4, active=(0, 1), nu=2, seed=40),
           "Q": dict(nx=3, active=(1,), nu=3, seed=50),
           "C": dict(nx=4, active=(1,), nu=1, seed=3)}
H6, DT = 6, 0.5
F32_BAR, F64_BAR = 5e-3, 1e-10


@functools.lru_cache(maxsize=None)
def _system(name, S):
  """The numpy side of a system and its oracle rollout (computed once, shared, never modified)."""
  c = SYSTEMS[name]
  nx, active, nu, seed = c["nx"], c["active"], c["nu"], c["seed"]
  na = len(active); ne = nx + na; nd = ne + nu
  rng = np.random.default_rng(seed)
  drift = oracle_params(make_svgp(nx, 50, nd, seed=seed + 1, ls_bounds=(0.8, 3.0)))
  drift.Z[..., ne:] = 4.0 * drift.Z[..., ne:] - 2.0                       # action axes in [-2, 2]
  pol = random_svgp_params(seed=seed + 2, L=nu, M=12, d=ne, whiten=True, ls_bounds=(0.8, 2.0), mean=True, separate_Z=True)
  pol.q_mu = 0.3 * pol.q_mu
  paths = pw.draw_paths(rng, drift, S, 130)
  paths.w *= 0.3; paths.v *= 0.3                                          # (keeps 6-step sample rollouts inside the data's support)
  x0 = rng.uniform(0.2, 0.8, size=(S, nx))
  target = np.zeros(ne); target[na:2 * na] = 1.0; target[2 * na:] = 0.1
  A = rng.standard_normal((ne, ne))
  precis = 0.5 * (A @ A.T) / ne + 0.5 * np.eye(ne)
  scale, shift = np.array(SCALE[:nu]), np.array(SHIFT[:nu])
  cost_o, states_o = pmo.policy_rollout_costs_nd(paths, drift, pol, scale, shift, active, target, precis, x0, H6, dt=DT, keep=True)
  return dict(c, S=S, na=na, ne=ne, nd=nd, drift=drift, pol=pol, paths=paths, x0=x0, target=target, precis=precis, scale=scale,
              shift=shift, cost_o=cost_o, states_o=states_o)


def _oracle(sy, H, pol=None, x0=None, **kw):
  return pmo.policy_rollout_costs_nd(sy["paths"], sy["drift"], sy["pol"] if pol is None else pol, sy["scale"], sy["shift"],
                                     sy["active"], sy["target"], sy["precis"], sy["x0"] if x0 is None else x0, H, dt=DT, **kw)


def _device_case(sy, device, dtype, nd_entries=None):
  from gpflowpilco_amd.pathwise import PolicyRollout, paths_from_arrays
  P, dr = sy["paths"], sy["drift"]
  gp_paths = paths_from_arrays(P.omega, P.phase, P.w, P.v, dr.Z, dr.lengthscales, dr.variance, dr.mean_c, dtype=dtype, device=device)
  pol_model = gp_model_from_oracle(sy["pol"], device)
  nu = sy["nu"]
  scale = float(sy["scale"][0]) if nu == 1 else tuple(sy["scale"])
  shift = float(sy["shift"][0]) if nu == 1 else tuple(sy["shift"])
  roll = PolicyRollout(gp_paths, pol_model.packed(F64, False, device), nx=sy["nx"], active_dims=sy["active"], head_scale=scale,
                       head_shift=shift, target=torch.tensor(sy["target"]), precis=torch.tensor(sy["precis"]), nd_entries=nd_entries)
  return gp_paths, pol_model, roll


# ---- CPU: the helper, the guards, the ABI, the closure's argument ----------------------------------------------------------
def test_helper_with_one_action_is_the_pathwise_oracle():
  sy = _system("C", 37)
  co, so = pw.policy_rollout_costs(sy["paths"], sy["drift"], sy["pol"], float(sy["scale"][0]), float(sy["shift"][0]), sy["active"],
                                   sy["target"], sy["precis"], sy["x0"], H6, dt=DT, keep=True)
  assert np.abs(sy["cost_o"] - co).max() == 0.0 and np.abs(sy["states_o"] - so).max() == 0.0


@pytest.mark.parametrize("name,S", [("P", 37), ("P", 300), ("Q", 37), ("Q", 300)])
def test_wrong_wirings_are_far_outside_the_f32_bar(name, S):
  """Well-posedness of the systems, and the two guards: the actions fed to the drift in rotated order, and every action
  evaluated from latent 0's parameters, each move the costs by at least 4x the f32 bar (relative to max |cost|, as the GPU
  comparison measures it): neither wiring could pass the f32 comparison."""
  sy = _system(name, S)
  nu = sy["nu"]
  assert np.isfinite(sy["cost_o"]).all() and np.abs(sy["states_o"]).max() < 3.0
  assert sy["cost_o"].max() < -0.05 and sy["cost_o"].min() > -0.999            # away from both ends of -exp(-q / 2)
  rot = scale_err(_oracle(sy, H6, feed_order=[(a + 1) % nu for a in range(nu)]), sy["cost_o"])
  lat0 = scale_err(_oracle(sy, H6, latent_of=[0] * nu), sy["cost_o"])
  print(f"guards {name} S={S}: rotated feed {rot:.2e}, every action from latent 0 {lat0:.2e}; states in "
        f"[{sy['states_o'].min():.2f}, {sy['states_o'].max():.2f}], costs in [{sy['cost_o'].min():.3f}, {sy['cost_o'].max():.3f}]")
  assert rot >= 4 * F32_BAR and lat0 >= 4 * F32_BAR


def test_argument_validation_and_sizes_of_the_nd_entries_without_gpu():
  lib = _lib.lib()
  buf = (ctypes.c_char * 64)()
  p = ctypes.addressof(buf)
  F64c, F32c = _lib.MM_F64, _lib.MM_F32
  E_ARG, E_DIM, E_DTYPE, E_WS = -1, -2, -3, -4
  act = (ctypes.c_int32 * 2)(0, 1)
  sc = (ctypes.c_double * 4)(2.0, 1.5, 1.0, 1.0)
  sh = (ctypes.c_double * 4)(-0.5, -0.4, -0.6, 0.0)
  # ---- size queries: nu = 1 is the one-action size; sizes grow with nu
  tb, tb1 = lib.mm_pathwise_tape_bytes_nd, lib.mm_pathwise_tape_bytes
  for dt_ in (F64c, F32c):
    for jac in (0, 1):
      assert tb(37, 6, 4, 1, 1, dt_, jac) == tb1(37, 6, 4, 1, dt_, jac) > 0
      assert tb(300, 6, 4, 2, 1, dt_, jac) == tb1(300, 6, 4, 2, dt_, jac)
  assert tb(3000, 6, 4, 2, 1, F64c, 1) < tb(3000, 6, 4, 2, 2, F64c, 1) < tb(3000, 6, 4, 2, 3, F64c, 1)
  assert tb(3000, 6, 4, 2, 2, F32c, 1) < tb(3000, 6, 4, 2, 2, F64c, 1) and tb(3000, 6, 4, 2, 2, F64c, 0) < tb(3000, 6, 4, 2, 2, F64c, 1)
  assert tb(37, 6, 4, 2, 0, F64c, 1) == 0 and tb(37, 6, 4, 2, 5, F64c, 1) == 0 and tb(0, 6, 4, 2, 2, F64c, 1) == 0
  assert tb(37, 6, 4, 5, 2, F64c, 1) == 0
  sb, sb1 = lib.mm_pathwise_backward_scratch_bytes_nd, lib.mm_pathwise_backward_scratch_bytes
  for S, M, ne in ((37, 12, 5), (300, 30, 5), (8192, 256, 7)):
    assert sb(S, M, ne, 1) == sb1(S, M, ne) > 0
  assert sb(300, 30, 6, 2) == 2 * sb(300, 30, 6, 1) and sb(300, 30, 4, 3) == 3 * sb(300, 30, 4, 1)
  assert sb(300, 30, 6, 0) == 0 and sb(300, 30, 4, 5) == 0 and sb(0, 30, 6, 2) == 0
  assert sb(300, 257, 6, 2) == 0 and sb(300, 30, 7, 2) == 0                      # M > 256; ne + nu > 8
  # the stated LDS bound: 8 (nu (M ne + M + ne) + ne + ne^2 + 8 + 4 nu (M ne + M + ne + 2)) <= 160 KiB
  def lds(nu, M, ne):
    return 8 * (nu * (M * ne + M + ne) + ne + ne * ne + 8 + 4 * nu * (M * ne + M + ne + 2))
  assert lds(2, 256, 6) <= 160 * 1024 < lds(4, 256, 4)
  assert sb(300, 256, 6, 2) > 0 and sb(300, 256, 4, 4) == 0                      # the double pendulum at M = 256 fits; nu 4 does not
  assert lds(4, 203, 4) <= 160 * 1024 < lds(4, 204, 4) and sb(300, 203, 4, 4) > 0 and sb(300, 204, 4, 4) == 0
  assert lds(3, 226, 5) <= 160 * 1024 < lds(3, 227, 5) and sb(300, 226, 5, 3) > 0 and sb(300, 227, 5, 3) == 0
  for nu in (1, 2, 3, 4):                                                          # every shape with M <= 64 and nd <= 8
    for ne in range(1, 9 - nu):
      assert sb(300, 64, ne, nu) > 0, (nu, ne)

  # ---- the forward entry
  def fwd(nu=2, nx=4, na=2, dtype=F64c, a=act, omega=p, pol=p, pol_bytes=1 << 30, pM=12, scale=sc, shift=sh, x0=p, tape=p,
          tape_bytes=1 << 40, S=37):
    return lib.mm_pathwise_policy_rollout_nd(S, 128, 256, dtype, 6, 0.5, nx, na, a, nu, omega, p, p, p, p, p, p, None, p, pol,
                                             pol_bytes, pM, scale, shift, p, p, x0, p, tape, tape_bytes, 1, None)
  assert fwd(nu=0) == E_DIM and fwd(nu=5) == E_DIM                                # 1 <= nu <= 4
  assert fwd(nu=3) == E_DIM                                                        # nx + na + nu = 9
  assert fwd(nx=5, na=2, nu=2) == E_DIM
  assert fwd(pM=257) == E_DIM
  assert fwd(omega=None) == E_ARG and fwd(pol=None) == E_ARG and fwd(scale=None) == E_ARG and fwd(shift=None) == E_ARG
  assert fwd(x0=None) == E_ARG and fwd(tape=None) == E_ARG and fwd(a=None) == E_ARG and fwd(S=0) == E_ARG
  assert fwd(dtype=7) == E_DTYPE
  need = tb(37, 6, 4, 2, 2, F64c, 1)
  assert fwd(tape_bytes=need - 1) == E_WS                                          # short tape
  assert fwd(tape_bytes=need, pol_bytes=64) == E_WS                                # short policy buffer

  # ---- the backward entry
  def bwd(nu=2, nx=4, na=2, dtype=F64c, a=act, pol=p, pol_bytes=1 << 30, pM=12, scale=sc, shift=sh, tape=p, tape_bytes=1 << 40,
          g_cost=p, g_pol=p, scratch=p, scratch_bytes=1 << 40):
    return lib.mm_pathwise_policy_rollout_backward_nd(37, dtype, 6, 0.5, nx, na, a, nu, pol, pol_bytes, pM, scale, shift, p, p, tape,
                                                      tape_bytes, g_cost, g_pol, None, scratch, scratch_bytes, None)
  assert bwd(nu=0) == E_DIM and bwd(nu=5) == E_DIM and bwd(nu=3) == E_DIM and bwd(pM=257) == E_DIM
  assert bwd(nx=2, na=2, nu=4, pM=256) == E_DIM                                    # ne = 4, nu = 4, M = 256: beyond the LDS bound
  assert bwd(pol=None) == E_ARG and bwd(scale=None) == E_ARG and bwd(shift=None) == E_ARG and bwd(tape=None) == E_ARG
  assert bwd(g_cost=None) == E_ARG and bwd(g_pol=None) == E_ARG and bwd(scratch=None) == E_ARG and bwd(a=None) == E_ARG
  assert bwd(dtype=7) == E_DTYPE
  assert bwd(tape_bytes=need - 1) == E_WS
  assert bwd(tape_bytes=need, scratch_bytes=sb(37, 12, 6, 2) - 1) == E_WS
  assert bwd(tape_bytes=need, scratch_bytes=sb(37, 12, 6, 2), pol_bytes=64) == E_WS
  assert lib.mm_abi_version() == 2


class _TorchPaths:
  """The sample paths in plain torch ops (CPU): what Paths.__call__ computes, for the closure's CPU test."""

  def __init__(self, paths, drift):
    t = lambda a: torch.tensor(np.asarray(a), dtype=F64)
    self.om, self.ph, self.w, self.v = t(paths.omega), t(paths.phase), t(paths.w), t(paths.v)
    self.Z, self.ls, self.var = t(drift.Z), t(drift.lengthscales), t(drift.variance)
    self.mean = None if drift.mean_c is None else t(drift.mean_c)

  def __call__(self, x):
    f = []
    for a in range(self.Z.shape[0]):
      phi = torch.sqrt(2.0 * self.var[a] / self.om.shape[1]) * torch.cos(x @ self.om[a].T + self.ph[a][None])
      kk = self.var[a] * torch.exp(-0.5 * (((x[:, None, :] - self.Z[a][None]) / self.ls[a]) ** 2).sum(-1))
      f.append((self.w[:, a] * phi).sum(-1) + (self.v[:, a] * kk).sum(-1))
    f = torch.stack(f, dim=-1)
    return f if self.mean is None else f + self.mean[None]


def _torch_system(sy, device):
  from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp
  from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
  from gpflowpilco_amd.pathwise import PathwiseSVGP
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=device)
  drift = gp_model_from_oracle(sy["drift"], device)
  pol_model = gp_model_from_oracle(sy["pol"], device)
  head = tfb.Chain([tfb.Scale(t(sy["scale"])), tfb.Shift(t(sy["shift"])), tfb.NormalCDF()])
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol_model), invlink=head)
  pdrift = PathwiseSVGP(kernel=drift.kernel, inducing_variable=drift.inducing_variable, q_mu=drift.q_mu, q_sqrt=drift.q_sqrt,
                        whiten=sy["drift"].whiten, mean_function=drift.mean_function, num_latent_gps=sy["nx"])
  system = dynamics.DynamicalSystem(drift=pdrift, policy=policy, encoder=TrigonometricEncoder(active_dims=sy["active"]),
                                    solver=dynamics.Euler())
  objective = GaussianObjective(target=t(sy["target"]), precis=t(sy["precis"]))
  return system, objective, pol_model


def test_closure_on_cpu_tensors_accepts_native_actions():
  """On CPU tensors the closure runs the torch composition whatever native_actions says: the helper's numbers."""
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _system("P", 37)
  system, objective, _ = _torch_system(sy, "cpu")
  x0 = torch.tensor(sy["x0"], dtype=F64)
  tp = _TorchPaths(sy["paths"], sy["drift"])
  with torch.no_grad(), warnings.catch_warnings():
    warnings.simplefilter("error")
    l_def = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, paths=tp)()
    l_na = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, paths=tp, native_actions=4)()
  assert torch.equal(l_def, l_na)
  assert scale_err(l_na, sy["cost_o"].sum(0)) < 1e-10


# ---- GPU: forward ---------------------------------------------------------------------------------------------------------------
def _forward_errors(name, S, dtype, device):
  """(cost error, state error) of the native rollout against the helper, with and without the Jacobian tape (bit-equal)."""
  sy = _system(name, S)
  _, _, roll = _device_case(sy, device, dtype)
  assert roll.nu == sy["nu"] and roll.nd_entries == (sy["nu"] > 1)
  x0 = torch.tensor(sy["x0"], dtype=dtype, device=device)
  cost, tape = roll(x0, H6, dt=DT, with_jacobians=False)
  cost_j, tape_j = roll(x0, H6, dt=DT, with_jacobians=True)
  assert torch.equal(cost, cost_j) and torch.equal(roll.states(tape, H6), roll.states(tape_j, H6))
  assert torch.equal(x0, torch.tensor(sy["x0"], dtype=dtype, device=device))           # the input is not modified
  return scale_err(cost, sy["cost_o"]), scale_err(roll.states(tape, H6), sy["states_o"])


@functools.lru_cache(maxsize=None)
def _one_action_f32_error(S, device):
  return max(_forward_errors("C", S, torch.float32, device))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [37, 300])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["P", "Q"])
def test_gpu_rollout_costs_and_states_match_the_helper(name, dtype, S, device):
  ec, es = _forward_errors(name, S, dtype, device)
  if dtype == torch.float32:
    one = _one_action_f32_error(S, str(device))
    print(f"forward {name} S={S} f32: cost {ec:.3e} states {es:.3e}; one-action system C, same recipe, same process: {one:.3e}")
  else:
    print(f"forward {name} S={S} f64: cost {ec:.3e} states {es:.3e}")
  tol = F64_BAR if dtype == torch.float64 else F32_BAR
  assert ec < tol and es < tol


# ---- GPU: nu = 1 through the _nd entries -------------------------------------------------------------------------------------------
def _tape_blocks(tape, S, H, nx, nd, es, jac):
  """The tape's blocks (states, drift inputs, the last step's drift sample, Jacobians), each padded to 256 bytes in the buffer
  (include/gpflowpilco_mm.h; the padding between them is never written)."""
  sizes = [(H + 1) * S * nx * es, H * S * nd * es, S * nx * es, H * S * nx * nd * es if jac else 0]
  out, off = [], 0
  for n in sizes:
    out.append(tape[off:off + n])
    off = (off + n + 255) // 256 * 256
  assert off == tape.numel()
  return out


@pytest.mark.gpu
@pytest.mark.parametrize("S", [37, 300])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_gpu_one_action_through_the_nd_entries_is_bit_equal(dtype, S, device):
  """The one-action entries are the ``_nd`` entries called with nu = 1, so both rollouts run the same kernels: what this checks
  is the wrappers' argument marshalling -- head constants by value against one-element arrays, the tape size of the one-action
  query, ``g_policy`` [npar] against [1, npar].  (While the one-action entries had kernels of their own, it was the evidence that
  the two pairs of kernels computed the same bits.)"""
  sy = _system("C", S)
  _, _, roll1 = _device_case(sy, device, dtype)
  _, _, rolln = _device_case(sy, device, dtype, nd_entries=True)
  assert not roll1.nd_entries and rolln.nd_entries
  x0 = torch.tensor(sy["x0"], dtype=dtype, device=device)
  g = torch.Generator(device="cpu").manual_seed(7)
  g_cost = torch.randn(H6, S, dtype=F64, generator=g).to(device)
  for jac in (False, True):
    c1, t1 = roll1(x0, H6, dt=DT, with_jacobians=jac)
    cn, tn = rolln(x0, H6, dt=DT, with_jacobians=jac)
    assert t1.numel() == tn.numel() and torch.equal(c1, cn)
    es = 8 if dtype == torch.float64 else 4
    for b1, bn in zip(_tape_blocks(t1, S, H6, 4, 6, es, jac), _tape_blocks(tn, S, H6, 4, 6, es, jac)):
      assert torch.equal(b1, bn)
  gp1, gx1 = roll1.backward(t1, g_cost, H6, dt=DT, want_state_grad=True)
  gpn, gxn = rolln.backward(tn, g_cost, H6, dt=DT, want_state_grad=True)
  assert gpn.shape == (1, gp1.numel()) and torch.equal(gp1, gpn.reshape(-1)) and torch.equal(gx1, gxn)
  assert float(gp1.abs().max()) > 0.0 and float(gx1.abs().max()) > 0.0


# ---- GPU: gradient ----------------------------------------------------------------------------------------------------------------
def _policy_params(pm, nu):
  ks = pm.kernel.kernels
  ivs = pm.inducing_variable.inducing_variables
  return {"q_mu": [pm.q_mu], "Z": [ivs[a].Z for a in range(nu)], "lengthscales": [ks[a].lengthscales for a in range(nu)],
          "variance": [ks[a].variance for a in range(nu)]}


@pytest.mark.gpu
@pytest.mark.parametrize("name,S", [("P", 37), ("Q", 37), ("P", 300)])
def test_gpu_gradient_of_the_mean_sample_loss(name, S, device):
  """d mean_s sum_h cost / d (q_mu, Z, lengthscales, variance of every latent, x0) through PolicyRolloutFunction, f64, H = 5:
  (i) torch autograd of a torch mirror of the composition, 1e-8 relative per tensor; (ii) central differences (h = 1e-6) of
  the numpy helper along one random direction per parameter group and for x0, 1e-6 max(1, |fd|); two backward calls on the
  same tape are bit-equal."""
  from gpflowpilco_amd.pathwise import PolicyRolloutFunction
  sy = _system(name, S)
  H, nu, nx, active = 5, sy["nu"], sy["nx"], sy["active"]
  _, pm, roll = _device_case(sy, device, F64)
  assert roll.supports_backward()
  groups = _policy_params(pm, nu)
  flat = [t for ts in groups.values() for t in ts]
  for t in flat:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)

  def native_loss():
    Zp, lsp, varp, betap, _, mcp = pm.precompute(device)
    assert Zp.shape[0] == nu and mcp.shape == (nu,)
    return PolicyRolloutFunction.apply(x0, Zp, lsp, varp, betap, mcp, roll, H, DT).sum(1).mean()       # cost [S, H]
  loss = native_loss()
  loss.backward()
  g_native = {k: [t.grad.detach().clone() for t in ts] for k, ts in groups.items()}
  g_native["x0"] = [x0.grad.detach().clone()]
  want = sy["cost_o"][:H].sum(0).mean()
  assert abs(float(loss) - want) < 1e-10

  # (i) the torch mirror: the same composition in differentiable torch ops on the path arrays
  P, dr = sy["paths"], sy["drift"]
  tt = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=device)
  om, ph, w, v = tt(P.omega), tt(P.phase), tt(P.w), tt(P.v)
  Zd, lsd, vard = tt(dr.Z), tt(dr.lengthscales), tt(dr.variance)
  target, precis = tt(sy["target"]), tt(sy["precis"])
  inactive = [i for i in range(nx) if i not in active]
  enc = lambda y: torch.cat([torch.sin(y[:, list(active)]), torch.cos(y[:, list(active)]), y[:, inactive]], dim=-1)

  def mirror_loss():
    Zp, lsp, varp, betap, _, mcp = pm.precompute(device)
    x = x0
    tot = 0.0
    for _ in range(H):
      e = enc(x)
      us = []
      for a in range(nu):
        r2 = (((e[:, None, :] - Zp[a][None]) / lsp[a]) ** 2).sum(-1)
        fp = (varp[a] * torch.exp(-0.5 * r2)) @ betap[a] + mcp[a]
        us.append(float(sy["scale"][a]) * (0.5 * torch.erfc(-fp / np.sqrt(2.0)) + float(sy["shift"][a])))
      dd = torch.cat([e, torch.stack(us, dim=-1)], dim=-1)
      f = []
      for a in range(nx):
        phi = torch.sqrt(2.0 * vard[a] / om.shape[1]) * torch.cos(dd @ om[a].T + ph[a][None])
        kk = vard[a] * torch.exp(-0.5 * (((dd[:, None, :] - Zd[a][None]) / lsd[a]) ** 2).sum(-1))
        f.append((w[:, a] * phi).sum(-1) + (v[:, a] * kk).sum(-1) + (0.0 if dr.mean_c is None else float(dr.mean_c[a])))
      x = x + DT * torch.stack(f, dim=-1)
      err = enc(x) - target
      tot = tot - torch.exp(-0.5 * ((err @ precis) * err).sum(-1))
    return tot.mean()
  for t in flat + [x0]:
    t.grad = None
  lm = mirror_loss()
  lm.backward()
  assert abs(float(lm) - float(loss)) < 1e-10
  for k, ts in list(groups.items()) + [("x0", [x0])]:
    for a, t in enumerate(ts):
      ref = t.grad.detach()
      err = float((g_native[k][a] - ref).abs().max()) / max(1e-14, float(ref.abs().max()))
      print(f"gradient {name} S={S} {k}[{a}]: native vs torch mirror {err:.2e}")
      assert err < 1e-8, (k, a, err)

  # (ii) central differences of the numpy helper along one random direction per parameter group
  rng = np.random.default_rng(5)

  def oracle_loss(pol, x_init):
    return _oracle(sy, H, pol=pol, x0=x_init).sum(0).mean()
  h = 1e-6
  for field in ("q_mu", "Z", "lengthscales", "variance"):
    base = np.asarray(getattr(sy["pol"], field), dtype=np.float64)
    dirn = rng.standard_normal(base.shape)
    vals = []
    for sgn in (1.0, -1.0):
      pol2 = copy.deepcopy(sy["pol"])
      setattr(pol2, field, base + sgn * h * dirn)
      vals.append(oracle_loss(pol2, sy["x0"]))
    fd = (vals[0] - vals[1]) / (2 * h)
    gn = g_native[field]
    got = gn[0].cpu().numpy() if field == "q_mu" else np.stack([t.cpu().numpy().reshape(base.shape[1:]) for t in gn])
    an = float((got.reshape(base.shape) * dirn).sum())
    print(f"gradient {name} S={S} {field}: native {an:+.8e} fd {fd:+.8e}")
    assert abs(fd - an) < 1e-6 * max(1.0, abs(fd)), (field, fd, an)
  dirx = rng.standard_normal(sy["x0"].shape)
  fd = (oracle_loss(sy["pol"], sy["x0"] + h * dirx) - oracle_loss(sy["pol"], sy["x0"] - h * dirx)) / (2 * h)
  an = float((g_native["x0"][0].cpu().numpy() * dirx).sum())
  assert abs(fd - an) < 1e-6 * max(1.0, abs(fd)), ("x0", fd, an)

  # two backward calls on the same tape: bit-equal (fixed-order sums, no atomics)
  with torch.no_grad():
    _, tape = roll(x0.detach(), H, dt=DT, with_jacobians=True)
    g_cost = torch.full((H, S), 1.0 / S, dtype=F64, device=device)
    a1, b1 = roll.backward(tape, g_cost, H, dt=DT, want_state_grad=True)
    a2, b2 = roll.backward(tape, g_cost, H, dt=DT, want_state_grad=True)
  assert a1.shape == (nu, 12 * sy["ne"] + 12 + sy["ne"] + 2) and torch.equal(a1, a2) and torch.equal(b1, b2)


# ---- GPU: the closure -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_closure_runs_two_actions_natively_when_asked(device):
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _system("P", 37)
  S, H = 37, 5
  system, objective, pm = _torch_system(sy, device)
  params = [t for ts in _policy_params(pm, 2).values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  g = torch.Generator(device=device).manual_seed(3)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)
  paths = system.drift.generate_paths(S, 256, dtype=F64, device=device, generator=g)

  def run(**kw):
    for t in params + [x0]:
      t.grad = None
    loss = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, **kw)()
    loss.mean().backward()
    return loss.detach(), [t.grad.detach().clone() for t in params + [x0]]
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    ln, gn = run(native_actions=2)
    lf, _ = run(native_actions=4, native=True)                                    # native=True does not raise
    lt, gt = run(native=False)
  assert ln.shape == (S,) and torch.equal(ln, lf)
  el = float((ln - lt).abs().max())
  print(f"closure P: native vs torch composition, loss {el:.2e}")
  assert el < 1e-10
  for a_, b_ in zip(gn, gt):
    eg = float((a_ - b_).abs().max()) / max(1e-12, float(b_.abs().max()))
    assert eg < 1e-8, eg
  with torch.no_grad(), warnings.catch_warnings():
    warnings.simplefilter("error")
    l0 = pathwise_policy_loss_closure(system, objective, lambda: x0.detach(), H, dt=DT, paths=paths, native_actions=2)()
  assert float((l0 - ln).abs().max()) < 1e-12
  # the default arguments: today's routing to the letter
  with torch.no_grad():
    with pytest.warns(RuntimeWarning, match=r"nu > 1"):
      ld = pathwise_policy_loss_closure(system, objective, lambda: x0.detach(), H, dt=DT, paths=paths)()
    lt0 = pathwise_policy_loss_closure(system, objective, lambda: x0.detach(), H, dt=DT, paths=paths, native=False)()
  assert torch.equal(ld, lt0)
  with pytest.raises(ValueError):
    pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, native=True)
  with pytest.raises(ValueError):
    pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, native=True, native_actions=1)


@pytest.mark.gpu
def test_gpu_closure_falls_back_for_nine_drift_inputs_and_names_the_dimension(device):
  """nx 5, two angles, two actions: nx + na + nu = 9 > 8.  native_actions=4 falls back, naming the dimension, with the torch
  composition's numbers."""
  from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp
  from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  from gpflowpilco_amd.pathwise import PathwiseSVGP
  nx, active, nu, S, H = 5, (0, 1), 2, 16, 3
  ne = nx + len(active)
  base = make_svgp(nx, 40, ne + nu, seed=61, ls_bounds=(0.9, 3.0)).to_model(device)
  drift = PathwiseSVGP(kernel=base.kernel, inducing_variable=base.inducing_variable, q_mu=base.q_mu, q_sqrt=base.q_sqrt, whiten=True,
                       num_latent_gps=nx)
  pol_o = random_svgp_params(seed=62, L=nu, M=10, d=ne, whiten=True, ls_bounds=(0.9, 2.0), mean=False)
  pol_o.q_mu = 0.2 * pol_o.q_mu
  pol = gp_model_from_oracle(pol_o, device)
  t = lambda a: torch.tensor(a, dtype=F64, device=device)
  head = tfb.Chain([tfb.Scale(t(SCALE[:nu])), tfb.Shift(t(SHIFT[:nu])), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=active), solver=dynamics.Euler())
  objective = GaussianObjective(target=torch.zeros(ne, dtype=F64, device=device), precis=torch.eye(ne, dtype=F64, device=device))
  g = torch.Generator(device=device).manual_seed(4)
  x0 = 0.2 + 0.6 * torch.rand(S, nx, dtype=F64, device=device, generator=g)
  paths = drift.generate_paths(S, 256, dtype=F64, device=device, generator=g)
  with torch.no_grad():
    with pytest.warns(RuntimeWarning, match=r"nx \+ na \+ nu = 9") as rec:
      closure = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, native_actions=4)
      l1 = closure()
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1 and "torch composition" in str(rec[0].message)
    with warnings.catch_warnings():
      warnings.simplefilter("error")                                              # once: the second call is silent
      closure()
      lt = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, native=False)()
  assert torch.equal(l1, lt) and torch.isfinite(l1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pol_M", [12, 100, 204], ids=["M12", "M100", "M204"])
def test_gpu_closure_with_four_actions_and_the_lds_bound(pol_M, device):
  """nx 2, both angles, four actions (ne 4, nd 8).  M = 12: loss and gradients run natively and equal the torch composition.
  M = 100: the same with 81 KB of LDS in the reverse sweep (above the 64 KB a kernel gets without asking).  M = 204: one centre past the reverse sweep's LDS bound for nu = 4, ne = 4 (203) -- supports_backward() is false, a gradient
  falls back naming the bound, and the forward (which has no such bound) still runs natively."""
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  from gpflowpilco_amd.pathwise import PolicyRollout
  nx, active, nu, S, H = 2, (0, 1), 4, 70, 3
  ne = 4
  drift = oracle_params(make_svgp(nx, 40, ne + nu, seed=71, ls_bounds=(0.8, 3.0)))
  drift.Z[..., ne:] = 4.0 * drift.Z[..., ne:] - 2.0
  pol = random_svgp_params(seed=72, L=nu, M=pol_M, d=ne, whiten=True, ls_bounds=(0.8, 2.0), mean=True, separate_Z=True)
  pol.q_mu = 0.3 * pol.q_mu
  rng = np.random.default_rng(73)
  sy = dict(nx=nx, active=active, nu=nu, drift=drift, pol=pol, scale=np.array([2.0, 1.5, 1.0, 0.8]),
            shift=np.array([-0.5, -0.4, -0.6, -0.3]), target=np.array([0.0, 0.0, 1.0, 1.0]), precis=np.eye(ne))
  system, objective, pm = _torch_system(sy, device)
  params = [t for ts in _policy_params(pm, nu).values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  g = torch.Generator(device=device).manual_seed(5)
  x0 = torch.tensor(rng.uniform(0.2, 0.8, size=(S, nx)), dtype=F64, device=device, requires_grad=True)
  paths = system.drift.generate_paths(S, 256, dtype=F64, device=device, generator=g)
  roll = PolicyRollout(paths, pm.packed(F64, False, device), nx=nx, active_dims=active, head_scale=tuple(sy["scale"]),
                       head_shift=tuple(sy["shift"]), target=objective.target, precis=objective.precis)
  assert roll.nu == 4 and roll.supports_backward() == (pol_M != 204)

  def run(**kw):
    for t in params + [x0]:
      t.grad = None
    loss = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, **kw)()
    loss.mean().backward()
    return loss.detach(), [t.grad.detach().clone() for t in params + [x0]]
  lt, gt = run(native=False)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    with torch.no_grad():                                                          # the forward: native for both sizes
      l0 = pathwise_policy_loss_closure(system, objective, lambda: x0.detach(), H, dt=DT, paths=paths, native_actions=4)()
      cost, _ = roll(x0.detach(), H, dt=DT)
  assert torch.equal(l0, cost.sum(0)) and float((l0 - lt).abs().max()) < 1e-10
  if pol_M != 204:
    with warnings.catch_warnings():
      warnings.simplefilter("error")
      ln, gn = run(native_actions=4)
    assert float((ln - lt).abs().max()) < 1e-10
    for a_, b_ in zip(gn, gt):
      assert float((a_ - b_).abs().max()) < 1e-8 * max(1e-12, float(b_.abs().max()))
  else:
    with pytest.warns(RuntimeWarning, match=r"LDS bound"):
      lw, gw = run(native_actions=4)
    assert torch.equal(lw, lt) and all(torch.equal(a_, b_) for a_, b_ in zip(gw, gt))
    with pytest.raises(ValueError, match="160 KiB"):
      roll.backward(torch.empty(8, dtype=torch.uint8, device=device), torch.zeros(H, S, dtype=F64, device=device), H, dt=DT)


# ---- GPU: capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_forward_replays_bit_equal_under_graph_capture(device):
  """One forward call captured into a HIP graph (after an eager warm-up on a side stream, as loops.GraphedPolicyLoss does):
  two replays give the eager numbers bit for bit."""
  sy = _system("P", 37)
  _, _, roll = _device_case(sy, device, F64)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device)
  dev = x0.device
  eager, _ = roll(x0, H6, dt=DT)
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  with torch.cuda.stream(side):
    roll(x0, H6, dt=DT)
  torch.cuda.current_stream(dev).wait_stream(side)
  torch.cuda.synchronize(dev)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    cost, _ = roll(x0, H6, dt=DT)
  for _ in range(2):
    cost.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(cost, eager)
  assert scale_err(cost, sy["cost_o"]) < F64_BAR
