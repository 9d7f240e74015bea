"""The pathwise side for 9 to 16 drift inputs: the Jacobian pass of the weight stream over half sample groups
(csrc/mm_pathwise.hip, Paths.eval_jac / Paths.__call__ under autograd), the _wide entries of the policy rollout and its reverse
sweep (csrc/mm_pathwise_policy.hip, pathwise.PolicyRollout(wide=True)) and loops.pathwise_policy_loss_closure(native_inputs=16),
against oracle.pathwise_oracle and its multi-action fold tests/pathwise_multiaction_oracle.py.

Systems (recipe of tests/test_pathwise_multiaction.py::_system: drift M 50, K 130, policy M 12 with its own Z per latent, w and v
x 0.3, H = 6, dt = 0.5, S = 37 and S = 300; here precis x 0.25, which keeps the costs of the wider encodings away from 0):
  W1  nx 6,  angles (2, 4),       nu 1 -> ne 8,  nd 9    (the cart-double-pendulum)     seed 70
  W2  nx 5,  angles (0, 1),       nu 2 -> ne 7,  nd 9                                   seed 80
  W3  nx 8,  angles (0, 2, 4, 6), nu 4 -> ne 12, nd 16   (the reverse sweep's tightest LDS case)  seed 90
  W4  nx 12, angle (0,),          nu 3 -> ne 13, nd 16                                  seed 100

Bars: f64 1e-10 and f32 5e-3 on costs and taped states; f 1e-11 / 2e-3 and J 1e-7 / 3e-3 for the paths and their Jacobian
(tests/test_pathwise.py's bars for the same quantities); gradients 1e-8 relative per tensor against torch autograd of a torch
mirror and 1e-6 max(1, |fd|) against central differences of the numpy helper."""
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
from tests import test_pathwise_multiaction as tm          # its torch wiring of a system, tape blocks and system P (nd 8)
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, scale_err

F64 = torch.float64
SCALE, SHIFT = (2.0, 1.5, 1.0, 1.2), (-0.5, -0.4, -0.6, -0.45)
SYSTEMS = {"W1": dict(nx=6, active=(2, 4), nu=1, seed=70),
           "W2": dict(nx=5, active=(0, 1), nu=2, seed=80),
           "W3": dict(nx=8, active=(0, 2, 4, 6), nu=4, seed=90),
           "W4": dict(nx=12, active=(0,), nu=3, seed=100)}
H6, DT = 6, 0.5
F32_BAR, F64_BAR = 5e-3, 1e-10


@functools.lru_cache(maxsize=None)
def _system(name, S, pol_M=12):
  """The numpy side of a system and its oracle rollout (computed once, shared, never modified)."""
  c = SYSTEMS[name]
  nx, active, nu, seed = c["nx"], c["active"], c["nu"], c["seed"]
  na = len(active); ne = nx + na; nd = ne + nu
  rng = np.random.default_rng(seed)
  drift = oracle_params(make_svgp(nx, 50, nd, seed=seed + 1, ls_bounds=(0.8, 3.0)))
  drift.Z[..., ne:] = 4.0 * drift.Z[..., ne:] - 2.0                       # action axes in [-2, 2]
  pol = random_svgp_params(seed=seed + 2, L=nu, M=pol_M, d=ne, whiten=True, ls_bounds=(0.8, 2.0), mean=True, separate_Z=True)
  pol.q_mu = 0.3 * pol.q_mu
  paths = pw.draw_paths(rng, drift, S, 130)
  paths.w *= 0.3; paths.v *= 0.3
  x0 = rng.uniform(0.2, 0.8, size=(S, nx))
  target = np.zeros(ne); target[na:2 * na] = 1.0; target[2 * na:] = 0.1
  A = rng.standard_normal((ne, ne))
  precis = 0.25 * (0.5 * (A @ A.T) / ne + 0.5 * np.eye(ne))
  scale, shift = np.array(SCALE[:nu]), np.array(SHIFT[:nu])
  cost_o, states_o = pmo.policy_rollout_costs_nd(paths, drift, pol, scale, shift, active, target, precis, x0, H6, dt=DT, keep=True)
  return dict(c, S=S, na=na, ne=ne, nd=nd, drift=drift, pol=pol, paths=paths, x0=x0, target=target, precis=precis, scale=scale,
              shift=shift, cost_o=cost_o, states_o=states_o)


def _oracle(sy, H, pol=None, x0=None, **kw):
  return pmo.policy_rollout_costs_nd(sy["paths"], sy["drift"], sy["pol"] if pol is None else pol, sy["scale"], sy["shift"],
                                     sy["active"], sy["target"], sy["precis"], sy["x0"] if x0 is None else x0, H, dt=DT, **kw)


def _device_case(sy, device, dtype, wide=True, nd_entries=None):
  from gpflowpilco_amd.pathwise import PolicyRollout, paths_from_arrays
  P, dr = sy["paths"], sy["drift"]
  gp_paths = paths_from_arrays(P.omega, P.phase, P.w, P.v, dr.Z, dr.lengthscales, dr.variance, dr.mean_c, dtype=dtype, device=device)
  pol_model = gp_model_from_oracle(sy["pol"], device)
  roll = PolicyRollout(gp_paths, pol_model.packed(F64, False, device), nx=sy["nx"], active_dims=sy["active"],
                       head_scale=tuple(sy["scale"]), head_shift=tuple(sy["shift"]), target=torch.tensor(sy["target"]),
                       precis=torch.tensor(sy["precis"]), nd_entries=nd_entries, wide=wide)
  return gp_paths, pol_model, roll


# ---- CPU: the systems, the ABI, the closure's argument ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W1", "W2", "W3", "W4"])
def test_systems_are_well_posed_and_wrong_wirings_are_far_outside_the_f32_bar(name):
  """Costs away from both ends of -exp(-q / 2), states inside the data's support; the actions fed to the drift in rotated order
  and every action evaluated from latent 0 each move the costs by at least 4x the f32 bar.  W1 has one action: there is no
  second input or latent to confuse, both permutations are the identity and the guards say nothing about it (asserted as 0)."""
  sy = _system(name, 37)
  nu = sy["nu"]
  assert np.isfinite(sy["cost_o"]).all() and np.abs(sy["states_o"]).max() < 3.0
  assert sy["cost_o"].max() < -0.05 and sy["cost_o"].min() > -0.999
  rot = scale_err(_oracle(sy, H6, feed_order=[(a + 1) % nu for a in range(nu)]), sy["cost_o"])
  lat0 = scale_err(_oracle(sy, H6, latent_of=[0] * nu), sy["cost_o"])
  print(f"guards {name}: rotated feed {rot:.2e}, every action from latent 0 {lat0:.2e}; |states| < {np.abs(sy['states_o']).max():.2f}, "
        f"costs in [{sy['cost_o'].min():.3f}, {sy['cost_o'].max():.3f}]")
  if nu == 1:
    assert rot == 0.0 and lat0 == 0.0
  else:
    assert rot >= 4 * F32_BAR and lat0 >= 4 * F32_BAR


def test_argument_validation_and_sizes_of_the_wide_entries_without_gpu():
  lib = _lib.lib()
  buf = (ctypes.c_char * 64)()
  p = ctypes.addressof(buf)
  F64c, F32c = _lib.MM_F64, _lib.MM_F32
  E_ARG, E_DIM, E_DTYPE, E_WS = -1, -2, -3, -4
  act = (ctypes.c_int32 * 2)(0, 1)
  sc = (ctypes.c_double * 4)(2.0, 1.5, 1.0, 1.0)
  sh = (ctypes.c_double * 4)(-0.5, -0.4, -0.6, 0.0)
  tb = lib.mm_pathwise_tape_bytes_nd
  sbw, sbn, sb1 = lib.mm_pathwise_backward_scratch_bytes_wide, lib.mm_pathwise_backward_scratch_bytes_nd, lib.mm_pathwise_backward_scratch_bytes
  # ---- the size query: the _nd sizes wherever both answer, beyond them up to ne + nu = 16
  for nu in (1, 2, 3, 4):
    for ne in range(1, 17):
      for M in (12, 64, 256):
        n, w = sbn(300, M, ne, nu), sbw(300, M, ne, nu)
        assert n == 0 or n == w, (nu, ne, M)
        if ne + nu > 16:
          assert w == 0
        elif M == 64:
          assert w > 0, (nu, ne)                                                   # every shape with M <= 64 and nd <= 16
  assert sbw(300, 30, 7, 2) == 2 * sb1(300, 30, 7) > 0 and sbn(300, 30, 7, 2) == 0
  assert sbw(300, 30, 6, 0) == 0 and sbw(300, 30, 4, 5) == 0 and sbw(0, 30, 6, 2) == 0 and sbw(300, 257, 6, 2) == 0
  assert sbw(300, 30, 13, 4) == 0 and sbw(300, 30, 16, 1) == 0                     # ne + nu = 17

  def lds(nu, M, ne):
    return 8 * (nu * (M * ne + M + ne) + ne + ne * ne + 8 + 4 * nu * (M * ne + M + ne + 2))
  assert lds(4, 77, 12) <= 160 * 1024 < lds(4, 78, 12)
  assert sbw(300, 77, 12, 4) > 0 and sbw(300, 78, 12, 4) == 0                      # the LDS bound at its edge

  # ---- the forward entry (defaults: nx 5, two angles, two actions: nd 9)
  def fwd(nu=2, nx=5, na=2, dtype=F64c, a=act, omega=p, pol=p, pol_bytes=1 << 30, pM=12, scale=sc, shift=sh, x0=p, tape=p,
          tape_bytes=1 << 40, S=37):
    return lib.mm_pathwise_policy_rollout_wide(S, 128, 256, dtype, 6, 0.5, nx, na, a, nu, omega, p, p, p, p, p, p, None, p, pol,
                                               pol_bytes, pM, scale, shift, p, p, x0, p, tape, tape_bytes, 1, None)
  assert fwd(nu=0) == E_DIM and fwd(nu=5) == E_DIM
  assert fwd(nx=13, na=2, nu=2) == E_DIM and fwd(nx=14, na=2, nu=1) == E_DIM       # nd = 17
  assert fwd(pM=257) == E_DIM
  assert fwd(omega=None) == E_ARG and fwd(pol=None) == E_ARG and fwd(scale=None) == E_ARG and fwd(x0=None) == E_ARG
  assert fwd(a=None) == E_ARG and fwd(S=0) == E_ARG and fwd(dtype=7) == E_DTYPE
  need = tb(37, 6, 5, 2, 2, F64c, 1)
  assert need > 0 and fwd(tape_bytes=need - 1) == E_WS                             # short tape: nd 9 passed the dimension check
  assert fwd(tape_bytes=need, pol_bytes=64) == E_WS
  assert fwd(nx=12, na=2, nu=2, tape_bytes=tb(37, 6, 12, 2, 2, F64c, 1) - 1) == E_WS   # nd 16 as well

  # ---- the backward entry
  def bwd(nu=2, nx=5, na=2, dtype=F64c, a=act, pol=p, pol_bytes=1 << 30, pM=12, scale=sc, shift=sh, tape=p, tape_bytes=1 << 40,
          g_cost=p, g_pol=p, scratch=p, scratch_bytes=1 << 40):
    return lib.mm_pathwise_policy_rollout_backward_wide(37, dtype, 6, 0.5, nx, na, a, nu, pol, pol_bytes, pM, scale, shift, p, p,
                                                        tape, tape_bytes, g_cost, g_pol, None, scratch, scratch_bytes, None)
  assert bwd(nu=0) == E_DIM and bwd(nu=5) == E_DIM and bwd(nx=13, na=2, nu=2) == E_DIM and bwd(pM=257) == E_DIM
  assert bwd(nx=10, na=2, nu=4, pM=78) == E_DIM                                    # ne 12, nu 4, M 78: beyond the LDS bound
  assert bwd(pol=None) == E_ARG and bwd(tape=None) == E_ARG and bwd(g_cost=None) == E_ARG and bwd(scratch=None) == E_ARG
  assert bwd(dtype=7) == E_DTYPE
  assert bwd(tape_bytes=need - 1) == E_WS
  assert bwd(tape_bytes=need, scratch_bytes=sbw(37, 12, 7, 2) - 1) == E_WS
  assert bwd(nx=10, na=2, nu=4, pM=77, tape_bytes=tb(37, 6, 10, 2, 4, F64c, 1) - 1) == E_WS   # the edge shape is taken
  # the narrow entries keep their bound, and the ABI its version
  assert lib.mm_pathwise_policy_rollout_nd(37, 128, 256, F64c, 6, 0.5, 5, 2, act, 2, p, p, p, p, p, p, p, None, p, p, 1 << 30, 12,
                                           sc, sh, p, p, p, p, p, 1 << 40, 1, None) == E_DIM
  assert lib.mm_abi_version() == 2
  assert F32c != F64c


def test_closure_on_cpu_tensors_accepts_native_inputs():
  """On CPU tensors the closure runs the torch composition whatever native_inputs says: the helper's numbers."""
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _system("W2", 37)
  system, objective, _ = tm._torch_system(sy, "cpu")
  x0 = torch.tensor(sy["x0"], dtype=F64)
  tp = tm._TorchPaths(sy["paths"], sy["drift"])
  with torch.no_grad(), warnings.catch_warnings():
    warnings.simplefilter("error")
    l_def = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, paths=tp)()
    l_wide = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, paths=tp, native_actions=4, native_inputs=16)()
    l_more = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, paths=tp, native_actions=4, native_inputs=40)()
  assert torch.equal(l_def, l_wide) and torch.equal(l_def, l_more)
  assert scale_err(l_wide, sy["cost_o"].sum(0)) < 1e-10


# ---- GPU 1: the Jacobian pass -----------------------------------------------------------------------------------------------------
JAC_LS = (0.5, 1.5)


@functools.lru_cache(maxsize=None)
def _jac_case(d, L, K, M):
  """Paths of L latents on d inputs and their oracle values: f, and J by central differences (h = 1e-6).

  The central differences carry their own rounding error, about eps sum_m |v_m k_m| / h: it grows with the update weights
  v = Kuu^-1 (u - Phi w), hence with the conditioning of Kuu.  With 100 centres in the unit cube and lengthscales in (0.8, 3.0)
  (|v| up to 280) the differences are themselves 1.2e-7 of max |J| from the closed-form Jacobian at d = 9, beyond the 1e-7 bar
  they are to serve; with lengthscales in (0.5, 1.5) they are within 1.3e-8 on every shape used here, an eighth of the bar
  (test_central_differences_of_the_oracle_are_a_reference_for_the_f64_bar asserts a quarter, without a GPU)."""
  S = 37
  po = oracle_params(make_svgp(L, M, d, seed=20 + d + L, ls_bounds=JAC_LS, mean_c=True))
  rng = np.random.default_rng(100 * d + L)
  paths = pw.draw_paths(rng, po, S, K)
  x = rng.uniform(0.2, 0.8, size=(S, d))
  fo = pw.eval_paths(paths, po, x)
  Jo = np.empty((S, L, d))
  h = 1e-6
  for k in range(d):
    dx = np.zeros(d); dx[k] = h
    Jo[:, :, k] = (pw.eval_paths(paths, po, x + dx) - pw.eval_paths(paths, po, x - dx)) / (2 * h)
  return po, paths, x, fo, Jo


def _analytic_jacobian(paths, po, x):
  """d f_s / d x_s of pw.eval_paths in closed form, float64 (its own rounding is 1e-13 of max |J| on these shapes)."""
  S, L, K = paths.w.shape
  J = np.zeros((S, L, x.shape[1]))
  for a in range(L):
    t = -np.sqrt(2.0 * po.variance[a] / K) * paths.w[:, a, :] * np.sin(x @ paths.omega[a].T + paths.phase[a][None, :])
    J[:, a, :] = t @ paths.omega[a]
    diff = (x[:, None, :] - po.Z[a][None]) / po.lengthscales[a]                    # [S, M, d]
    tv = paths.v[:, a, :] * po.variance[a] * np.exp(-0.5 * np.sum(diff * diff, -1))
    J[:, a, :] -= np.sum(tv[:, :, None] * diff / po.lengthscales[a], 1)
  return J


@functools.lru_cache(maxsize=None)
def _narrow_f32_jacobian_error(device):
  """The f32 Jacobian error of the d = 6 case of tests/test_pathwise.py::_policy_case (the narrow pass), same process."""
  from tests.test_pathwise import _policy_case
  c = _policy_case(device, torch.float32)
  x = np.random.default_rng(9).uniform(0.2, 0.8, size=(37, 6))
  _, J = c["gp_paths"].eval_jac(torch.tensor(x, dtype=torch.float32, device=device))
  Jo = np.empty((37, 4, 6))
  for k in range(6):
    dx = np.zeros(6); dx[k] = 1e-6
    Jo[:, :, k] = (pw.eval_paths(c["paths"], c["drift"], x + dx) - pw.eval_paths(c["paths"], c["drift"], x - dx)) / 2e-6
  return scale_err(J, Jo)


# where the launch rule (dk + 1)(K + M) sizeof(T) <= 144 KiB puts a shape with dk = 16: K + M <= 1084 (f64), 2168 (f32), after
# padding to 128 (f64) / 256 (f32) terms
_KM = {("lds", torch.float64): (200, 100),    # 256 + 128
       ("lds", torch.float32): (200, 100),    # 256 + 256
       ("plain", torch.float64): (1000, 100), # 1024 + 128
       ("plain", torch.float32): (2048, 100)} # 2048 + 256


@pytest.mark.parametrize("K", [200, 1000, 2048])
@pytest.mark.parametrize("L", [3, 6])
@pytest.mark.parametrize("d", [9, 13, 16])
def test_central_differences_of_the_oracle_are_a_reference_for_the_f64_bar(d, L, K):
  """The reference of the GPU Jacobian test against the closed-form Jacobian of the same numpy paths: its own error has to sit
  well inside the 1e-7 bar it serves (a quarter is asserted; the printed figures are the record)."""
  po, paths, x, _, Jo = _jac_case(d, L, K, 100)
  e = scale_err(_analytic_jacobian(paths, po, x), Jo)
  print(f"central differences d={d} L={L} K={K}: {e:.3e} of max |J| from the closed form; |v| < {np.abs(paths.v).max():.1f}")
  assert e < 2.5e-8


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["lds", "plain"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [3, 6])
@pytest.mark.parametrize("d", [9, 13, 16])
def test_gpu_wide_jacobian_of_the_paths(d, L, dtype, kernel, device):
  """f bit-equal to the plain pass and within the bar of the oracle; J against central differences of the oracle; autograd
  through Paths.__call__ gives the column sums of J.  Both kernels: operands in LDS, and streamed (six latents give a wave of
  the streaming kernel a second latent).  f32 J: 3e-3, or twice the narrow pass's own f32 error on the d = 6 case measured in the
  same process should a shape miss 3e-3 while f64 passes (the printed figures are the record).  Measured on an MI355X: f64 f
  1.1e-14 ... 1.0e-13, J 1.5e-9 ... 1.1e-8 (the central differences' own error, see _jac_case); f32 f 4.2e-6 ... 3.2e-5, J 1.9e-6 ...
  9.2e-6, so no shape needed the narrow pass's figure."""
  from gpflowpilco_amd.pathwise import paths_from_arrays
  K, M = _KM[(kernel, dtype)]
  po, paths, x, fo, Jo = _jac_case(d, L, K, M)
  gp_paths = paths_from_arrays(paths.omega, paths.phase, paths.w, paths.v, po.Z, po.lengthscales, po.variance, po.mean_c,
                               dtype=dtype, device=device)
  _, _, Mp, Kp, _ = gp_paths._dims()
  es = 8 if dtype == torch.float64 else 4
  assert (17 * (Kp + Mp) * es <= 144 * 1024) == (kernel == "lds")
  xt = torch.tensor(x, dtype=dtype, device=device)
  f, J = gp_paths.eval_jac(xt)
  assert J.shape == (37, L, d)
  assert torch.equal(f, gp_paths(xt))
  ef, eJ = scale_err(f, fo), scale_err(J, Jo)
  print(f"wide jacobian d={d} L={L} {kernel} {'f64' if es == 8 else 'f32'}: f {ef:.3e} J {eJ:.3e}")
  assert ef < (1e-11 if dtype == torch.float64 else 2e-3)
  barJ = 1e-7 if dtype == torch.float64 else 3e-3
  if dtype == torch.float32 and eJ >= barJ:
    narrow = _narrow_f32_jacobian_error(str(device))
    print(f"  narrow pass, d = 6 case, f32, same process: J {narrow:.3e}")
    barJ = max(barJ, 2 * narrow)
  assert eJ < barJ
  xg = xt.clone().requires_grad_(True)
  fg = gp_paths(xg)
  assert torch.equal(fg.detach(), f)
  (gx,) = torch.autograd.grad(fg.sum(), xg)
  assert scale_err(gx, J.double().sum(1).cpu().numpy()) < (1e-13 if dtype == torch.float64 else 1e-6)


@pytest.mark.gpu
def test_gpu_jacobian_is_refused_beyond_sixteen_inputs(device):
  from gpflowpilco_amd.pathwise import paths_from_arrays
  po = oracle_params(make_svgp(2, 20, 17, seed=4, ls_bounds=(0.8, 3.0)))
  paths = pw.draw_paths(np.random.default_rng(0), po, 8, 64)
  gp_paths = paths_from_arrays(paths.omega, paths.phase, paths.w, paths.v, po.Z, po.lengthscales, po.variance, po.mean_c,
                               dtype=F64, device=device)
  x = torch.full((8, 17), 0.5, dtype=F64, device=device)
  assert torch.isfinite(gp_paths(x)).all()
  with pytest.raises(Exception, match="mm_pathwise_eval_jac"):
    gp_paths.eval_jac(x)


# ---- GPU 2: forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("S", [37, 300])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["W1", "W2", "W3", "W4"])
def test_gpu_wide_rollout_costs_and_states_match_the_helper(name, dtype, S, device):
  sy = _system(name, S)
  _, _, roll = _device_case(sy, device, dtype)
  assert roll.nu == sy["nu"] and roll.nd == sy["nd"] and roll.wide and roll.nd_entries
  x0 = torch.tensor(sy["x0"], dtype=dtype, device=device)
  cost, tape = roll(x0, H6, dt=DT, with_jacobians=False)
  cost_j, tape_j = roll(x0, H6, dt=DT, with_jacobians=True)
  assert torch.equal(cost, cost_j) and torch.equal(roll.states(tape, H6), roll.states(tape_j, H6))
  assert torch.equal(x0, torch.tensor(sy["x0"], dtype=dtype, device=device))
  ec, es = scale_err(cost, sy["cost_o"]), scale_err(roll.states(tape, H6), sy["states_o"])
  print(f"wide forward {name} S={S} {dtype}: cost {ec:.3e} states {es:.3e}")
  tol = F64_BAR if dtype == torch.float64 else F32_BAR
  assert ec < tol and es < tol


@pytest.mark.gpu
def test_gpu_wide_forward_with_policy_blocks_above_64_kb_of_lds(device):
  """W3's wiring with 200 centres per latent: the head kernel's four policy blocks take 84 KB of LDS (more than a kernel gets
  without asking); the reverse sweep does not take the shape."""
  sy = _system("W3", 37, pol_M=200)
  _, _, roll = _device_case(sy, device, F64)
  assert not roll.supports_backward()
  cost, tape = roll(torch.tensor(sy["x0"], dtype=F64, device=device), H6, dt=DT)
  assert scale_err(cost, sy["cost_o"]) < F64_BAR and scale_err(roll.states(tape, H6), sy["states_o"]) < F64_BAR


def test_wide_rollout_refuses_more_than_sixteen_inputs_and_narrow_more_than_eight():
  from gpflowpilco_amd.pathwise import PolicyRollout

  class _Paths:
    num_samples, dtype = 8, F64
    def __init__(self, L, d): self.L, self.d = L, d
    def _dims(self): return 8, self.L, 128, 128, self.d

  class _Pack:
    def __init__(self, L, d): self.L, self.M, self.d = L, 12, d
  with pytest.raises(ValueError, match="<= 16"):
    PolicyRollout(_Paths(12, 17), _Pack(4, 13), nx=12, active_dims=(0,), head_scale=1.0, head_shift=0.0, target=None, precis=None,
                  wide=True)
  with pytest.raises(ValueError, match="<= 8"):
    PolicyRollout(_Paths(5, 9), _Pack(2, 7), nx=5, active_dims=(0, 1), head_scale=1.0, head_shift=0.0, target=None, precis=None)


# ---- GPU 3: nd <= 8 through the wide entries ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_gpu_system_p_through_the_wide_entries_is_bit_equal(dtype, device):
  sy = tm._system("P", 37)
  S = 37
  _, _, rolln = _device_case(sy, device, dtype, wide=False)
  _, _, rollw = _device_case(sy, device, dtype, wide=True)
  assert rolln.nd_entries and not rolln.wide and rollw.wide and rollw.nd == 8
  x0 = torch.tensor(sy["x0"], dtype=dtype, device=device)
  g_cost = torch.randn(H6, S, dtype=F64, generator=torch.Generator(device="cpu").manual_seed(7)).to(device)
  es = 8 if dtype == torch.float64 else 4
  for jac in (False, True):
    cn, tn = rolln(x0, H6, dt=DT, with_jacobians=jac)
    cw, tw = rollw(x0, H6, dt=DT, with_jacobians=jac)
    assert tn.numel() == tw.numel() and torch.equal(cn, cw)
    for bn, bw in zip(tm._tape_blocks(tn, S, H6, 4, 8, es, jac), tm._tape_blocks(tw, S, H6, 4, 8, es, jac)):
      assert torch.equal(bn, bw)
  gpn, gxn = rolln.backward(tn, g_cost, H6, dt=DT, want_state_grad=True)
  gpw, gxw = rollw.backward(tw, g_cost, H6, dt=DT, want_state_grad=True)
  assert torch.equal(gpn, gpw) and torch.equal(gxn, gxw) and float(gpn.abs().max()) > 0.0 and float(gxn.abs().max()) > 0.0


# ---- GPU 4: gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,S", [("W1", 37), ("W2", 37), ("W3", 37), ("W4", 37), ("W2", 300)])
def test_gpu_wide_gradient_of_the_mean_sample_loss(name, S, device):
  """d mean_s sum_h cost / d (q_mu, Z, lengthscales, variance of every latent, x0) through PolicyRolloutFunction on the wide
  entries, f64, H = 5: (i) torch autograd of a torch mirror of the composition, 1e-8 relative per tensor; (ii) central
  differences (h = 1e-6) of the numpy helper along one random direction per parameter group and for x0, 1e-6 max(1, |fd|); two
  backward calls on the same tape are bit-equal."""
  from gpflowpilco_amd.pathwise import PolicyRolloutFunction
  sy = _system(name, S)
  H, nu, nx, active = 5, sy["nu"], sy["nx"], sy["active"]
  _, pm, roll = _device_case(sy, device, F64)
  assert roll.supports_backward()
  groups = tm._policy_params(pm, nu)
  flat = [t for ts in groups.values() for t in ts]
  for t in flat:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)
  Zp, lsp, varp, betap, _, mcp = pm.precompute(device)
  loss = PolicyRolloutFunction.apply(x0, Zp, lsp, varp, betap, mcp, roll, H, DT).sum(1).mean()
  loss.backward()
  g_native = {k: [t.grad.detach().clone() for t in ts] for k, ts in groups.items()}
  g_native["x0"] = [x0.grad.detach().clone()]
  assert abs(float(loss.detach()) - sy["cost_o"][:H].sum(0).mean()) < 1e-10

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
      print(f"wide gradient {name} S={S} {k}[{a}]: native vs torch mirror {err:.2e}")
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
    print(f"wide gradient {name} S={S} {field}: native {an:+.8e} fd {fd:+.8e}")
    assert abs(fd - an) < 1e-6 * max(1.0, abs(fd)), (field, fd, an)
  dirx = rng.standard_normal(sy["x0"].shape)
  fd = (oracle_loss(sy["pol"], sy["x0"] + h * dirx) - oracle_loss(sy["pol"], sy["x0"] - h * dirx)) / (2 * h)
  an = float((g_native["x0"][0].cpu().numpy() * dirx).sum())
  assert abs(fd - an) < 1e-6 * max(1.0, abs(fd)), ("x0", fd, an)

  with torch.no_grad():
    _, tape = roll(x0.detach(), H, dt=DT, with_jacobians=True)
    g_cost = torch.full((H, S), 1.0 / S, dtype=F64, device=device)
    a1, b1 = roll.backward(tape, g_cost, H, dt=DT, want_state_grad=True)
    a2, b2 = roll.backward(tape, g_cost, H, dt=DT, want_state_grad=True)
  assert a1.shape == (nu, 12 * sy["ne"] + 12 + sy["ne"] + 2) and torch.equal(a1, a2) and torch.equal(b1, b2)


# ---- GPU 5: the closure -------------------------------------------------------------------------------------------------------------
def _closure_case(sy, device, S, nbases=256, seed=3):
  system, objective, pm = tm._torch_system(sy, device)
  params = [t for ts in tm._policy_params(pm, sy["nu"]).values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  g = torch.Generator(device=device).manual_seed(seed)
  x0 = torch.tensor(sy["x0"][:S], dtype=F64, device=device, requires_grad=True)
  paths = system.drift.generate_paths(S, nbases, dtype=F64, device=device, generator=g)
  return system, objective, pm, params, x0, paths


@pytest.mark.gpu
def test_gpu_closure_runs_nine_inputs_natively_when_asked(device):
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _system("W2", 37)
  S, H = 37, 5
  system, objective, pm, params, x0, paths = _closure_case(sy, device, S)

  def run(**kw):
    for t in params + [x0]:
      t.grad = None
    loss = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, **kw)()
    loss.mean().backward()
    return loss.detach(), [t.grad.detach().clone() for t in params + [x0]]
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    ln, gn = run(native_inputs=16, native_actions=4)
    lf, _ = run(native_inputs=99, native_actions=4, native=True)
    lt, gt = run(native=False)                       # the torch composition: differentiable through the wide Jacobian pass
    with torch.no_grad():
      l0 = pathwise_policy_loss_closure(system, objective, lambda: x0.detach(), H, dt=DT, paths=paths, native_inputs=16,
                                        native_actions=4)()
  assert ln.shape == (S,) and torch.equal(ln, lf)
  el = float((ln - lt).abs().max())
  print(f"closure W2: native vs torch composition, loss {el:.2e}")
  assert el < 1e-10 and float((l0 - ln).abs().max()) < 1e-12
  for a_, b_ in zip(gn, gt):
    eg = float((a_ - b_).abs().max()) / max(1e-12, float(b_.abs().max()))
    assert eg < 1e-8, eg
  # the default stays today's routing: nine inputs fall back, naming the dimension
  with torch.no_grad(), pytest.warns(RuntimeWarning, match=r"nx \+ na \+ nu = 9 > 8"):
    ld = pathwise_policy_loss_closure(system, objective, lambda: x0.detach(), H, dt=DT, paths=paths, native_actions=4)()
  assert float((ld - lt).abs().max()) < 1e-10


@pytest.mark.gpu
def test_gpu_closure_beyond_the_lds_bound_and_beyond_sixteen_inputs(device):
  """W3's wiring with 78 centres per latent -- one past the reverse sweep's LDS bound for nu 4 on ne 12: a gradient falls back
  once, naming the bound, with the torch composition's numbers; the forward stays native and silent.  A 17-input wiring (nx 12,
  one angle, four actions) falls back naming 16."""
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  from gpflowpilco_amd.pathwise import PolicyRollout
  S, H = 16, 3
  sy = _system("W3", 37, pol_M=78)
  system, objective, pm, params, x0, paths = _closure_case(sy, device, S)
  roll = PolicyRollout(paths, pm.packed(F64, False, device), nx=sy["nx"], active_dims=sy["active"], head_scale=tuple(sy["scale"]),
                       head_shift=tuple(sy["shift"]), target=objective.target, precis=objective.precis, wide=True)
  assert not roll.supports_backward()
  closure = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, native_inputs=16, native_actions=4)
  with pytest.warns(RuntimeWarning, match=r"LDS bound") as rec:
    lw = closure()
    lw.mean().backward()
  said = [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning)]
  assert len(said) == 1 and "torch composition" in said[0]
  gw = [t.grad.detach().clone() for t in params + [x0]]
  for t in params + [x0]:
    t.grad = None
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    closure().mean().backward()                                                    # once: the second call is silent
    lt = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=paths, native=False)()
    with torch.no_grad():
      l0 = pathwise_policy_loss_closure(system, objective, lambda: x0.detach(), H, dt=DT, paths=paths, native_inputs=16,
                                        native_actions=4)()
      cost, _ = roll(x0.detach(), H, dt=DT)
  assert torch.equal(lw.detach(), lt.detach()) and all(torch.equal(a_, t.grad) for a_, t in zip(gw, params + [x0]))
  assert torch.equal(l0, cost.sum(0)) and float((l0 - lt.detach()).abs().max()) < 1e-10

  # seventeen inputs
  nx, active, nu = 12, (0,), 4
  ne = nx + 1
  dr = oracle_params(make_svgp(nx, 30, ne + nu, seed=111, ls_bounds=(0.9, 3.0)))
  pol = random_svgp_params(seed=112, L=nu, M=10, d=ne, whiten=True, ls_bounds=(0.9, 2.0), mean=True, separate_Z=True)
  pol.q_mu = 0.2 * pol.q_mu
  sy17 = dict(nx=nx, active=active, nu=nu, drift=dr, pol=pol, scale=np.array(SCALE), shift=np.array(SHIFT), target=np.zeros(ne),
              precis=0.1 * np.eye(ne))
  system, objective, _ = tm._torch_system(sy17, device)
  g = torch.Generator(device=device).manual_seed(4)
  x17 = 0.2 + 0.6 * torch.rand(S, nx, dtype=F64, device=device, generator=g)
  paths17 = system.drift.generate_paths(S, 256, dtype=F64, device=device, generator=g)
  with torch.no_grad():
    with pytest.warns(RuntimeWarning, match=r"nx \+ na \+ nu = 17 > 16"):
      l17 = pathwise_policy_loss_closure(system, objective, lambda: x17, H, dt=DT, paths=paths17, native_inputs=16, native_actions=4)()
    lt17 = pathwise_policy_loss_closure(system, objective, lambda: x17, H, dt=DT, paths=paths17, native=False)()
  assert torch.equal(l17, lt17) and torch.isfinite(l17).all()


# ---- GPU 6: capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_wide_forward_replays_bit_equal_under_graph_capture(device):
  sy = _system("W1", 37)
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
