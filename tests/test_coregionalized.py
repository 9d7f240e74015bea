"""Native moment-matched rollouts with a COREGIONALISED drift (``native_coregionalized=True``): the mixing f = W g + c of
csrc/mm_mix.h, the ``_nd_mixed`` entries (csrc/mm_compose_nd.hip, csrc/mm_compose_bwd_nd.hip), ``ops.ComposedRollout(mix_W=...)``
and the routing of ``loops.policy_loss_closure``.

Systems (H = 4, drift M = 20, policy M = 10, B = 3 and B = 1; ``random_svgp_params(..., W_rows=nx)``, W then replaced by a signed,
unnormalised normal draw, the output mean scaled by 0.3, the action axes of Z moved to [-2, 2]):
  L1  nx 4, angle (1,), one action, Lg 2     rectangular W; nu = 1 through the nd path
  L2  nx 3, angles (0, 2), two actions, Lg 3  square, non-symmetric W: W and W^T are distinguishable
  L3  nx 2, no encoder, one action, Lg 1      one latent, no off-diagonal pair, na = 0
The comparator is the committed oracle (``oracle.mm_compose_oracle.policy_rollout_loss`` with ``SVGPParams.W`` set) with the policy
of tests/multiaction_oracle.py.  Every parity test rests on the wiring guards of ``test_wiring_guards``: a dropped output mean,
swapped rows or columns of W, or W^T move the oracle's states by at least 10x the f32 bar."""
import copy
import ctypes
import functools
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib
from gpflowpilco_amd import bijectors as tfb
from gpflowpilco_amd import dynamics, models as gp
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
from gpflowpilco_amd.synthetic import generate_covariance
from oracle import mm_compose_oracle as co
from tests import multiaction_oracle as mao
from tests.helpers import gp_model_from_oracle, random_svgp_params, scale_err, to_dev

F64 = torch.float64
H4 = 4
SCALE, SHIFT = (2.0, 1.5), (-0.5, -0.4)
WEIGHTS = (1.0, 0.6, 0.8)
F64_BAR, F32_BAR = 1e-7, 2e-4
CASES = {"L1": dict(nx=4, active=(1,), nu=1, Lg=2, seed=40),
         "L2": dict(nx=3, active=(0, 2), nu=2, Lg=3, seed=50),
         "L3": dict(nx=2, active=(), nu=1, Lg=1, seed=60)}
HOSTLIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "libmm_mix_host.so")


def _rollout_oracle(sy, drift_o, H, B=None):
  mu0, S0 = (sy["mu0"], sy["S0"]) if B is None else (sy["mu0"][:B], sy["S0"][:B])
  return co.policy_rollout_loss(mu0, S0, drift_o, sy["policy_fn"], sy["active"], sy["target"], sy["precis"], H, keep=True)


@functools.lru_cache(maxsize=None)
def _system(name, H=H4, Md=20):
  """The numpy side of L1 .. L3 and its oracle rollout (computed once, shared, never modified)."""
  c = CASES[name]
  nx, active, nu, Lg, s = c["nx"], c["active"], c["nu"], c["Lg"], c["seed"]
  na = len(active); ne = nx + na; nd = ne + nu
  drift_o = random_svgp_params(seed=s, L=Lg, M=Md, d=nd, whiten=True, ls_bounds=(0.8, 3.0), mean=True, W_rows=nx)
  drift_o.Z[..., ne:] = 4.0 * drift_o.Z[..., ne:] - 2.0                          # action axes in [-2, 2]
  rng = np.random.default_rng(s + 3)
  drift_o.W = rng.standard_normal((nx, Lg))                                      # signed, unnormalised
  drift_o.mean_c = 0.3 * drift_o.mean_c
  pol_o = random_svgp_params(seed=s + 1, L=nu, M=10, d=ne, whiten=True, ls_bounds=(0.3, 0.8), mean=False, separate_Z=False)
  pol_o.q_mu = 2.0 * pol_o.q_mu
  rng = np.random.default_rng(s + 2)
  mu0 = rng.uniform(0.0, 0.6, (3, nx))
  S0 = generate_covariance(rng, nx, (3,), 0.3)
  A = rng.standard_normal((ne, ne))
  precis = A @ A.T / ne
  target = np.zeros(ne); target[na:2 * na] = 1.0
  scale, shift = np.array(SCALE[:nu]), np.array(SHIFT[:nu])
  sy = dict(c, name=name, H=H, na=na, ne=ne, nd=nd, drift_o=drift_o, pol_o=pol_o, mu0=mu0, S0=S0, target=target, precis=precis,
            scale=scale, shift=shift, policy_fn=lambda st: mao.mm_policy_nd(st, pol_o, scale, shift))
  sy["loss_o"], sy["traj_o"] = _rollout_oracle(sy, drift_o, H)
  return sy


def _variants(sy):
  """Wrong wirings of the mixing, as oracle drifts: name -> SVGPParams."""
  d = sy["drift_o"]
  out = {}
  v = copy.copy(d); v.mean_c = None; out["dropped mean"] = v
  v = copy.copy(d); v.W = d.W.copy(); v.W[[0, 1]] = d.W[[1, 0]]; out["rows swapped"] = v
  if sy["Lg"] > 1:
    v = copy.copy(d); v.W = d.W.copy(); v.W[:, [0, 1]] = d.W[:, [1, 0]]; out["columns swapped"] = v
  if sy["Lg"] == sy["nx"]:
    v = copy.copy(d); v.W = d.W.T.copy(); out["W transposed"] = v
  return out


def _torch_system(sy, device, dtype=F64, drift_o=None):
  drift = gp_model_from_oracle(sy["drift_o"] if drift_o is None else drift_o, device)
  pol_model = gp_model_from_oracle(sy["pol_o"], device)
  if sy["nu"] == 1:
    head = [tfb.Scale(float(sy["scale"][0])), tfb.Shift(float(sy["shift"][0])), tfb.NormalCDF()]
  else:
    head = [tfb.Scale(to_dev(sy["scale"], device, dtype)), tfb.Shift(to_dev(sy["shift"], device, dtype)), tfb.NormalCDF()]
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol_model), invlink=tfb.Chain(head))
  encoder = TrigonometricEncoder(active_dims=sy["active"]) if sy["active"] else None
  objective = GaussianObjective(target=to_dev(sy["target"], device, dtype), precis=to_dev(sy["precis"], device, dtype))
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=encoder, solver=dynamics.MomentMatchingEuler())
  return system, objective, drift, pol_model


def _options(sy):
  """The closure options that take the system natively."""
  kw = dict(native_coregionalized=True)
  if sy["nu"] > 1:
    kw["native_actions"] = sy["nu"]
  if not sy["active"]:
    kw["native_no_encoder"] = True
  return kw


def _rollout(sy, device, dtype, drift_o=None):
  from gpflowpilco_amd import ops
  d = sy["drift_o"] if drift_o is None else drift_o
  drift = gp_model_from_oracle(d, device)
  pol_model = gp_model_from_oracle(sy["pol_o"], device)
  head = dict(head_scale=float(sy["scale"][0]), head_shift=float(sy["shift"][0])) if sy["nu"] == 1 else \
      dict(head_scale=tuple(sy["scale"]), head_shift=tuple(sy["shift"]))
  return ops.ComposedRollout(drift.packed(dtype, True, device), pol_model.packed(dtype, False, device), nx=sy["nx"],
                             active_dims=sy["active"], target=to_dev(sy["target"], device, dtype),
                             precis=to_dev(sy["precis"], device, dtype), mix_W=to_dev(d.W, device, F64),
                             mix_c=None if d.mean_c is None else to_dev(d.mean_c, device, F64), **head)


# ---- 1. guards -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_wiring_guards(name):
  """Each wrong wiring of the mixing moves the oracle's mean and covariance after steps 0 and 1 by at least 10x the f32 bar (a
  dropped mean cannot move the covariance at step 0: judged on the mean there and on both at step 1).  The rollouts stay positive
  definite."""
  sy = _system(name)
  ev = min(np.linalg.eigvalsh(S).min() for _, S in sy["traj_o"])
  print(f"{name}: smallest trajectory eigenvalue {ev:.3f}")
  assert ev > 0.0
  for what, d in _variants(sy).items():
    _, traj = _rollout_oracle(sy, d, 2)
    for h in (0, 1):
      dm, dS = scale_err(traj[h][0], sy["traj_o"][h][0]), scale_err(traj[h][1], sy["traj_o"][h][1])
      print(f"guard {name} {what} step {h}: mean {dm:.2e} cov {dS:.2e}")
      assert dm >= 10 * F32_BAR, (what, h, dm)
      if not (what == "dropped mean" and h == 0):
        assert dS >= 10 * F32_BAR, (what, h, dS)


# ---- 2. host check ----------------------------------------------------------------------------------------------------------------
def _dp(a):
  return a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def _host_mix_lib():
  """tests/hostcheck/libmm_mix_host.so, built by ``__graft_entry__.build()``; rebuilt here when it is missing or older than its
  sources, as tests/test_adjoint_host.py does for its library."""
  hostcheck = os.path.dirname(HOSTLIB)
  deps = [os.path.join(hostcheck, "mm_mix_host.hip"), os.path.join(os.path.dirname(hostcheck), os.pardir, "gpflowpilco_amd", "csrc", "mm_mix.h")]
  if not os.path.exists(HOSTLIB) or os.path.getmtime(HOSTLIB) < max(os.path.getmtime(p) for p in deps):
    subprocess.run(["bash", os.path.join(hostcheck, "build_mix.sh")], check=True)
  return ctypes.CDLL(HOSTLIB)


@pytest.mark.parametrize("nx,Lg,nd", [(4, 2, 6), (3, 3, 7), (2, 1, 3)])
def test_host_mixing_and_adjoint_match_torch(nx, Lg, nd):
  """mma_mix_fwd / mma_mix_bwd (csrc/mm_mix.h, built for the host) against torch f64 and its autograd, 1e-13 relative (the
  step-adjoint bar of tests/test_adjoint_nd_host.py); Sff comes out exactly symmetric; the adjoint is seeded with an unsymmetric
  g Sff."""
  hc = _host_mix_lib()
  rng = np.random.default_rng(100 * nx + 10 * Lg + nd)
  W, c = rng.standard_normal((nx, Lg)), rng.standard_normal(nx)
  g1 = rng.standard_normal(Lg); Sgg = generate_covariance(rng, Lg, (), 0.7); cg = rng.standard_normal((nd, Lg))
  f1, Sff, cross = np.zeros(nx), np.zeros((nx, nx)), np.zeros((nd, nx))
  hc.hc_mix_fwd(nx, Lg, nd, _dp(W), _dp(c), _dp(g1), _dp(Sgg), _dp(cg), _dp(f1), _dp(Sff), _dp(cross))
  t = lambda a: torch.tensor(a, dtype=F64, requires_grad=True)
  Wt, g1t, St, cgt = torch.tensor(W), t(g1), t(Sgg), t(cg)
  f1_t, Sff_t, cross_t = Wt @ g1t + torch.tensor(c), Wt @ St @ Wt.T, cgt @ Wt.T
  for what, got, want in (("f1", f1, f1_t), ("Sff", Sff, Sff_t), ("cross", cross, cross_t)):
    err = scale_err(got, want.detach().numpy())
    print(f"mix fwd ({nx},{Lg},{nd}) {what}: {err:.2e}")
    assert err <= 1e-13
  assert np.array_equal(Sff, Sff.T)
  # no output mean: a null pointer
  f0 = np.zeros(nx)
  hc.hc_mix_fwd(nx, Lg, nd, _dp(W), None, _dp(g1), _dp(Sgg), _dp(cg), _dp(f0), _dp(Sff), _dp(cross))
  assert scale_err(f0, W @ g1) <= 1e-13
  # float moments: f64 arithmetic rounded on store -- the f32 rounding of the f64 result of the rounded inputs
  r32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
  g32, S32, c32 = r32(g1), r32(Sgg), r32(cg)
  f1s, Sffs, crs = (np.zeros(s, dtype=np.float32) for s in ((nx,), (nx, nx), (nd, nx)))
  hc.hc_mix_fwd_f32(nx, Lg, nd, _dp(W), _dp(c), _dp(g32), _dp(S32), _dp(c32), _dp(f1s), _dp(Sffs), _dp(crs))
  assert scale_err(f1s, W @ g32.astype(float) + c) <= 2.0 ** -23 and np.array_equal(Sffs, Sffs.T)
  assert scale_err(Sffs, W @ S32.astype(float) @ W.T) <= 2.0 ** -23 and scale_err(crs, c32.astype(float) @ W.T) <= 2.0 ** -23
  # adjoint
  gf1, gSff, gcross = rng.standard_normal(nx), rng.standard_normal((nx, nx)), rng.standard_normal((nd, nx))
  assert np.abs(gSff - gSff.T).max() > 0.1
  gg1, gSgg, gcg = np.zeros(Lg), np.zeros((Lg, Lg)), np.zeros((nd, Lg))
  hc.hc_mix_bwd(nx, Lg, nd, _dp(W), _dp(gf1), _dp(gSff), _dp(gcross), _dp(gg1), _dp(gSgg), _dp(gcg))
  obj = (f1_t * torch.tensor(gf1)).sum() + (Sff_t * torch.tensor(gSff)).sum() + (cross_t * torch.tensor(gcross)).sum()
  wg1, wS, wcg = torch.autograd.grad(obj, (g1t, St, cgt))
  for what, got, want in (("g g1", gg1, wg1), ("g Sgg", gSgg, wS), ("g cross_g", gcg, wcg)):
    err = scale_err(got, want.numpy())
    print(f"mix bwd ({nx},{Lg},{nd}) {what}: {err:.2e}")
    assert err <= 1e-13
  if nx == Lg:                                               # W and W^T are distinguishable
    assert scale_err(gSgg, W @ gSff @ W.T) > 1e-2


# ---- 3. validation without a GPU ---------------------------------------------------------------------------------------------------
def test_argument_validation_of_the_mixed_entries_without_gpu():
  lib = _lib.lib()
  buf = (ctypes.c_char * 64)()
  p = ctypes.addressof(buf)
  F64c, F32c = _lib.MM_F64, _lib.MM_F32
  act = (ctypes.c_int32 * 2)(0, 1)
  sc = (ctypes.c_double * 4)(2.0, 1.5, 1.0, 1.0)
  sh = (ctypes.c_double * 4)(-0.5, -0.4, -0.6, 0.0)
  B, H, nx, na, nu, Md, Mp = 3, 30, 4, 2, 2, 100, 30
  # size queries: at drift_L = nx the tape and the backward workspace are the _nd ones plus the staging block of the mixing
  # (three 256-byte-aligned blocks here); 0 for drift_L = 0 and nx + 1
  stage = lib.mm_compose_nd_mixed_workspace_bytes(B, nx, na, nu, nx, F64c) - lib.mm_compose_nd_workspace_bytes(B, nx, na, nu, F64c)
  al = lambda v: (v + 255) // 256 * 256
  assert stage == al(B * nx * 8) + al(B * nx * nx * 8) + al(B * 8 * nx * 8)
  assert lib.mm_compose_tape_bytes_nd_mixed(B, H, nx, na, nu, nx, Md, F64c) == lib.mm_compose_tape_bytes_nd(B, H, nx, na, nu, Md, F64c) + stage
  assert (lib.mm_compose_backward_workspace_bytes_nd_mixed(B, nx, na, nu, nx, Md, Mp)
          == lib.mm_compose_backward_workspace_bytes_nd(B, nx, na, nu, Md, Mp) + stage)
  assert lib.mm_compose_tape_bytes_nd_mixed(B, H, nx, na, nu, 2, Md, F64c) < lib.mm_compose_tape_bytes_nd(B, H, nx, na, nu, Md, F64c)
  for bad in (0, nx + 1):
    assert lib.mm_compose_nd_mixed_workspace_bytes(B, nx, na, nu, bad, F64c) == 0
    assert lib.mm_compose_tape_bytes_nd_mixed(B, H, nx, na, nu, bad, Md, F64c) == 0
    assert lib.mm_compose_backward_workspace_bytes_nd_mixed(B, nx, na, nu, bad, Md, Mp) == 0
  assert lib.mm_compose_tape_bytes_nd_mixed(B, H, nx, na, nu, 2, Md, F32c) == 0              # the tape is f64
  assert lib.mm_compose_backward_workspace_bytes_nd_mixed(B, nx, na, nu, 2, Md, 300) == 0    # the sweep's policy bound

  def fwd(L=2, W=p, nu_=nu, drift_d=8, dtype=F64c, wsc_bytes=1 << 20):
    return lib.mm_rollout_composed_nd_mixed(p, 64, L, Md, drift_d, p, 64, Mp, 6, dtype, B, H, 1.0, nx, na, act, nu_, sc, sh, p, p,
                                            p, p, p, None, None, p, 64, p, 64, p, wsc_bytes, None, None, W, None)

  def taped(L=2, W=p, dtype=F64c, tape_bytes=1 << 30):
    return lib.mm_rollout_composed_taped_nd_mixed(p, 64, L, Md, 8, p, 64, Mp, 6, dtype, B, H, 1.0, nx, na, act, nu, sc, sh, p, p,
                                                  p, p, p, p, 64, p, 64, p, tape_bytes, None, None, W, None)

  def bwd(L=2, W=p, seeds=(None, None), tape_bytes=1 << 30, wb_bytes=1 << 30):
    return lib.mm_rollout_composed_backward_nd_mixed(p, 64, L, Md, 8, p, 64, Mp, 6, F64c, B, H, 1.0, nx, na, act, nu, sc, sh, p, p,
                                                     p, tape_bytes, p, seeds[0], seeds[1], p, None, None, p, 64, p, wb_bytes,
                                                     None, None, W)
  for f in (fwd, taped, bwd):
    assert f(L=0) == -2 and f(L=nx + 1) == -2                                          # MM_E_DIM
    assert f(W=None) == -1                                                             # MM_E_ARG
    assert f() == -4 and f(L=nx) == -4                                                 # past the checks: the 64-byte buffers
  assert fwd(nu_=0) == -2 and fwd(drift_d=7) == -6 and fwd(dtype=7) == -3
  assert fwd(wsc_bytes=lib.mm_compose_nd_workspace_bytes(B, nx, na, nu, F64c)) == -4   # the _nd workspace lacks the staging block
  assert taped(dtype=F32c) == -3
  assert taped(tape_bytes=lib.mm_compose_tape_bytes_nd_mixed(B, H, nx, na, nu, 2, Md, F64c) - 1) == -4
  assert bwd(seeds=(p, None)) == -1                                                    # both seeds or neither
  assert bwd(wb_bytes=lib.mm_compose_backward_workspace_bytes_nd_mixed(B, nx, na, nu, 2, Md, Mp) - 1) == -4
  assert lib.mm_abi_version() == 2


# ---- 4. routing -------------------------------------------------------------------------------------------------------------------
def test_routing_of_the_coregionalized_option():
  from gpflowpilco_amd.loops import _native_parts
  sy = _system("L1")
  system, objective, drift, _ = _torch_system(sy, "cpu")
  why = []
  assert _native_parts(system, objective, why, True) is None
  assert why == ["a LinearCoregionalization kernel (its mixing stays on the host)"]        # the option off: today's reason
  why = []
  parts = _native_parts(system, objective, why, True, coregionalized=True)
  assert parts is not None and parts[2] is drift and not why
  # a coregionalised policy
  pol_lcm = random_svgp_params(seed=41, L=1, M=10, d=sy["ne"], whiten=True, ls_bounds=(0.3, 0.8), mean=False, W_rows=1)
  sys_p, obj_p, _, _ = _torch_system(dict(sy, pol_o=pol_lcm), "cpu")
  for on in (False, True):
    why = []
    assert _native_parts(sys_p, obj_p, why, True, coregionalized=on) is None
    assert ("coregionalised policy" in why[0]) if on else (why[0] == "a LinearCoregionalization kernel (its mixing stays on the host)")
  # more latents than outputs
  wide = random_svgp_params(seed=42, L=sy["nx"] + 1, M=20, d=sy["nd"], whiten=True, ls_bounds=(0.8, 3.0), mean=True, W_rows=sy["nx"])
  sys_w, obj_w, _, _ = _torch_system(sy, "cpu", drift_o=wide)
  why = []
  assert _native_parts(sys_w, obj_w, why, True, coregionalized=True) is None
  assert "more latents than outputs" in why[0] and "Lg = 5 > nx = 4" in why[0]
  # an ordinary drift: the option changes nothing
  plain = random_svgp_params(seed=43, L=sy["nx"], M=20, d=sy["nd"], whiten=True, ls_bounds=(0.8, 3.0), mean=True)
  sys_s, obj_s, _, _ = _torch_system(sy, "cpu", drift_o=plain)
  assert _native_parts(sys_s, obj_s, None, True, coregionalized=True) is not None
  assert _native_parts(sys_s, obj_s, None, True) is not None


# ---- 5. forward parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_gpu_forward_matches_oracle(name, dtype, B, device):
  sy = _system(name)
  tol = F64_BAR if dtype == torch.float64 else F32_BAR
  loss_o, traj_o = (sy["loss_o"], sy["traj_o"]) if B == 3 else _rollout_oracle(sy, sy["drift_o"], H4, B)
  roll = _rollout(sy, device, dtype)
  assert roll.mixed and roll.uses_nd and not roll.supports_backward()
  mx, Sxx = to_dev(sy["mu0"][:B], device, dtype), to_dev(sy["S0"][:B], device, dtype)
  m_H, S_H, cost, tmu, tS = roll(mx, Sxx, H4, keep_trajectory=True)
  roll.drift.check_status(B)
  for h in range(H4):
    em, eS = scale_err(tmu[h], traj_o[h][0]), scale_err(tS[h], traj_o[h][1])
    print(f"forward {name} {dtype} B={B} step {h}: mean {em:.2e} cov {eS:.2e}")
    assert em < tol and eS < tol, h
  el = scale_err(cost.sum(1), loss_o)
  print(f"forward {name} {dtype} B={B}: loss {el:.2e}")
  assert el < tol
  assert torch.equal(m_H, tmu[-1]) and torch.equal(S_H, tS[-1])
  if dtype == torch.float64:                                                    # the taped forward computes the same
    m_t, S_t, cost_t, _ = roll.taped_nd(mx, Sxx, H4)
    assert max(scale_err(m_t, m_H.cpu().numpy()), scale_err(S_t, S_H.cpu().numpy()), scale_err(cost_t.T, cost.cpu().numpy())) < 1e-12
    with pytest.raises(NotImplementedError):
      roll.taped(mx, Sxx, H4)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_gpu_closure_takes_the_native_path(name, device):
  from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
  sy = _system(name)
  system, objective, _, _ = _torch_system(sy, device)
  init = get_state_initializer(to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64))
  with warnings.catch_warnings():
    warnings.simplefilter("error")                                                # no fall-back warning
    loss_n = policy_loss_closure(system, objective, init, H4, native=True, **_options(sy))()
    loss_t = policy_loss_closure(system, objective, init, H4, native=False)()
  assert scale_err(loss_n, loss_t.cpu().numpy()) < 1e-9 and scale_err(loss_n, sy["loss_o"]) < F64_BAR
  # the option off: today's routing, with today's reason
  kw = {k: v for k, v in _options(sy).items() if k != "native_coregionalized"}
  with pytest.warns(RuntimeWarning, match=r"a LinearCoregionalization kernel \(its mixing stays on the host\)"):
    loss_d = policy_loss_closure(system, objective, init, H4, **kw)()
  assert torch.equal(loss_d, loss_t)
  with pytest.raises(ValueError):
    policy_loss_closure(system, objective, init, H4, native=True, **kw)


# ---- 6. identity mixing -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_identity_mixing_reproduces_the_independent_drift(device):
  """A SeparateIndependent drift with a Constant mean through mm_rollout_composed_nd, and the same latents as a coregionalised
  drift with W = I, c = that mean through the mixed entry: every product is with 0 or 1."""
  sy = _system("L2")
  nx = sy["nx"]
  plain = random_svgp_params(seed=51, L=nx, M=20, d=sy["nd"], whiten=True, ls_bounds=(0.8, 3.0), mean=True)
  plain.Z[..., sy["ne"]:] = 4.0 * plain.Z[..., sy["ne"]:] - 2.0
  plain.mean_c = 0.3 * plain.mean_c
  lcm = copy.copy(plain); lcm.W = np.eye(nx)
  from gpflowpilco_amd import ops
  drift = gp_model_from_oracle(plain, device); pol_model = gp_model_from_oracle(sy["pol_o"], device)
  ref = ops.ComposedRollout(drift.packed(F64, True, device), pol_model.packed(F64, False, device), nx=nx,
                            active_dims=sy["active"], head_scale=tuple(sy["scale"]), head_shift=tuple(sy["shift"]),
                            target=to_dev(sy["target"], device, F64), precis=to_dev(sy["precis"], device, F64))
  mixed = _rollout(sy, device, F64, drift_o=lcm)
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  a = ref(mx, Sxx, H4, keep_trajectory=True)
  b = mixed(mx, Sxx, H4, keep_trajectory=True)
  errs = [scale_err(y, x.cpu().numpy()) for x, y in zip(a, b)]
  print(f"identity mixing: bit-equal {all(torch.equal(x, y) for x, y in zip(a, b))}, errors {errs}")
  assert max(errs) <= 1e-13


# ---- 7. gradient ------------------------------------------------------------------------------------------------------------------
def _setup(sy, device, drift_o=None, state_grad=True):
  from tests.test_multiaction_grad import _trainable
  system, objective, drift, pol_model = _torch_system(sy, device, drift_o=drift_o)
  params = _trainable(pol_model, sy["nu"])
  m0 = to_dev(sy["mu0"], device, F64).requires_grad_(state_grad)
  S0 = to_dev(sy["S0"], device, F64).requires_grad_(state_grad)
  return system, objective, drift, pol_model, params, m0, S0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_gpu_native_gradient_matches_the_torch_composition(name, device):
  from tests.test_multiaction_grad import _grads, _group_err
  sy = _system(name)
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")                                                # no fall-back warning
    loss_n, gn = _grads(system, objective, params, m0, S0, H4, **_options(sy))
  loss_t, gt = _grads(system, objective, params, m0, S0, H4, native=False)
  drift.packed(F64, True, device).check_status(3)
  print(f"gradient {name}: loss err {np.abs(loss_n - loss_t).max():.2e}")
  assert np.abs(loss_n - loss_t).max() < 1e-9
  assert scale_err(loss_n, sy["loss_o"]) < F64_BAR
  for k in gt:
    err = _group_err(gn[k], gt[k])
    print(f"gradient {name} {k}: native vs torch composition {err:.2e}")
    assert err < 1e-7, (k, err)
  if name == "L2":                       # guard: W^T instead of W moves every group far past the bar
    sys_T, obj_T, _, _, params_T, m0_T, S0_T = _setup(sy, device, drift_o=_variants(sy)["W transposed"])
    _, gT = _grads(sys_T, obj_T, params_T, m0_T, S0_T, H4, native=False)
    for k in gt:
      far = _group_err(gT[k], gt[k])
      print(f"guard {name} {k}: W^T moves the gradient by {far:.2e}")
      assert far > 10 * 1e-7, (k, far)


@pytest.mark.gpu
def test_gpu_native_gradient_matches_finite_differences_of_the_oracle(device):
  from tests.test_multiaction_grad import _grads
  sy = _system("L1")
  H = 3
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    loss, g = _grads(system, objective, params, m0, S0, H, **_options(sy))
  wts = np.array(WEIGHTS)

  def oracle_loss(q_mu):
    pol = copy.copy(sy["pol_o"]); pol.q_mu = q_mu
    fn = lambda st: mao.mm_policy_nd(st, pol, sy["scale"], sy["shift"])
    l = co.policy_rollout_loss(sy["mu0"], sy["S0"], sy["drift_o"], fn, sy["active"], sy["target"], sy["precis"], H)
    return float((wts * l).sum())
  base = oracle_loss(sy["pol_o"].q_mu)
  assert abs(base - float((wts * loss).sum())) < 1e-7 * max(1.0, abs(base))
  eps = 1e-5
  for m in (0, 4, 9):
    qp, qm = sy["pol_o"].q_mu.copy(), sy["pol_o"].q_mu.copy()
    qp[m, 0] += eps; qm[m, 0] -= eps
    want = (oracle_loss(qp) - oracle_loss(qm)) / (2 * eps)
    got = float(g["q_mu"][m, 0])
    print(f"finite differences L1 q_mu[{m},0]: native {got:+.8e} fd {want:+.8e}")
    assert abs(got - want) < 2e-5 * max(1.0, abs(want)), (m, got, want)


# ---- 8. both tape regimes ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_tape_with_and_without_the_kept_drift_blocks(device):
  """L1's wiring with drift M = 100, H = 4: at B = 3 the tape keeps the drift's per-step workspace and sums (sized by Lg); the
  large batch is the first at which the mixed tape-size query returns the bare tape -- slots, states, staging block and the ONE
  scratch buffer the taped forward sweeps the drift's sums into, nothing kept per step.  Batch elements are independent: element b
  of the large batch reproduces element b % 3 of the small one, the gradients to 1e-12.

  This draw of the drift is ill-conditioned (M = 100 random centres in the unit cube, lengthscales up to 3: max |beta| = 280), and
  ``mm_moment_match`` and ``mm_moment_match_with_sums`` return an Sff that differs by 9.9e-11 of its scale on it (4.9e-14 at M = 20;
  measured on an MI355X).  A taped forward that took the first routine on the bare tape and the second on the kept one missed the
  bar (g_policy 5.07e-12); the mixed taped forward therefore reads the drift's value off the backward's sums in every regime."""
  H = H4
  sy = _system("L1", H, 100)
  lib = _lib.lib()
  nx, na, nu, Lg, Md = sy["nx"], sy["na"], sy["nu"], sy["Lg"], 100
  al = lambda v: (v + 255) // 256 * 256

  def bare(B):
    slot = lib.mm_compose_nd_workspace_bytes(B, nx, na, nu, _lib.MM_F64)
    stage = lib.mm_compose_nd_mixed_workspace_bytes(B, nx, na, nu, Lg, _lib.MM_F64) - slot
    scratch = al(lib.mm_moment_match_backward_bytes_dtype(B, Lg, Md, sy["nd"], _lib.MM_F64, 3))     # one, not one per step
    return (H + 1) * slot + al((H + 1) * B * nx * 8) + al((H + 1) * B * nx * nx * 8) + stage + scratch
  tape_bytes = lambda B: lib.mm_compose_tape_bytes_nd_mixed(B, H, nx, na, nu, Lg, Md, _lib.MM_F64)
  ws_step = al(lib.mm_workspace_bytes(3, Lg, Md, sy["nd"], _lib.MM_F64, 3))
  gp_step = al(lib.mm_moment_match_backward_bytes_dtype(3, Lg, Md, sy["nd"], _lib.MM_F64, 3))
  assert tape_bytes(3) == bare(3) + H * ws_step + (H - 1) * gp_step               # B = 3: both kept per step, sized by Lg
  big = next(B for B in (1024, 2048, 4096, 8192, 16384) if tape_bytes(B) == bare(B))
  print(f"nothing kept from B = {big}")
  roll = _rollout(sy, device, F64)
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  g3 = to_dev(np.random.default_rng(0).uniform(0.5, 1.5, (H, 3)), device, F64)
  _, _, cost3, tape3 = roll.taped_nd(mx, Sxx, H)
  assert scale_err(cost3.sum(0), sy["loss_o"]) < F64_BAR
  ref = roll.backward_nd(tape3, g3, 3, H)
  idx = torch.arange(big, device=device) % 3
  _, _, costB, tapeB = roll.taped_nd(mx[idx], Sxx[idx], H)
  got = roll.backward_nd(tapeB, g3[:, idx].contiguous(), big, H)
  roll.drift.check_status(big)
  print(f"B = {big} costs: against the fully kept tape {scale_err(costB, cost3[:, idx].cpu().numpy()):.2e}")
  assert scale_err(costB.sum(0), sy["loss_o"][idx.cpu().numpy()]) < F64_BAR
  for what, a, b in zip(("g_policy", "g_mx0", "g_Sxx0"), got, ref):
    err = scale_err(a, b[idx].cpu().numpy())
    print(f"B = {big} {what}: against the fully kept tape {err:.2e}")
    assert err < 1e-12, (what, err)


# ---- 9. trajectory route ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_trajectory_route_with_a_caller_defined_objective(device):
  """native_objective=True with the time-weighted quadratic objective of tests/test_native_objective.py on L1, against the torch
  composition at that file's bars (loss 1e-9, every group 1e-7 of its largest entry)."""
  from tests.test_native_objective import _grads, _group_err, _quadratic
  sy = _system("L1")
  system, _, drift, pol_model, params, m0, S0 = _setup(sy, device)
  quad = _quadratic(system, m0, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    loss_n, gn = _grads(system, quad, params, m0, S0, native_objective=True, **_options(sy))
  loss_t, gt = _grads(system, quad, params, m0, S0, native=False)
  assert float((loss_n - loss_t).abs().max()) < 1e-9 * max(1.0, float(loss_t.abs().max()))
  for k in gt:
    err = _group_err(gn[k], gt[k])
    print(f"trajectory route {k}: {err:.2e}")
    assert err < 1e-7, (k, err)


# ---- 10. determinism and capture ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L1", "L2"])
def test_gpu_reverse_sweep_is_deterministic(name, device):
  sy = _system(name)
  roll = _rollout(sy, device, F64)
  assert roll.supports_backward_nd()
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  _, _, _, tape = roll.taped_nd(mx, Sxx, H4)
  g_cost = torch.ones(H4, 3, dtype=F64, device=device)
  a = [t.clone() for t in roll.backward_nd(tape, g_cost, 3, H4)]
  b = roll.backward_nd(tape, g_cost, 3, H4)
  assert all(torch.equal(x, y) for x, y in zip(a, b))
  assert float(a[0].abs().max()) > 0.0 and torch.isfinite(a[0]).all()


@pytest.mark.gpu
def test_gpu_captured_replay_and_in_place_changes_of_the_mixing(device):
  from gpflowpilco_amd.loops import GraphedPolicyLoss, get_state_initializer, policy_loss_closure
  sy = _system("L1")
  system, objective, drift, pol_model, params, m0, S0 = _setup(sy, device, state_grad=False)
  init = get_state_initializer(m0, S0)
  closure = policy_loss_closure(system, objective, init, H4, **_options(sy))
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
    assert float(ge[0].abs().max()) > 0.0
    # in-place changes of W and of the mean: the next eager call reads them
    reference = policy_loss_closure(system, objective, init, H4, native=False)
    with torch.no_grad():
      before = closure()
      drift.kernel.W.mul_(1.1)
      after_W = closure()
      assert scale_err(after_W, reference().cpu().numpy()) < 1e-9 and scale_err(after_W, before.cpu().numpy()) > 1e-4
      drift.mean_function.c.add_(0.05)
      after_c = closure()
      assert scale_err(after_c, reference().cpu().numpy()) < 1e-9 and scale_err(after_c, after_W.cpu().numpy()) > 1e-4
