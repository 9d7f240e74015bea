"""A mean-only drift on the pathwise solver (the reference's ``build_dynamics(..., model_uncertainty=False)``: the drift in a
``KernelRegressor``): the C ABI's refusals, ``MeanDrift``'s operands and the closure's torch composition (CPU), and every native
route -- the shared-weight mean pass, the policy rollouts with their gradients, the closure's routing and its graph capture --
against the float64 numpy helper ``tests/pathwise_mean_oracle.py`` (GPU).

Bars (all the project's own): f64 values 1e-10 of max |f|, Jacobian 1e-8 of max |J| and 1e-6 against
central differences of the helper (``tests/test_pathwise_matern.py``); an f32 value within ``BOUND_ULPS u var sum |beta k|`` of the
helper, per (sample, latent); f32 Jacobian 3e-3 of max |J|; policy rollouts f64 1e-10 / f32 5e-3 of the cost's scale; gradients
1e-8 against the torch composition of the same closure and 1e-6 against central differences of the helper."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, models as gp
from gpflowpilco_amd.synthetic import make_svgp
from tests import pathwise_mean_oracle as pmean
from tests import test_pathwise_matern as tm
from tests.helpers import gp_model_from_oracle, oracle_params, random_svgp_params, scale_err
from tests.test_abi import declared_functions

F64, F32 = torch.float64, torch.float32
FAMILY = {"se": 0, "matern32": 1, "matern52": 2}
F64_VALUE_BAR, F64_JAC_BAR, FD_BAR, F32_JAC_BAR = 1e-10, 1e-8, 1e-6, 3e-3
F64_BAR, F32_BAR = 1e-10, 5e-3                        # policy rollouts: tests/test_pathwise_multiaction.py
GRAD_BAR = 1e-8
H6, DT = 6, 0.5
E_ARG, E_DIM, E_DTYPE, E_WORKSPACE = -1, -2, -3, -4


# ---- CPU: the C ABI ----------------------------------------------------------------------------------------------------------------
def test_header_and_signatures_carry_the_new_entries():
  names = declared_functions()
  assert "mm_pathwise_mean_eval" in names and "mm_pathwise_policy_rollout_mean" in names
  assert set(_lib.SIGNATURES) == set(names)


def test_mean_entries_validate_without_a_gpu():
  lib = _lib.lib()
  buf = (ctypes.c_char * 64)()
  p = ctypes.addressof(buf)
  ev = lambda S=4, L=2, M=37, d=3, dtype=0, ptrs=None, jac=p, kernel=0: lib.mm_pathwise_mean_eval(
      S, L, M, d, dtype, *([p] * 7 if ptrs is None else ptrs), p, jac, None, kernel)
  assert ev(kernel=3) == E_ARG and ev(kernel=-1) == E_ARG
  assert ev(S=0) == E_ARG and ev(L=0) == E_ARG and ev(M=0) == E_ARG and ev(d=0) == E_ARG
  assert ev(d=17) == E_DIM and ev(d=33) == E_DIM
  assert ev(dtype=7) == E_DTYPE
  for i in (0, 1, 2, 3, 4, 6):                                                        # x, zs_t, hz, x_scale, variance, beta
    ptrs = [p] * 7
    ptrs[i] = None
    assert ev(ptrs=ptrs) == E_ARG, i
  assert lib.mm_pathwise_mean_eval(4, 2, 37, 3, 0, *([p] * 7), None, None, None, 0) == E_ARG      # f_out
  act = (ctypes.c_int32 * 2)(0, 1)

  def ro(S=4, M=37, dtype=0, H=2, nx=4, na=1, nu=1, beta=p, zs=p, pol_M=12, tape=p, Lg=0, mix_W=None, kernel=0):
    return lib.mm_pathwise_policy_rollout_mean(S, M, dtype, H, 1.0, nx, na, act, nu, zs, p, p, p, p, beta, p, 64, pol_M, p, p, p, p,
                                               p, p, tape, 64, 0, None, Lg, mix_W, None, kernel)
  assert ro(kernel=3) == E_ARG and ro(beta=None) == E_ARG and ro(zs=None) == E_ARG and ro(tape=None) == E_ARG
  assert ro(S=0) == E_ARG and ro(M=0) == E_ARG and ro(H=0) == E_ARG
  assert ro(dtype=5) == E_DTYPE
  assert ro(nx=14, na=2, nu=1) == E_DIM and ro(nu=5) == E_DIM and ro(pol_M=300) == E_DIM        # nd = 17; nu; policy centres
  assert ro(Lg=5, mix_W=p) == E_DIM                                                              # Lg > nx
  assert ro(Lg=2, mix_W=None) == E_ARG                                                           # mixing without W
  assert ro() == E_WORKSPACE                                                                     # the 64-byte tape


# ---- CPU: operands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "matern32", "matern52", "se-coregionalised", "matern52-coregionalised"])
def test_mean_drift_operands_are_those_of_the_model(name):
  from gpflowpilco_amd.pathwise import MeanDrift, generate_paths
  kern, coreg = name.split("-")[0], name.endswith("coregionalised")
  L, M, d = 3, 21, 4
  p = random_svgp_params(seed=3, L=L, M=M, d=d, whiten=True, ls_bounds=(0.8, 2.0), mean=True, W_rows=4 if coreg else None)
  model = tm._model(p, "cpu", kern)
  md = MeanDrift.from_model(model, F64, "cpu")
  Z, ls, var, beta, mean_c = model._mean_weights("cpu", FAMILY[kern])
  Mp = md.zs.shape[-1]
  assert md.kernel == FAMILY[kern] and md.num_centres == M and Mp % MeanDrift.PAD == 0 and Mp >= M
  assert md.beta.dtype == F64 and torch.equal(md.beta[:, :M], beta) and not md.beta[:, M:].any()
  assert scale_err(md.beta[:, :M], pmean.mean_weights(p, FAMILY[kern])) < 1e-6      # (Kuu^-1 with jitter 1e-6: two factorisations)
  ref = generate_paths(model, 4, 8, dtype=F64, device="cpu", generator=torch.Generator().manual_seed(0))
  assert torch.equal(md.zs[..., :M], ref.zs[..., :M]) and torch.equal(md.hz[:, :M], ref.hz[:, :M])
  assert not md.zs[..., M:].any() and not md.hz[:, M:].any()
  assert torch.equal(md.lengthscales, ref.lengthscales) and torch.equal(md.variance, ref.variance)
  if coreg:
    assert md.mean_c is None and torch.equal(md.mix_W, torch.tensor(p.W)) and torch.equal(md.mix_c, torch.tensor(p.mean_c))
  else:
    assert md.mix_W is None and md.mix_c is None and torch.equal(md.mean_c, torch.tensor(p.mean_c))
  # a KernelRegressor around it is the same model; f32 operands are the rounded f64 ones; beta stays f64
  assert MeanDrift.from_model(gp.KernelRegressor(model), F64, "cpu") is md
  md32 = MeanDrift.from_model(model, F32, "cpu")
  assert md32.zs.dtype == F32 and md32.beta.dtype == F64 and torch.equal(md32.zs, md.zs.float()) and torch.equal(md32.beta, md.beta)
  # cached per version of the parameters
  with torch.no_grad():
    model.q_mu.mul_(2.0)
  md2 = MeanDrift.from_model(model, F64, "cpu")
  assert md2 is not md and scale_err(md2.beta, 2.0 * md.beta.numpy()) < 1e-12 and MeanDrift.from_model(model, F64, "cpu") is md2
  with pytest.raises(TypeError):
    MeanDrift.from_model(object(), F64, "cpu")


# ---- CPU: the closure's torch composition ------------------------------------------------------------------------------------------
def _cpu_system(wrap_pathwise=True, kernel="se"):
  """nx 4, one angle, one action (nd 6), small well-conditioned models: (system with the drift in a KernelRegressor, objective, x0,
  numpy drift, numpy policy)."""
  from gpflowpilco_amd import bijectors as tfb, dynamics
  from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64)
  dr = random_svgp_params(seed=21, L=4, M=10, d=6, whiten=True, ls_bounds=(0.8, 2.0), mean=True)
  dr.q_mu = 0.3 * dr.q_mu
  dr.mean_c = 0.1 * dr.mean_c
  po = random_svgp_params(seed=22, L=1, M=8, d=5, whiten=True, ls_bounds=(0.8, 2.0), mean=True)
  drift = tm._model(dr, "cpu", kernel, pathwise=wrap_pathwise)
  pol = gp_model_from_oracle(po, "cpu")
  head = tfb.Chain([tfb.Scale(t(2.0)), tfb.Shift(t(-0.5)), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=gp.KernelRegressor(drift), policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=(1,)), solver=dynamics.Euler())
  rng = np.random.default_rng(23)
  A = rng.standard_normal((5, 5))
  target, precis = np.array([0.0, 1.0, 0.1, 0.1, 0.1]), 0.5 * (A @ A.T) / 5 + 0.5 * np.eye(5)
  x0 = rng.uniform(0.2, 0.8, size=(7, 4))
  return system, GaussianObjective(target=t(target), precis=t(precis)), t(x0), dr, po, pol, (target, precis, x0)


@pytest.mark.parametrize("kernel", ["se", "matern52"])
@pytest.mark.parametrize("wrap_pathwise", [True, False], ids=["PathwiseSVGP", "SVGP"])
def test_closure_on_cpu_is_the_euler_fold_of_the_mean(wrap_pathwise, kernel):
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  system, objective, x0, dr, po, pol, (target, precis, x0n) = _cpu_system(wrap_pathwise, kernel)
  H = 4
  cost_o, _ = pmean.policy_rollout(dr, FAMILY[kernel], po, 2.0, -0.5, (1,), target, precis, x0n, H, dt=DT)
  pol.q_mu.requires_grad_(True)
  loss = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT)()
  err = float(np.abs(loss.detach().numpy() - cost_o.sum(0)).max()) / float(np.abs(cost_o).max())
  print(f"CPU closure {kernel}: loss vs helper {err:.2e} of the cost's scale")
  assert err < 1e-12
  loss.mean().backward()
  assert pol.q_mu.grad is not None and float(pol.q_mu.grad.abs().max()) > 0.0
  # paths / generator / num_bases / native_sampler: accepted, never read
  sentinel = object()
  again = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, paths=sentinel, num_bases=7,
                                       generator=torch.Generator().manual_seed(1), native_sampler=True)()
  assert torch.equal(again, loss)


def test_closure_still_refuses_a_plain_svgp_drift():
  from gpflowpilco_amd.loops import _native_parts, pathwise_policy_loss_closure
  system, objective, x0, *_ = _cpu_system(wrap_pathwise=False)
  why = []
  assert _native_parts(system, objective, why, moment_solver=False) is not None and not why     # the wrapper is looked through
  assert _native_parts(system, objective, why, moment_solver=True) is None                      # ... by the Euler solver only
  assert why == ["a solver other than MomentMatchingEuler"]
  from gpflowpilco_amd import dynamics
  system.solver = dynamics.MomentMatchingEuler()
  why = []
  assert _native_parts(system, objective, why, moment_solver=True) is None and why == ["the policy or the drift is not an SVGP"]
  system.drift = system.drift.model                                                             # a bare SVGP: no paths to read
  with pytest.raises(TypeError, match="needs a PathwiseSVGP drift"):
    pathwise_policy_loss_closure(system, objective, lambda: x0, 2)


# ---- GPU: values and Jacobian ------------------------------------------------------------------------------------------------------
# (S, M, d, L, family, mean): S 5 / 130 / 515 -- fewer samples than a block, a ragged last block, several blocks; M 37 / 200 / 777 --
# below one wave, no multiple of 64, several LDS chunks (PWM_MC = 256); d 3 / 8 / 9 / 16 -- DK 8 and 16 with and without padding;
# L 1 / 4 / 6.  Every value of every axis meets every family, and each pair (S, M), (M, d), (d, L) occurs.  The last three rows reach
# the larger sample blocks the launch picks when the batch alone fills the chip (16, 32 and 64 samples per workgroup; the rows above
# all run 8), each with a ragged last block.
EVAL_CASES = [(5, 37, 3, 1, "se", True), (130, 200, 8, 4, "matern32", False), (515, 777, 9, 6, "matern52", True),
              (130, 37, 16, 4, "se", False), (5, 777, 8, 6, "matern32", True), (515, 200, 3, 1, "matern52", False),
              (130, 777, 16, 1, "se", True), (515, 37, 9, 4, "matern32", False), (5, 200, 16, 6, "matern52", True),
              (515, 200, 8, 4, "se", True),
              (700, 200, 8, 6, "matern52", True), (1400, 37, 9, 6, "se", False), (2800, 37, 3, 6, "matern32", True)]
EVAL_IDS = ["S{}M{}d{}L{}-{}-{}".format(*c[:5], "mean" if c[5] else "nomean") for c in EVAL_CASES]


@functools.lru_cache(maxsize=None)
def _eval_case(case):
  """numpy model, its weights, inputs and the helper's f / sum |terms| / J / central differences (computed once, never modified).
  Two samples sit exactly on an inducing point."""
  S, M, d, L, name, mean = case
  fam = FAMILY[name]
  p = random_svgp_params(seed=100 + S + M + d, L=L, M=M, d=d, whiten=True, ls_bounds=(0.8, 3.0), mean=mean, separate_Z=True)
  beta = pmean.mean_weights(p, fam)
  rng = np.random.default_rng(7 + S + M)
  x = rng.uniform(size=(S, d))
  x[1], x[3] = p.Z[0][5], p.Z[L - 1][M - 1]
  x32 = x.astype(np.float32).astype(np.float64)                                     # the inputs an f32 pass receives
  g, ab = pmean.latent_values(p, fam, x32, beta)
  dirn = rng.standard_normal(x.shape)
  h = 1e-6
  fd = (pmean.mean_values(p, fam, x + h * dirn, beta) - pmean.mean_values(p, fam, x - h * dirn, beta)) / (2 * h)
  return dict(p=p, beta=beta, x=x, x32=x32, fam=fam, f=pmean.mean_values(p, fam, x, beta), J=pmean.mean_jac(p, fam, x, beta),
              f32=g if p.mean_c is None else g + p.mean_c[None], ab32=ab, J32=pmean.mean_jac(p, fam, x32, beta), dirn=dirn, fd=fd)


def _device_mean(c, dtype, device, beta=None):
  from gpflowpilco_amd.pathwise import MeanDrift
  p = c["p"]
  return MeanDrift.from_arrays(p.Z, p.lengthscales, p.variance, c["beta"] if beta is None else beta, p.mean_c, dtype=dtype,
                               device=device, kernel=c["fam"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", EVAL_CASES, ids=EVAL_IDS)
def test_gpu_f64_values_and_jacobian_match_the_helper(case, device):
  c = _eval_case(case)
  md = _device_mean(c, F64, device)
  x = torch.tensor(c["x"], dtype=F64, device=device)
  f = md(x)
  fj, J = md.eval_jac(x)
  assert torch.equal(f, fj) and torch.isfinite(f).all() and torch.isfinite(J).all()
  ef, eJ = scale_err(f, c["f"]), scale_err(J, c["J"])
  Jd = np.einsum('sld,sd->sl', J.cpu().numpy(), c["dirn"])
  efd = float(np.abs(Jd - c["fd"]).max() / max(1.0, np.abs(c["fd"]).max()))
  on = [1, 3]
  print(f"mean pass {case} f64: values {ef:.2e} Jacobian {eJ:.2e} vs central differences {efd:.2e}")
  assert ef < F64_VALUE_BAR and eJ < F64_JAC_BAR and efd < FD_BAR
  assert scale_err(f[on], c["f"][on]) < F64_VALUE_BAR and scale_err(J[on], c["J"][on]) < F64_JAC_BAR
  xg = x.clone().requires_grad_(True)                                                            # autograd through __call__
  md(xg).sum().backward()
  assert scale_err(xg.grad, c["J"].sum(1)) < F64_JAC_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("case", EVAL_CASES, ids=EVAL_IDS)
def test_gpu_f32_values_lie_inside_the_rounding_bound(case, device):
  """Per (sample, latent): |f - helper| <= BOUND_ULPS u var sum_m |beta_m k_m|, the helper in float64 at the inputs the device
  received.  The worst ratio is printed."""
  from gpflowpilco_amd.pathwise import BOUND_ULPS
  c = _eval_case(case)
  md = _device_mean(c, F32, device)
  x = torch.tensor(c["x"], dtype=F32, device=device)
  f, J = md.eval_jac(x)
  assert torch.equal(f, md(x)) and torch.isfinite(f).all() and torch.isfinite(J).all()
  bound = BOUND_ULPS * 0.5 * float(torch.finfo(F32).eps) * c["ab32"]
  ratio = np.abs(f.double().cpu().numpy() - c["f32"]) / bound
  eJ = scale_err(J, c["J32"])
  print(f"mean pass {case} f32: worst |error| / bound = {float(ratio.max()):.3f}; Jacobian {eJ:.2e}")
  assert float(ratio.max()) <= 1.0
  assert eJ < F32_JAC_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("case", [EVAL_CASES[1], EVAL_CASES[2], EVAL_CASES[6]], ids=[EVAL_IDS[1], EVAL_IDS[2], EVAL_IDS[6]])
def test_gpu_mean_pass_agrees_with_the_weight_stream(case, device):
  """The same function through the existing stream pass: ``paths_from_arrays`` with zero prior weights and v = beta for every
  sample.  Two results each within 1e-10 (1e-8) of the helper: 2e-10 of max |f|, 2e-8 of max |J|."""
  from gpflowpilco_amd.pathwise import paths_from_arrays
  c = _eval_case(case)
  p, (S, M, d, L, _, _) = c["p"], case
  stream = paths_from_arrays(np.zeros((L, 1, d)), np.zeros((L, 1)), np.zeros((S, L, 1)), np.broadcast_to(c["beta"], (S, L, M)).copy(),
                             p.Z, p.lengthscales, p.variance, p.mean_c, dtype=F64, device=device, kernel=c["fam"])
  x = torch.tensor(c["x"], dtype=F64, device=device)
  fs, Js = stream.eval_jac(x)
  fm, Jm = _device_mean(c, F64, device).eval_jac(x)
  ef = float((fs - fm).abs().max() / fs.abs().max())
  eJ = float((Js - Jm).abs().max() / Js.abs().max())
  print(f"mean pass vs weight stream {case}: values {ef:.2e} Jacobian {eJ:.2e}")
  assert ef < 2e-10 and eJ < 2e-8


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_gpu_mean_pass_is_reproducible_and_padding_adds_nothing(dtype, device):
  """Two runs are bit-equal; the entry with the unpadded M (any M is accepted) returns the bits of the padded call: a padded centre
  (beta = 0) adds exactly 0."""
  from gpflowpilco_amd.ops import _dtype_code, _ptr, _stream
  case = EVAL_CASES[2]
  c = _eval_case(case)
  S, M, d, L, _, _ = case
  md = _device_mean(c, dtype, device)
  x = torch.tensor(c["x"], dtype=dtype, device=device)
  f1, J1 = md.eval_jac(x)
  f2, J2 = md.eval_jac(x)
  assert torch.equal(f1, f2) and torch.equal(J1, J2) and md.zs.shape[-1] > M
  zs, hz, beta = md.zs[..., :M].contiguous(), md.hz[:, :M].contiguous(), md.beta[:, :M].contiguous()
  f3, J3 = torch.zeros_like(f1), torch.zeros_like(J1)
  rc = _lib.lib().mm_pathwise_mean_eval(S, L, M, d, _dtype_code(dtype), x.data_ptr(), zs.data_ptr(), hz.data_ptr(),
                                        md.lengthscales.data_ptr(), md.variance.data_ptr(), _ptr(md.mean_c), beta.data_ptr(),
                                        f3.data_ptr(), J3.data_ptr(), _stream(x.device), md.kernel)
  assert rc == 0 and torch.equal(f3, f1) and torch.equal(J3, J1)


# ---- GPU: policy rollouts ----------------------------------------------------------------------------------------------------------
S_ROLL, M_DRIFT, M_POLICY = 130, 200, 30
SCALE, SHIFT = (2.0, 1.5), (-0.5, -0.4)
SYSTEMS = {"A": dict(nx=4, active=(1,), nu=1, seed=140, Lg=None, name="se"),         # one action with an encoder, nd 6
           "B": dict(nx=4, active=(0, 1), nu=2, seed=141, Lg=None, name="se"),       # two actions, nd 8
           "W": dict(nx=6, active=(1, 2), nu=1, seed=142, Lg=None, name="se"),       # wide, nd 9
           "N": dict(nx=4, active=(), nu=1, seed=143, Lg=None, name="se"),           # no encoder, nd 5
           "G": dict(nx=4, active=(1,), nu=1, seed=144, Lg=3, name="se"),            # coregionalised: Lg 3 < nx 4
           "K": dict(nx=4, active=(1,), nu=1, seed=145, Lg=None, name="matern52")}   # a Matern-5/2 drift
FLAGS = dict(native_actions=4, native_inputs=16, native_coregionalized=True, native_no_encoder=True)


@functools.lru_cache(maxsize=None)
def _system(sysname):
  c = SYSTEMS[sysname]
  nx, active, nu, seed, Lg, fam = c["nx"], c["active"], c["nu"], c["seed"], c["Lg"], FAMILY[c["name"]]
  na = len(active); ne = nx + na; nd = ne + nu
  rng = np.random.default_rng(seed)
  if Lg is None:
    drift = oracle_params(make_svgp(nx, M_DRIFT, nd, seed=seed + 1, ls_bounds=(0.8, 3.0)))
  else:
    drift = random_svgp_params(seed=seed + 1, L=Lg, M=M_DRIFT, d=nd, whiten=True, ls_bounds=(0.8, 3.0), mean=True, W_rows=nx)
    drift.mean_c = 0.1 * drift.mean_c
  drift.q_mu = 0.3 * drift.q_mu
  drift.Z[..., ne:] = 4.0 * drift.Z[..., ne:] - 2.0                       # action axes in [-2, 2]
  pol = random_svgp_params(seed=seed + 2, L=nu, M=M_POLICY, d=ne, whiten=True, ls_bounds=(0.8, 2.0), mean=True, separate_Z=True)
  pol.q_mu = 0.3 * pol.q_mu
  x0 = rng.uniform(0.2, 0.8, size=(S_ROLL, nx))
  target = np.zeros(ne); target[na:2 * na] = 1.0; target[2 * na:] = 0.1
  A = rng.standard_normal((ne, ne))
  precis = 0.5 * (A @ A.T) / ne + 0.5 * np.eye(ne)
  scale, shift = np.array(SCALE[:nu]), np.array(SHIFT[:nu])
  beta = pmean.mean_weights(drift, fam)
  cost_o, states_o = pmean.policy_rollout(drift, fam, pol, scale, shift, active, target, precis, x0, H6, dt=DT, beta=beta)
  return dict(c, fam=fam, na=na, ne=ne, nd=nd, drift=drift, pol=pol, x0=x0, target=target, precis=precis, scale=scale, shift=shift,
              beta=beta, cost_o=cost_o, states_o=states_o)


def _roll_case(sy, device, dtype, beta=None):
  from gpflowpilco_amd.pathwise import MeanDrift, PolicyRollout
  if beta is None:
    md = MeanDrift.from_model(gp.KernelRegressor(tm._model(sy["drift"], device, sy["name"])), dtype, device)
  else:
    dr, mixed = sy["drift"], sy["drift"].W is not None
    md = MeanDrift.from_arrays(dr.Z, dr.lengthscales, dr.variance, beta, None if mixed else dr.mean_c, dtype=dtype, device=device,
                               mix_W=dr.W, mix_c=dr.mean_c if mixed else None, kernel=sy["fam"])
  nu = sy["nu"]
  scale = float(sy["scale"][0]) if nu == 1 else tuple(sy["scale"])
  shift = float(sy["shift"][0]) if nu == 1 else tuple(sy["shift"])
  roll = PolicyRollout(md, gp_model_from_oracle(sy["pol"], device).packed(F64, False, device), nx=sy["nx"], active_dims=sy["active"],
                       head_scale=scale, head_shift=shift, target=torch.tensor(sy["target"]), precis=torch.tensor(sy["precis"]),
                       num_samples=S_ROLL)
  return md, roll


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("sysname", list(SYSTEMS))
def test_gpu_policy_rollout_matches_the_helper(sysname, dtype, device):
  sy = _system(sysname)
  md, roll = _roll_case(sy, device, dtype)
  assert roll.mean and roll.wide and roll.nd_entries and roll.mixed == (sy["Lg"] is not None) and roll.kernel == sy["fam"]
  x0 = torch.tensor(sy["x0"], dtype=dtype, device=device)
  cost, tape = roll(x0, H6, dt=DT, with_jacobians=False)
  cost_j, tape_j = roll(x0, H6, dt=DT, with_jacobians=True)
  assert torch.equal(cost, cost_j) and torch.equal(roll.states(tape, H6), roll.states(tape_j, H6))
  ec, es = scale_err(cost, sy["cost_o"]), scale_err(roll.states(tape, H6), sy["states_o"])
  print(f"mean-only policy rollout {sysname} {dtype}: cost {ec:.3e} states {es:.3e}")
  tol = F64_BAR if dtype == F64 else F32_BAR
  assert ec < tol and es < tol


@pytest.mark.gpu
def test_gpu_swapped_weights_are_far_outside_the_tolerance_and_runs_are_bit_equal(device):
  """Latents 0 and 1 with each other's beta: the cost moves by at least 10 x the f32 bar (a wrong index map cannot hide inside the
  tolerance).  Two runs of the rollout and of its reverse sweep are bit-equal."""
  sy = _system("B")
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device)
  _, roll = _roll_case(sy, device, F64, beta=sy["beta"])
  swapped = sy["beta"].copy()
  swapped[[0, 1]] = swapped[[1, 0]]
  _, roll_s = _roll_case(sy, device, F64, beta=swapped)
  cost, tape = roll(x0, H6, dt=DT, with_jacobians=True)
  cost_s, _ = roll_s(x0, H6, dt=DT)
  assert scale_err(cost, sy["cost_o"]) < F64_BAR
  moved = scale_err(cost_s, sy["cost_o"])
  print(f"swapped beta: the cost moves by {moved:.2e} of its scale")
  assert moved >= 10 * F32_BAR
  cost2, tape2 = roll(x0, H6, dt=DT, with_jacobians=True)
  assert torch.equal(cost, cost2) and torch.equal(roll.states(tape, H6), roll.states(tape2, H6))
  g_cost = torch.full((H6, S_ROLL), 1.0 / S_ROLL, dtype=F64, device=device)
  a1, b1 = roll.backward(tape, g_cost, H6, dt=DT, want_state_grad=True)
  a2, b2 = roll.backward(tape2, g_cost, H6, dt=DT, want_state_grad=True)
  assert torch.equal(a1, a2) and torch.equal(b1, b2) and float(a1.abs().max()) > 0.0


def _torch_system(sy, device):
  """``tests/test_pathwise_matern.py``'s torch system with the drift in a KernelRegressor (and no encoder for system N)."""
  system, objective, pm = tm._torch_system(sy, device)
  system.drift = gp.KernelRegressor(system.drift)
  if not sy["active"]:
    system.encoder = None
  return system, objective, pm


def _run(system, objective, params, x0, H, **kw):
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  for t in params + [x0]:
    t.grad = None
  loss = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=DT, **kw)()
  loss.mean().backward()
  return loss.detach(), [t.grad.detach().clone() for t in params + [x0]]


@pytest.mark.gpu
@pytest.mark.parametrize("sysname", list(SYSTEMS))
def test_gpu_gradient_through_the_closure(sysname, device):
  """d mean_s sum_h cost / d (the policy's q_mu, Z, lengthscales, variance; x0), f64: the native route against the torch
  composition of the same closure on the GPU (1e-8 relative per tensor), and against central differences (h = 1e-6) of the helper
  along one random direction of q_mu, of Z and of x0 (1e-6 max(1, |fd|))."""
  import copy
  sy = _system(sysname)
  H, nu = H6, sy["nu"]
  system, objective, pm = _torch_system(sy, device)
  groups = tm._policy_params(pm, nu)
  params = [t for ts in groups.values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)
  with warnings.catch_warnings():
    warnings.simplefilter("error")                                                   # (no fallback: the native route ran)
    ln, gn = _run(system, objective, params, x0, H, native=True, **FLAGS)
    lt, gt = _run(system, objective, params, x0, H, native=False)
  want = sy["cost_o"].sum(0)
  assert scale_err(ln, want) < F64_BAR and scale_err(lt, want) < F64_BAR
  names = [f"{k}[{a}]" for k, ts in groups.items() for a in range(len(ts))] + ["x0"]
  for nm, a_, b_ in zip(names, gn, gt):
    e = float((a_ - b_).abs().max()) / max(1e-14, float(b_.abs().max()))
    print(f"gradient {sysname} {nm}: native vs torch composition {e:.2e}")
    assert e < GRAD_BAR, (nm, e)

  rng = np.random.default_rng(5)

  def oracle_loss(pol, x_init):
    return pmean.policy_rollout(sy["drift"], sy["fam"], pol, sy["scale"], sy["shift"], sy["active"], sy["target"], sy["precis"],
                                x_init, H, dt=DT, beta=sy["beta"])[0].sum(0).mean()
  h = 1e-6
  for field, first in (("q_mu", 0), ("Z", 1)):
    base = np.asarray(getattr(sy["pol"], field), dtype=np.float64)
    dirn = rng.standard_normal(base.shape)
    vals = []
    for sgn in (1.0, -1.0):
      pol2 = copy.deepcopy(sy["pol"])
      setattr(pol2, field, base + sgn * h * dirn)
      vals.append(oracle_loss(pol2, sy["x0"]))
    fd = (vals[0] - vals[1]) / (2 * h)
    got = gn[0].cpu().numpy() if field == "q_mu" else np.stack([t.cpu().numpy() for t in gn[first:first + nu]])
    an = float((got.reshape(base.shape) * dirn).sum())
    print(f"gradient {sysname} {field}: native {an:+.8e} fd {fd:+.8e}")
    assert abs(fd - an) < FD_BAR * max(1.0, abs(fd)), (field, fd, an)
  dirx = rng.standard_normal(sy["x0"].shape)
  fd = (oracle_loss(sy["pol"], sy["x0"] + h * dirx) - oracle_loss(sy["pol"], sy["x0"] - h * dirx)) / (2 * h)
  an = float((gn[-1].cpu().numpy() * dirx).sum())
  assert abs(fd - an) < FD_BAR * max(1.0, abs(fd)), ("x0", fd, an)


@pytest.mark.gpu
@pytest.mark.parametrize("sysname", ["A", "B", "G"])
def test_gpu_seeded_sweep_with_a_quadratic_objective_of_the_states(sysname, device):
  """``native_objective=True`` with a caller's objective: the seeded reverse sweep against the torch composition, 1e-8."""
  sy = _system(sysname)
  system, _, pm = _torch_system(sy, device)
  params = [t for ts in tm._policy_params(pm, sy["nu"]).values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)
  tgt = torch.tensor(sy["target"], dtype=F64, device=device)
  objective = lambda x, t=None: 0.5 * ((x - tgt) ** 2).sum(-1) * (1.0 + 0.1 * float(t))
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    ln, gn = _run(system, objective, params, x0, H6, native=True, native_objective=True, **FLAGS)
    lt, gt = _run(system, objective, params, x0, H6, native=False)
  el = float((ln - lt).abs().max() / lt.abs().max())
  assert el < GRAD_BAR, el
  for i, (a_, b_) in enumerate(zip(gn, gt)):
    e = float((a_ - b_).abs().max()) / max(1e-14, float(b_.abs().max()))
    assert e < GRAD_BAR, (i, e)


# ---- GPU: the closure's routing ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_closure_routes_a_mean_only_drift(device):
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _system("A")
  system, objective, pm = _torch_system(sy, device)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device)
  want = sy["cost_o"].sum(0)
  with torch.no_grad(), warnings.catch_warnings():
    warnings.simplefilter("error")                                                   # native=None: native, silent
    auto = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT)()
    forced = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, native=True)()
    composed = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, native=False)()
  assert torch.equal(auto, forced)
  assert scale_err(auto, want) < F64_BAR and scale_err(composed, want) < F64_BAR
  # a trainable drift: the gradient route falls back once, by name; the forward stays native
  drift = system.drift.model
  drift.q_mu.requires_grad_(True)
  pm.q_mu.requires_grad_(True)
  closure = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT)
  with pytest.warns(RuntimeWarning, match="mean-only drift's parameters require a gradient") as rec:
    closure().mean().backward()
    closure().mean().backward()
  assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
  assert drift.q_mu.grad is not None and float(drift.q_mu.grad.abs().max()) > 0.0
  with torch.no_grad(), warnings.catch_warnings():
    warnings.simplefilter("error")
    assert torch.equal(pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT)(), auto)
  with pytest.raises(ValueError, match="mean-only drift's parameters require a gradient"):
    pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, native=True)()
  drift.q_mu.requires_grad_(False)
  # a Matern policy: refused when the closure is built
  sys_p, obj_p, x0_p = tm._cartpole(device, drift_kernel="se", policy_kernel="matern32")
  sys_p.drift = gp.KernelRegressor(sys_p.drift)
  with pytest.raises(ValueError, match="Matern32 policy"):
    pathwise_policy_loss_closure(sys_p, obj_p, lambda: x0_p, 2, native=True)
  # nd = 17 (nx 12, two angles, three actions): native=True names the bound
  from gpflowpilco_amd import bijectors as tfb, dynamics
  from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=device)
  dr17 = tm._model(random_svgp_params(seed=31, L=12, M=10, d=17, whiten=True, ls_bounds=(0.8, 2.0)), device, "se")
  pol17 = gp_model_from_oracle(random_svgp_params(seed=32, L=3, M=8, d=14, whiten=True, ls_bounds=(0.8, 2.0)), device)
  head = tfb.Chain([tfb.Scale(t(1.0)), tfb.Shift(t(-0.5)), tfb.NormalCDF()])
  sys17 = dynamics.DynamicalSystem(drift=gp.KernelRegressor(dr17), policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol17), invlink=head),
                                   encoder=TrigonometricEncoder(active_dims=(0, 1)), solver=dynamics.Euler())
  obj17 = GaussianObjective(target=t(np.zeros(14)), precis=t(np.eye(14)))
  x17 = t(np.random.default_rng(33).uniform(0.2, 0.8, size=(9, 12)))
  with torch.no_grad():
    with pytest.raises(ValueError, match=r"nx \+ na \+ nu = 17 > 16"):
      pathwise_policy_loss_closure(sys17, obj17, lambda: x17, 2, native=True, native_actions=4, native_inputs=16)()
    with pytest.warns(RuntimeWarning, match=r"nx \+ na \+ nu = 17 > 16"):
      l17 = pathwise_policy_loss_closure(sys17, obj17, lambda: x17, 2, native_actions=4, native_inputs=16)()
    assert torch.equal(l17, pathwise_policy_loss_closure(sys17, obj17, lambda: x17, 2, native=False)())


@pytest.mark.gpu
def test_gpu_graphed_closure_replays_the_eager_loss_and_gradient(device):
  from gpflowpilco_amd.loops import GraphedPolicyLoss, pathwise_policy_loss_closure
  sy = _system("B")
  system, objective, pm = _torch_system(sy, device)
  params = [t for ts in tm._policy_params(pm, 2).values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device)
  closure = pathwise_policy_loss_closure(system, objective, lambda: x0, 4, dt=DT, native=True, **FLAGS)
  # (the graphs first, the eager runs after them and without keeping their autograd graphs, as tests/test_pathwise_objective.py
  # does: an autograd graph alive across the capture keeps the parameters' gradient accumulators on the stream it was built on)
  graphed = GraphedPolicyLoss(lambda: closure().mean(), params)
  for it in range(2):
    for t in params:
      t.grad = None
    le = closure().mean()
    le.backward()
    ge = [t.grad.detach().clone() for t in params]
    le = le.detach().clone()
    lg, gg = graphed.loss_and_grad()
    # bit for bit, or 1e-12 where the captured policy pack is built from the parameters inside the graph (as the capture tests allow)
    assert float((lg - le).abs()) <= 1e-12 * float(le.abs())
    for a, b in zip(gg, ge):
      assert float((a - b).abs().max()) <= 1e-12 * max(1e-300, float(b.abs().max()))
    if it == 0:
      # (the forward-only graph of a built-in-cost closure reads the policy pack taken at capture, for a sampled drift too -- see
      # the closure's no-gradient branch: it is compared before the parameters move)
      assert float((graphed.loss() - le).abs()) <= 1e-12 * float(le.abs())
    with torch.no_grad():
      params[0].mul_(0.9)                                                              # q_mu: the replay follows the parameters
      x0.add_(0.01)
  graphed.check()
