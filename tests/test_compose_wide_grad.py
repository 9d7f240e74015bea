"""The native moment-matched policy gradient for 8 < ne <= 16 encoded dims: the tapes of the ``_nd`` family
(``mm_rollout_composed_taped_nd`` / ``_taped_nd_mixed``) and the wide reverse sweep ``mm_compose_wide_backward*``
(csrc/mm_compose_bwd_nd.hip, the one-wave dense paths of csrc/mm_adjoint.h), opt-in through ``native_wide=``.

Cases (B 3, drift M 40, policy M 12; the generator and ``_torch_system`` are those of tests/test_gpu_compose_wide.py, whose CPU
guards cover the conditioning of w9, w16, n13 and mix11):
  w9     nx 7,  angles (4, 1),        1 action   ne 9 / nd 10    first size past every <= 8 path; angles out of order
  w16    nx 12, angles (0, 3, 5, 8),  1 action   16 / 17         top of the range; the drift's d > 16 generic path
  n13    nx 10, angle (2,),           2 actions  11 / 13         pair items
  n20    nx 12, angles (0, 3, 5, 8),  4 actions  16 / 20         the corner of the range (seed 320; H 2)
  mix11  nx 9,  angle (0,), Lg 4,     1 action   10 / 11         the mixed entries
  e9     nx 9,  no angle,             1 action   9 / 10          no encoder: ``native_no_encoder``

Reference: float64 autograd ON THE CPU of the torch composition with every GP match evaluated by
``autodiff.moment_match_torch`` from ``precompute()`` (the materialised evaluation of ``tests/helpers.materialised_reference``;
``moment_matching.models._run_kernels`` is replaced for the duration).  On the GPU the torch composition's drift gradient runs the
drift adjoint kernels the native sweep runs too: it is a second comparison, not an independent one.
Bars: loss 1e-9, every parameter group and m0 / S0 1e-7 of the group's scale -- those of tests/test_multiaction_grad.py."""
import copy
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, autodiff
from gpflowpilco_amd.moment_matching import models as mm_models
from oracle import mm_compose_oracle as co
from tests import multiaction_oracle as mao
from tests import test_gpu_compose_wide as wide
from tests.helpers import scale_err, to_dev
from tests.test_gpu_cost_pivoting import eliminate
from tests.test_multiaction_grad import _group_err, _trainable

F64 = torch.float64
MD, MP = 40, 12
WEIGHTS = (1.0, 0.6, 0.8)
LOSS_BAR, GRAD_BAR = 1e-9, 1e-7
NAMES = ("w9", "w16", "n13", "n20", "mix11", "e9")
# the generator's table is keyed by name: the new rows are added under names of their own (its own tests run over the tuple of
# names it took at import)
wide.CASES.setdefault("n20", dict(nx=12, active=(0, 3, 5, 8), nu=4, Mp=MP, H=2, seed=320))
wide.CASES.setdefault("e9", dict(nx=9, active=(), nu=1, Mp=MP, H=3, seed=330))
wide.CASES.setdefault("s1", dict(nx=4, active=(0, 1), nu=1, Mp=MP, H=3, seed=340))          # narrow shapes, through both families
wide.CASES.setdefault("s2", dict(nx=4, active=(0, 1), nu=2, Mp=MP, H=3, seed=350))


def _dims(name):
  c = wide.CASES[name]
  return c["nx"], len(c["active"]), c["nu"]


def _m_star(nx, na, nu):
  """The largest policy M the wide size function admits at (ne, nu)."""
  w = _lib.lib().mm_compose_backward_workspace_bytes_wide
  return max(M for M in range(1, 257) if w(2, nx, na, nu, MD, M) > 0)


def _route(sy):
  kw = dict(native_wide=True)
  if sy["nu"] > 1:
    kw["native_actions"] = sy["nu"]
  if sy["mixed"]:
    kw["native_coregionalized"] = True
  if sy["na"] == 0:
    kw["native_no_encoder"] = True
  return kw


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _materialised_run_kernels(x, model, full_output_cov, model_uncertainty, jitter, latent_full_cov=None):
  """``moment_matching.models._run_kernels`` without a kernel: the materialised evaluation, wherever the tensors live."""
  mu, Sxx, union = mm_models._sliced_state(x, model.latent_kernels)
  assert union is None and mu.ndim == 2
  full = full_output_cov if latent_full_cov is None else latent_full_cov
  Z, ls, var, beta, C, mean_c = model.precompute(mu.device)
  return autodiff.moment_match_torch(mu, Sxx, Z, ls, var, beta, C if model_uncertainty else None, mean_c, full,
                                     bool(model_uncertainty))


def _setup(sy, device, state_grad=True, idx=None):
  system, objective = wide._torch_system(sy, device)
  pol_model = system.policy.model.model
  params = _trainable(pol_model, sy["nu"])
  mu0, S0 = (sy["mu0"], sy["S0"]) if idx is None else (sy["mu0"][idx], sy["S0"][idx])
  m0 = to_dev(mu0, device, F64).requires_grad_(state_grad)
  S0 = to_dev(S0, device, F64).requires_grad_(state_grad)
  return system, objective, pol_model, params, m0, S0


def _grads(system, objective, params, m0, S0, H, weights=WEIGHTS, **kw):
  """-> (loss [B] numpy, {group: gradient of the weighted loss})."""
  from gpflowpilco_amd.loops import get_state_initializer, policy_loss_closure
  for t in list(params.values()) + [m0, S0]:
    t.grad = None
  loss = policy_loss_closure(system, objective, get_state_initializer(m0, S0), H, **kw)()
  wts = torch.tensor(weights[:loss.shape[0]], dtype=loss.dtype, device=loss.device)
  (loss * wts).sum().backward()
  out = {k: t.grad.detach().clone() for k, t in params.items()}
  if m0.requires_grad:
    out["m0"], out["S0"] = m0.grad.detach().clone(), 0.5 * (S0.grad + S0.grad.transpose(1, 2)).detach()
  return loss.detach().cpu().numpy(), out


def _reference_of(sy, idx=None, weights=WEIGHTS, objective=None):
  """Loss [B] and gradients of the weighted loss by float64 autograd on the CPU, every GP match materialised."""
  system, gaussian, _, params, m0, S0 = _setup(sy, "cpu", idx=idx)
  keep = mm_models._run_kernels
  mm_models._run_kernels = _materialised_run_kernels
  try:
    loss, g = _grads(system, gaussian if objective is None else objective, params, m0, S0, sy["H"], weights=weights, native=False)
  finally:
    mm_models._run_kernels = keep
  return loss, {k: v.numpy() for k, v in g.items()}


@functools.lru_cache(maxsize=None)
def _reference(name):
  """Computed once per case, shared, never modified."""
  return _reference_of(wide._system(name))


def _compare(tag, got, want, bar=GRAD_BAR):
  worst = 0.0
  for k, w in want.items():
    w = torch.as_tensor(w).detach().cpu()
    err = _group_err(got[k].detach().cpu(), w)
    worst = max(worst, err)
    print(f"wide gradient {tag} {k}: {err:.2e}")
    assert err < bar, (tag, k, err)
  return worst


# ---- CPU: sizes and argument validation ------------------------------------------------------------------------------------------
def test_size_function_of_the_wide_entries_without_gpu():
  lib = _lib.lib()
  w, wm = lib.mm_compose_backward_workspace_bytes_wide, lib.mm_compose_backward_workspace_bytes_wide_mixed
  for name in NAMES:
    nx, na, nu = _dims(name)
    for M in (1, MP, 30):
      assert w(3, nx, na, nu, MD, M) > 0, (name, M)
  assert wm(3, 9, 1, 1, 4, MD, MP) > 0 and wm(3, 9, 1, 1, 0, MD, MP) == 0 and wm(3, 9, 1, 1, 10, MD, MP) == 0
  assert w(3, 13, 4, 1, MD, MP) == 0                                                    # ne = 17
  assert w(3, 7, 2, 0, MD, MP) == 0 and w(3, 7, 2, 5, MD, MP) == 0 and w(0, 7, 2, 1, MD, MP) == 0
  assert w(3, 7, 2, 1, MD, 257) == 0 and w(3, 7, 2, 1, 0, MP) == 0
  for nu in (1, 4):
    Ms = _m_star(12, 4, nu)
    print(f"wide size function: ne 16, nu {nu}: M* = {Ms}")
    assert w(3, 12, 4, nu, MD, Ms) > 0 and w(3, 12, 4, nu, MD, Ms + 1) == 0 and Ms >= 30
  assert w(6, 7, 2, 1, MD, MP) > w(3, 7, 2, 1, MD, MP)
  # where both families take a shape their workspaces are the same; past ne = 8 only the wide one does
  assert w(3, 4, 2, 2, 100, 30) == lib.mm_compose_backward_workspace_bytes_nd(3, 4, 2, 2, 100, 30) > 0
  assert lib.mm_compose_backward_workspace_bytes_nd(3, 7, 2, 1, MD, MP) == 0
  assert lib.mm_abi_version() == 2


@pytest.mark.parametrize("entry", ["mm_compose_wide_backward", "mm_compose_wide_backward_seeded", "mm_compose_wide_backward_mixed",
                                   "mm_compose_wide_backward_mixed_seeded"])
def test_argument_validation_of_the_wide_entries_without_gpu(entry):
  """Code by code, as tests/test_multiaction_grad.py does for the ``_nd`` entries; at w9's dims (nx 7, two angles, one action)."""
  lib = _lib.lib()
  buf = (ctypes.c_char * 64)()
  p = ctypes.addressof(buf)
  F64c, F32c = _lib.MM_F64, _lib.MM_F32
  act = (ctypes.c_int32 * 2)(4, 1)
  sc, sh = (ctypes.c_double * 4)(2.0, 1.5, 1.0, 1.0), (ctypes.c_double * 4)(-0.5, -0.4, -0.6, 0.0)
  seeded, mixed = entry.endswith("_seeded"), "_mixed" in entry
  Lg = 4 if mixed else 7
  if mixed:
    tA = lib.mm_compose_tape_bytes_nd_mixed(3, 30, 7, 2, 1, Lg, 100, F64c)
    wA = lib.mm_compose_backward_workspace_bytes_wide_mixed(3, 7, 2, 1, Lg, 100, 30)
  else:
    tA = lib.mm_compose_tape_bytes_nd(3, 30, 7, 2, 1, 100, F64c)
    wA = lib.mm_compose_backward_workspace_bytes_wide(3, 7, 2, 1, 100, 30)
  assert tA > 0 and wA > 0
  big = 1 << 40

  def bargs(nx=7, nu=1, drift_L=Lg, drift_d=10, pol_d=9, pol_M=30, dtype=F64c, drift=p, scale=sc, tape=p, tape_bytes=big, gpol=p,
            gm=None, gS=None, wd=p, wb=p, wb_bytes=big, gxm=None, gxS=None, W=p):
    seeds = (gxm, gxS) if seeded else ()
    return (drift, 64, drift_L, 100, drift_d, p, 64, pol_M, pol_d, dtype, 3, 30, 1.0, nx, 2, act, nu, scale, sh, p, p,
            tape, tape_bytes, p, *seeds, gpol, gm, gS, wd, 64, wb, wb_bytes, None, None, *((W,) if mixed else ()))
  g = getattr(lib, entry)
  assert g(*bargs(nu=0)) == -2 and g(*bargs(nu=5)) == -2                              # MM_E_DIM
  assert g(*bargs(nx=15, drift_L=15 if not mixed else Lg, drift_d=18, pol_d=17)) == -2   # ne = 17
  assert g(*bargs(pol_M=257)) == -2                                                   # past M <= 256 / the LDS bound
  assert g(*bargs(drift=None)) == -1 and g(*bargs(scale=None)) == -1 and g(*bargs(tape=None)) == -1      # MM_E_ARG
  assert g(*bargs(gpol=None)) == -1 and g(*bargs(wd=None)) == -1 and g(*bargs(wb=None)) == -1
  assert g(*bargs(gm=p)) == -1 and g(*bargs(gS=p)) == -1                              # both state gradients or neither
  if seeded:
    assert g(*bargs(gxm=p)) == -1 and g(*bargs(gxS=p)) == -1                          # both seeds or neither
  if mixed:
    assert g(*bargs(W=None)) == -1
    assert g(*bargs(drift_L=0)) == -2 and g(*bargs(drift_L=8)) == -2                  # Lg outside 1 .. nx
  else:
    assert g(*bargs(drift_L=6)) == -6                                                 # MM_E_STATE: the drift has nx latents
  assert g(*bargs(dtype=F32c)) == -3                                                  # MM_E_DTYPE: f64 only
  assert g(*bargs(drift_d=9)) == -6 and g(*bargs(pol_d=8)) == -6                      # MM_E_STATE
  assert g(*bargs(tape_bytes=tA - 1)) == -4 and g(*bargs(wb_bytes=wA - 1)) == -4      # MM_E_WORKSPACE
  assert g(*bargs(tape_bytes=tA, wb_bytes=wA)) == -4                                  # ... then the drift's workspace / the packs


def test_the_wide_family_of_a_rollout_without_gpu():
  """``supports_backward_wide`` / ``backward_wide_refusal`` on stub packs, beside the unchanged narrow predicates."""
  from gpflowpilco_amd import ops
  from tests.test_compose_entries import _Pack

  def roll(nx, active, nu, Mp, Lg=None):
    ne = nx + len(active)
    mix = dict(mix_W=torch.ones(nx, Lg, dtype=F64)) if Lg else {}
    head = dict(head_scale=2.0, head_shift=-0.5) if nu == 1 else dict(head_scale=(2.0,) * nu, head_shift=(-0.5,) * nu)
    return ops.ComposedRollout(_Pack(Lg or nx, MD, ne + nu, True), _Pack(nu, Mp, ne, False), nx=nx, active_dims=active,
                               target=torch.zeros(ne, dtype=F64), precis=torch.eye(ne, dtype=F64), **head, **mix)
  for name in NAMES:
    c = wide.CASES[name]
    r = roll(c["nx"], c["active"], c["nu"], MP, c.get("Lg"))
    assert r.supports_backward_wide() and r.backward_wide_refusal() is None
    assert not r.supports_backward() and not r.supports_backward_nd() and not r.use_wide
  narrow = roll(4, (0, 1), 2, MP)
  assert narrow.supports_backward_wide() and narrow.supports_backward_nd()
  r17 = roll(13, (0, 1, 2, 3), 1, MP)
  assert not r17.supports_backward_wide() and "16" in r17.backward_wide_refusal() and "ne = 17" in r17.backward_wide_refusal()
  Ms = _m_star(12, 4, 2)
  big = roll(12, (0, 3, 5, 8), 2, Ms + 1)
  assert roll(12, (0, 3, 5, 8), 2, Ms).supports_backward_wide() and big.max_policy_M_wide() == Ms
  assert "LDS bound" in big.backward_wide_refusal() and f"M <= {Ms}" in big.backward_wide_refusal()


# ---- CPU: guards on the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_reference_is_well_posed(name):
  """Conditions on the inputs: the reference's loss is the oracle's, no gradient group is small against the bar, and evaluating
  the batch in reverse order moves nothing: the reference has no digits to lose at 1e-7."""
  sy = wide._system(name)
  assert sy["loss_o"].max() < -0.05 * sy["H"] and sy["loss_o"].min() > -0.999 * sy["H"]
  loss, g = _reference(name)
  gap = np.abs(loss - sy["loss_o"]).max()
  small = min(float(np.abs(v).max()) for v in g.values())
  rev = [2, 1, 0]
  loss_r, g_r = _reference_of(sy, idx=rev, weights=tuple(WEIGHTS[i] for i in rev))
  moved = max(float(np.abs(g_r[k][rev] - g[k]).max() / np.abs(g[k]).max()) if k in ("m0", "S0")
              else float(np.abs(g_r[k] - g[k]).max() / np.abs(g[k]).max()) for k in g)
  print(f"wide reference {name}: loss vs oracle {gap:.2e}, smallest group {small:.2e}, batch reversed {moved:.2e}")
  assert gap < 1e-12 and small >= 1e-5 and moved < 1e-12 and np.abs(loss_r[rev] - loss).max() < 1e-12


def test_the_reference_matches_finite_differences_of_the_oracle():
  """w9: central differences of the numpy oracle's loss (step and bar of
  tests/test_multiaction_grad.py::test_gpu_native_gradient_matches_finite_differences_of_the_oracle)."""
  sy = wide._system("w9")
  _, g = _reference("w9")
  wts, H = np.array(WEIGHTS), sy["H"]

  def oracle_loss(q_mu=None, mu0=None):
    pol = copy.copy(sy["pol_o"])
    if q_mu is not None:
      pol.q_mu = q_mu
    fn = lambda st: co.mm_policy(st, pol, float(sy["scale"][0]), float(sy["shift"][0]))
    l = co.policy_rollout_loss(sy["mu0"] if mu0 is None else mu0, sy["S0"], sy["drift_o"], fn, sy["active"], sy["target"],
                               sy["precis"], H)
    return float((wts * l).sum())
  eps = 1e-5

  def fd(name_, arr, idx):
    ap, am = arr.copy(), arr.copy(); ap[idx] += eps; am[idx] -= eps
    return (oracle_loss(**{name_: ap}) - oracle_loss(**{name_: am})) / (2 * eps)
  checks = [(f"q_mu[{m},0]", fd("q_mu", sy["pol_o"].q_mu, (m, 0)), g["q_mu"][m, 0]) for m in (0, 5, 11)]
  checks += [(f"m0[{b},{i}]", fd("mu0", sy["mu0"], (b, i)), g["m0"][b, i]) for b, i in ((0, 4), (1, 1), (2, 6))]
  for what, want, got in checks:
    print(f"finite differences w9 {what}: reference {float(got):+.8e} fd {want:+.8e}")
    assert abs(float(got) - want) < 2e-5 * max(1.0, abs(want)), (what, float(got), want)


# ---- CPU: the adjoint bodies at d = 9 and d = 16 (the generic arithmetic the one-wave paths must reproduce) ----------------------
@pytest.mark.parametrize("d", [9, 16])
def test_host_adjoints_at_wide_dims(d):
  from tests import test_adjoint_host as th, test_adjoint_nd_host as tn
  from gpflowpilco_amd.cost import expected_gaussian_cost
  from gpflowpilco_amd.synthetic import generate_covariance
  hc = tn._load("mm_adjoint_nd_host", "build_nd.sh", "mm_adjoint_nd.h", "mm_adjoint.h")
  hc1 = tn._load("mm_adjoint_host", "build.sh", "mm_adjoint.h")
  _p, _c, _t, _rel, _sym = tn._p, tn._c, tn._t, tn._rel, tn._sym
  # the policy match with two latents: two latent items and one pair item, three SPD inverses at d each
  nu, M = 2, 12
  rng = np.random.default_rng(1000 + d)
  lp = 0.5 * np.sqrt(d / 4.0)
  Z = rng.uniform(size=(nu, M, d)); ls = np.exp(rng.uniform(np.log(lp), np.log(2.4 * lp), size=(nu, d)))
  var = 0.6 + 0.5 * rng.uniform(size=nu); beta = rng.standard_normal((nu, M)); meanc = rng.standard_normal(nu)
  mu = rng.uniform(0.2, 0.8, size=d); Sigma = generate_covariance(rng, d, (), 0.15)
  gf1, gSff, gcross = rng.standard_normal(nu), rng.standard_normal((nu, nu)), rng.standard_normal((d, nu))
  Zt, lst, vart, bt, mct = _t(Z, True), _t(ls, True), _t(var, True), _t(beta, True), _t(meanc, True)
  mut, St = _t(mu[None], True), _t(Sigma, True)
  f1, Sff, cross = autodiff.moment_match_torch(mut, (0.5 * (St + St.T))[None], Zt, lst, vart, bt, None, mct, True, False)
  val = (f1[0] * _t(gf1)).sum() + (Sff[0] * _t(gSff)).sum() + (cross[0] * _t(gcross)).sum()
  want = torch.autograd.grad(val, (mut, St, Zt, bt, lst, vart, mct))
  gmu = np.zeros(d); gS = np.zeros((d, d)); gpar = np.zeros((nu, tn._glen(M, d)))
  rc = hc.hc_policy_nd_bwd(nu, M, d, _p(_c(Z)), _p(_c(beta)), _p(_c(ls * ls)), _p(_c(var)), _p(_c(mu)), _p(_c(Sigma)), _p(_c(gf1)),
                           _p(_c(gSff)), _p(_c(gcross)), _p(gmu), _p(gS), _p(gpar))
  assert rc == 0
  tol = 2e-10
  assert _rel(gmu, want[0].numpy()[0]) < tol and _rel(gS, _sym(want[1].numpy())) < tol
  tn._check_policy_groups(gpar, want[2:], nu, M, d, ls, tol)
  # the cost adjoint: the pivoted solve with n = nr = d
  mean = rng.standard_normal(d); cov = generate_covariance(rng, d, (), 0.5); target = rng.standard_normal(d)
  W = generate_covariance(rng, d, (), 1.5) / d
  mt, ct = _t(mean, True), _t(cov, True)
  cost = expected_gaussian_cost(mt, 0.5 * (ct + ct.T), _t(target), _t(W))
  gm_w, gc_w = torch.autograd.grad(1.7 * cost, (mt, ct))
  gm = np.zeros(d); gc = np.zeros((d, d))
  hc1.hc_cost_bwd.restype = ctypes.c_double
  got = hc1.hc_cost_bwd(d, _p(_c(mean)), _p(_c(cov)), _p(_c(target)), _p(_c(W)), ctypes.c_double(1.7), _p(gm), _p(gc))
  assert abs(got - float(cost.detach())) < 1e-13
  assert _rel(gm, gm_w.numpy()) < 1e-11 and _rel(_sym(gc), _sym(gc_w.numpy())) < 1e-11


# ---- the precision whose cost adjoint exchanges rows -----------------------------------------------------------------------------
def _pivoting_precision(ne, seed=5):
  """tests/test_gpu_cost_pivoting.py::gen's covariance as a precision: a near-rank-one correlation with row scales over 1.6
  decades, ascending, times 30."""
  rng = np.random.default_rng(seed)
  Q = rng.standard_normal((ne, ne))
  R0 = Q @ Q.T / ne + 0.02 * np.eye(ne)
  r = np.sqrt(np.diag(R0))
  R0 = R0 / r[:, None] / r[None, :]
  s = np.sort(10.0 ** rng.uniform(-1.6, 0.0, size=ne))
  sg = rng.choice([-1.0, 1.0], size=ne)
  R = 0.1 * R0 + 0.9 * sg[:, None] * sg[None, :]
  return 30.0 * R * s[:, None] * s[None, :]


@functools.lru_cache(maxsize=None)
def _pivoting_case():
  """w9 with that precision: -> (sy, step costs [H, B], exchanged [H, B] bool: the elimination of I + W S exchanges rows)."""
  base = wide._system("w9")
  sy = dict(base, precis=_pivoting_precision(base["ne"]))
  sy["loss_o"], sy["traj_o"], sy["cost_o"] = wide._oracle(sy, sy["active"])
  exchanged = np.zeros((sy["H"], sy["B"]), dtype=bool)
  for h, (mu, S) in enumerate(sy["traj_o"]):
    enc = co.mm_encoder((mu, S, True), sy["active"])["y"]
    me, See = enc[0], co.covariance(enc)
    for b in range(sy["B"]):
      # eliminate() factors I + cov W: called with the precision as its cov and See as its W that is the cost adjoint's
      # I + W See, pivot for pivot (the first largest entry)
      _, sw = eliminate(me[b:b + 1], sy["precis"][None], sy["target"], See[b], ft=np.float64)
      exchanged[h, b] = sw.any()
  return sy, sy["cost_o"], exchanged


def test_the_pivoting_precision_exchanges_rows():
  sy, costs, exchanged = _pivoting_case()
  print(f"wide pivoting: {int(exchanged.sum())} of {exchanged.size} (element, step) pairs exchange rows; step costs "
        f"{costs.min():.2f} .. {costs.max():.2f}")
  assert exchanged.sum() >= 3 and costs.min() > -0.95 and costs.max() < -0.05


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_taped_forward_equals_the_untaped_forward(name, device):
  sy = wide._system(name)
  roll = wide._rollout(sy, device, F64)
  assert roll.supports_backward_wide() and not roll.supports_backward() and not roll.supports_backward_nd()
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  H = sy["H"]
  m_H, S_H, cost = roll(mx, Sxx, H)
  m_t, S_t, cost_t, tape = roll.taped_wide(mx, Sxx, H)
  roll.drift.check_status(3)
  assert cost_t.shape == (H, 3)
  errs = (scale_err(m_t, m_H.cpu().numpy()), scale_err(S_t, S_H.cpu().numpy()), scale_err(cost_t.T, cost.cpu().numpy()))
  print(f"wide taped vs untaped {name}: {errs}")
  assert max(errs) < 1e-12
  assert scale_err(cost_t.sum(0), sy["loss_o"]) < 1e-7
  assert torch.equal(mx, to_dev(sy["mu0"], device, F64))
  with pytest.raises(ValueError):
    roll.taped_nd(mx, Sxx, H)                                           # the narrow family keeps refusing


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_native_gradient_matches_the_reference(name, device):
  sy = wide._system(name)
  loss_r, g_r = _reference(name)
  system, objective, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")                                      # no fall-back warning
    loss_n, gn = _grads(system, objective, params, m0, S0, sy["H"], **_route(sy))
  loss_t, gt = _grads(system, objective, params, m0, S0, sy["H"], native=False)
  system.drift.packed(F64, True, device).check_status(3)
  print(f"wide gradient {name}: loss vs reference {np.abs(loss_n - loss_r).max():.2e}, vs torch composition "
        f"{np.abs(loss_n - loss_t).max():.2e}")
  assert np.abs(loss_n - loss_r).max() < LOSS_BAR and np.abs(loss_n - loss_t).max() < LOSS_BAR
  worst = _compare(f"{name} vs reference", gn, g_r)
  worst_t = _compare(f"{name} vs torch composition", gn, gt)
  print(f"wide gradient {name}: worst group vs reference {worst:.2e}, vs torch composition {worst_t:.2e}")


@pytest.mark.gpu
def test_gpu_default_routing_is_unchanged(device):
  """Without ``native_wide``: one RuntimeWarning with today's text, the torch composition's gradients bit for bit."""
  sy = wide._system("w9")
  system, objective, pol_model, params, m0, S0 = _setup(sy, device)
  _, gt = _grads(system, objective, params, m0, S0, sy["H"], native=False)
  with pytest.warns(RuntimeWarning, match=r"encoded dim <= 8") as rec:
    _, gd = _grads(system, objective, params, m0, S0, sy["H"])
  mine = [w for w in rec if issubclass(w.category, RuntimeWarning)]
  assert len(mine) == 1 and "torch composition" in str(mine[0].message)
  assert all(torch.equal(gd[k], gt[k]) for k in gt)
  sy2 = wide._system("n13")
  system, objective, pol_model, params, m0, S0 = _setup(sy2, device)
  _, gt = _grads(system, objective, params, m0, S0, sy2["H"], native=False)
  with pytest.warns(RuntimeWarning, match=r"LDS bound of the multi-action reverse sweep") as rec:
    _, gd = _grads(system, objective, params, m0, S0, sy2["H"], native_actions=2)
  assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
  assert all(torch.equal(gd[k], gt[k]) for k in gt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s1", "s2"])
def test_gpu_narrow_shapes_through_the_wide_entries(name, device):
  """nx 4, two angles (ne 6), one action and two: the wide sweep against the ``_nd`` sweep over the same tape."""
  sy = wide._system(name)
  roll = wide._rollout(sy, device, F64)
  assert roll.supports_backward_nd() and roll.supports_backward_wide()
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  H = sy["H"]
  g_cost = to_dev(np.random.default_rng(1).uniform(0.5, 1.5, (H, 3)), device, F64)
  _, _, c1, tape1 = roll.taped_nd(mx, Sxx, H)
  ref = roll.backward_nd(tape1, g_cost, 3, H)
  _, _, c2, tape2 = roll.taped_wide(mx, Sxx, H)
  got = roll.backward_wide(tape2, g_cost, 3, H)
  roll.drift.check_status(3)
  assert torch.equal(c1, c2) and tape1.numel() == tape2.numel()
  errs = [scale_err(a, b.cpu().numpy()) for a, b in zip(got, ref)]
  print(f"narrow {name} through the wide entries vs the nd entries: {errs}")
  assert max(errs) < 1e-9 and float(ref[0].abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w9", "n20", "mix11"])
def test_gpu_two_sweeps_over_one_tape_are_bit_equal(name, device):
  sy = wide._system(name)
  roll = wide._rollout(sy, device, F64)
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  H = sy["H"]
  _, _, _, tape = roll.taped_wide(mx, Sxx, H)
  g_cost = torch.ones(H, 3, dtype=F64, device=device)
  a = [t.clone() for t in roll.backward_wide(tape, g_cost, 3, H)]
  b = roll.backward_wide(tape, g_cost, 3, H)
  assert all(torch.equal(x, y) for x, y in zip(a, b))
  assert float(a[0].abs().max()) > 0.0 and torch.isfinite(a[0]).all()
  c = roll.backward_wide(tape, g_cost, 3, H, want_state_grad=False)
  assert c[1] is None and c[2] is None and torch.equal(c[0], a[0])


@pytest.mark.gpu
@pytest.mark.parametrize("H", [2, 5], ids=["H2", "H5-nothing-kept"])
def test_gpu_large_batch_without_the_kept_drift_blocks(H, device):
  """w9 at B = 256: its first three elements reproduce the B = 3 run.  By the rule of mm_compose_tape_bytes (512 MB for the drift's
  per-step blocks) the tape at drift M = 40 still keeps the drift's workspace and sums at H = 2 and the workspace alone at H = 3
  and 4; from H = 5 on it keeps neither and the sweep re-runs the q stage and the sweeps -- hence the second horizon (the oracle
  rollout stays positive definite there: smallest eigenvalue 0.038 at step 1, growing; step costs -0.89 .. -0.31)."""
  sy = wide._system("w9")
  B = 256
  lib = _lib.lib()
  per3 = lib.mm_compose_tape_bytes_nd(3, H, 7, 2, 1, MD, _lib.MM_F64) / 3
  if H == 5:
    assert lib.mm_compose_tape_bytes_nd(B, H, 7, 2, 1, MD, _lib.MM_F64) / B < 0.01 * per3
  roll = wide._rollout(sy, device, F64)
  mx, Sxx = to_dev(sy["mu0"], device, F64), to_dev(sy["S0"], device, F64)
  g3 = to_dev(np.random.default_rng(0).uniform(0.5, 1.5, (H, 3)), device, F64)
  _, _, cost3, tape3 = roll.taped_wide(mx, Sxx, H)
  ref = roll.backward_wide(tape3, g3, 3, H)
  idx = torch.arange(B, device=device) % 3
  _, _, costB, tapeB = roll.taped_wide(mx[idx], Sxx[idx], H)
  got = roll.backward_wide(tapeB, g3[:, idx].contiguous(), B, H)
  roll.drift.check_status(B)
  assert scale_err(costB[:, :3], cost3.cpu().numpy()) < 1e-12
  for what, a, b in zip(("g_policy", "g_mx0", "g_Sxx0"), got, ref):
    err = scale_err(a[:3], b.cpu().numpy())
    print(f"wide B = {B} H = {H} {what}: first three elements against the B = 3 run {err:.2e}")
    assert err < 1e-9, (what, err)


@pytest.mark.gpu
def test_gpu_largest_policy_takes_the_raised_lds_limit(device):
  """Policy M = M* at ne 16 with two actions (B 2, H 2): past the 64 KB default of dynamic LDS, against the reference."""
  Ms = _m_star(12, 4, 2)
  wide.CASES.setdefault("mstar", dict(nx=12, active=(0, 3, 5, 8), nu=2, Mp=Ms, H=2, seed=360, B=2))
  sy = wide._system("mstar")
  assert sy["loss_o"].max() < -0.05 * 2 and sy["loss_o"].min() > -0.999 * 2
  loss_r, g_r = _reference_of(sy)
  assert min(float(np.abs(v).max()) for v in g_r.values()) >= 1e-5
  system, objective, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    loss_n, gn = _grads(system, objective, params, m0, S0, 2, **_route(sy))
  system.drift.packed(F64, True, device).check_status(2)
  print(f"wide M* = {Ms}: loss vs reference {np.abs(loss_n - loss_r).max():.2e}")
  assert np.abs(loss_n - loss_r).max() < LOSS_BAR
  _compare(f"M* = {Ms}", gn, g_r)


@pytest.mark.gpu
def test_gpu_gradient_through_row_exchanges(device):
  """w9 with the pivoting precision: the swap branch of the one-wave solve runs in at least 3 (element, step) pairs."""
  sy, costs, exchanged = _pivoting_case()
  assert exchanged.sum() >= 3 and costs.min() > -0.95 and costs.max() < -0.05
  loss_r, g_r = _reference_of(sy)
  assert np.abs(loss_r - sy["loss_o"]).max() < 1e-12
  system, objective, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    loss_n, gn = _grads(system, objective, params, m0, S0, sy["H"], **_route(sy))
  print(f"wide pivoting: loss vs reference {np.abs(loss_n - loss_r).max():.2e}")
  assert np.abs(loss_n - loss_r).max() < LOSS_BAR
  _compare("pivoting", gn, g_r)


class _Quadratic:
  """(1 + 0.1 t) E[(e - tau)^T W (e - tau)] of the encoded state's moments."""

  def __init__(self, W, tau):
    self.W, self.tau = W, tau

  def __call__(self, x, t=None):
    e = x.mean() - self.tau
    return (1.0 + 0.1 * t) * ((e * (e @ self.W)).sum(-1) + (self.W * x.covariance(dense=True)).sum((-1, -2)))


@pytest.mark.gpu
def test_gpu_custom_objective_through_the_seeded_sweep(device):
  sy = wide._system("w9")
  rng = np.random.default_rng(7)
  A = rng.standard_normal((sy["ne"], sy["ne"]))
  obj = _Quadratic(to_dev(A @ A.T / sy["ne"] + 0.5 * np.eye(sy["ne"]), device, F64), to_dev(rng.uniform(0.0, 0.5, sy["ne"]), device, F64))
  system, _, pol_model, params, m0, S0 = _setup(sy, device)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    loss_n, gn = _grads(system, obj, params, m0, S0, sy["H"], native_objective=True, **_route(sy))
  loss_t, gt = _grads(system, obj, params, m0, S0, sy["H"], native=False)
  err = float(np.abs(loss_n - loss_t).max() / np.abs(loss_t).max())
  print(f"wide custom objective: loss {err:.2e}")
  assert err < GRAD_BAR
  _compare("custom objective vs torch composition", gn, gt)


@pytest.mark.gpu
def test_gpu_captured_replay_of_the_wide_gradient(device):
  from gpflowpilco_amd.loops import GraphedPolicyLoss, get_state_initializer, policy_loss_closure
  sy = wide._system("w9")
  system, objective, pol_model, params, m0, S0 = _setup(sy, device, state_grad=False)
  closure = policy_loss_closure(system, objective, get_state_initializer(m0, S0), sy["H"], native_wide=True)
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
      with torch.no_grad():
        pol_model.q_mu.mul_(0.9)
  assert float(ge[0].abs().max()) > 0.0


@pytest.mark.gpu
def test_gpu_fallbacks_name_their_reason(device):
  def one_warning(match, sy, **kw):
    system, objective, pol_model, params, m0, S0 = _setup(sy, device)
    params = {"q_mu": params["q_mu"]}
    with pytest.warns(RuntimeWarning, match=match) as rec:
      got = _grads(system, objective, params, m0, S0, 2, **kw)
    mine = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(mine) == 1 and "torch composition" in str(mine[0].message)
    want = _grads(system, objective, params, m0, S0, 2, native=False)
    assert np.abs(got[0] - want[0]).max() < 1e-12
    for k in want[1]:
      assert _group_err(got[1][k], want[1][k]) < 1e-10, k
  # ne = 17: nx 13 with four angles
  wide.CASES.setdefault("w17", dict(nx=13, active=(0, 3, 5, 8), nu=1, Mp=MP, H=2, seed=370))
  one_warning(r"ne = 17 > 16", wide._system("w17"), native_wide=True)
  # a policy of M* + 1 centres at ne 16 with two actions
  Ms = _m_star(12, 4, 2)
  wide.CASES.setdefault("mstar1", dict(nx=12, active=(0, 3, 5, 8), nu=2, Mp=Ms + 1, H=2, seed=360, B=2))
  one_warning(rf"LDS bound of the wide reverse sweep.*M <= {Ms}", wide._system("mstar1"), native_wide=True, native_actions=2)
