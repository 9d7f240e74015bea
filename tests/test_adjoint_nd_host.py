"""The hand-derived multi-action adjoints of csrc/mm_adjoint_nd.h, checked on the CPU.

``tests/hostcheck/mm_adjoint_nd_host.hip`` compiles the header's arithmetic for one host thread (test infrastructure, built by
``__graft_entry__.build()`` through tests/hostcheck/build_nd.sh).  As in tests/test_adjoint_host.py each adjoint is compared with torch
autograd of a torch mirror of the forward it differentiates -- mmc_step_body_nd and k_compose_head_nd (csrc/mm_compose_nd.hip) written
on ``special.ndtr / owens_t / bvn_cdf``, and ``autodiff.moment_match_torch`` with L = nu latents -- under that file's bars for the
same kind of check.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from gpflowpilco_amd import autodiff
from gpflowpilco_amd.special import bvn_cdf, ndtr, owens_t
from gpflowpilco_amd.synthetic import generate_covariance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
P = C.POINTER(C.c_double)


def _load(name, script, *headers):
  so = os.path.join(ROOT, "tests", "hostcheck", f"lib{name}.so")
  deps = [os.path.join(ROOT, "tests", "hostcheck", f"{name}.hip")]
  deps += [os.path.join(ROOT, "gpflowpilco_amd", "csrc", h) for h in headers]
  if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
    subprocess.run(["bash", os.path.join(ROOT, "tests", "hostcheck", script)], check=True)
  return C.CDLL(so)


@pytest.fixture(scope="module")
def hc():
  return _load("mm_adjoint_nd_host", "build_nd.sh", "mm_adjoint_nd.h", "mm_adjoint.h")


@pytest.fixture(scope="module")
def hc1():
  return _load("mm_adjoint_host", "build.sh", "mm_adjoint.h")


def _p(a):
  return a.ctypes.data_as(P)


def _ip(a):
  return a.ctypes.data_as(C.POINTER(C.c_int32))


def _c(a):
  return np.ascontiguousarray(a, dtype=np.float64)


def _sym(A):
  return 0.5 * (A + np.swapaxes(A, -1, -2))


def _t(a, grad=False):
  return torch.tensor(np.asarray(a), dtype=F64, requires_grad=grad)


def _rel(got, want):
  return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-300))


# ---- step ---------------------------------------------------------------------------------------------------------------------
def _step_forward_nd(D, dt, m, S, Sxe, cp, Sdd, df1, dSff, dcross):
  """mmc_step_body_nd (csrc/mm_compose_nd.hip) in torch: cp [ne, nu]."""
  nx, na, ne, nd, active, inactive = D
  n2 = 2 * na
  rows = []
  for r in range(nx):
    rows.append(torch.cat([Sxe[r], Sxe[r] @ cp]) if r in active else Sdd[n2 + inactive.index(r)])
  Sxf = torch.stack(rows) @ dcross
  return m + dt * df1, S + dt * (Sxf + Sxf.T) + dt * dt * dSff


def _step_case(rng, nx, active, nu):
  na = len(active); ne = nx + na; nd = ne + nu
  vals = dict(Sxe=rng.standard_normal((nx, ne)), cp=rng.standard_normal((ne, nu)), Sdd=rng.standard_normal((nd, nd)),
              df1=rng.standard_normal(nx), dSff=rng.standard_normal((nx, nx)), dcross=rng.standard_normal((nd, nx)))
  return vals, rng.standard_normal(nx), rng.standard_normal((nx, nx))


_STEP_NAMES = ["Sxe", "cp", "Sdd", "df1", "dSff", "dcross"]


def _step_nd(hc, nx, active, nu, dt, vals, gm1, gS1):
  out = {k: np.zeros_like(vals[k]) for k in _STEP_NAMES}
  act = np.array(active, dtype=np.int32)
  rc = hc.hc_step_bwd_nd(nx, len(active), nu, _ip(act), C.c_double(dt), _p(_c(vals["Sxe"])), _p(_c(vals["cp"])), _p(_c(vals["Sdd"])),
                         _p(_c(vals["dcross"])), _p(_c(gm1)), _p(_c(gS1)), _p(out["Sxe"]), _p(out["cp"]), _p(out["Sdd"]),
                         _p(out["df1"]), _p(out["dSff"]), _p(out["dcross"]))
  assert rc == 0
  return out


@pytest.mark.parametrize("nu", [2, 3])
def test_step_adjoint_nd(hc, nu):
  rng = np.random.default_rng(50 + nu)
  nx, active, dt = 5, (3, 1), 0.7
  na = len(active); ne = nx + na; nd = ne + nu
  inactive = [r for r in range(nx) if r not in active]
  vals, gm1, gS1 = _step_case(rng, nx, active, nu)
  ts = {k: _t(v, True) for k, v in vals.items()}
  m, S = _t(rng.standard_normal(nx), True), _t(rng.standard_normal((nx, nx)), True)
  m1, S1 = _step_forward_nd((nx, na, ne, nd, active, inactive), dt, m, S, **ts)
  want = torch.autograd.grad((m1 * _t(gm1)).sum() + (S1 * _t(gS1)).sum(), [ts[k] for k in _STEP_NAMES] + [m, S])
  out = _step_nd(hc, nx, active, nu, dt, vals, gm1, gS1)
  for k, w in zip(_STEP_NAMES, want):
    assert _rel(out[k], w.numpy()) < 1e-13, k
  assert _rel(gm1, want[-2].numpy()) < 1e-15 and _rel(gS1, want[-1].numpy()) < 1e-15     # the direct terms


# ---- head ---------------------------------------------------------------------------------------------------------------------
def _head_forward_nd(scale, shift, pf1, pSff, pcross, See, me):
  """k_compose_head_nd (csrc/mm_compose_nd.hip) in torch, on special.ndtr / owens_t / bvn_cdf: -> cp, md, Sdd."""
  nu = pf1.shape[0]
  vx = torch.clamp(torch.diagonal(pSff), min=0.0)
  isq = torch.rsqrt(vx + 1.0); z = isq * pf1
  y1 = ndtr(z)
  y2 = torch.diag_embed(y1 - 2.0 * owens_t(z, torch.rsqrt(1.0 + 2.0 * vx)))
  iu = torch.triu_indices(nu, nu, 1)
  if iu.shape[1]:
    rho = (pSff * isq[:, None] * isq[None, :])[iu[0], iu[1]]
    pair = bvn_cdf(z[iu[0]], z[iu[1]], rho.clamp(-1.0, 1.0))
    y2 = y2.clone()
    y2[iu[0], iu[1]] = pair
    y2[iu[1], iu[0]] = pair
  hpre = isq * (2.0 * math.pi) ** -0.5 * torch.exp(-0.5 * z * z) * scale
  cp = pcross * hpre[None, :]
  Seu = See @ cp
  mu_u = scale * (y1 + shift)
  Suu = scale[:, None] * scale[None, :] * (y2 - y1[:, None] * y1[None, :])
  md = torch.cat([me, mu_u])
  Sdd = torch.cat([torch.cat([See, Seu], 1), torch.cat([Seu.T, Suu], 1)], 0)
  return cp, md, Sdd


def _head_draws(rng, nu):
  """(pf1, pSff) draws: correlations around 0.3, one |rho| ~ 0.95, a negative rho, a diagonal pSff."""
  out = []
  for kind in ("mild", "high", "negative", "diagonal"):
    sd = np.exp(rng.uniform(np.log(0.4), np.log(1.5), size=nu))
    R = np.eye(nu)
    if kind == "mild":
      R = np.full((nu, nu), 0.3) + 0.7 * np.eye(nu)
    elif kind == "high":
      # |rho_01| = |pSff_01| / sqrt((1 + v_0)(1 + v_1)) ~ 0.95 needs large variances: v = 40, correlation 0.974
      sd[0] = sd[1] = math.sqrt(40.0)
      R[0, 1] = R[1, 0] = 0.95 * 41.0 / 40.0
    elif kind == "negative":
      R[0, nu - 1] = R[nu - 1, 0] = -0.6
    pSff = R * sd[:, None] * sd[None, :]
    assert np.linalg.eigvalsh(pSff).min() > 0.0
    out.append((kind, rng.uniform(-1.2, 1.2, size=nu), pSff))
  return out


@pytest.mark.parametrize("nu", [2, 3, 4])
def test_head_adjoint_nd(hc, nu):
  rng = np.random.default_rng(70 + nu)
  ne = 5; nd = ne + nu
  scale = np.array([2.0, 0.7, 1.3, 3.1])[:nu]; shift = np.array([-0.5, 0.2, -0.8, -0.4])[:nu]
  for kind, pf1v, pSffv in _head_draws(rng, nu):
    if kind == "high":
      isq = 1.0 / np.sqrt(np.diag(pSffv) + 1.0)
      assert abs(abs(pSffv[0, 1] * isq[0] * isq[1]) - 0.95) < 1e-12
    pf1, pSff = _t(pf1v, True), _t(pSffv, True)
    pcross = _t(rng.standard_normal((ne, nu)), True); See = _t(generate_covariance(rng, ne, (), 0.3), True)
    me = _t(rng.standard_normal(ne), True)
    cp, md, Sdd = _head_forward_nd(_t(scale), _t(shift), pf1, pSff, pcross, See, me)
    gmd, gSdd, gcp = rng.standard_normal(nd), rng.standard_normal((nd, nd)), rng.standard_normal((ne, nu))
    want = torch.autograd.grad((md * _t(gmd)).sum() + (Sdd * _t(gSdd)).sum() + (cp * _t(gcp)).sum(), (me, See, pcross, pf1, pSff))
    gme = np.zeros(ne); gSee = np.zeros((ne, ne)); gpc = np.zeros((ne, nu)); gpf1 = np.zeros(nu); gpSff = np.zeros((nu, nu))
    hc.hc_head_bwd_nd(ne, nu, _p(_c(scale)), _p(_c(shift)), _p(_c(pf1v)), _p(_c(pSffv)), _p(_c(pcross.detach().numpy())),
                      _p(_c(See.detach().numpy())), _p(_c(gmd)), _p(_c(gSdd)), _p(_c(gcp)), _p(gme), _p(gSee), _p(gpc), _p(gpf1),
                      _p(gpSff))
    assert _rel(gme, want[0].numpy()) < 1e-12 and _rel(gSee, want[1].numpy()) < 1e-12, kind
    assert _rel(gpc, want[2].numpy()) < 1e-12, kind
    w1, w2 = want[3].numpy(), want[4].numpy()                         # Owen's T: 48-point quadrature vs closed form
    assert np.all(np.abs(gpf1 - w1) < 1e-9 * np.maximum(1.0, np.abs(w1))), (kind, gpf1, w1)
    assert np.all(np.abs(gpSff - w2) < 1e-9 * np.maximum(1.0, np.abs(w2))), (kind, gpSff, w2)
    if kind != "diagonal":
      assert np.abs(w2[np.triu_indices(nu, 1)]).max() > 1e-3            # the pair terms are there to be missed


# ---- policy match ---------------------------------------------------------------------------------------------------------------
def _policy_case(rng, nu, M, d):
  Z = rng.uniform(size=(nu, M, d)); ls = np.exp(rng.uniform(np.log(0.6), np.log(2.0), size=(nu, d)))
  var = 0.6 + 0.5 * rng.uniform(size=nu)
  beta = rng.standard_normal((nu, M)); meanc = rng.standard_normal(nu)
  mu = rng.uniform(0.2, 0.8, size=d); Sigma = generate_covariance(rng, d, (), 0.15)
  return Z, ls, var, beta, meanc, mu, Sigma


def _glen(M, d):
  return M * d + M + d + 2


def _check_policy_groups(gpar, want, nu, M, d, ls, tol):
  """gpar [nu, glen] against autograd's (dZ, dbeta, dls, dvar, dmean), latent by latent."""
  for a in range(nu):
    g = gpar[a]
    assert _rel(g[:M * d].reshape(M, d), want[0].numpy()[a]) < tol, ("dZ", a)
    assert _rel(g[M * d:M * d + M], want[1].numpy()[a]) < tol, ("dbeta", a)
    assert _rel(2.0 * ls[a] * g[M * d + M:M * d + M + d], want[2].numpy()[a]) < tol, ("dls", a)      # d/d ls = 2 ls d/d ls^2
    wv, wm = float(want[3][a]), float(want[4][a])
    assert abs(g[-2] - wv) < tol * max(1.0, abs(wv)), ("dvar", a)
    assert abs(g[-1] - wm) < tol * max(1.0, abs(wm)), ("dmean", a)


@pytest.mark.parametrize("nu,M,d", [(2, 30, 6), (3, 7, 2), (4, 12, 4)])
def test_policy_match_adjoint_nd_inputs_and_parameters(hc, nu, M, d):
  rng = np.random.default_rng(100 * nu + M + d)
  Z, ls, var, beta, meanc, mu, Sigma = _policy_case(rng, nu, M, d)
  gf1, gSff, gcross = rng.standard_normal(nu), rng.standard_normal((nu, nu)), rng.standard_normal((d, nu))
  Zt, lst, vart, bt, mct = _t(Z, True), _t(ls, True), _t(var, True), _t(beta, True), _t(meanc, True)
  mut, St = _t(mu[None], True), _t(Sigma, True)
  f1, Sff, cross = autodiff.moment_match_torch(mut, (0.5 * (St + St.T))[None], Zt, lst, vart, bt, None, mct, True, False)
  val = (f1[0] * _t(gf1)).sum() + (Sff[0] * _t(gSff)).sum() + (cross[0] * _t(gcross)).sum()
  want = torch.autograd.grad(val, (mut, St, Zt, bt, lst, vart, mct))
  gmu = np.zeros(d); gS = np.zeros((d, d)); gpar = np.zeros((nu, _glen(M, d)))
  rc = hc.hc_policy_nd_bwd(nu, M, d, _p(_c(Z)), _p(_c(beta)), _p(_c(ls * ls)), _p(_c(var)), _p(_c(mu)), _p(_c(Sigma)), _p(_c(gf1)),
                           _p(_c(gSff)), _p(_c(gcross)), _p(gmu), _p(gS), _p(gpar))
  assert rc == 0
  tol = 2e-10
  assert _rel(gmu, want[0].numpy()[0]) < tol and _rel(gS, _sym(want[1].numpy())) < tol
  _check_policy_groups(gpar, want[2:], nu, M, d, ls, tol)


@pytest.mark.parametrize("M,d", [(30, 6), (7, 2)])
def test_policy_pair_adjoint_alone(hc, M, d):
  """mma_policy_pair_bwd by itself: the adjoint of Sff[0, 1] of a two-latent match, seeded through both triangle entries."""
  rng = np.random.default_rng(7 * M + d)
  Z, ls, var, beta, meanc, mu, Sigma = _policy_case(rng, 2, M, d)
  g01, g10 = 0.9, -0.35
  Zt, lst, vart, bt = _t(Z, True), _t(ls, True), _t(var, True), _t(beta, True)
  mut, St = _t(mu[None], True), _t(Sigma, True)
  _, Sff, _ = autodiff.moment_match_torch(mut, (0.5 * (St + St.T))[None], Zt, lst, vart, bt, None, _t(meanc), True, False)
  want = torch.autograd.grad(g01 * Sff[0, 0, 1] + g10 * Sff[0, 1, 0], (mut, St, Zt, bt, lst, vart))
  gmu = np.zeros(d); gS = np.zeros((d, d)); gpar = np.zeros((2, _glen(M, d)))
  hc.hc_policy_pair_bwd.restype = C.c_int
  rc = hc.hc_policy_pair_bwd(M, d, _p(_c(Z[0])), _p(_c(beta[0])), _p(_c(ls[0] ** 2)), C.c_double(var[0]), _p(_c(Z[1])),
                             _p(_c(beta[1])), _p(_c(ls[1] ** 2)), C.c_double(var[1]), _p(_c(mu)), _p(_c(Sigma)), C.c_double(g01 + g10),
                             _p(gmu), _p(gS), _p(gpar[0]), _p(gpar[1]))
  assert rc == 0
  tol = 2e-10
  assert _rel(gmu, want[0].numpy()[0]) < tol and _rel(gS, _sym(want[1].numpy())) < tol
  zero = torch.zeros(2, dtype=F64)
  _check_policy_groups(gpar, tuple(want[2:]) + (zero,), 2, M, d, ls, tol)      # the means do not enter a centred pair


# ---- nu = 1: the nd functions against the one-action ones -------------------------------------------------------------------------
def test_one_action_through_the_nd_functions(hc, hc1):
  rng = np.random.default_rng(11)
  # step
  nx, active, dt = 5, (3, 1), 0.7
  vals, gm1, gS1 = _step_case(rng, nx, active, 1)
  out = _step_nd(hc, nx, active, 1, dt, vals, gm1, gS1)
  ref = {k: np.zeros_like(vals[k]) for k in _STEP_NAMES}
  act = np.array(active, dtype=np.int32)
  hc1.hc_step_bwd(nx, len(active), _ip(act), C.c_double(dt), _p(_c(vals["Sxe"])), _p(_c(vals["cp"])), _p(_c(vals["Sdd"])),
                  _p(_c(vals["dcross"])), _p(_c(gm1)), _p(_c(gS1)), _p(ref["Sxe"]), _p(ref["cp"]), _p(ref["Sdd"]), _p(ref["df1"]),
                  _p(ref["dSff"]), _p(ref["dcross"]))
  for k in _STEP_NAMES:
    assert _rel(out[k], ref[k]) < 1e-13, k
  # head
  ne = 5; nd = ne + 1
  for pf1v, pSffv in ((0.3, 0.6), (-1.2, 0.05), (0.0, 2.0)):
    pcross = rng.standard_normal(ne); See = generate_covariance(rng, ne, (), 0.3)
    gmd, gSdd, gcp = rng.standard_normal(nd), rng.standard_normal((nd, nd)), rng.standard_normal(ne)
    gme = np.zeros(ne); gSee = np.zeros((ne, ne)); gpc = np.zeros(ne); gpf1 = np.zeros(1); gpSff = np.zeros(1)
    hc.hc_head_bwd_nd(ne, 1, _p(_c([2.0])), _p(_c([-0.5])), _p(_c([pf1v])), _p(_c([pSffv])), _p(_c(pcross)), _p(_c(See)), _p(_c(gmd)),
                      _p(_c(gSdd)), _p(_c(gcp)), _p(gme), _p(gSee), _p(gpc), _p(gpf1), _p(gpSff))
    rme = np.zeros(ne); rSee = np.zeros((ne, ne)); rpc = np.zeros(ne); rp2 = np.zeros(2)
    hc1.hc_head_bwd(ne, C.c_double(2.0), C.c_double(-0.5), C.c_double(pf1v), C.c_double(pSffv), _p(_c(pcross)), _p(_c(See)),
                    _p(_c(gmd)), _p(_c(gSdd)), _p(_c(gcp)), _p(rme), _p(rSee), _p(rpc), _p(rp2))
    assert _rel(gme, rme) < 1e-13 and _rel(gSee, rSee) < 1e-13 and _rel(gpc, rpc) < 1e-13
    assert _rel(gpf1, rp2[:1]) < 1e-13 and _rel(gpSff, rp2[1:]) < 1e-13
  # policy match
  M, d = 30, 5
  Z, ls, var, beta, meanc, mu, Sigma = _policy_case(rng, 1, M, d)
  gf1, gSff, gcross = 0.7, -1.3, rng.standard_normal(d)
  gmu = np.zeros(d); gS = np.zeros((d, d)); gpar = np.zeros(_glen(M, d))
  assert hc.hc_policy_nd_bwd(1, M, d, _p(_c(Z)), _p(_c(beta)), _p(_c(ls * ls)), _p(_c(var)), _p(_c(mu)), _p(_c(Sigma)), _p(_c([gf1])),
                             _p(_c([gSff])), _p(_c(gcross)), _p(gmu), _p(gS), _p(gpar)) == 0
  rmu = np.zeros(d); rS = np.zeros((d, d)); rpar = np.zeros(_glen(M, d))
  assert hc1.hc_policy_small_bwd(M, d, _p(_c(Z[0])), _p(_c(beta[0])), _p(_c(ls[0] ** 2)), C.c_double(var[0]), _p(_c(mu)), _p(_c(Sigma)),
                                 C.c_double(gf1), C.c_double(gSff), _p(_c(gcross)), _p(rmu), _p(rS), _p(rpar)) == 0
  assert _rel(gmu, rmu) < 1e-13 and _rel(gS, rS) < 1e-13 and _rel(gpar, rpar) < 1e-13
