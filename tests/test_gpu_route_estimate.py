"""The f32 pack's accuracy contract item by item (csrc/mm_route.hip): every (batch element, off-diagonal pair)
item carries the sweep's estimate `est` of its own f32 error; k_route_decide re-reduces in f64 the items with est > MM_ROUTE_TOL x
scale_b and trusts the others.  Here each item is compared with a float64 reference of the same f32-rounded state:

  (a) an item left in f32 is within its own estimate (+ the f32 rounding of the output entry);
  (b) every item is within MM_ROUTE_TOL of its batch element's largest |off-diagonal covariance|;
  (c) scale_b is the quantity the contract names: max over the element's pairs of |s12 - f1 f1'|, s12 = the orders of the
      second moment the f64 moments carry (0..2, and the cubic C0 b^3 where the item has a collapsed row group);
  (d) the routed count is #{est > MM_ROUTE_TOL scale_b}, and a routed item is the f64 re-reduce's value.

The draws are built on the host to reach the collapse classes of k_item_classes / k_offdiag_stats (mm_common.h, mm_mono.h):
the item's Cauchy-Schwarz bound X = sqrt(max_i |A_i|^2 max_j |zc'_j|^2), A_i = G^T zc_i, decides degree 4 only (X <= 1/40),
degrees 4-5 (X <= 1/16), degree 6 wholly inside (X <= 1/4: no tile work), collapsed with tiles screened (X <= 1/2), collapsed
by 64-row group only (partly), not collapsed.  X is recomputed here from the model and the state, and the class counts are
cross-checked against the kernel's own (mm_offdiag_stats)."""
from itertools import combinations

import numpy as np
import pytest
import torch
from scipy.linalg import solve_triangular

from gpflowpilco_amd import ops
from gpflowpilco_amd.synthetic import make_inputs, make_svgp
from oracle import mm_oracle as mo
from tests.helpers import contract_err, f32_state, gp_model_from_oracle, oracle_params, random_svgp_params, to_dev

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64

TOL = 3.0e-4                                   # MM_ROUTE_TOL
OUT_ROUND = 2.0 ** -23                         # f32 rounding of the output entry Sff[b, a, a2] (one ulp)
X4_2, X5_2 = float(np.float32(1.0 / 1600.0)), float(np.float32(1.0 / 256.0))     # MM_C6_X4_2, MM_C6_X5_2
COLL2 = 0.25                                   # MM_COLLAPSE_BOUND2
INSIDE2 = float(np.float32(0.998) * np.float32(0.0625))                            # MM_INSIDE_BOUND2
C0, C2, C3 = (float(np.float32(v)) for v in (1.666663289e-01, 8.350561373e-03, 1.391559141e-03))
SYS2 = float(np.float32(6.33e-6))              # MM_C6_SYS2
EST_UNIT = 2.0 ** -24 * (2.0 / 3.0)            # mmx_est: est = EST_UNIT sqrt(E2)
GROUP = 64                                     # MM_GROUP_ROWS


def _pairs(L):
  """(a, a2) of off-diagonal item po: mmx_decode_pair_o (mm_route.hip) walks the upper triangle row by row, (0, 1), (0, 2), ...,
  (1, 2), ...  (pinned against the kernel by the est of the items with no tile work, in _check)."""
  return list(combinations(range(L), 2))


# ---- host side: the item's bilinear form, its bound, its class -------------------------------------------------------------

def _G(S, la, lb):
  """b_ij = zc_i^T G zc'_j: the cross term of the pair's exponent (oracle eKuffu_se_pair: z1^T (V - V (Sigma + V)^-1 V) z2
  scaled by 1/V1, 1/V2), Lambda's as vectors."""
  V = la * lb / (la + lb)
  T = V[:, None] * np.linalg.solve(S + np.diag(V), S)
  T = 0.5 * (T + T.T)
  return T / la[:, None] / lb[None, :]


def _item_geometry(p, mu, S, a, a2, perm=None, allow=True):
  """What k_pairvec_reg decides for one (state, pair): rows recentred or not, |A_i|^2, the item's bound X^2, the collapsed
  64-row groups (packed order `perm`: position -> caller index), amaxc (max |A_i|^2 over collapsed groups)."""
  Z, ls = p.Z, p.lengthscales
  la, lb = ls[a] ** 2, ls[a2] ** 2
  G = _G(S, la, lb)
  zbar, zbar2 = Z[a].mean(0), Z[a2].mean(0)
  zc2 = Z[a2] - zbar2
  zmax2 = float((zc2 * zc2).sum(1).max())
  t0 = (G.T @ (mu - zbar))                                   # T (mu - zbar_a) / La / Lb
  recentred = float(t0 @ t0) * zmax2 <= 16.0 ** 2            # MM_RECENTRE_CMAX
  rows = (Z[a] - zbar) if recentred else (Z[a] - mu)
  A = rows @ G
  a2row = (A * A).sum(1)
  X2 = float(a2row.max()) * zmax2
  M = Z.shape[1]
  order = np.arange(M) if perm is None else perm[a]
  ng = (M + GROUP - 1) // GROUP
  gmax = np.array([a2row[order[g * GROUP:(g + 1) * GROUP]].max() for g in range(ng)])
  gcoll = (gmax * zmax2 <= COLL2) & recentred & allow
  amaxc = float(gmax[gcoll].max()) if gcoll.any() else 0.0
  npad = (M + 127) // 128 * 2 - ng                          # row groups of the padding (Mp = M rounded up to 128): zero rows
  return dict(G=G, rows=rows, zc2=zc2, zmax2=zmax2, recentred=recentred, X2=X2, X=np.sqrt(X2), ngroups=ng,
              ncoll=int(gcoll.sum()), gflags=int(gcoll.sum()) + (npad if recentred and allow else 0), Xc2=amaxc * zmax2, gmargin=float(np.min(np.abs(gmax * zmax2 / COLL2 - 1.0))))


def _cls(g):
  if g["ncoll"] == 0:
    return "none"
  if g["ncoll"] < g["ngroups"]:
    return "partly"
  if g["Xc2"] <= X4_2:
    return "deg4"
  if g["Xc2"] <= X5_2:
    return "deg5"
  return "inside" if g["X2"] <= INSIDE2 else "screened"


def _beta(p):
  """K_uu^-1 m per latent, as the oracle forms it (mm_gauss_svgp_mo: iKuu_qmu)."""
  L, M, _ = p.Z.shape
  out = np.empty((L, M))
  for a in range(L):
    Lu = np.linalg.cholesky(mo.se_kernel(p.Z[a], None, p.lengthscales[a], p.variance[a]) + p.kuu_jitter * np.eye(M))
    q = p.q_mu[:, a] if p.whiten else solve_triangular(Lu, p.q_mu[:, a], lower=True)
    out[a] = solve_triangular(Lu.T, q, lower=False)
  return out


def _host_items(p, mu, S, perm, allow=True):
  """Per (b, po): the item's geometry and class, and from the oracle's intermediate terms (eKfu, eKuffu, K_uu^-1 m):
  s12 - f1 f1' (the route decision's per-pair quantity), |what|_2 |what'|_2 (what_i what'_j = beta_i <k k'>_ij beta'_j e^-b_ij),
  and the pair's full covariance (ties this decomposition to the oracle)."""
  B = mu.shape[0]
  L = p.Z.shape[0]
  beta = _beta(p)
  f1raw = np.stack([mo.eKfu_se(mu, S, p.Z[a], p.lengthscales[a], p.variance[a]) @ beta[a] for a in range(L)], axis=1)
  items = {}
  for po, (a, a2) in enumerate(_pairs(L)):
    E = mo.eKuffu_se_pair(mu, S, p.lengthscales[a], p.variance[a], p.Z[a], p.lengthscales[a2], p.variance[a2], p.Z[a2],
                          False, False)
    for b in range(B):
      g = _item_geometry(p, mu[b], S[b], a, a2, perm, allow)
      bij = g["rows"] @ g["G"] @ g["zc2"].T
      P = beta[a][:, None] * E[b] * beta[a2][None, :]
      W = P * np.exp(-bij)                                   # what_i what'_j
      poly = 1.0 + bij * (1.0 + bij * (0.5 + (C0 * bij if g["ncoll"] else 0.0)))
      ff = f1raw[b, a] * f1raw[b, a2]
      items[b, po] = dict(g, a=a, a2=a2, cls=_cls(g), s12c=float((W * poly).sum() - ff), cov=float(P.sum() - ff),
                          wnorm=float(np.sqrt((W * W).sum())))
  return items


def _scaled_for(p, mu, S0, a, a2, X):
  """c > 0 with the bound of item (a, a2) at state (mu, c S0) equal to X (X grows with c: bisection on log c)."""
  lo, hi = -30.0, 12.0
  for _ in range(80):
    mid = 0.5 * (lo + hi)
    if _item_geometry(p, mu, np.exp(mid) * S0, a, a2)["X"] < X:
      lo = mid
    else:
      hi = mid
  return float(np.exp(0.5 * (lo + hi)))


# ---- one f32 match against the reference, item by item -------------------------------------------------------------------

def _reference(p, mu, S, model, device, M):
  """float64 off-diagonal reference at the f32-rounded state: the oracle up to M = 700; beyond, the f64 pack, tied to the oracle
  on the first batch element."""
  if M <= 700:
    return mo.mm_gauss_svgp_mo(mu, S, p)[1]
  pm64 = model.packed(F64, True, device)
  ref = ops.moment_match(pm64, to_dev(mu, device, F64), to_dev(S, device, F64))[1].cpu().numpy()
  _, So, _ = mo.mm_gauss_svgp_mo(mu[:1], S[:1], p)
  assert np.abs(ref[:1] - So).max() <= 1e-9 * np.abs(So).max()
  return ref


def _check(p, model, mu, S, device, name, fused=False):
  """Run one f32 match of (mu, S) (f32-rounded first) and assert (a)-(d) on every item.  Returns the host items with the
  measured err, est, scale attached."""
  mu, S = f32_state(mu, S)
  B, L, M = mu.shape[0], p.Z.shape[0], p.Z.shape[1]
  pm = model.packed(F32, True, device)
  mu32, S32 = to_dev(mu, device, F32), to_dev(S, device, F32)
  flags = ops.make_flags(True, True)
  pm.status().zero_()
  if fused:
    _, Sff, _, _, _ = ops.moment_match_with_sums(pm, mu32, S32)
    pm.check_status(B)
    routed = pm.routed()[1]
  else:
    _, Sff, _ = ops.moment_match(pm, mu32, S32)
    routed = pm.routed()[0]
  rep = ops.route_estimates(pm, B, flags).cpu().numpy()
  # the routed items' reference: the f64 pack, whose sweep k_route_f64 repeats from the same f64 operands (at |what||what'| of
  # 1e8 x the scale the float64 oracle and the float64 pack already differ by ~5e-7 of it: both round 1e5 terms of that size)
  want64 = ops.moment_match(model.packed(F64, True, device), mu32.double(), S32.double())[1].cpu().numpy()
  c, n, inside = ops.offdiag_stats(pm, B, flags)
  partly, gcoll, _ = ops.offdiag_row_groups(pm, B, flags)
  perm = pm.perm().cpu().numpy()
  got = Sff.double().cpu().numpy()
  ref = _reference(p, mu, S, model, device, M)
  items = _host_items(p, mu, S, perm, allow=not fused)     # (the fused path's q stage collapses nothing: MM_ISTAGE_NO_M56)

  # the class of every item as the kernel decided it: host bound vs the kernel's counts
  for it in items.values():
    assert it["gmargin"] > 1e-4, (name, "a row group's bound sits on 1/2: its class is not decidable on the host")
  if not fused:
    full = [it for it in items.values() if it["ncoll"] == it["ngroups"]]
    assert (c, n) == (len(full), B * (L * (L - 1) // 2)), (name, c, n, len(full))
    assert inside == sum(it["X2"] <= INSIDE2 for it in full), (name, inside)
    assert partly == sum(it["cls"] == "partly" for it in items.values()), (name, partly)
    assert gcoll == sum(it["gflags"] for it in items.values()), (name, gcoll)

  nroute, worst = 0, {}
  for (b, po), it in items.items():
    a, a2 = it["a"], it["a2"]
    est, sc = rep[b, po]
    r = ref[b, a, a2]
    err = abs(got[b, a, a2] - r)
    own = np.abs(ref[b][~np.eye(L, dtype=bool)]).max()
    it.update(err=err, est=est, scale=sc, ratio=it["wnorm"] / sc)
    # (c) the decision's scale: the largest |s12 - f1 f1'| of the batch element, recomputed from the oracle's terms
    sc_host = max(abs(items[b, q]["s12c"]) for q in range(L * (L - 1) // 2))
    assert abs(sc - sc_host) <= 1e-6 * sc_host, (name, b, sc, sc_host)
    assert abs(it["cov"] - r) <= 1e-10 * it["wnorm"] + 1e-12 * abs(r), (name, b, po, it["cov"], r)
    # (b) the contract, item by item
    assert err <= TOL * own, (name, b, po, it["cls"], err / own, est / own)
    if est > TOL * sc:
      nroute += 1
      # (d) a routed item is the f64 re-reduce's value
      e64 = abs(got[b, a, a2] - want64[b, a, a2])
      assert e64 <= 1e-7 * sc + OUT_ROUND * abs(r), (name, b, po, it["cls"], e64 / sc)
      continue
    # (a) an unrouted item is within its own estimate; the only other f32 part of the entry is the output's rounding (f1, the
    # orders the f64 moments carry and the diagonal are float64: DESIGN.md 2.3)
    tol_a = est + OUT_ROUND * abs(r)
    key = it["cls"]
    worst[key] = max(worst.get(key, (0.0, 0.0)), (err / max(est, 1e-300), err / (TOL * sc)))
    assert err <= tol_a, (name, b, po, it["cls"], f"err/est {err / max(est, 1e-300):.3g}", err, est, abs(r))
    if not fused and it["cls"] == "inside":
      # no tile of the item is swept (estO = 0): est is mm6_estS alone, an explicit function of X and |what| |what'| -- which also
      # pins the (b, po) -> (a, a2) order of the report against the host's
      X = np.sqrt(it["Xc2"])
      amp = min(1.0, 64.0 * X ** 3)
      amp += 0.0 if it["Xc2"] > X5_2 else C3 * X ** 6 / 5.8e-10
      amp += 0.0 if it["Xc2"] > X4_2 else C2 * X ** 5 / 5.8e-10
      want = EST_UNIT * np.sqrt(SYS2) * amp * it["wnorm"]
      assert abs(est - want) <= 1e-3 * want, (name, b, po, est, want)
  # (d) the routed count is the report's: the report shows the estimate k_route_decide read (k_route_f64 writes the slab only)
  assert routed == nroute, (name, routed, nroute)
  off, dia = contract_err(got, ref)
  assert off < TOL and dia < 2e-5, (name, off, dia)
  print(f"\n{name}: routed {routed}/{len(items)}, max |what||what'|/scale "
        f"{max(it['ratio'] for it in items.values()):.2e}, max err/est | err/(3e-4 scale) per class: "
        + ", ".join(f"{k} {v[0]:.2e} | {v[1]:.2e}" for k, v in sorted(worst.items())))
  return items


@pytest.fixture(scope="module")
def device():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


# ---- per d and per class ------------------------------------------------------------------------------------------------

CLASS_X = (("deg4", 0.6 / 40.0), ("deg5", 0.044), ("inside", 0.18), ("screened", 0.4), ("partly", 0.75), ("none", 6.0))


def ls_for(d):
  """Lengthscales short enough that a wide state takes every row group beyond 1/2 (X -> |zc| |zc'| / (l^2 + l'^2) as Sigma grows)."""
  return (0.08, 0.2) if d <= 3 else (0.2, 0.5)


@pytest.mark.parametrize("d", [1, 2, 3, 5, 6, 7, 8])
def test_every_collapse_class_is_within_its_estimate(d, device):
  """One batch element per class: the state's covariance scaled so that item (0, 1)'s bound X lands in it."""
  L, M = 3, 320
  syn = make_svgp(L, M, d, seed=700 + d, ls_bounds=ls_for(d), stable=False)
  p = oracle_params(syn)
  model = syn.to_model(device)
  mu0, S0 = make_inputs(len(CLASS_X), d, seed=900 + d, scale=0.1, lo=0.35, hi=0.65)
  S = np.stack([_scaled_for(p, mu0[k], S0[k], 0, 1, X) * S0[k] for k, (_, X) in enumerate(CLASS_X)])
  items = _check(p, model, mu0, S, device, f"d={d}")
  for k, (cls, _) in enumerate(CLASS_X):
    assert items[k, 0]["cls"] == cls, (d, k, cls, items[k, 0]["cls"], items[k, 0]["X"])


# ---- class boundaries ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [3, 6])
def test_class_bounds_are_crossed_without_a_dropped_or_doubled_term(d, device):
  """Item (0, 1) 3 % below and 3 % above each bound of its collapse degree and coverage: 1/40, 1/16, 1/4, 1/2."""
  L, M = 3, 384
  syn = make_svgp(L, M, d, seed=760 + d, ls_bounds=ls_for(d), stable=False)
  p = oracle_params(syn)
  model = syn.to_model(device)
  mu0, S0 = make_inputs(1, d, seed=960 + d, scale=0.1, lo=0.4, hi=0.6)
  sides = []
  for X, below, above in ((1 / 40, "deg4", "deg5"), (1 / 16, "deg5", "inside"), (0.25, "inside", "screened"),
                          (0.5, "screened", None)):
    sides += [(0.97 * X, below), (1.03 * X, above)]
  S = np.stack([_scaled_for(p, mu0[0], S0[0], 0, 1, X) * S0[0] for X, _ in sides])
  mu = np.repeat(mu0, len(sides), axis=0)
  items = _check(p, model, mu, S, device, f"bounds d={d}")
  for k, (X, cls) in enumerate(sides):
    got = items[k, 0]["cls"]
    if cls is None:
      assert got in ("partly", "none"), (d, X, got)
    else:
      assert got == cls, (d, X, cls, got)


# ---- high cancellation -------------------------------------------------------------------------------

def _collapsed_mid(items):
  return [it for it in items.values() if it["cls"] in ("inside", "screened") and 0.125 < it["X"] <= 0.5]


def test_wide_model_narrowed_into_the_collapsed_range(device):
  """tests/test_gpu_route.py's wide model (beta up to 1e4), the states narrowed until its items are collapsed with X in
  (1/8, 1/2]: the degree-6 moments from the bf16 split and the f32 contraction carry sums |what||what'| far above the scale."""
  L, M, d, B = 5, 639, 4, 2
  p = random_svgp_params(seed=3013, L=L, M=M, d=d, whiten=True, ls_bounds=(0.5, 1.5), mean=True)
  model = gp_model_from_oracle(p, device)
  rng = np.random.default_rng(3014)
  mu = rng.uniform(0.25, 0.75, size=(B, d))
  S0 = make_inputs(B, d, seed=3015, scale=0.25)[1]
  S = np.stack([_scaled_for(p, mu[b], S0[b], 0, 1, 0.3) * S0[b] for b in range(B)])
  items = _check(p, model, mu, S, device, "wide narrowed")
  mid = _collapsed_mid(items)
  assert len(mid) >= 6, len(mid)
  assert max(it["ratio"] for it in mid) >= 1e7, max(it["ratio"] for it in mid)


def _dense_case():
  """A denser, worse-conditioned model than the wide one (640 points in 3 dimensions, lengthscales 0.6-1.2): collapsed items at
  X in (1/8, 1/2] whose |what|_2 |what'|_2 reaches 1e7 of the covariance scale and beyond."""
  L, M, d, B = 3, 640, 3, 2
  p = random_svgp_params(seed=4021, L=L, M=M, d=d, whiten=True, ls_bounds=(0.6, 1.2), mean=True)
  rng = np.random.default_rng(4022)
  mu = rng.uniform(0.3, 0.7, size=(B, d))
  S0 = make_inputs(B, d, seed=4023, scale=0.2)[1]
  S = np.stack([_scaled_for(p, mu[b], S0[b], 0, 1, 0.35) * S0[b] for b in range(B)])
  return p, mu, S


def test_dense_model_at_1e7_cancellation(device):
  p, mu, S = _dense_case()
  items = _check(p, gp_model_from_oracle(p, device), mu, S, device, "dense 1e7")
  mid = _collapsed_mid(items)
  assert mid and max(it["ratio"] for it in mid) >= 1e7, [f"{it['ratio']:.2e}" for it in mid]


def test_pilco_recipe_cut_down(device):
  """bench.py's pilco recipe (lengthscales 0.7-3, stable targets, states about the data's centre) at L = 3, M = 700, d = 8."""
  L, M, d, B = 3, 700, 8, 2
  syn = make_svgp(L, M, d, seed=1003, ls_bounds=(0.7, 3.0), stable=True)
  mu, S = make_inputs(B, d, seed=2000 + 1003, scale=0.1, lo=0.3, hi=0.7)
  items = _check(oracle_params(syn), syn.to_model(device), mu, S, device, "pilco")
  assert any(it["ncoll"] for it in items.values())


def test_fused_value_keeps_the_contract_at_high_cancellation(device):
  """mm_moment_match_with_sums takes the off-diagonal covariances from the backward sweeps (no collapse there: every row through
  the remainder aggregates), routed by their own estimate: the report then shows that estimate alone."""
  p, mu, S = _dense_case()
  model = gp_model_from_oracle(p, device)
  items = _check(p, model, mu, S, device, "dense 1e7 fused", fused=True)
  assert max(it["ratio"] for it in items.values()) >= 1e7
