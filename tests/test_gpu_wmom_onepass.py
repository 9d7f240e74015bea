"""The forward's f64 weight moments (csrc/mm_moments.hip): the one-pass GEMM tiling k_wmom_gemm1 and the one-wave-per-item
contraction k_spoly_wave8 against the 64 x 128 tiling and the one-workgroup-per-item k_spoly they replace, which
MM_ISTAGE_OLD_WMOM selects on the same build.  Every output element of the GEMM sees the same sequence of MFMA accumulations and
the contraction replays the old kernel's summation order, so

  * f1, Sff and cross agree to the bit (f32 pack, full covariance, model uncertainty), and so do the per-item route estimates
    (their scale comes from s12), the routed count and mm_offdiag_stats;
  * this holds where collapsed and other items share a latent's GEMM and the collapsed rows end inside a 64-row block, and for
    items that keep their rows centred at mu (the binomial shift by dmu in the contraction).

Both paths write into the same cached workspace and nothing clears it between calls, so a moment or an s12 entry the new kernels
left out would still hold the other run's bit-identical value.  Every pass therefore starts from a workspace filled with 0xFF
bytes (all-ones doubles are NaN; the kernels reset their own counters and lists), and the new path runs first.

States: part of the batch at std 0.1 (every item collapsed on these models), the rest at std 0.5 (none), interleaved."""
from itertools import combinations

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, ops
from gpflowpilco_amd.synthetic import make_inputs, make_svgp
from tests.helpers import f32_state, to_dev

pytestmark = pytest.mark.gpu
F32 = torch.float32
OLD_WMOM = _lib.MM_ISTAGE_OLD_WMOM
WORST = _lib.MM_FORCE_WORST_TIER
# (L, M, d, B, batch elements at the small std, extra flags):
#   R = 74: a partial row block; Mp = 384: six K blocks per slice; 30 collapsed rows per latent
#   R = 5 < 64
#   d = 3: 20 columns, two column tiles (one below degree 3)
#   d = 16: degree 2, 153 columns in ten tiles, k_spoly<32, 5>
#   forced worst tier: no cubic column at all
CASES = [(3, 300, 8, 37, 15, 0), (2, 300, 8, 5, 2, 0), (3, 300, 3, 16, 7, 0), (2, 130, 16, 8, 3, 0), (3, 300, 8, 37, 15, WORST)]
IDS = ["d8-L3-B37", "d8-L2-B5", "d3-L3-B16", "d16-L2-B8", "d8-worst-tier"]


@pytest.fixture(scope="module")
def device():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


_cache = {}


def _model(L, M, d, device):
  """(synthetic model, f32 pack) of a shape, built once per module."""
  key = (L, M, d)
  if key not in _cache:
    syn = make_svgp(L, M, d, seed=4100 + M + d, device=str(device), ls_bounds=(0.3, 3.0), stable=False)
    _cache[key] = (syn, syn.to_model(device).packed(F32, True, device))
  return _cache[key]


def _state(B, d, nsmall, seed):
  """B states, nsmall of them (spread over the batch) at std 0.1, the others at std 0.5."""
  mu, S1 = make_inputs(B, d, seed=seed, scale=0.1)
  _, S5 = make_inputs(B, d, seed=seed + 1, scale=0.5)
  small = np.zeros(B, dtype=bool)
  small[np.linspace(0, B - 1, nsmall).round().astype(int)] = True
  assert small.sum() == nsmall
  return mu, np.where(small[:, None, None], S1, S5)


def _match(pm, mu, S, extra):
  B = mu.shape[0]
  flags = ops.make_flags(True, True) | extra
  pm.status().zero_()
  pm.workspace(B, flags, peek=True).fill_(0xFF)          # whatever this pass does not write reads as NaN
  f1, Sff, cross = (t.clone() for t in ops.moment_match(pm, mu, S, extra_flags=extra))
  return dict(f1=f1, Sff=Sff, cross=cross, est=ops.route_estimates(pm, B, flags), routed=ops.offdiag_routed(pm, B, flags),
              stats=ops.offdiag_stats(pm, B, flags), groups=ops.offdiag_row_groups(pm, B, flags))


def _assert_same(got, ref):
  for k in ("f1", "Sff", "cross", "est"):
    assert torch.equal(got[k], ref[k]), (k, float((got[k].double() - ref[k].double()).abs().max()))
  assert got["routed"] == ref["routed"] and got["stats"] == ref["stats"] and got["groups"] == ref["groups"], (got, ref)
  for k in ("f1", "Sff", "cross", "est"):
    assert bool(torch.isfinite(got[k]).all()) and bool(torch.isfinite(ref[k]).all()), k


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_pass_moments_agree_to_the_bit(case, device):
  L, M, d, B, nsmall, extra = case
  _, pm = _model(L, M, d, device)
  mu, S = _state(B, d, nsmall, seed=5200 + M + d)
  mu, S = to_dev(mu, device, F32), to_dev(S, device, F32)
  got = _match(pm, mu, S, extra)
  ref = _match(pm, mu, S, extra | OLD_WMOM)
  print("stats", ref["stats"], "groups", ref["groups"], "routed", ref["routed"])
  _assert_same(got, ref)


def test_mixed_draw_cubic_tiles_stop_inside_a_row_block(device):
  """L = 3, B = 80: every latent's GEMM has R = 160 rows in three row blocks.  50 batch elements collapse, so 100 rows per latent
  are collapsed: the first block holds collapsed rows only, the second both kinds (the cubic tiles stop inside it), the third,
  a partial one, none."""
  L, M, d, B, nsmall = 3, 300, 8, 80, 50
  syn, pm = _model(L, M, d, device)
  mu, S = _state(B, d, nsmall, seed=5300)
  # host: which (b, pair) items have a collapsed row group, hence the collapsed rows of every latent's GEMM
  bound = _group_bounds(syn, *f32_state(mu, S), pm.perm().cpu().numpy())          # [B, Po, 3]: shift, largest, smallest group
  assert np.all(bound[:, :, 0] < 0.5 * 256.0)                                     # every item recentred at the centroid
  has_group = bound[:, :, 2] <= 0.25
  margin = np.abs(bound[:, :, 1:] / 0.25 - 1.0).min()
  assert margin > 0.02, margin                                                    # no decision near the threshold (f32 round-up: 1e-6)
  rows = np.zeros(L, dtype=int)
  for po, (a, a2) in enumerate(combinations(range(L), 2)):
    rows[a] += has_group[:, po].sum()
    rows[a2] += has_group[:, po].sum()
  print("collapsed rows per latent (host)", rows, "of", (L - 1) * B)
  assert np.all(rows % 64 != 0) and np.all(rows > 64) and np.all(rows < (L - 1) * B - 32), rows
  mu, S = to_dev(mu, device, F32), to_dev(S, device, F32)
  got = _match(pm, mu, S, 0)
  ref = _match(pm, mu, S, OLD_WMOM)
  whole, total, _ = ref["stats"]
  partly = ref["groups"][0]
  print("collapsed in every row group", whole, "partly", partly, "of", total)
  assert total == B * 3
  ncoll = whole + partly                  # items the GEMM forms the cubic columns for: at least one collapsed row group
  assert 0 < ncoll < total, "the draw must hold collapsed and other items"
  assert ncoll == int(has_group.sum()) and whole == int((bound[:, :, 1] <= 0.25).sum()), (whole, partly, int(has_group.sum()))
  _assert_same(got, ref)


def _group_bounds(syn, mu, S, perm):
  """Host restatement of the collapse decision per (b, pair) (csrc/mm_mono.h; as tools/pack_order_study.py 4b): [B, Po, 3] =
  the recentring predicate's left side |G^T (mu - zbar)|^2 max|zc'|^2, and the largest and the smallest over the 64-row groups
  (packed order of the row latent) of max_i |A_i|^2 max_j |zc'_j|^2 -- a group is collapsed at <= 1/4."""
  Z, ls = syn.Z, syn.lengthscales
  M = Z.shape[0]
  zbar = Z.mean(0)
  zc = Z - zbar
  zm2 = float((zc * zc).sum(1).max())
  pairs = list(combinations(range(ls.shape[0]), 2))
  out = np.zeros((mu.shape[0], len(pairs), 3))
  for b in range(mu.shape[0]):
    for po, (a, a2) in enumerate(pairs):
      La, Lb = ls[a] ** 2, ls[a2] ** 2
      V = La * Lb / (La + Lb)
      T = V[:, None] * np.linalg.solve(S[b] + np.diag(V), S[b])
      T = 0.5 * (T + T.T)
      G = T / La[:, None] / Lb[None, :]
      t0 = G.T @ (mu[b] - zbar)
      an = ((zc @ G) ** 2).sum(1)[perm[a]]
      gm = np.array([an[g:g + 64].max() for g in range(0, M, 64)]) * zm2
      out[b, po] = float(t0 @ t0) * zm2, gm.max(), gm.min()
  return out


def _shifted_items(syn, mu, S):
  """Host predicate of the items that keep their rows centred at mu (k_pairvec_reg, MM_RECENTRE_CMAX; as tools/pack_order_study.py
  4b): |G^T (mu - zbar)|^2 max_j |zc'_j|^2 > 256.  -> the predicate's left side per (b, pair)."""
  Z, ls = syn.Z, syn.lengthscales
  zbar = Z.mean(0)
  zc = Z - zbar
  zm2 = float((zc * zc).sum(1).max())
  out = []
  for b in range(mu.shape[0]):
    for (a, a2) in combinations(range(ls.shape[0]), 2):
      La, Lb = ls[a] ** 2, ls[a2] ** 2
      V = La * Lb / (La + Lb)
      T = V[:, None] * np.linalg.solve(S[b] + np.diag(V), S[b])
      T = 0.5 * (T + T.T)
      G = T / La[:, None] / Lb[None, :]
      t0 = G.T @ (mu[b] - zbar)
      out.append(float(t0 @ t0) * zm2)
  return np.array(out)


def test_items_on_the_binomial_shift_path(device):
  """mu ten units outside the unit cube of the inducing points for half of the batch: those items keep their rows centred at mu
  and the contraction shifts the row moments by dmu = mu - zbar."""
  L, M, d, B = 3, 300, 8, 16
  syn, pm = _model(L, M, d, device)
  mu, S = _state(B, d, 6, seed=5400)
  mu[::2] += 10.0
  mu64, S64 = f32_state(mu, S)
  lhs = _shifted_items(syn, mu64, S64)
  print("shift predicate: min %.3g max %.3g, items over 256: %d of %d" % (lhs.min(), lhs.max(), (lhs > 256.0).sum(), lhs.size))
  assert (lhs > 2 * 256.0).sum() >= 1 and (lhs < 0.5 * 256.0).sum() >= 1, "the draw must hold shifted and recentred items"
  mu, S = to_dev(mu, device, F32), to_dev(S, device, F32)
  got = _match(pm, mu, S, 0)
  ref = _match(pm, mu, S, OLD_WMOM)
  _assert_same(got, ref)
