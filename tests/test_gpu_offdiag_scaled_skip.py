"""Bound-based tile skipping of the f32 off-diagonal sweep (csrc/mm_mfma.hip: ct_first / ct_end, wave_inside, the need loops,
k_offdiag_worklist).  A collapsed 64-row group skips the column tiles that a Cauchy-Schwarz bound puts inside the collapsed range;
by default the bound is taken in the metric scaled by the column latent's lengthscales, |A_i . zc'_j| <= |A_i o l'| |zc'_j / l'|
(gmax2s from k_pairvec_reg x zt2s from the pack), MM_ISTAGE_OLD_SKIP_BOUND takes the Euclidean one at every site and
MM_ISTAGE_NO_BOUND_SKIP sends every tile of a collapsed group through the screening product.  A skipped tile is one the screening
would have left without adding anything, so

  * the three modes agree to the bit -- Sff, the per-item error estimates, the routed counts, mm_offdiag_stats -- on both sweeps
    (the persistent one and, under MM_ISTAGE_OLD_OFFDIAG, the per-(b, pair) grid);
  * the scaled bound lists no more items for the persistent sweep than the Euclidean one, and fewer where the metrics differ;
  * the two arrays are what a float64 restatement on the host says, rounded up.

Models: make_svgp(..., ls_bounds=(0.3, 3.0)) -- lengthscales over a decade, so that the two metrics differ."""
from itertools import combinations

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, ops
from gpflowpilco_amd.synthetic import make_inputs, make_svgp
from tests.helpers import f32_state, to_dev

pytestmark = pytest.mark.gpu
F32 = torch.float32
OLD_SWEEP = 1 << 23                   # MM_ISTAGE_OLD_OFFDIAG (csrc/mm_common.h)
OLD_BOUND = _lib.MM_ISTAGE_OLD_SKIP_BOUND
NO_SKIP = _lib.MM_ISTAGE_NO_BOUND_SKIP
# (L, M, d, B): Mp = 384, 6 row groups, 12 column tiles | d < 8, Mp = 256 with padded rows and a trailing tile of padding alone,
# pack in the caller's order (M <= 256) | a row group straddling M (Mp = 640)
SHAPES = [(3, 300, 8, 4), (3, 200, 5, 3), (4, 520, 8, 2)]
STDS = [0.1, 0.03]
ROUND_UP = 1.000001                   # both arrays: x 1.000001, cast to f32 (k_pack_vectors, k_pairvec_reg)
# the restatement's own f64 evaluation of G (a solve against Sigma + V) differs from the kernel's in the last digits
HOST_EPS = 1e-9


@pytest.fixture(scope="module")
def device():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


_cache = {}


def _model(shape, device):
  """(synthetic model, f32 pack) of a shape, built once per module."""
  if shape not in _cache:
    L, M, d, _ = shape
    syn = make_svgp(L, M, d, seed=4100 + M + d, device=str(device), ls_bounds=(0.3, 3.0), stable=False)
    _cache[shape] = (syn, syn.to_model(device).packed(F32, True, device))
  return _cache[shape]


def _state(shape, std):
  _, M, d, B = shape
  return make_inputs(B, d, seed=4200 + M + int(1000 * std), scale=std, lo=0.0, hi=1.0)


def _match(pm, mu, S, extra):
  B = mu.shape[0]
  flags = ops.make_flags(True, True) | extra
  pm.status().zero_()
  Sff = ops.moment_match(pm, mu, S, extra_flags=extra)[1].clone()
  return dict(Sff=Sff, est=ops.route_estimates(pm, B, flags), routed=ops.offdiag_routed(pm, B, flags),
              stats=ops.offdiag_stats(pm, B, flags), groups=ops.offdiag_row_groups(pm, B, flags),
              listed=ops.offdiag_worklist_len(pm, B, flags))


@pytest.mark.parametrize("sweep", [0, OLD_SWEEP], ids=["persistent", "grid"])
@pytest.mark.parametrize("std", STDS + [0.2])     # (0.2: items with collapsed and dense row groups side by side)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "L%d-M%d-d%d-B%d" % s)
def test_three_skip_modes_agree_to_the_bit(shape, std, sweep, device):
  _, pm = _model(shape, device)
  mu, S = _state(shape, std)
  mu, S = to_dev(mu, device, F32), to_dev(S, device, F32)
  ref = _match(pm, mu, S, sweep)
  partly, gcoll, ngroups = ref["groups"]
  assert gcoll > 0, ("no collapsed row group: the comparison would be vacuous", ref["groups"], ref["stats"])
  for mode in (OLD_BOUND, NO_SKIP):
    got = _match(pm, mu, S, sweep | mode)
    assert torch.equal(got["Sff"], ref["Sff"]), mode
    assert torch.equal(got["est"], ref["est"]), mode
    assert got["routed"] == ref["routed"] and got["stats"] == ref["stats"] and got["groups"] == ref["groups"], (mode, got, ref)


def test_scaled_bound_lists_fewer_items(device):
  """The persistent sweep's work list: the scaled bound lists a subset of what the Euclidean one lists (an item is listed when a
  group of its has a tile to visit), strictly fewer for at least one of the two state widths; with no bound-based skipping every
  item with a collapsed group is listed."""
  shape = SHAPES[0]
  _, pm = _model(shape, device)
  drops = []
  for std in STDS:
    mu, S = _state(shape, std)
    mu, S = to_dev(mu, device, F32), to_dev(S, device, F32)
    new, old, all_ = (_match(pm, mu, S, m)["listed"] for m in (0, OLD_BOUND, NO_SKIP))
    print(f"std {std}: listed items scaled {new}, Euclidean {old}, no bound skip {all_}")
    assert new <= old <= all_, (std, new, old, all_)
    drops.append(old - new)
  assert max(drops) > 0, drops


# ---- host restatement of the two arrays ----------------------------------------------------------------------------------------

def _G(S, la, lb):
  """b_ij = zc_i^T G zc'_j: the cross term of the pair's exponent, Lambda's as vectors (as tests/test_gpu_route_estimate.py)."""
  V = la * lb / (la + lb)
  T = V[:, None] * np.linalg.solve(S + np.diag(V), S)
  T = 0.5 * (T + T.T)
  return T / la[:, None] / lb[None, :]


def host_zt2s(Z, ls, perm, Mp):
  """[L, Mp/32]: per 32-point tile of the packed order max_m sum_k (z_mk - zbar_k)^2 / l_k^2 over the tile's real points."""
  L, d = ls.shape
  M = Z.shape[0]
  out = np.zeros((L, Mp // 32))
  zc = Z - Z.mean(0)
  for a in range(L):
    key = ((zc / ls[a]) ** 2).sum(1)[perm[a]]
    for t in range((M + 31) // 32):
      out[a, t] = key[32 * t:32 * (t + 1)].max()
  return out


def host_gmax2s(Z, ls, perm, Mp, mu, S, zmax2):
  """[B, Po, Mp/64]: per 64-row group of the packed order max_i |A_i o l_a'|^2, A_i = G^T (z_i - zbar) (rows recentred at the
  centroid; G^T (z_i - mu) where k_pairvec_reg keeps them at mu: MM_RECENTRE_CMAX)."""
  L, d = ls.shape
  M = Z.shape[0]
  pairs = list(combinations(range(L), 2))
  out = np.zeros((mu.shape[0], len(pairs), Mp // 64))
  zbar = Z.mean(0)
  for b in range(mu.shape[0]):
    for po, (a, a2) in enumerate(pairs):
      G = _G(S[b], ls[a] ** 2, ls[a2] ** 2)
      t0 = G.T @ (mu[b] - zbar)
      recentred = float(t0 @ t0) * zmax2 <= 16.0 ** 2
      A = ((Z - zbar) if recentred else (Z - mu[b])) @ G
      n2 = ((A * ls[a2]) ** 2).sum(1)[perm[a]]
      for g in range((M + 63) // 64):
        out[b, po, g] = n2[64 * g:64 * (g + 1)].max()
  return out


def _rounded_up(got, exact, host_eps):
  """got is the f32 round-up of exact: never below it, and within x 1.000001 and two f32 roundings (the cast, and for gmax2s the
  f32 product with 1.000001f) of it."""
  got = got.astype(np.float64)
  assert got.shape == exact.shape
  assert np.all(got >= exact), float((got / np.maximum(exact, 1e-300)).min())
  assert np.all(got <= exact * ROUND_UP * (1.0 + 2.0 ** -23) * (1.0 + host_eps)), float((got / np.maximum(exact, 1e-300)).max())


@pytest.mark.parametrize("std", STDS)
def test_arrays_against_host_restatement(std, device):
  shape = SHAPES[0]
  L, M, d, B = shape
  syn, pm = _model(shape, device)
  mu, S = _state(shape, std)
  _match(pm, to_dev(mu, device, F32), to_dev(S, device, F32), 0)
  zt2s, gmax2s = ops.offdiag_skip_bounds(pm, B, ops.make_flags(True, True))
  Mp = zt2s.shape[1] * 32
  perm = pm.perm().cpu().numpy()
  want_z = host_zt2s(syn.Z, syn.lengthscales, perm, Mp)
  _rounded_up(zt2s.cpu().numpy(), want_z, 0.0)
  assert np.all(zt2s.cpu().numpy()[:, (M + 31) // 32:] == 0.0)        # tiles of padding alone
  mu64, S64 = f32_state(mu, S)
  zc = syn.Z - syn.Z.mean(0)
  want_g = host_gmax2s(syn.Z, syn.lengthscales, perm, Mp, mu64, S64, float((zc * zc).sum(1).max()))
  _rounded_up(gmax2s.cpu().numpy(), want_g, HOST_EPS)
  assert np.all(gmax2s.cpu().numpy()[:, :, (M + 63) // 64:] == 0.0)   # row groups of padding alone
