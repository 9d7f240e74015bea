"""The d = 8 form of the degree-4..6 contraction (csrc/mm_moments6.hip: mm6_step8 in k_spoly56<true> / k_spoly4<true>: every size a
compile-time constant) against the generic steps it replaces at d = 8 (mm6_step, forced on the same build by
MM_ISTAGE_OLD_SPOLY56): every stored value and every sum keeps its operation order, so s56 and estS -- and with them Sff, the
route estimates, the routed counts and mm_offdiag_stats -- must agree to the bit: over every collapse class (the degree-4 items
of k_spoly4, degree <= 5, degree 6), more items than workgroups of the persistent grid, d != 8 (the flag changes nothing) and a
graph replay."""
import numpy as np
import pytest
import torch

from gpflowpilco_amd import ops
from gpflowpilco_amd.synthetic import make_inputs, make_svgp
from tests.helpers import f32_state, oracle_params, to_dev
from tests.test_gpu_route_estimate import CLASS_X, _cls, _item_geometry, _scaled_for, ls_for

pytestmark = pytest.mark.gpu
F32 = torch.float32
OLD = 1 << 24                        # MM_ISTAGE_OLD_SPOLY56 (csrc/mm_common.h)


@pytest.fixture(scope="module")
def device():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _states(B, d, seed, device, spread=(1e-2, 30.0)):
  """Covariance scales spread over three decades: items from the degree-4 class to dense ones."""
  mu, S = make_inputs(B, d, seed=seed, scale=0.1, lo=0.0, hi=1.0)
  S = S * np.geomspace(spread[0], spread[1], B)[:, None, None]
  return to_dev(mu, device, F32), to_dev(S, device, F32)


def _match(pm, mu, S, extra):
  B = mu.shape[0]
  flags = ops.make_flags(True, True) | extra
  pm.status().zero_()
  Sff = ops.moment_match(pm, mu, S, extra_flags=extra)[1].clone()
  stats = (ops.offdiag_stats(pm, B, flags), ops.offdiag_row_groups(pm, B, flags), ops.offdiag_routed(pm, B, flags))
  return Sff, pm.routed()[0], stats, ops.route_estimates(pm, B, flags).clone()


def _same(pm, mu, S):
  new, old = _match(pm, mu, S, 0), _match(pm, mu, S, OLD)
  assert torch.equal(new[0], old[0])
  assert torch.equal(new[3], old[3])                              # (est carries estS)
  assert new[1] == old[1] and new[2] == old[2], (new[1:3], old[1:3])
  assert torch.isfinite(new[0]).all()
  return new


def test_every_collapse_class(device):
  """d = 8, L = 3, M = 320, one batch element per class of item (0, 1): degree 4 only (k_spoly4), degree <= 5, degree 6 inside,
  screened, partly collapsed, none."""
  d, L, M = 8, 3, 320
  syn = make_svgp(L, M, d, seed=700 + d, ls_bounds=ls_for(d), stable=False)
  p = oracle_params(syn)
  mu0, S0 = make_inputs(len(CLASS_X), d, seed=900 + d, scale=0.1, lo=0.35, hi=0.65)
  S = np.stack([_scaled_for(p, mu0[k], S0[k], 0, 1, X) * S0[k] for k, (_, X) in enumerate(CLASS_X)])
  mu, S = f32_state(mu0, S)
  pm = syn.to_model(device).packed(F32, True, device)
  perm = pm.perm().cpu().numpy()
  for k, (cls, _) in enumerate(CLASS_X):
    assert _cls(_item_geometry(p, mu[k], S[k], 0, 1, perm)) == cls, (k, cls)
  new = _same(pm, to_dev(mu, device, F32), to_dev(S, device, F32))
  (coll, total, inside), (partly, _, _), _ = new[2]
  assert total == len(CLASS_X) * 3 and coll >= 4 and inside >= 3 and partly >= 1, new[2]
  assert float(new[3][:4, 0, 0].min()) > 0.0                     # the wholly collapsed items carry estS


def _many_items(device):
  pm = make_svgp(3, 192, 8, seed=1310, device=str(device), ls_bounds=(0.3, 3.0), stable=False).to_model(device).packed(F32, True, device)
  return pm, _states(100, 8, 1311, device)


def test_more_items_than_workgroups(device):
  """d = 8, L = 3, M = 192, B = 100: 300 items, the workgroups of the persistent grids loop over items and reuse their LDS image."""
  pm, (mu, S) = _many_items(device)
  new = _same(pm, mu, S)
  (coll, total, inside), _, _ = new[2]
  assert total == 300 and 0 < inside <= coll < total, new[2]


@pytest.mark.parametrize("d", [5, 7])
def test_other_d_takes_the_generic_steps(d, device):
  pm = make_svgp(2, 200, d, seed=1320 + d, device=str(device), ls_bounds=(0.3, 3.0), stable=False).to_model(device).packed(F32, True, device)
  mu, S = _states(5, d, 1330 + d, device)
  new = _same(pm, mu, S)
  assert new[2][0][0] > 0, new[2]                                 # (some item is collapsed: the contraction ran)


def test_graph_replayed_twice(device):
  pm, (mu, S) = _many_items(device)
  want = _match(pm, mu, S, OLD)[0]
  want2 = _match(pm, mu * 0.9, S * 1.5, OLD)[0]
  ms, Ss = mu.clone(), S.clone()
  side = torch.cuda.Stream(device)
  side.wait_stream(torch.cuda.current_stream(device))
  with torch.cuda.stream(side):
    for _ in range(2):
      ops.moment_match(pm, ms, Ss)
  torch.cuda.current_stream(device).wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = ops.moment_match(pm, ms, Ss)[1]
  ms.copy_(mu * 0.9); Ss.copy_(S * 1.5)
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(out, want2)
  ms.copy_(mu); Ss.copy_(S)
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(out, want)
