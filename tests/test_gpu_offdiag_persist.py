"""The persistent off-diagonal f32 sweep (csrc/mm_mfma.hip: k_offdiag_worklist + k_qred_f32_mfma_persist, taken where d <= 8 and
Mp <= 2048) against the per-(b, pair) grid it replaces (k_qred_f32_mfma, forced on the same build by MM_ISTAGE_OLD_OFFDIAG): both
run the same per-wave code and sum the panels in the same order, so Sff, the routed counts, mm_offdiag_stats and mm_route_estimates
must agree to the bit -- over d, M (the LDS limit and past it), L, B, both recipes, the forced worst tier, graph replay, two caller
streams and a workspace reused across regimes."""
import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, ops
from gpflowpilco_amd.synthetic import make_inputs, make_svgp
from tests.helpers import to_dev

pytestmark = pytest.mark.gpu
F32 = torch.float32
OLD = 1 << 23                        # MM_ISTAGE_OLD_OFFDIAG (csrc/mm_common.h)
WORST = _lib.MM_FORCE_WORST_TIER
RECIPE = {"baseline": dict(ls_bounds=(0.3, 3.0), stable=False), "pilco": dict(ls_bounds=(0.7, 3.0), stable=True)}


@pytest.fixture(scope="module")
def device():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


# (_pm and _states also make the inputs of tests/test_gpu_offdiag_slot_golden.py, whose fixture is compared to the bit: a change of
# their seeds, recipes or spread means recording tests/golden/offdiag_slot_parent.npz again)
def _pm(L, M, d, seed, recipe, device):
  syn = make_svgp(L, M, d, seed=seed, device=str(device), **RECIPE[recipe])
  return syn.to_model(device).packed(F32, True, device)


def _states(B, d, seed, device, spread=(1e-2, 30.0)):
  """Covariance scales spread over three decades: items from wholly inside the collapsed range to dense ones."""
  mu, S = make_inputs(B, d, seed=seed, scale=0.1, lo=0.0, hi=1.0)
  S = S * np.geomspace(spread[0], spread[1], B)[:, None, None] if B > 1 else S
  return to_dev(mu, device, F32), to_dev(S, device, F32)


def _match(pm, mu, S, extra):
  B = mu.shape[0]
  flags = ops.make_flags(True, True) | extra
  pm.status().zero_()
  Sff = ops.moment_match(pm, mu, S, extra_flags=extra)[1].clone()
  stats = (ops.offdiag_stats(pm, B, flags), ops.offdiag_row_groups(pm, B, flags), ops.offdiag_routed(pm, B, flags))
  return Sff, pm.routed()[0], stats, ops.route_estimates(pm, B, flags)


def _same(pm, mu, S, extra=0):
  new, old = _match(pm, mu, S, extra), _match(pm, mu, S, extra | OLD)
  assert torch.equal(new[0], old[0])
  assert new[1] == old[1] and new[2] == old[2], (new[1:3], old[1:3])
  assert torch.equal(new[3], old[3])
  return new


@pytest.mark.parametrize("d", range(1, 9))
def test_every_d_identity_pack(d, device):
  pm = _pm(2, 200, d, 300 + d, "baseline", device)
  mu, S = _states(5, d, 400 + d, device)
  _same(pm, mu, S)


@pytest.mark.parametrize("M", [40, 1000, 2000, 2048, 2100])
def test_every_M_to_the_lds_limit_and_past_it(M, device):
  """M = 2100: Mp = 2176 exceeds the LDS image -- both flags take the old sweep."""
  pm = _pm(3, M, 8, 500 + M, "baseline", device)
  mu, S = _states(7, 8, 600 + M, device)
  _same(pm, mu, S)


def test_single_batch_element(device):
  pm = _pm(3, 1000, 6, 701, "baseline", device)
  mu, S = _states(1, 6, 702, device)
  _same(pm, mu, S)


@pytest.mark.parametrize("recipe", ["baseline", "pilco"])
def test_c3_shape_every_item_class(recipe, device):
  """L = 8, M = 2000, d = 8, B = 256 (bench.py's C3): items wholly inside, screened, partly collapsed, dense and routed."""
  B = 256
  pm = _pm(8, 2000, 8, 1002, recipe, device)
  mu, S = _states(B, 8, 3002, device, spread=(1e-2, 30.0) if recipe == "baseline" else (1e-2, 3.0))
  Sff, routed, stats, _ = _same(pm, mu, S)
  (coll, total, inside), (partly, gcoll, ngroups), _ = stats
  assert total == B * 28, stats
  if recipe == "baseline":                                      # (the pilco recipe's items are wholly inside at these states)
    assert 0 < inside < coll < total and partly > 0 and gcoll < ngroups, stats
    assert routed > 0, "no item was routed: widen the spread"


def test_forced_worst_tier(device):
  """The forced worst tier stays on k_qred_f32_mfma (every group dense: the persistent sweep measured slower there); the flag changes
  nothing."""
  pm = _pm(4, 1000, 8, 801, "pilco", device)
  mu, S = _states(9, 8, 802, device)
  _same(pm, mu, S, WORST)


def test_workspace_reused_from_pilco_states_to_baseline_states(device):
  """Narrow states (every item inside: an empty list) then wide ones on the same workspace: the list and its counters are reset."""
  pm = _pm(4, 1000, 8, 901, "baseline", device)
  mu, S = _states(16, 8, 902, device)
  narrow = _match(pm, mu, S * 1e-4, 0)
  assert narrow[2][0][2] == narrow[2][0][1], narrow[2]           # (all wholly inside)
  wide_after = _match(pm, mu, S, 0)
  wide_old = _match(pm, mu, S, OLD)
  assert torch.equal(wide_after[0], wide_old[0]) and torch.equal(wide_after[3], wide_old[3])
  assert wide_after[1:3] == wide_old[1:3]
  assert torch.equal(_match(pm, mu, S * 1e-4, 0)[0], narrow[0])


def test_graph_replayed_twice(device):
  L, d, B = 6, 8, 48                                             # P B = 1008: the q stage forks onto the side stream
  pm = _pm(L, 1000, d, 1101, "baseline", device)
  mu, S = _states(B, d, 1102, device)
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


def test_two_caller_streams(device):
  runs = []
  for seed, B in ((1201, 32), (1207, 40)):
    pm = _pm(6, 1000, 8, seed, "baseline", device)
    mu, S = _states(B, 8, seed + 1, device)
    runs.append((pm, mu, S, _match(pm, mu, S, OLD)[0]))
  sa, sb = torch.cuda.Stream(device), torch.cuda.Stream(device)
  cur = torch.cuda.current_stream(device)
  sa.wait_stream(cur); sb.wait_stream(cur)
  outs = [[], []]
  for _ in range(4):
    for k, st in enumerate((sa, sb)):
      pm, mu, S, _ = runs[k]
      with torch.cuda.stream(st):
        outs[k].append(ops.moment_match(pm, mu, S)[1])
  torch.cuda.synchronize()
  for k in range(2):
    for o in outs[k]:
      assert torch.equal(o, runs[k][3])
