"""The XCD map of the forward's diagonal f64 sweep: k_qred_f64_mfma deals the consecutive tiles of every (latent, batch chunk) over
the eight XCDs (work item = block index) -- against the contiguous range per XCD it replaces, forced on the same build by
MM_ISTAGE_OLD_DIAG_MAP.  Only the decode from block index to work item differs: every slab slot is written by the same code on the
same operands, so f1, Sff and cross must agree to the bit.  Between the two runs compared the same workspace is run once on OTHER
states: a work item the new decode never reaches would otherwise pass on what the run before left.  The backward's k_bwd_diag
keeps its contiguous map: there, as in the one-launch sweep of a small f64 model, the bit must change nothing."""
import pytest
import torch

from gpflowpilco_amd import _lib, ops
from gpflowpilco_amd.synthetic import make_inputs, make_svgp
from tests.helpers import to_dev

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
OLD = 1 << 25                        # MM_ISTAGE_OLD_DIAG_MAP (csrc/mm_common.h)
WORST = _lib.MM_FORCE_WORST_TIER


@pytest.fixture(scope="module")
def device():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _pm(L, M, d, seed, device, dtype=F32):
  syn = make_svgp(L, M, d, seed=seed, device=str(device), ls_bounds=(0.3, 3.0), stable=False)
  return syn.to_model(device).packed(dtype, True, device)


def _states(B, d, seed, device, dtype=F32):
  mu, S = make_inputs(B, d, seed=seed, scale=0.1, lo=0.0, hi=1.0)
  return to_dev(mu, device, dtype), to_dev(S, device, dtype)


def _fwd(pm, mu, S, extra):
  pm.status().zero_()
  out = tuple(t.clone() for t in ops.moment_match(pm, mu, S, extra_flags=extra))
  pm.check_status(mu.shape[0])
  return out


def _same_forward(pm, mu, S, extra=0):
  old = _fwd(pm, mu, S, extra | OLD)
  other = _fwd(pm, mu * 0.8 + 0.05, S * 2.0, extra | OLD)          # (the slab now holds another state's sums)
  new = _fwd(pm, mu, S, extra)
  assert not torch.equal(other[1], old[1])
  for n, o in zip(new, old):
    assert torch.isfinite(n).all() and torch.equal(n, o)
  return new


@pytest.mark.parametrize("d", [3, 8])
def test_nwork_no_multiple_of_8_two_uneven_chunks(d, device):
  """L = 3, M = 130 (Mp 256: 10 tile pairs), B = 33: two chunks of 17 and 16, nwork = 60; d = 3 / 8: one / two K = 4 steps."""
  pm = _pm(3, 130, d, 2500 + d, device)
  mu, S = _states(33, d, 2600 + d, device)
  _same_forward(pm, mu, S)


def test_fewer_work_items_than_xcds(device):
  pm = _pm(1, 64, 4, 2511, device)
  mu, S = _states(1, 4, 2611, device)
  old = _fwd(pm, mu, S, OLD)
  _fwd(pm, mu * 0.8 + 0.05, S * 2.0, OLD)
  for n, o in zip(_fwd(pm, mu, S, 0), old):
    assert torch.equal(n, o)


def test_nwork_a_multiple_of_8(device):
  pm = _pm(8, 200, 8, 2512, device)
  mu, S = _states(40, 8, 2612, device)
  _same_forward(pm, mu, S)


def test_forced_worst_tier(device):
  pm = _pm(3, 130, 8, 2513, device)
  mu, S = _states(33, 8, 2613, device)
  _same_forward(pm, mu, S, WORST)


def test_f64_model_one_launch_for_both_kinds_of_pairs(device):
  """L = 2, M = 100, B = 5: k_qred_f64_both keeps its map -- the flag changes nothing."""
  pm = _pm(2, 100, 5, 2514, device, F64)
  mu, S = _states(5, 5, 2614, device, F64)
  _same_forward(pm, mu, S)


def test_f64_model_two_launches(device):
  """L = 4, M = 1000, B = 32: the diagonal launch deals, the off-diagonal one keeps the contiguous ranges."""
  pm = _pm(4, 1000, 6, 2515, device, F64)
  mu, S = _states(32, 6, 2615, device, F64)
  _same_forward(pm, mu, S)


def _grads(pm, mu, S, g, extra):
  pm.status().zero_()
  out = tuple(t.clone() for t in ops.moment_match_backward(pm, mu, S, *g, stages=extra))
  pm.check_status(mu.shape[0])
  return out


@pytest.mark.parametrize("L,M,B,dtype", [(3, 130, 5, F32), (8, 200, 3, F32), (3, 130, 5, F64)])
def test_backward_keeps_its_map(L, M, B, dtype, device):
  """k_bwd_diag (12 column strips of 3 latents; 32 of 8; the Taylor tiers of an f64 pack) keeps one contiguous range of work items per
  XCD: the gradients with and without the bit are the same launches, and must be the same bits."""
  d = 8
  pm = _pm(L, M, d, 2520 + L, device, dtype)
  mu, S = _states(B, d, 2620 + L, device, dtype)
  gen = torch.Generator(device="cpu").manual_seed(2720 + L)
  g = tuple(torch.randn(s, generator=gen, dtype=F64).to(device) for s in ((B, L), (B, L, L), (B, d, L)))
  old = _grads(pm, mu, S, g, OLD)
  other = _grads(pm, mu * 0.8 + 0.05, S * 2.0, g, OLD)
  new = _grads(pm, mu, S, g, 0)
  assert not torch.equal(other[0], old[0])
  for n, o in zip(new, old):
    assert torch.isfinite(n).all() and torch.equal(n, o)


def test_graph_replayed_twice(device):
  L, d, B = 6, 8, 48
  pm = _pm(L, 1000, d, 2531, device)
  mu, S = _states(B, d, 2631, device)
  want = _fwd(pm, mu, S, OLD)
  want2 = _fwd(pm, mu * 0.9, S * 1.5, OLD)
  ms, Ss = mu.clone(), S.clone()
  side = torch.cuda.Stream(device)
  side.wait_stream(torch.cuda.current_stream(device))
  with torch.cuda.stream(side):
    for _ in range(2):
      ops.moment_match(pm, ms, Ss)
  torch.cuda.current_stream(device).wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = ops.moment_match(pm, ms, Ss)
  for m_, S_, w in ((mu * 0.9, S * 1.5, want2), (mu, S, want)):
    ms.copy_(m_); Ss.copy_(S_)
    graph.replay()
    torch.cuda.synchronize()
    for n, o in zip(out, w):
      assert torch.equal(n, o)
