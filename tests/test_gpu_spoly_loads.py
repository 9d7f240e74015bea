"""Where the degree-4..6 contraction loads from (csrc/mm_moments6.hip: k_spoly56, k_spoly4): by default an item's prologue issues
all its loads -- the f32 moments, the element of G, the group flags and the weights of estS -- and waits once, and every barrier
phase's first step takes its tables from a request made before the barrier in front of it; MM_ISTAGE_OLD_SPOLY_LOADS selects, on
the same build, the loops of load / wait / use they replace.  The arithmetic and every order of summation are the same, so

  * s56, estS and s12 in the workspace, f1, Sff and cross, the per-item route estimates, the routed count, mm_offdiag_stats and
    the row-group counts agree TO THE BIT;
  * this holds for d = 8 (mm6_step8) at Mp = 384 (768 threads: the estS sums have threads with no and with one element) and at
    Mp = 1024 (a second element for part of them), for d = 5 (the generic mm6_step), and with MM_FORCE_WORST_TIER (nothing is
    collapsed: no contraction runs, k_item_classes writes the zeros).

Both paths write into the same cached workspace and nothing clears it between calls, so a value the new path left out would still
hold the other run's bit-identical one.  Every pass therefore starts from a workspace filled with 0xFF bytes (all-ones doubles and
floats are NaN; the kernels reset their own counters and lists), and the new path runs first.

The draws are built on the host, as in tests/test_gpu_route_estimate.py: one batch element per collapse class of item (0, 1) --
degree 4 only (k_spoly4), degrees 4-5, degree 6 (wholly inside, and with screened tiles), collapsed in some 64-row groups only
(mixed group flags: the select of the estS sums), no collapsed group (zeros from k_item_classes).  The class counts of the whole
batch are asserted against the kernel's own work lists, so no class can be empty without the test failing."""
import ctypes
import gc
import os

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, ops
from gpflowpilco_amd.synthetic import make_inputs, make_svgp
from tests.helpers import f32_state, oracle_params, to_dev
from tests.test_gpu_route_estimate import X4_2, X5_2, _item_geometry, _cls, _pairs, _scaled_for, ls_for

pytestmark = pytest.mark.gpu
F32 = torch.float32
OLD = _lib.MM_ISTAGE_OLD_SPOLY_LOADS
WORST = _lib.MM_FORCE_WORST_TIER
# bound X of item (0, 1) per batch element -> its class; "partly" is searched for (see _draw)
DRAW = (("deg4", 0.6 / 40.0), ("deg5", 0.044), ("inside", 0.18), ("screened", 0.4), ("partly", None), ("none", 6.0),
        ("deg5", 0.055), ("inside", 0.12))
# (L, M, d, extra flags)
CASES = [(3, 300, 8, 0), (3, 1000, 8, 0), (3, 200, 5, 0), (3, 300, 8, WORST)]
IDS = ["d8-Mp384", "d8-Mp1024", "d5-generic", "d8-worst-tier"]


@pytest.fixture(scope="module")
def device():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _release_module_state():
  """The packs and workspaces of this module (the M = 1000 one is 0.2 GB) go when its tests are done: nothing of it -- cached
  tensors, or garbage a later collection would free in the middle of another module's test -- is left on the device."""
  yield
  _cache.clear()
  gc.collect()
  if torch.cuda.is_available():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


_layout = None


def _offsets(pm, B, flags):
  """Byte offsets of s12, s56, estS and ilist in the workspace, Po (tests/hostcheck/mm_ws_layout_host.cpp)."""
  global _layout
  if _layout is None:
    _layout = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "libmm_ws_layout_host.so"))
    _layout.mm_test_ws_offsets.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_ulonglong)]
  out = (ctypes.c_ulonglong * 6)()
  assert _layout.mm_test_ws_offsets(B, pm.L, pm.M, pm.d, _lib.MM_F32, flags, out) == 0
  return [int(v) for v in out]


_cache = {}


def _case(L, M, d, device):
  """(host parameters, f32 pack, mu, S, host class of every item) of a shape, built once per module."""
  key = (L, M, d)
  if key not in _cache:
    syn = make_svgp(L, M, d, seed=700 + d, ls_bounds=ls_for(d), stable=False)
    p = oracle_params(syn)
    pm = syn.to_model(device).packed(F32, True, device)
    perm = pm.perm().cpu().numpy()
    mu0, S0 = make_inputs(len(DRAW), d, seed=900 + d, scale=0.1, lo=0.35, hi=0.65)
    S = []
    for k, (cls, X) in enumerate(DRAW):
      if X is not None:
        S.append(_scaled_for(p, mu0[k], S0[k], 0, 1, X) * S0[k])
        continue
      # some row groups collapsed, others not: the first bound beyond 1/2 at which the host says so, away from every threshold
      for X in np.geomspace(0.52, 3.0, 40):
        Sk = _scaled_for(p, mu0[k], S0[k], 0, 1, X) * S0[k]
        g = _item_geometry(p, *(v[0] for v in f32_state(mu0[k:k + 1], Sk[None])), 0, 1, perm)
        if _cls(g) == "partly" and g["gmargin"] > 1e-3:
          break
      else:
        raise AssertionError("no partly collapsed draw for item (0, 1)")
      S.append(Sk)
    mu, S = f32_state(mu0, np.stack(S))
    items = {(b, po): _item_geometry(p, mu[b], S[b], a, a2, perm) for b in range(len(DRAW)) for po, (a, a2) in enumerate(_pairs(L))}
    _cache[key] = (pm, to_dev(mu, device, F32), to_dev(S, device, F32), items)
  return _cache[key]


def _match(pm, mu, S, extra):
  B = mu.shape[0]
  flags = ops.make_flags(True, True) | extra
  pm.status().zero_()
  ws = pm.workspace(B, flags, peek=True)
  ws.fill_(0xFF)                                             # whatever this pass does not write reads as NaN
  f1, Sff, cross = (t.clone() for t in ops.moment_match(pm, mu, S, extra_flags=extra))
  torch.cuda.synchronize()
  o_s12, o_s56, o_estS, o_ilist, Po, total = _offsets(pm, B, flags)
  assert total == ws.numel() and Po == pm.L * (pm.L - 1) // 2
  n = B * Po
  return dict(f1=f1, Sff=Sff, cross=cross,
              s12=ws[o_s12:o_s12 + 8 * n].view(torch.float64).clone(), s56=ws[o_s56:o_s56 + 8 * n].view(torch.float64).clone(),
              estS=ws[o_estS:o_estS + 4 * n].view(torch.float32).clone(), lists=ws[o_ilist:o_ilist + 16].view(torch.int32).tolist(),
              est=ops.route_estimates(pm, B, flags), routed=ops.offdiag_routed(pm, B, flags), stats=ops.offdiag_stats(pm, B, flags),
              groups=ops.offdiag_row_groups(pm, B, flags))


TENSORS = ("s56", "estS", "s12", "f1", "Sff", "cross", "est")


def _assert_same(got, ref):
  for k in TENSORS:
    assert bool(torch.isfinite(got[k]).all()) and bool(torch.isfinite(ref[k]).all()), k
    assert torch.equal(got[k], ref[k]), (k, float((got[k].double() - ref[k].double()).abs().max()))
  for k in ("routed", "stats", "groups", "lists"):
    assert got[k] == ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_load_placement_changes_no_bit(case, device):
  L, M, d, extra = case
  pm, mu, S, items = _case(L, M, d, device)
  # host: the class of every item of the batch
  for k, (cls, _) in enumerate(DRAW):
    assert _cls(items[k, 0]) == cls, (k, cls, _cls(items[k, 0]), items[k, 0]["X"])
  assert min(g["gmargin"] for g in items.values()) > 1e-4                   # no group's bound sits on 1/2
  coll = [g for g in items.values() if g["ncoll"] > 0]                      # items the contraction runs for
  margin = min(abs(g["Xc2"] / t - 1.0) for g in coll for t in (X4_2, X5_2))
  assert margin > 1e-4, margin                                             # no collapse degree sits on its bound (f32 round-up: 1e-6)
  n4 = sum(g["Xc2"] <= X4_2 for g in coll)
  n5 = sum(X4_2 < g["Xc2"] <= X5_2 for g in coll)
  n6 = sum(g["Xc2"] > X5_2 for g in coll)
  npartly = sum(0 < g["ncoll"] < g["ngroups"] for g in items.values())
  nnone = len(items) - len(coll)
  print("host classes: degree 4 %d, degree 5 %d, degree 6 %d (partly collapsed %d), none %d" % (n4, n5, n6, npartly, nnone))
  assert n4 >= 1 and n5 >= 2 and n6 >= 3 and npartly >= 1 and nnone >= 1
  got = _match(pm, mu, S, extra)                                            # (the new path first: see the module's docstring)
  ref = _match(pm, mu, S, extra | OLD)
  print("lists", ref["lists"], "stats", ref["stats"], "groups", ref["groups"], "routed", ref["routed"])
  _assert_same(got, ref)
  # the kernel's own work lists: {degree-6 and -5 items (k_spoly56), -, degree-4 items (k_spoly4), -}
  if extra & WORST:
    assert ref["lists"][0] == 0 and ref["lists"][2] == 0, ref["lists"]
    assert not bool(ref["s56"].any()) and not bool(ref["estS"].any())       # k_item_classes' zeros
  else:
    assert ref["lists"][0] == n5 + n6 and ref["lists"][2] == n4, (ref["lists"], n4, n5, n6)
    assert ref["groups"][0] == npartly, (ref["groups"], npartly)
    s56 = ref["s56"].view(len(DRAW), -1).cpu().numpy()
    estS = ref["estS"].view(len(DRAW), -1).cpu().numpy()
    for (b, po), g in items.items():
      if g["ncoll"] > 0:
        assert s56[b, po] != 0.0 and estS[b, po] > 0.0, (b, po, s56[b, po], estS[b, po])
      else:
        assert s56[b, po] == 0.0 and estS[b, po] == 0.0, (b, po, s56[b, po], estS[b, po])
