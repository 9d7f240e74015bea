"""The slot sweep's instantiations (csrc/mm_mfma.hip: k_qred_f32_mfma<ND8, LDSZ>) that have no A/B twin on one build -- d > 8
(ND8 = 2, 3, 4), Mp past both LDS limits (<1, false>) and the forced worst tier (<1, true>, which its own test compares with itself)
-- to the bit against tests/golden/offdiag_slot_parent.npz: Sff, mm_route_estimates and the routed count recorded from a build of the
commit BEFORE the two sweeps shared one per-wave body (the fixture's `note` names it and the compiler).

To record again (a change that is meant to move these bits), build the earlier commit's library beside this one and run this module
against it with the switch set to the file to write:

  GPFLOWPILCO_MM_LIB=/path/to/libparent.so OFFDIAG_SLOT_GOLDEN_RECORD=out.npz OFFDIAG_SLOT_GOLDEN_NOTE="<commit>; <hipcc version>" \
      python -m pytest tests/test_gpu_offdiag_slot_golden.py

then copy the file over the fixture.  A missing fixture or case fails.  The bits are those of one compiler (the `note`): a new
hipcc may schedule the same arithmetic differently only in ways that keep them, but contraction or reassociation choices can move
them -- if every case fails after a compiler bump and the A/B tests of tests/test_gpu_offdiag_persist.py still pass, record again
from the same earlier commit built with the new compiler.  The inputs are _pm and _states of tests/test_gpu_offdiag_persist.py."""
import os

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, ops
from tests.test_gpu_offdiag_persist import _pm, _states

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offdiag_slot_parent.npz")
RECORD = os.environ.get("OFFDIAG_SLOT_GOLDEN_RECORD")
L, B = 3, 3
# M = 130: Mp = 256, one panel whose last waves are padding; M = 300: Mp = 384, a second panel with waves at row0 >= Mp
CASES = [(d, M, 0) for d in (9, 16, 17, 32) for M in (130, 300)]
CASES += [(8, 2100, 0),                                   # Mp = 2176: past the persistent sweep's and the staged image's limits
          (8, 1000, _lib.MM_FORCE_WORST_TIER)]


@pytest.fixture(scope="module")
def device():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
  if RECORD:
    return None
  assert os.path.exists(GOLDEN), "the fixture is missing: " + GOLDEN
  with np.load(GOLDEN) as z:
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("d,M,extra", CASES, ids=["d%d-M%d%s" % (d, M, "-worst" if e else "") for d, M, e in CASES])
def test_slot_sweep_matches_the_recorded_parent(d, M, extra, device, golden):
  pm = _pm(L, M, d, 2000 + 10 * d + M, "baseline", device)
  mu, S = _states(B, d, 3000 + 10 * d + M, device)
  flags = ops.make_flags(True, True) | extra
  pm.status().zero_()
  Sff = ops.moment_match(pm, mu, S, extra_flags=extra)[1]
  got = {"Sff": Sff.cpu().numpy(), "est": ops.route_estimates(pm, B, flags).cpu().numpy(),
         "routed": np.asarray(ops.offdiag_routed(pm, B, flags), dtype=np.int64)}
  key = "d%d_M%d_x%d_" % (d, M, extra)
  if RECORD:
    old = {}
    if os.path.exists(RECORD):
      with np.load(RECORD) as z:
        old = {k: z[k] for k in z.files}
    old.update({key + k: v for k, v in got.items()})
    old["note"] = np.asarray(os.environ.get("OFFDIAG_SLOT_GOLDEN_NOTE", ""))
    np.savez(RECORD, **old)
    return
  for k, v in got.items():
    assert key + k in golden, "the fixture has no " + key + k
    want = golden[key + k]
    assert want.dtype == v.dtype and want.shape == v.shape, (k, want.dtype, v.dtype)
    assert want.tobytes() == v.tobytes(), (k, want, v)                               # to the bit (a NaN would compare too)
  assert np.all(np.isfinite(got["Sff"])) and np.all(got["est"][..., 0] >= 0)
