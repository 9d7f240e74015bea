"""The Ctx-templated adjoint code of csrc/mm_adjoint.h, mm_adjoint_nd.h and mm_mix.h at the device's lane counts, on the CPU:
tests/hostcheck/adjoint_lanes.hip runs every function on one host thread per lane (64, 256 or 512, as its kernels are launched) with
buffers and scratch of exactly the documented sizes, scratch and assigned outputs filled with NaN, and compares with the one-lane
result.  The program is built three times -- plain, AddressSanitizer + UndefinedBehaviorSanitizer, ThreadSanitizer -- as stand-alone
executables: a missing barrier is a reported race, a short scratch formula a reported overflow, scratch read before it is written a NaN.
Two more runs prove that the check can fail: barriers off must give a race in the header, scratch one double short an overflow."""
import functools
import os
import re
import subprocess

import pytest

HOSTCHECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
BUILDS = {"plain": "adjoint_lanes", "asan": "adjoint_lanes_asan", "tsan": "adjoint_lanes_tsan"}
SANITIZER_LINE = re.compile(r"ThreadSanitizer|AddressSanitizer|runtime error")

# (function, lanes) -> number of shapes: the lists of adjoint_lanes.hip, written out so that a case the driver skips is missed here.
# 64: k_compose_tail_bwd(_nd), k_compose_encode_bwd0, k_compose_mix(_bwd)_nd;  256: k_policy_head_bwd_small / _nd, k_gp_bwd_items,
# k_gp_bwd_moments;  256 and 512: k_pair_agg (beside the diagonal sweep / on its own).
EXPECTED = {
  ("mma_mm", 256): 5, ("mma_spd_inverse", 256): 5, ("mma_solve_pivot", 64): 7,
  ("mma_encode_bwd", 64): 8, ("mma_cost_bwd", 64): 5, ("mma_step_bwd", 64): 8, ("mma_step_bwd_nd", 64): 6,
  ("mma_head_bwd", 256): 4, ("mma_head_bwd_nd", 256): 5,
  ("mma_policy_small_bwd", 256): 8, ("mma_policy_pair_bwd", 256): 5, ("mma_policy_nd_bwd", 256): 5,
  ("mma_pair_poly", 256): 5, ("mma_pair_poly", 512): 5, ("mma_pair_convert", 256): 3, ("mma_pair_convert", 512): 3,
  ("mma_pair_convert_rows", 256): 3, ("mma_pair_convert_rows", 512): 3,
  ("mma_raw_moments", 256): 6,
  ("mma_gp_item_moments", 256): 8 + 3,        # 8 shapes; 3 of them again with the off-diagonal pairs as aggregates
  ("mma_gp_item_bwd", 256): 2 * (8 + 3),      # each of those plain and from chunked partials
  ("mma_mix_fwd<double>", 64): 5, ("mma_mix_fwd<float>", 64): 5, ("mma_mix_bwd", 64): 5,
  ("seq_pair_agg", 256): 4, ("seq_pair_agg", 512): 4,
  ("seq_tail_bwd", 64): 4, ("seq_tail_bwd_nd", 64): 3,
  ("seq_policy_head_bwd", 256): 4, ("seq_policy_head_bwd_nd", 256): 2, ("seq_policy_head_bwd_wide", 256): 2,
}


@functools.lru_cache(maxsize=None)
def _built():
  """The three executables, built by ``__graft_entry__.build()``; rebuilt here when one is missing or older than its sources, as
  tests/test_predict_host.py does for its library."""
  csrc = os.path.join(HOSTCHECK, os.pardir, os.pardir, "gpflowpilco_amd", "csrc")
  deps = [os.path.join(HOSTCHECK, "adjoint_lanes.hip"), os.path.join(HOSTCHECK, "build_lanes.sh")]
  deps += [os.path.join(csrc, h) for h in ("mm_adjoint.h", "mm_adjoint_nd.h", "mm_mix.h", "mm_adjoint_lds.h", "mm_compose.h", "mm_mono.h",
                                            "mm_common.h")]
  exes = [os.path.join(HOSTCHECK, e) for e in BUILDS.values()]
  newest = max(os.path.getmtime(p) for p in deps)
  if any(not os.path.exists(e) or os.path.getmtime(e) < newest for e in exes):
    subprocess.run(["bash", os.path.join(HOSTCHECK, "build_lanes.sh")], check=True)
  return True


def _run(build, *args):
  assert _built()
  return subprocess.run([os.path.join(HOSTCHECK, BUILDS[build])] + list(args), capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("build", list(BUILDS))
def test_every_function_agrees_with_one_lane_at_the_device_lane_counts(build):
  r = _run(build)
  bad = [ln for ln in r.stderr.splitlines() if SANITIZER_LINE.search(ln)]
  failed = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")]
  assert r.returncode == 0 and not bad and not failed, (r.returncode, bad[:10], failed[:10])
  ran = {}
  for ln in r.stdout.splitlines():
    m = re.match(r"case (\S+) nl=(\d+) .* ok$", ln)
    if m:
      ran[(m.group(1), int(m.group(2)))] = ran.get((m.group(1), int(m.group(2))), 0) + 1
  assert ran == EXPECTED
  m = re.search(r"^cases: (\d+)$", r.stdout, re.M)
  assert m and int(m.group(1)) == sum(EXPECTED.values())
  assert re.search(r"^failures: 0$", r.stdout, re.M)


def test_barriers_off_is_a_reported_race_in_the_header():
  """The same driver with sync() a no-op for mma_step_bwd: ThreadSanitizer names lines of csrc/mm_adjoint.h."""
  r = _run("tsan", "--no-sync", "mma_step_bwd")
  assert r.returncode != 0
  assert "WARNING: ThreadSanitizer: data race" in r.stderr
  assert re.search(r"SUMMARY: ThreadSanitizer: data race \S*mm_adjoint\.h:\d+", r.stderr) and "mma_step_bwd<MMATeamCtx>" in r.stderr
  assert _run("tsan", "--only", "mma_step_bwd").returncode == 0           # ... and none with the barriers in place


def test_scratch_one_double_short_is_a_reported_overflow():
  """mma_step_bwd's scratch (nx (2 nd + nx) doubles, used to the last one) one double short: AddressSanitizer reports the access."""
  r = _run("asan", "--short-scratch", "mma_step_bwd")
  assert r.returncode != 0
  assert "ERROR: AddressSanitizer: heap-buffer-overflow" in r.stderr
  assert re.search(r"mma_step_bwd<MMATeamCtx>.*mm_adjoint\.h:\d+", r.stderr)
