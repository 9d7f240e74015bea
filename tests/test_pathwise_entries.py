"""The pathwise entries pass one operand bundle from Python to the launches (csrc/mm_pathwise_drift.h, ``Paths._operands``): what
that can get wrong is an argument list -- nearly every argument is a void or double pointer, so neither the compiler nor ctypes
sees a swap.  Without a GPU:

* every pathwise entry answers a table of refused calls as the library did before its host side took the bundle
  (tests/golden/pathwise_entry_refusals.json; the one-action entries have theirs in tests/test_pathwise.py);
* the entry ``pathwise.py`` picks for each kind of drift and the argument tuple it builds fit the entry's ctypes signature, and
  the library takes the tuple as far as the one buffer left a byte short.

Refusals precede every HIP call.  ``python -m tests.test_pathwise_entries OUT.json`` records the table against the library in
``GPFLOWPILCO_MM_LIB`` (or the in-tree build); it writes nothing unless every entry call was refused.
"""
import ctypes as C
import json
import os

import pytest
import torch

from gpflowpilco_amd import _lib, pathwise
from tests.test_pathwise import _call_refusal_row

F32, F64 = _lib.MM_F32, _lib.MM_F64
MM_E_WORKSPACE = -4
REFUSALS = (-1, -2, -3, -4, -6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pathwise_entry_refusals.json")

# ---- the argument names of every entry, in ABI order -----------------------------------------------------------------------------
_DRIFT = ["omega_t", "phase", "zs_t", "hz", "x_scale", "prior_scale", "variance", "mean_c", "wb"]
_MEAN_DRIFT = ["zs_t", "hz", "x_scale", "variance", "mean_c", "beta"]
_POLICY = ["policy", "policy_bytes", "policy_M", "head_scale", "head_shift", "target", "precis"]
_FORWARD = ["x0", "cost", "tape", "tape_bytes", "with_jacobians", "stream"]
_SHAPE = ["H", "dt", "nx", "na", "active_dims", "nu"]
_MIXING = ["Lg", "mix_W", "mix_c"]
_SWEEP = ["S", "dtype"] + _SHAPE + _POLICY + ["tape", "tape_bytes", "g_cost", "g_policy", "g_x0", "scratch", "scratch_bytes", "stream"]
_SEEDED = _SWEEP[:_SWEEP.index("g_cost") + 1] + ["g_x"] + _SWEEP[_SWEEP.index("g_cost") + 1:]
_SAMPLE = ["S", "L", "M", "K", "d", "dtype"]
NAMES = {
    "mm_pathwise_eval": _SAMPLE + ["x"] + _DRIFT + ["f_out", "stream"],
    "mm_pathwise_eval_jac": _SAMPLE + ["x"] + _DRIFT + ["f_out", "jac_out", "stream"],
    "mm_pathwise_eval_bound": _SAMPLE + ["x"] + _DRIFT + ["f_out", "abs_out", "stream"],
    "mm_pathwise_rollout": _SAMPLE + ["H", "dt", "x", "x_tmp"] + _DRIFT + ["traj", "stream"],
    "mm_pathwise_mean_eval": ["S", "L", "M", "d", "dtype", "x"] + _MEAN_DRIFT + ["f_out", "jac_out", "stream", "kernel"],
    "mm_pathwise_policy_rollout_nd": ["S", "M", "K", "dtype"] + _SHAPE + _DRIFT + _POLICY + _FORWARD,
    "mm_pathwise_policy_rollout_mean": ["S", "M", "dtype"] + _SHAPE + _MEAN_DRIFT + _POLICY + _FORWARD + _MIXING + ["kernel"],
    "mm_pathwise_policy_rollout_backward_nd": _SWEEP,
    "mm_pathwise_policy_rollout_backward_nd_seeded": _SEEDED,
    "mm_pathwise_policy_rollout_backward_mixed": _SEEDED + ["Lg", "mix_W"],
    "mm_pathwise_tape_bytes_nd": ["S", "H", "nx", "na", "nu", "dtype", "with_jacobians"],
    "mm_pathwise_tape_bytes_mixed": ["S", "H", "nx", "na", "nu", "Lg", "dtype", "with_jacobians"],
    "mm_pathwise_backward_scratch_bytes_nd": ["S", "policy_M", "ne", "nu"],
}
for _stem in ("eval", "eval_jac", "eval_bound", "rollout"):
  NAMES[f"mm_pathwise_{_stem}_kern"] = NAMES[f"mm_pathwise_{_stem}"] + ["kernel"]
NAMES["mm_pathwise_policy_rollout_wide"] = NAMES["mm_pathwise_policy_rollout_nd"]
NAMES["mm_pathwise_policy_rollout_mixed"] = NAMES["mm_pathwise_policy_rollout_nd"] + _MIXING
NAMES["mm_pathwise_policy_rollout_kern"] = NAMES["mm_pathwise_policy_rollout_mixed"] + ["kernel"]
NAMES["mm_pathwise_policy_rollout_backward_wide"] = _SWEEP
NAMES["mm_pathwise_policy_rollout_backward_wide_seeded"] = _SEEDED
NAMES["mm_pathwise_backward_scratch_bytes_wide"] = NAMES["mm_pathwise_backward_scratch_bytes_nd"]
QUERIES = tuple(n for n in NAMES if "_bytes" in n)
SAMPLE_ENTRIES = tuple(n for n in NAMES if "policy" not in n and n not in QUERIES)
FORWARD_ENTRIES = tuple(n for n in NAMES if "policy_rollout" in n and "backward" not in n)
SWEEP_ENTRIES = tuple(n for n in NAMES if "backward" in n and n not in QUERIES)


def test_the_names_cover_the_pathwise_entries_and_fit_their_signatures():
  """The table below is written by argument name: the names of an entry are as many as its ctypes signature has arguments, and
  the entries are all the pathwise ones but those recorded in tests/test_pathwise.py and the two path-sampler kernels."""
  for entry, names in NAMES.items():
    assert len(names) == len(set(names)) == len(_lib.SIGNATURES[entry][1]), entry
  elsewhere = {"mm_pathwise_policy_rollout", "mm_pathwise_policy_rollout_backward", "mm_pathwise_policy_rollout_backward_seeded",
               "mm_pathwise_tape_bytes", "mm_pathwise_backward_scratch_bytes", "mm_pathwise_basis", "mm_pathwise_pack_stream"}
  assert set(NAMES) | elsewhere == {n for n in _lib.SIGNATURES if n.startswith("mm_pathwise")}
  assert (len(SAMPLE_ENTRIES), len(FORWARD_ENTRIES), len(SWEEP_ENTRIES), len(QUERIES)) == (9, 5, 5, 4)


# ---- the table of refused calls ----------------------------------------------------------------------------------------------------
def _up256(n):
  return (n + 255) // 256 * 256


def _tape_bytes(S, H, nx, na, nu, Lf, es, jac):
  """MMPwTapeLayout (csrc/mm_pathwise_policy_dev.h): states, drift inputs, the step's sample [S][Lf], its Jacobians."""
  nd = nx + na + nu
  return (_up256((H + 1) * S * nx * es) + _up256(H * S * nd * es) + _up256(S * Lf * es)
          + _up256(H * S * Lf * nd * es if jac else 0))


def _pack_bytes(L, M, d):
  """The float64 blocks of a policy pack, up to Zc64 (mm_model_layout, csrc/mm_common.h): what the pathwise entries read."""
  Mp = (M + 127) // 128 * 128
  return (_up256(L * M * d * 8) + _up256(L * d * Mp * 8) + 2 * _up256(L * d * 8) + 2 * _up256(L * 8) + _up256(L * M * 8))


def _scratch_bytes(S, M, ne, nu):
  return (S + 255) // 256 * 4 * nu * (M * ne + M + ne + 2) * 8


# the shape of every base call: S = 5, nx = 3, one angle, two actions, H = 2, a drift of M = K = 128 (one f64 block), policy M = 12
S_, NX_, NU_, H_, PM_, LG_ = 5, 3, 2, 2, 12, 2
NE_ = NX_ + 1
HUGE = 1 << 40


def refusal_table(two_faults=None):
  """[(entry, [argument, ...])] in the format of tests/golden/pathwise_one_action_refusals.json: an argument is a number, None
  (NULL), "buf" (a 64-byte dummy buffer) or a list of ints (an int32 array).  Every row of an entry that launches carries at least
  one fault, so no call gets past the checks; the rows of the size queries only compute.  ``two_faults``: a dict that is given,
  per entry, the number of its rows with two arguments changed."""
  rows = []

  def add(entry, base, **kw):
    names = NAMES[entry]
    assert kw and set(kw) <= set(names), (entry, kw)
    rows.append((entry, [kw.get(n, base[n]) for n in names]))
    if two_faults is not None and len(kw) >= 2:
      two_faults[entry] = two_faults.get(entry, 0) + 1

  def base_of(entry, **values):
    """Every argument valid: the named values, "buf" for every other pointer (the optional ones included)."""
    base = dict(values, stream=None)
    base.update({n: "buf" for n in NAMES[entry] if n not in base})
    return base

  pointers = lambda base: [n for n, v in base.items() if v == "buf"]

  # -- the sample entries: eval, eval_jac, eval_bound, rollout (each plain and _kern) and the mean's eval
  for entry in SAMPLE_ENTRIES:
    kern, mean, rollout, jac = entry.endswith("_kern"), "mean" in entry, "rollout" in entry, "jac" in entry
    base = base_of(entry, S=S_, L=3, M=128, K=128, d=3, dtype=F64, H=H_, dt=0.5, kernel=1)
    base = {n: v for n, v in base.items() if n in NAMES[entry]}
    sizes = [n for n in ("S", "L", "M", "K", "d", "H") if n in base]
    cases = [{n: v} for n in sizes for v in (0, -1)] + [dict(dtype=7), dict(dtype=-1), dict(d=33)]
    cases += [{n: None} for n in pointers(base) if n not in ("mean_c", "traj") and (n != "jac_out" or not mean)]
    if kern or mean:
      cases += [dict(kernel=-1), dict(kernel=3), dict(kernel=3, S=0), dict(kernel=3, dtype=7), dict(kernel=-1, x=None)]
    if mean:                                                   # any M; the Jacobian pass's bound on d is the entry's
      cases += [dict(d=17), dict(d=17, dtype=7), dict(d=17, beta=None)]
    else:                                                      # K and M in blocks of 128 (f64) or 256 (f32) terms
      cases += [dict(K=64), dict(M=192), dict(dtype=F32), dict(dtype=F32, K=256), dict(dtype=F32, M=256), dict(K=64, x=None),
                dict(K=64, dtype=7), dict(d=33, K=64)]
    if jac:                                                    # (the other passes take d up to 32)
      cases += [dict(d=17), dict(d=17, K=64), dict(d=17, f_out=None), dict(d=17, dtype=7)]
    if rollout:                                                # the Euler form needs d == L
      cases += [dict(L=4), dict(d=2), dict(L=4, H=0), dict(L=4, x_tmp=None), dict(L=4, dtype=7), dict(L=4, K=64)]
    cases += [dict(dtype=7, x=None), dict(S=0, dtype=7), dict(d=33, dtype=7), dict(d=33, wb=None) if "wb" in base else dict(d=33, hz=None)]
    for kw in cases:
      add(entry, base, **kw)

  # -- the forward entries of the policy rollout
  need = {(es, j, Lf): _tape_bytes(S_, H_, NX_, 1, NU_, Lf, es, j) for es in (4, 8) for j in (0, 1) for Lf in (NX_, LG_)}
  pack = _pack_bytes(NU_, PM_, NE_)
  for entry in FORWARD_ENTRIES:
    mixed, kern, mean = entry.endswith("_mixed"), entry.endswith("_kern"), entry.endswith("_mean")
    nd8 = entry.endswith("_nd")
    base = base_of(entry, S=S_, M=128, K=128, dtype=F64, H=H_, dt=0.5, nx=NX_, na=1, active_dims=[1], nu=NU_, policy_bytes=1 << 30,
                   policy_M=PM_, tape_bytes=HUGE, with_jacobians=1, Lg=LG_, kernel=1)
    if kern or mean:                                           # (these two mix when either Lg or mix_W is set)
      base.update(Lg=0, mix_W=None, mix_c=None)
    base = {n: v for n, v in base.items() if n in NAMES[entry]}
    Lf = LG_ if mixed else NX_
    short = need[8, 1, Lf] - 1
    sizes = [n for n in ("S", "M", "K", "H", "policy_M") if n in base]
    cases = [{n: v} for n in sizes for v in (0, -1)]
    cases += [dict(dtype=7), dict(dtype=-1), dict(nx=0), dict(nx=17), dict(na=-1), dict(na=4, active_dims=[0, 1, 2, 0]), dict(nu=0), dict(nu=5),
              dict(active_dims=None), dict(active_dims=[3]), dict(active_dims=[-1]), dict(na=2, active_dims=[1, 1]),
              dict(policy_M=257), dict(policy_M=256, tape_bytes=0)]
    # nd = nx + na + nu one past the entry's bound (8 | 16), and at it
    cases += ([dict(nx=6), dict(nx=5, tape_bytes=0)] if nd8 else
              [dict(nx=12, na=3, active_dims=[0, 1, 2]), dict(nx=11, na=3, active_dims=[0, 1, 2], tape_bytes=0)])
    cases += [dict({n: None}, tape_bytes=short) for n in pointers(base)]
    cases += [dict(tape_bytes=short), dict(tape_bytes=0), dict(with_jacobians=0, tape_bytes=need[8, 0, Lf] - 1),
              dict(dtype=F32, tape_bytes=need[4, 1, Lf] - 1), dict(tape_bytes=short + 1, policy_bytes=pack - 1),
              dict(tape_bytes=short + 1, policy_bytes=64)]
    if mixed or kern or mean:
      on = dict() if mixed else dict(mix_W="buf")
      cases += [dict(on, Lg=0), dict(on, Lg=NX_ + 1), dict(on, Lg=-1), dict(on, Lg=0, target=None), dict(on, Lg=0, dtype=7),
                dict(on, Lg=NX_, tape_bytes=need[8, 1, NX_] - 1), dict(on, Lg=LG_, tape_bytes=need[8, 1, LG_] - 1),
                dict(on, Lg=LG_, mix_c=None, tape_bytes=need[8, 1, LG_] - 1), dict(Lg=LG_, mix_W=None)]
    if kern or mean:
      cases += [dict(kernel=-1), dict(kernel=3), dict(kernel=3, S=0), dict(kernel=-1, dtype=7), dict(kernel=3, nu=5),
                dict(kernel=0, tape_bytes=short), dict(kernel=2, tape_bytes=short)]
    if mean:
      cases += [dict(beta=None), dict(beta=None, dtype=7), dict(beta=None, nu=5)]
    # two faults at once: which is reported
    cases += [dict(dtype=7, x0=None), dict(S=0, dtype=7), dict(dtype=7, nu=5), dict(nu=5, policy=None), dict(policy_M=257, tape_bytes=0),
              dict(policy_M=257, cost=None), dict(active_dims=None, dtype=7), dict(active_dims=None, nu=5),
              dict(tape_bytes=short, policy_bytes=pack - 1), dict(tape=None, tape_bytes=0), dict(nx=17, x0=None)]
    for kw in cases:
      add(entry, base, **kw)

  # -- the reverse sweeps
  sb = _scratch_bytes(S_, PM_, NE_, NU_)
  for entry in SWEEP_ENTRIES:
    mixed, seeded, nd8 = entry.endswith("_mixed"), not entry.endswith(("_nd", "_wide")), "_nd" in entry
    base = base_of(entry, S=S_, dtype=F64, H=H_, dt=0.5, nx=NX_, na=1, active_dims=[1], nu=NU_, policy_bytes=1 << 30, policy_M=PM_,
                   tape_bytes=HUGE, scratch_bytes=HUGE, Lg=LG_)
    base = {n: v for n, v in base.items() if n in NAMES[entry]}
    exact = need[8, 1, LG_ if mixed else NX_]
    cases = [{n: v} for n in ("S", "H", "policy_M") for v in (0, -1)]
    cases += [dict(dtype=7), dict(dtype=-1), dict(nx=0), dict(nx=17), dict(na=-1), dict(na=4, active_dims=[0, 1, 2, 0]), dict(nu=0), dict(nu=5),
              dict(active_dims=None), dict(active_dims=[3]), dict(na=2, active_dims=[1, 1]), dict(policy_M=257),
              dict(policy_M=256, tape_bytes=0)]
    cases += ([dict(nx=6), dict(nx=5, tape_bytes=0)] if nd8 else
              [dict(nx=12, na=3, active_dims=[0, 1, 2]), dict(nx=11, na=3, active_dims=[0, 1, 2], policy_M=64, tape_bytes=0)])
    # the sweep's LDS bound: nu = 4 on ne = 4 stops at M = 203
    cases += [dict(nu=4, policy_M=204), dict(nu=4, policy_M=203, tape_bytes=0), dict(nu=4, policy_M=256, tape=None)]
    cases += [dict({n: None}, tape_bytes=exact - 1) for n in pointers(base)]
    if seeded:
      cases += [dict(g_cost=None, g_x=None), dict(g_cost=None, g_x=None, tape_bytes=exact - 1), dict(g_cost=None, g_x=None, dtype=7)]
    cases += [dict(tape_bytes=exact - 1), dict(tape_bytes=0), dict(tape_bytes=need[8, 0, LG_ if mixed else NX_]),
              dict(dtype=F32, tape_bytes=need[4, 1, LG_ if mixed else NX_] - 1), dict(tape_bytes=exact, scratch_bytes=sb - 1),
              dict(tape_bytes=exact, scratch_bytes=0), dict(tape_bytes=exact, scratch_bytes=sb, policy_bytes=pack - 1),
              dict(tape_bytes=exact, scratch_bytes=sb, policy_bytes=64),
              dict(S=300, tape_bytes=_tape_bytes(300, H_, NX_, 1, NU_, LG_ if mixed else NX_, 8, 1), scratch_bytes=2 * sb - 1)]
    if mixed:
      cases += [dict(Lg=0), dict(Lg=NX_ + 1), dict(Lg=0, mix_W=None), dict(Lg=0, dtype=7), dict(Lg=NX_, tape_bytes=need[8, 1, NX_] - 1)]
    cases += [dict(dtype=7, tape=None), dict(S=0, dtype=7), dict(g_cost=None, S=0), dict(policy_M=257, g_policy=None),
              dict(tape_bytes=exact - 1, scratch_bytes=sb - 1), dict(tape_bytes=exact, scratch_bytes=sb - 1, policy_bytes=pack - 1),
              dict(scratch=None, scratch_bytes=0), dict(active_dims=None, dtype=7), dict(nu=5, policy=None)]
    for kw in cases:
      add(entry, base, **kw)

  # -- the size queries
  for jac in (0, 1):
    for a in [(S_, H_, NX_, 1, NU_, F64), (S_, H_, NX_, 1, NU_, F32), (300, 6, 4, 1, 1, F64), (S_, H_, NX_, 0, 4, F64),
              (S_, H_, 16, 8, 4, F64), (0, H_, NX_, 1, NU_, F64), (-1, H_, NX_, 1, NU_, F64), (S_, 0, NX_, 1, NU_, F64),
              (S_, H_, 0, 0, NU_, F64), (S_, H_, 17, 1, NU_, F64), (S_, H_, NX_, -1, NU_, F64), (S_, H_, NX_, 4, NU_, F64),
              (S_, H_, 16, 9, NU_, F64), (S_, H_, NX_, 1, 0, F64), (S_, H_, NX_, 1, 5, F64)]:
      rows.append(("mm_pathwise_tape_bytes_nd", list(a) + [jac]))
      for Lg in (0, 1, a[2], a[2] + 1):
        rows.append(("mm_pathwise_tape_bytes_mixed", list(a[:5]) + [Lg, a[5], jac]))
  for query in ("mm_pathwise_backward_scratch_bytes_nd", "mm_pathwise_backward_scratch_bytes_wide"):
    for S in (S_, 300):
      for M in (12, 77, 78, 203, 204, 257):
        for ne, nu in ((4, 1), (4, 4), (5, 3), (6, 2), (7, 2), (12, 4), (13, 4), (16, 1)):
          rows.append((query, [S, M, ne, nu]))
    for a in ((0, 12, 4, 2), (-1, 12, 4, 2), (S_, 0, 4, 2), (S_, 12, 0, 2), (S_, 12, 4, 0), (S_, 12, 4, 5)):
      rows.append((query, list(a)))
  return rows


def test_pathwise_entries_refuse_as_recorded_before_their_host_side_took_the_bundle():
  """tests/golden/pathwise_entry_refusals.json holds what the last commit at which every entry passed its operands on as a
  positional list (83121cc) returned for the calls of refusal_table(): `[{"entry", "args", "ret"}]`.  The table and the recording
  list the same calls, every recorded call of an entry that launches was refused, and the library answers each as recorded --
  with two faults at once the one that was reported then is reported now."""
  with open(GOLDEN) as fh:
    recorded = json.load(fh)
  two_faults = {}
  table = refusal_table(two_faults)
  assert [(r["entry"], r["args"]) for r in recorded] == [(e, a) for e, a in table]
  assert {r["entry"] for r in recorded} == set(NAMES)
  lib = _lib.lib()
  for r in recorded:
    if r["entry"] not in QUERIES:
      assert r["ret"] in REFUSALS, r                                               # (never replay a call that was not refused)
    assert _call_refusal_row(lib, r["entry"], r["args"]) == r["ret"], r
  launching = set(NAMES) - set(QUERIES)
  assert set(two_faults) == launching and min(two_faults.values()) >= 6           # the rows that pin a precedence


# ---- argument assembly on stub operands --------------------------------------------------------------------------------------------
S, NX, ACTIVE, MD, KD, MP, H = 5, 3, (1,), 128, 128, 12, 2
NE = NX + len(ACTIVE)


class _Pack:
  """What ``PolicyRollout`` reads of an ``ops.PackedModel``, on host memory of the packed size."""

  def __init__(self, L, M, d):
    self.L, self.M, self.d = L, M, d
    self.nbytes = _lib.lib().mm_packed_model_bytes(L, M, d, F64, 0)
    assert self.nbytes > 0
    self.buf = torch.zeros(self.nbytes, dtype=torch.uint8)


def _paths(L, d, kernel=0, mix_W=None):
  z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
  return pathwise.Paths(omega=z(L, d, KD), phase=z(L, KD), zs=z(L, d, MD), hz=z(L, MD), wb=z((S + 3) // 4, L, (KD + MD) // 128, 4, 128),
                        num_samples=S, lengthscales=z(L, d), prior_scale=z(L), variance=z(L), mean_c=None if mix_W is not None else z(L),
                        mix_W=mix_W, mix_c=None if mix_W is None else z(NX), kernel=kernel)


def _mean_drift(L, d, kernel=0):
  z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
  return pathwise.MeanDrift(zs=z(L, d, 32), hz=z(L, 32), beta=z(L, 32), lengthscales=z(L, d), variance=z(L), mean_c=z(L), kernel=kernel,
                            num_centres=20)


class _Recorder:
  """Stands in for ``_lib.lib()``: the size queries answer as the library does (``short``: that query one byte less, so that the
  wrapper allocates and passes a buffer one byte short); an entry call is recorded, and handed to the library only when a buffer
  is short -- the library then refuses it before any HIP call."""

  def __init__(self, real, short=None):
    self.real, self.short, self.calls = real, short, []

  def __getattr__(self, name):
    fn = getattr(self.real, name)
    if "_bytes" in name:
      return lambda *a: fn(*a) - (1 if self.short and self.short in name else 0)

    def entry(*args):
      self.calls.append((name, args))
      return fn(*args) if self.short else 0
    return entry


@pytest.fixture
def on_host(monkeypatch):
  """``pathwise`` on host tensors: no device requirement, a NULL stream, and a recording library."""
  real = _lib.lib()

  def install(short=None):
    rec = _Recorder(real, short)
    monkeypatch.setattr(pathwise._lib, "lib", lambda: rec)
    return rec
  monkeypatch.setattr(pathwise, "_require_device", lambda *tensors: None)
  monkeypatch.setattr(pathwise, "_stream", lambda device: None)
  return install


def _fits(entry, args):
  argtypes = _lib.SIGNATURES[entry][1]
  assert len(args) == len(argtypes) == len(NAMES[entry]), (entry, len(args), len(argtypes))
  for i, (a, ty) in enumerate(zip(args, argtypes)):
    try:
      ty.from_param(a)
    except (TypeError, C.ArgumentError) as e:
      raise AssertionError(f"{entry}: argument {i} ({NAMES[entry][i]}) = {a!r} is no {ty.__name__}") from e
  return dict(zip(NAMES[entry], args))


def _drift_operands(P):
  return dict(omega_t=P.omega.data_ptr(), phase=P.phase.data_ptr(), zs_t=P.zs.data_ptr(), hz=P.hz.data_ptr(),
              x_scale=P.lengthscales.data_ptr(), prior_scale=P.prior_scale.data_ptr(), variance=P.variance.data_ptr(),
              mean_c=None if P.mean_c is None else P.mean_c.data_ptr(), wb=P.wb.data_ptr())


@pytest.mark.parametrize("kernel", [0, 2])
def test_the_sample_entries_get_the_operands_by_name(on_host, kernel):
  rec = on_host()
  P = _paths(NX, NX, kernel=kernel)
  x = torch.zeros(S, NX, dtype=torch.float64)
  f = P(x)
  _, jac = P.eval_jac(x)
  _, err = P.eval_with_bound(x)
  xH, traj = P.rollout(x, H, dt=0.25, keep_trajectory=True)
  assert P.rollout(x, H).shape == (S, NX)
  sfx = "_kern" if kernel else ""
  stems = ["mm_pathwise_eval", "mm_pathwise_eval_jac", "mm_pathwise_eval_bound", "mm_pathwise_rollout", "mm_pathwise_rollout"]
  assert [c[0] for c in rec.calls] == [s + sfx for s in stems]
  assert (f.shape, jac.shape, err.shape, xH.shape, traj.shape) == ((S, NX), (S, NX, NX), (S, NX), (S, NX), (H, S, NX))
  for entry, args in rec.calls:
    a = _fits(entry, args)
    assert (a["S"], a["L"], a["M"], a["K"], a["d"], a["dtype"], a["stream"]) == (S, NX, MD, KD, NX, F64, None)
    assert {k: a[k] for k in _DRIFT} == _drift_operands(P)
    assert a.get("kernel", 0) == kernel
  a = [_fits(*c) for c in rec.calls]
  assert a[0]["x"] == a[1]["x"] == a[2]["x"] == x.data_ptr() and a[0]["f_out"] == f.data_ptr()
  assert a[1]["jac_out"] == jac.data_ptr() and a[2]["abs_out"] not in (None, a[2]["f_out"])
  assert (a[3]["H"], a[3]["dt"], a[3]["x"], a[3]["traj"]) == (H, 0.25, xH.data_ptr(), traj.data_ptr())
  assert a[3]["x_tmp"] not in (None, a[3]["x"], x.data_ptr()) and a[4]["traj"] is None
  with pytest.raises(ValueError, match=r"expected x \[5,3\] of torch.float64, got \(4, 3\) torch.float64"):
    P(torch.zeros(4, NX, dtype=torch.float64))
  with pytest.raises(ValueError, match=r"expected x \[5,3\] of torch.float64, got \(5, 3\) torch.float32"):
    P.eval_jac(torch.zeros(S, NX))


def test_the_mean_entry_gets_the_operands_by_name(on_host):
  rec = on_host()
  D = _mean_drift(NX, NX, kernel=1)
  x = torch.zeros(7, NX, dtype=torch.float64)
  f, jac = D.eval_jac(x)
  D(x)
  assert [c[0] for c in rec.calls] == ["mm_pathwise_mean_eval"] * 2
  a, b = (_fits(*c) for c in rec.calls)
  assert (a["S"], a["L"], a["M"], a["d"], a["dtype"], a["kernel"]) == (7, NX, 32, NX, F64, 1)
  assert (a["x"], a["zs_t"], a["hz"], a["x_scale"]) == (x.data_ptr(), D.zs.data_ptr(), D.hz.data_ptr(), D.lengthscales.data_ptr())
  assert (a["variance"], a["mean_c"], a["beta"]) == (D.variance.data_ptr(), D.mean_c.data_ptr(), D.beta.data_ptr())
  assert (a["f_out"], a["jac_out"], b["jac_out"]) == (f.data_ptr(), jac.data_ptr(), None)


# kind -> (the rollout's keywords, forward entry, tape query, scratch query, unseeded sweep, seeded sweep)
_RO, _BS = "mm_pathwise_policy_rollout", "mm_pathwise_backward_scratch_bytes"
KINDS = {
    "one": (dict(nu=1), _RO, "mm_pathwise_tape_bytes", _BS, f"{_RO}_backward", f"{_RO}_backward_seeded"),
    "nd": (dict(nu=2), f"{_RO}_nd", "mm_pathwise_tape_bytes_nd", f"{_BS}_nd", f"{_RO}_backward_nd", f"{_RO}_backward_nd_seeded"),
    "wide": (dict(nu=2, wide=True), f"{_RO}_wide", "mm_pathwise_tape_bytes_nd", f"{_BS}_wide", f"{_RO}_backward_wide",
             f"{_RO}_backward_wide_seeded"),
    "mixed": (dict(nu=2, mixed=True), f"{_RO}_mixed", "mm_pathwise_tape_bytes_mixed", f"{_BS}_wide", f"{_RO}_backward_mixed",
              f"{_RO}_backward_mixed"),
    "matern": (dict(nu=1, kernel=2), f"{_RO}_kern", "mm_pathwise_tape_bytes_nd", f"{_BS}_wide", f"{_RO}_backward_wide",
               f"{_RO}_backward_wide_seeded"),
    "mean": (dict(nu=2, mean=True), f"{_RO}_mean", "mm_pathwise_tape_bytes_nd", f"{_BS}_wide", f"{_RO}_backward_wide",
             f"{_RO}_backward_wide_seeded"),
}
SCALES, SHIFTS = (2.0, 1.5), (-0.5, -0.4)
NAMES_ONE = {_RO: [n for n in NAMES[f"{_RO}_nd"] if n != "nu"], f"{_RO}_backward": [n for n in _SWEEP if n != "nu"],
             f"{_RO}_backward_seeded": [n for n in _SEEDED if n != "nu"]}


def _policy_rollout(nu, wide=False, mixed=False, kernel=0, mean=False):
  L, d = (2 if mixed else NX), NE + nu
  mix_W = torch.ones(NX, L, dtype=torch.float64) if mixed else None
  drift = _mean_drift(L, d) if mean else _paths(L, d, kernel=kernel, mix_W=mix_W)
  head = dict(head_scale=SCALES[0], head_shift=SHIFTS[0]) if nu == 1 else dict(head_scale=SCALES, head_shift=SHIFTS)
  return pathwise.PolicyRollout(drift, _Pack(nu, MP, NE), nx=NX, active_dims=ACTIVE, wide=wide, num_samples=S if mean else None,
                                target=torch.zeros(NE, dtype=torch.float64), precis=torch.eye(NE, dtype=torch.float64), **head)


def _named(entry, args):
  if entry in NAMES_ONE:                                       # the one-action entries: no action count, head constants by value
    assert len(args) == len(NAMES_ONE[entry]) == len(_lib.SIGNATURES[entry][1])
    for a, ty in zip(args, _lib.SIGNATURES[entry][1]):
      ty.from_param(a)
    return dict(zip(NAMES_ONE[entry], args))
  return _fits(entry, args)


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_policy_rollout_picks_its_entries_and_assembles_their_arguments(on_host, kind):
  kw, forward, tape_query, scratch_query, sweep, seeded = KINDS[kind]
  rec = on_host()
  roll = _policy_rollout(**kw)
  nu = kw["nu"]
  assert (roll._forward, roll._tape_query, roll._scratch_query, roll._sweeps) == (forward, tape_query, scratch_query, (sweep, seeded))
  x0 = torch.zeros(S, NX, dtype=torch.float64)
  cost, tape = roll(x0, H, dt=0.25, with_jacobians=True)
  g_cost, g_states = torch.zeros(H, S, dtype=torch.float64), torch.zeros(H, S, NX, dtype=torch.float64)
  g_pol, g_x0 = roll.backward(tape, g_cost, H, dt=0.25, want_state_grad=True)
  roll.backward(tape, None, H, dt=0.25, g_states=g_states)
  assert [c[0] for c in rec.calls] == [forward, sweep, seeded]
  assert cost.shape == (H, S) and g_x0.shape == (S, NX)
  assert g_pol.shape == ((MP * NE + MP + NE + 2,) if kind == "one" else (nu, MP * NE + MP + NE + 2))
  f, b, s = (_named(*c) for c in rec.calls)
  P, pol = roll.paths, roll.policy
  # the drift part
  assert (f["S"], f["M"], f["dtype"]) == (S, 32 if kind == "mean" else MD, F64) and f.get("K", KD) == KD
  if kind == "mean":
    assert [f[k] for k in _MEAN_DRIFT] == [P.zs.data_ptr(), P.hz.data_ptr(), P.lengthscales.data_ptr(), P.variance.data_ptr(),
                                           P.mean_c.data_ptr(), P.beta.data_ptr()]
  else:
    assert {k: f[k] for k in _DRIFT} == _drift_operands(P)
  # what the three share
  for a in (f, b, s):
    assert (a["H"], a["dt"], a["nx"], a["na"], list(a["active_dims"]), a.get("nu", 1)) == (H, 0.25, NX, 1, list(ACTIVE), nu)
    assert (a["policy"], a["policy_bytes"], a["policy_M"]) == (pol.buf.data_ptr(), pol.nbytes, MP)
    if kind == "one":
      assert (a["head_scale"], a["head_shift"]) == (SCALES[0], SHIFTS[0])
    else:
      assert (list(a["head_scale"]), list(a["head_shift"])) == (list(SCALES[:nu]) if nu > 1 else [SCALES[0]],
                                                                list(SHIFTS[:nu]) if nu > 1 else [SHIFTS[0]])
    assert (a["target"], a["precis"], a["stream"]) == (roll.target.data_ptr(), roll.precis.data_ptr(), None)
    assert (a["tape"], a["tape_bytes"]) == (tape.data_ptr(), tape.numel())
  assert (f["x0"], f["cost"], f["with_jacobians"]) == (x0.data_ptr(), cost.data_ptr(), 1)
  mixing = (2, roll._mix_W.data_ptr(), roll._mix_c.data_ptr()) if kind == "mixed" else (0, None, None)
  if kind in ("mixed", "matern", "mean"):
    assert (f["Lg"], f["mix_W"], f["mix_c"]) == mixing
  assert f.get("kernel", 0) == kw.get("kernel", 0) and ("kernel" in f) == (kind in ("matern", "mean"))
  assert (b["g_cost"], b.get("g_x"), b["g_policy"], b["g_x0"]) == (g_cost.data_ptr(), None, g_pol.data_ptr(), g_x0.data_ptr())
  assert s["g_cost"] is None and s["g_x"] not in (None, s["g_policy"]) and s["g_x0"] is None
  for a in (b, s):
    assert a["scratch"] is not None and a["scratch_bytes"] == getattr(_lib.lib(), scratch_query)(*(S, MP, NE) + ((nu,) if kind != "one" else ()))
    assert (a.get("Lg"), a.get("mix_W")) == (mixing[:2] if kind == "mixed" else (None, None))


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_library_takes_the_assembled_arguments_as_far_as_the_short_buffer(on_host, kind):
  """With the tape -- or the sweep's scratch -- one byte short and every other argument as ``PolicyRollout`` assembles it, the
  library says MM_E_WORKSPACE and nothing else: sizes, dtype, dimensions, the mixing and every pointer were accepted."""
  kw, forward, _, _, sweep, seeded = KINDS[kind]
  x0 = torch.zeros(S, NX, dtype=torch.float64)
  g_cost, g_states = torch.zeros(H, S, dtype=torch.float64), torch.zeros(H, S, NX, dtype=torch.float64)
  rec = on_host()
  roll = _policy_rollout(**kw)
  _, tape = roll(x0, H, with_jacobians=True)
  for with_jac in (False, True):
    rec = on_host(short="tape")
    with pytest.raises(ValueError, match=f"^{forward}: MM_E_WORKSPACE"):
      roll(x0, H, with_jacobians=with_jac)
    assert rec.calls[-1][0] == forward
  rec = on_host(short="scratch")
  for entry, seeds in ((sweep, dict()), (seeded, dict(g_states=g_states))):
    with pytest.raises(ValueError, match=f"^{entry}: MM_E_WORKSPACE"):
      roll.backward(tape, g_cost, H, want_state_grad=True, **seeds)
    with pytest.raises(ValueError, match=f"^{entry}: MM_E_WORKSPACE"):
      roll.backward(tape[:-1], g_cost, H, **seeds)
  assert [c[0] for c in rec.calls] == [sweep, sweep, seeded, seeded]


if __name__ == "__main__":
  import sys
  lib_, out_ = _lib.lib(), []
  for entry_, args_ in refusal_table():
    ret_ = _call_refusal_row(lib_, entry_, args_)
    assert entry_ in QUERIES or ret_ in REFUSALS, (entry_, args_, ret_)
    out_.append({"entry": entry_, "args": args_, "ret": ret_})
  with open(sys.argv[1], "w") as fh_:
    fh_.write("[\n" + ",\n".join(json.dumps(r) for r in out_) + "\n]\n")
  print(f"{len(out_)} rows from {_lib.LIB_PATH}")
