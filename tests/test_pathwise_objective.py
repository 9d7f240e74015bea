"""Caller-defined objectives on the native pathwise policy rollouts (``native_objective=True``): the seeded reverse sweeps
``mm_pathwise_policy_rollout_backward_seeded`` / ``_nd_seeded`` / ``_wide_seeded`` (csrc/mm_pathwise_policy.hip), ``pathwise.PolicyRollout.backward(g_states=...)`` / ``.trajectory``,
``pathwise.PolicyTrajectoryFunction`` and the routing of ``loops.pathwise_policy_loss_closure``.

Systems (the ones the pathwise tests share; drift M 50 (M0: 40), K 130 (M0: 64), policy M 12; H = 6, dt = 0.5; S = 37: one partial
wave -- the shape at which idle lanes that read a seed would count sample S - 1 twice; S = 300: two workgroups):
  C   nx 4, one angle, one action       the one-action entries        tests/test_pathwise_multiaction.py::_system
  P   nx 4, two angles, two actions     the _nd entries
  Q   nx 3, one angle, three actions    (timing guard only)
  W2  nx 5, two angles, two actions     nd 9: the _wide entries       tests/test_pathwise_wide.py::_system
  M0  nx 2, no encoder, one action                                    tests/test_no_encoder.py::_pw_system
The objective is defined here, on tensors:   (1 + 0.1 t / dt) (e - tau)^T W (e - tau)   with W symmetric positive definite and tau
from seed 5 (the recipe of tests/test_native_objective.py::_quadratic).  The per-step weights differ, so a seed applied one step
off cannot pass (test_reversed_time_weights_move_every_gradient_of_the_comparator).

Bars: the closure against the torch composition of the same closure on the same paths (``native=False``): loss 1e-10, every policy
parameter tensor and x0 1e-8 relative -- the bars of test_gpu_closure_runs_*_natively_when_asked.  The seed identity (the built-in
cost's own gradient fed back as a seed): downstream of the seed both sweeps do identical f64 arithmetic, 1e-8 relative per tensor,
the project's gradient bar; the measured figure is printed and is rounding-level."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
from tests import test_no_encoder as tn
from tests import test_pathwise_multiaction as tm
from tests import test_pathwise_wide as tw
from tests.helpers import to_dev

F64 = torch.float64
H6, DT = 6, 0.5
GRAD_BAR, LOSS_BAR = 1e-8, 1e-10


class QuadraticObjective:
  """(1 + 0.1 t / dt) (e - tau)^T W (e - tau) of a tensor of encoded states; ``reverse``: the weights of steps 1 .. H reversed."""

  def __init__(self, W, tau, reverse=False):
    self.W, self.tau, self.reverse = W, tau, reverse

  def __call__(self, x, t=None):
    e = x - self.tau
    k = t / DT
    wt = 1.0 + 0.1 * ((H6 + 1 - k) if self.reverse else k)
    return wt * (e * (e @ self.W)).sum(-1)


def _quadratic(ne, device, seed=5, reverse=False):
  rng = np.random.default_rng(seed)
  A = rng.standard_normal((ne, ne))
  W = to_dev(A @ A.T / ne + 0.5 * np.eye(ne), device, F64)
  tau = to_dev(rng.uniform(0.0, 0.5, ne), device, F64)
  return QuadraticObjective(W, tau, reverse)


def _sys(name, S):
  if name == "W2":
    return tw._system("W2", S)
  if name == "M0":
    sy = dict(tn._pw_system("M0", S))
    sy.update(active=(), na=0)
    return sy
  return tm._system(name, S)


def _torch_system(name, sy, device):
  return tn._pw_torch_system(sy, device) if name == "M0" else tm._torch_system(sy, device)


def _device_case(name, sy, device, dtype):
  if name == "W2":
    return tw._device_case(sy, device, dtype)
  if name == "M0":
    return tn._pw_device_case(sy, device, dtype)
  return tm._device_case(sy, device, dtype)


# which options the closure needs to run a system natively
ROUTE = {"C": dict(), "P": dict(native_actions=4), "Q": dict(native_actions=4), "W2": dict(native_inputs=16, native_actions=4),
         "M0": dict(native_no_encoder=True)}


def _rel(got, want):
  return float((got - want).abs().max()) / max(1e-300, float(want.abs().max()))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_seeded_entries_are_declared_exported_and_refuse_like_their_siblings_without_gpu():
  lib = _lib.lib()
  names = ["mm_pathwise_policy_rollout_backward_seeded", "mm_pathwise_policy_rollout_backward_nd_seeded",
           "mm_pathwise_policy_rollout_backward_wide_seeded"]
  for n in names:
    sib = n[:-len("_seeded")]
    assert n in _lib.SIGNATURES and hasattr(lib, n)
    res, args = _lib.SIGNATURES[n]
    sres, sargs = _lib.SIGNATURES[sib]
    assert res is sres and len(args) == len(sargs) + 1
    i = len(sargs) - 6                                                             # g_cost's place: ..., g_cost, g_policy, g_x0, scratch, bytes, stream
    assert args[:i + 1] == sargs[:i + 1] and args[i + 1] is ctypes.c_void_p and args[i + 2:] == sargs[i + 1:]
  assert lib.mm_abi_version() == 2
  buf = (ctypes.c_char * 64)()
  p = ctypes.addressof(buf)
  F64c = _lib.MM_F64
  E_ARG, E_DIM, E_DTYPE, E_WS = -1, -2, -3, -4
  act = (ctypes.c_int32 * 2)(0, 1)
  sc = (ctypes.c_double * 4)(2.0, 1.5, 1.0, 1.0)
  sh = (ctypes.c_double * 4)(-0.5, -0.4, -0.6, 0.0)

  # ---- the one-action entry (cartpole: nx 4, one angle)
  def one(seeded, S=37, nx=4, na=1, dtype=F64c, a=act, pol=p, pol_bytes=1 << 30, pM=12, target=p, tape=p, tape_bytes=1 << 40,
          g_cost=p, g_x=p, g_pol=p, scratch=p, scratch_bytes=1 << 40):
    if seeded:
      return lib.mm_pathwise_policy_rollout_backward_seeded(S, dtype, 6, 0.5, nx, na, a, pol, pol_bytes, pM, 2.0, -0.5, target, p, tape,
                                                            tape_bytes, g_cost, g_x, g_pol, None, scratch, scratch_bytes, None)
    return lib.mm_pathwise_policy_rollout_backward(S, dtype, 6, 0.5, nx, na, a, pol, pol_bytes, pM, 2.0, -0.5, target, p, tape,
                                                   tape_bytes, g_cost, g_pol, None, scratch, scratch_bytes, None)
  need1 = lib.mm_pathwise_tape_bytes(37, 6, 4, 1, F64c, 1)
  sb1 = lib.mm_pathwise_backward_scratch_bytes(37, 12, 5)
  assert need1 > 0 and sb1 > 0
  assert one(True, g_cost=None, g_x=None) == E_ARG                                 # both seeds null
  assert one(True, g_cost=None, tape_bytes=need1 - 1) == E_WS                      # either alone gets as far as the size checks
  assert one(True, g_x=None, tape_bytes=need1 - 1) == E_WS
  for kw, code in ((dict(S=0), E_ARG), (dict(dtype=7), E_DTYPE), (dict(nx=7, na=1), E_DIM), (dict(pM=257), E_DIM),
                   (dict(pol=None), E_ARG), (dict(target=None), E_ARG), (dict(tape=None), E_ARG),
                   (dict(g_pol=None), E_ARG), (dict(scratch=None), E_ARG), (dict(tape_bytes=need1 - 1), E_WS),
                   (dict(tape_bytes=need1, scratch_bytes=sb1 - 1), E_WS),
                   (dict(tape_bytes=need1, scratch_bytes=sb1, pol_bytes=64), E_WS),
                   (dict(S=0, dtype=7, pM=257, pol=None), E_ARG), (dict(dtype=7, pM=257, pol=None), E_DTYPE),      # the order
                   (dict(pM=257, pol=None, tape_bytes=0), E_DIM), (dict(pol=None, tape_bytes=0), E_ARG)):
    assert one(False, **kw) == code, kw
    for seeds in (dict(), dict(g_cost=None), dict(g_x=None)):
      assert one(True, **kw, **seeds) == code, (kw, seeds)
  # both null is reported where the sibling reports its null g_cost: after sizes, dtype and dimensions
  assert one(True, g_cost=None, g_x=None, S=0) == E_ARG and one(True, g_cost=None, g_x=None, dtype=7) == E_DTYPE
  assert one(True, g_cost=None, g_x=None, pM=257) == E_DIM and one(True, g_cost=None, g_x=None, tape_bytes=0) == E_ARG

  # ---- the _nd and _wide entries (defaults: two angles, two actions; _nd nx 4 -> nd 8, _wide nx 5 -> nd 9)
  for sfx, nx0, nd_over, lds_over in (("nd", 4, dict(nx=5, na=2, nu=2), dict(nx=2, na=2, nu=4, pM=256)),
                                      ("wide", 5, dict(nx=13, na=2, nu=2), dict(nx=10, na=2, nu=4, pM=78))):
    f_sib = getattr(lib, f"mm_pathwise_policy_rollout_backward_{sfx}")
    f_seed = getattr(lib, f"mm_pathwise_policy_rollout_backward_{sfx}_seeded")
    sbq = getattr(lib, f"mm_pathwise_backward_scratch_bytes_{sfx}")

    def nd(seeded, S=37, nu=2, nx=nx0, na=2, dtype=F64c, a=act, pol=p, pol_bytes=1 << 30, pM=12, scale=sc, shift=sh, tape=p,
           tape_bytes=1 << 40, g_cost=p, g_x=p, g_pol=p, scratch=p, scratch_bytes=1 << 40):
      if seeded:
        return f_seed(S, dtype, 6, 0.5, nx, na, a, nu, pol, pol_bytes, pM, scale, shift, p, p, tape, tape_bytes, g_cost, g_x, g_pol,
                      None, scratch, scratch_bytes, None)
      return f_sib(S, dtype, 6, 0.5, nx, na, a, nu, pol, pol_bytes, pM, scale, shift, p, p, tape, tape_bytes, g_cost, g_pol, None,
                   scratch, scratch_bytes, None)
    need = lib.mm_pathwise_tape_bytes_nd(37, 6, nx0, 2, 2, F64c, 1)
    sbn = sbq(37, 12, nx0 + 2, 2)
    assert need > 0 and sbn > 0
    assert nd(True, g_cost=None, g_x=None) == E_ARG
    assert nd(True, g_cost=None, tape_bytes=need - 1) == E_WS and nd(True, g_x=None, tape_bytes=need - 1) == E_WS
    for kw, code in ((dict(S=0), E_ARG), (dict(a=None), E_ARG), (dict(dtype=7), E_DTYPE), (dict(nu=0), E_DIM), (dict(nu=5), E_DIM),
                     (nd_over, E_DIM), (dict(pM=257), E_DIM), (lds_over, E_DIM), (dict(pol=None), E_ARG), (dict(scale=None), E_ARG),
                     (dict(shift=None), E_ARG), (dict(tape=None), E_ARG), (dict(g_pol=None), E_ARG), (dict(scratch=None), E_ARG),
                     (dict(tape_bytes=need - 1), E_WS), (dict(tape_bytes=need, scratch_bytes=sbn - 1), E_WS),
                     (dict(tape_bytes=need, scratch_bytes=sbn, pol_bytes=64), E_WS),
                     (dict(S=0, dtype=7, nu=5, pol=None), E_ARG), (dict(dtype=7, nu=5, pol=None), E_DTYPE),
                     (dict(nu=5, pol=None, tape_bytes=0), E_DIM), (dict(pol=None, tape_bytes=0), E_ARG),
                     (dict(lds_over, pol=None), E_ARG), (dict(lds_over, tape_bytes=0), E_DIM)):            # null pointers, THEN the LDS bound
      assert nd(False, **kw) == code, (sfx, kw)
      for seeds in (dict(), dict(g_cost=None), dict(g_x=None)):
        assert nd(True, **kw, **seeds) == code, (sfx, kw, seeds)
    assert nd(True, g_cost=None, g_x=None, dtype=7) == E_DTYPE and nd(True, g_cost=None, g_x=None, nu=5) == E_DIM
    assert nd(True, g_cost=None, g_x=None, tape_bytes=0) == E_ARG
  # the scratch queries are the siblings' (no seeded variant: the scratch does not grow)
  assert not any("scratch_bytes" in n and "seeded" in n for n in _lib.SIGNATURES)


@pytest.mark.parametrize("name", ["C", "P"])
def test_closure_on_cpu_tensors_accepts_native_objective(name):
  """On CPU tensors the closure runs the torch composition whatever native_objective says."""
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _sys(name, 37)
  system, gaussian, _ = tm._torch_system(sy, "cpu")
  x0 = torch.tensor(sy["x0"], dtype=F64)
  tp = tm._TorchPaths(sy["paths"], sy["drift"])
  for objective in (_quadratic(sy["ne"], "cpu"), gaussian):
    with torch.no_grad(), warnings.catch_warnings():
      warnings.simplefilter("error")
      l_def = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, paths=tp)()
      l_opt = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, paths=tp, native_objective=True,
                                           **ROUTE[name])()
    assert l_def.shape == (37,) and torch.isfinite(l_def).all() and torch.equal(l_def, l_opt)


def _cpu_gradients(name, reverse):
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy = _sys(name, 37)
  system, _, pm = tm._torch_system(sy, "cpu")
  groups = tm._policy_params(pm, sy["nu"])
  flat = [(f"{k}[{a}]", t) for k, ts in groups.items() for a, t in enumerate(ts)]
  for _, t in flat:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, requires_grad=True)
  tp = tm._TorchPaths(sy["paths"], sy["drift"])
  loss = pathwise_policy_loss_closure(system, _quadratic(sy["ne"], "cpu", reverse=reverse), lambda: x0, H6, dt=DT, paths=tp,
                                      native=False)()
  loss.mean().backward()
  return {k: t.grad.detach().clone() for k, t in flat + [("x0", x0)]}


@pytest.mark.parametrize("name", ["C", "P", "Q"])
def test_reversed_time_weights_move_every_gradient_of_the_comparator(name):
  """Timing guard, on the comparator alone (the CPU torch composition): with the time weights of steps 1 .. H reversed every
  gradient tensor -- each policy parameter and x0 -- moves by at least 10 x the gradient bar, so a sweep that applied seed block
  h to x_h instead of x_{h+1} could not pass the GPU comparison.  A condition on the inputs, not on the code under test."""
  fwd, rev = _cpu_gradients(name, False), _cpu_gradients(name, True)
  moved = {k: _rel(rev[k], fwd[k]) for k in fwd}
  print(f"timing guard {name}: smallest movement {min(moved.values()):.2e} ({min(moved, key=moved.get)})")
  for k, m in moved.items():
    assert float(fwd[k].abs().max()) > 0.0 and m >= 10 * GRAD_BAR, (k, m)


# ---- GPU: the entries --------------------------------------------------------------------------------------------------------------
def _seeded_entry(roll, tape, g_cost, g_x, H, want_state_grad=True):
  """The seeded entry itself, also with a NULL g_x (``PolicyRollout.backward`` sends g_states=None to the unseeded one)."""
  return roll._sweep(roll.policy, tape, g_cost, g_x, H, DT, want_state_grad, seeded=True)


def _taped(name, S, dtype, device):
  sy = _sys(name, S)
  _, _, roll = _device_case(name, sy, device, dtype)
  assert roll.nd_entries == (name != "C") and roll.wide == (name == "W2") and roll.supports_backward()
  x0 = torch.tensor(sy["x0"], dtype=dtype, device=device)
  _, tape = roll(x0, H6, dt=DT, with_jacobians=True)
  g = torch.Generator(device="cpu").manual_seed(11)
  w = torch.randn(H6, S, dtype=F64, generator=g).to(device)
  return sy, roll, tape, w


def _blocks(roll, g_pol, g_x0):
  """The gradient as named tensors: per latent dZ, dbeta, d ls^2, dvar, dmean of the packed policy, and g_x0."""
  M, ne = roll.policy.M, roll.ne
  g = g_pol.reshape(roll.nu, -1)
  out = {}
  for a in range(roll.nu):
    out[f"dZ[{a}]"], out[f"dbeta[{a}]"] = g[a, :M * ne], g[a, M * ne:M * ne + M]
    out[f"dls2[{a}]"], out[f"dvar[{a}]"], out[f"dmean[{a}]"] = g[a, M * ne + M:M * ne + M + ne], g[a, M * ne + M + ne], g[a, M * ne + M + ne + 1]
  out["x0"] = g_x0
  return out


CASES = [(n, S) for n in ("C", "P", "W2") for S in (37, 300)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,S", CASES)
def test_gpu_seeded_entry_with_a_null_seed_is_the_unseeded_entry(name, S, dtype, device):
  """Bit-equality of the seeded entry with g_x = NULL and the unseeded entry on one tape.  With g_x NULL and g_cost given the host
  launches the same unseeded kernel instantiation for both, so this checks the seeded entries' argument plumbing and dispatch
  only; the seeded kernel code is covered by test_gpu_seed_identity_of_the_built_in_cost and the closure tests below."""
  sy, roll, tape, w = _taped(name, S, dtype, device)
  gp0, gx0 = roll.backward(tape, w, H6, dt=DT, want_state_grad=True)
  gp1, gx1 = _seeded_entry(roll, tape, w, None, H6)
  assert torch.equal(gp0, gp1) and torch.equal(gx0, gx1)
  assert float(gp0.abs().max()) > 0.0 and float(gx0.abs().max()) > 0.0 and torch.isfinite(gp0).all()
  gp2, _ = _seeded_entry(roll, tape, w, None, H6, want_state_grad=False)           # g_x0 stays optional
  assert torch.equal(gp0, gp2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,S", CASES)
def test_gpu_seed_identity_of_the_built_in_cost(name, S, dtype, device):
  """The built-in cost's own gradient w.r.t. the taped states, computed in torch f64 from the tape, fed back as the seed with
  g_cost = NULL, gives the unseeded sweep's gradient: the step index and the idle lanes of the seed, independent of any torch
  autograd of the rollout.  Also through ``PolicyRollout.backward(g_states=...)``, and seeds and g_cost together are their sum."""
  sy, roll, tape, w = _taped(name, S, dtype, device)
  want = _blocks(roll, *roll.backward(tape, w, H6, dt=DT, want_state_grad=True))
  xs = roll.trajectory(tape, H6)
  assert xs.shape == (H6, S, sy["nx"]) and torch.equal(xs, roll.states(tape, H6)[1:])
  x = xs.double().clone().requires_grad_(True)
  active = list(sy["active"])
  inactive = [i for i in range(sy["nx"]) if i not in active]
  e = torch.cat([torch.sin(x[..., active]), torch.cos(x[..., active]), x[..., inactive]], dim=-1)
  err = e - roll.target.double()
  c = -torch.exp(-0.5 * ((err @ roll.precis.double().T) * err).sum(-1))            # [H, S]: block h is the cost of x_{h+1}
  (g_x,) = torch.autograd.grad((w * c).sum(), x)
  got = _blocks(roll, *_seeded_entry(roll, tape, None, g_x, H6))
  worst = 0.0
  for k in want:
    assert float(want[k].abs().max()) > 0.0, k
    r = _rel(got[k], want[k])
    worst = max(worst, r)
    assert r < GRAD_BAR, (k, r)
  print(f"seed identity {name} S={S} {dtype}: worst tensor {worst:.2e} of its largest entry")
  api = roll.backward(tape, None, H6, dt=DT, want_state_grad=True, g_states=g_x)
  assert all(torch.equal(a, b) for a, b in zip(api, _seeded_entry(roll, tape, None, g_x, H6)))
  both = _blocks(roll, *roll.backward(tape, w, H6, dt=DT, want_state_grad=True, g_states=g_x))
  for k in want:
    assert _rel(both[k], 2.0 * want[k]) < GRAD_BAR, k
  with pytest.raises(ValueError):
    roll.backward(tape, None, H6, dt=DT)
  with pytest.raises(ValueError):
    roll.backward(tape, None, H6, dt=DT, g_states=g_x[:-1])


# ---- GPU: the closure ------------------------------------------------------------------------------------------------------------
def _closure_case(name, S, device):
  sy = _sys(name, S)
  gp_paths, _, _ = _device_case(name, sy, device, F64)
  system, gaussian, pm = _torch_system(name, sy, device)
  params = [t for ts in tm._policy_params(pm, sy["nu"]).values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)
  return sy, system, gaussian, gp_paths, params, x0


def _run(system, objective, paths, leaves, x0, **kw):
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  for t in leaves:
    t.grad = None
  loss = pathwise_policy_loss_closure(system, objective, lambda: x0, H6, dt=DT, paths=paths, **kw)()
  loss.mean().backward()
  return loss.detach(), [t.grad.detach().clone() for t in leaves]


CLOSURE_CASES = [("C", 37), ("P", 37), ("P", 300), ("W2", 37), ("M0", 37)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,S", CLOSURE_CASES)
def test_gpu_closure_runs_a_custom_objective_natively_when_asked(name, S, device):
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  sy, system, _, paths, params, x0 = _closure_case(name, S, device)
  obj = _quadratic(sy["ne"], device)
  kw = dict(native_objective=True, **ROUTE[name])
  leaves = params + [x0]
  with warnings.catch_warnings():
    warnings.simplefilter("error")                                                 # no fall-back
    ln, gn = _run(system, obj, paths, leaves, x0, **kw)
    lf, _ = _run(system, obj, paths, leaves, x0, native=True, **kw)                # native=True does not raise
    with torch.no_grad():
      l0 = pathwise_policy_loss_closure(system, obj, lambda: x0.detach(), H6, dt=DT, paths=paths, **kw)()
    lt, gt = _run(system, obj, paths, leaves, x0, native=False)
  assert ln.shape == (S,) and torch.equal(ln, lf)
  el = float((ln - lt).abs().max())
  eg = [_rel(a, b) for a, b in zip(gn, gt)]
  print(f"closure {name} S={S}: native objective route vs torch composition, loss {el:.2e}, gradients {max(eg):.2e}")
  assert el < LOSS_BAR
  for b, e in zip(gt, eg):
    assert float(b.abs().max()) > 0.0 and e < GRAD_BAR, e
  assert float((l0 - ln).abs().max()) < 1e-12
  # the objective's own parameter: its gradient comes from the torch part
  obj.W.requires_grad_(True)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    lw, gw = _run(system, obj, paths, leaves + [obj.W], x0, **kw)
    ltw, gtw = _run(system, obj, paths, leaves + [obj.W], x0, native=False)
    # ... also when nothing else requires a gradient: the rollout runs forward only, its states are constants
    for t in params:
      t.requires_grad_(False)
    (go,) = torch.autograd.grad(pathwise_policy_loss_closure(system, obj, lambda: x0.detach(), H6, dt=DT, paths=paths, **kw)().mean(),
                                obj.W)
    for t in params:
      t.requires_grad_(True)
  assert float((lw - ltw).abs().max()) < LOSS_BAR
  for a, b in zip(gw, gtw):
    assert _rel(a, b) < GRAD_BAR
  assert float(gtw[-1].abs().max()) > 0.0 and _rel(go, gtw[-1]) < GRAD_BAR
  obj.W.requires_grad_(False)
  # with the option off: today's warning, once, and exactly the torch composition's numbers
  with pytest.warns(RuntimeWarning, match=r"objective QuadraticObjective \(the native rollout implements GaussianObjective\)") as rec:
    closure = pathwise_policy_loss_closure(system, obj, lambda: x0, H6, dt=DT, paths=paths, **ROUTE[name])
    for t in leaves:
      t.grad = None
    ld = closure()
    ld.mean().backward()
    gd = [t.grad.detach().clone() for t in leaves]
    closure()
  assert len([w_ for w_ in rec if issubclass(w_.category, RuntimeWarning)]) == 1
  assert torch.equal(ld.detach(), lt) and all(torch.equal(a, b) for a, b in zip(gd, gt))


@pytest.mark.gpu
@pytest.mark.parametrize("name,S", CLOSURE_CASES)
def test_gpu_closure_gaussian_objectives_under_native_objective(name, S, device):
  """A GaussianObjective with a trainable target takes the trajectory route and matches the torch composition; a constant one keeps
  the in-kernel cost: bit-equal to the run without the option."""
  sy, system, gaussian, paths, params, x0 = _closure_case(name, S, device)
  leaves = params + [x0]
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    l1, g1 = _run(system, gaussian, paths, leaves, x0, native_objective=True, **ROUTE[name])
    l2, g2 = _run(system, gaussian, paths, leaves, x0, **ROUTE[name])
  assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2)) and float(g1[0].abs().max()) > 0.0
  trained = GaussianObjective(target=gaussian.target.detach().clone().requires_grad_(True), precis=gaussian.precis)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    ln, gn = _run(system, trained, paths, leaves + [trained.target], x0, native_objective=True, **ROUTE[name])
    lt, gt = _run(system, trained, paths, leaves + [trained.target], x0, native=False)
  assert float((ln - lt).abs().max()) < LOSS_BAR
  for a, b in zip(gn, gt):
    assert float(b.abs().max()) > 0.0 and _rel(a, b) < GRAD_BAR
  # the option off: the pinned message and the torch composition
  with pytest.warns(RuntimeWarning, match="objective.target requires a gradient"):
    ld, gd = _run(system, trained, paths, leaves + [trained.target], x0, **ROUTE[name])
  assert torch.equal(ld, lt) and all(torch.equal(a, b) for a, b in zip(gd, gt))


# ---- GPU: determinism and capture -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C", "P"])
def test_gpu_trajectory_function_outputs_and_two_backward_passes(name, device):
  from gpflowpilco_amd.pathwise import PolicyRolloutFunction, PolicyTrajectoryFunction
  S = 37
  sy = _sys(name, S)
  _, pm, roll = _device_case(name, sy, device, F64)
  params = [t for ts in tm._policy_params(pm, sy["nu"]).values() for t in ts]
  for t in params:
    t.requires_grad_(True)
  x0 = torch.tensor(sy["x0"], dtype=F64, device=device, requires_grad=True)
  obj = _quadratic(sy["ne"], device)
  enc = TrigonometricEncoder(active_dims=sy["active"])
  Zp, lsp, varp, betap, _, mcp = pm.precompute(device)
  cost, xs = PolicyTrajectoryFunction.apply(x0, Zp, lsp, varp, betap, mcp, roll, H6, DT)
  cost1 = PolicyRolloutFunction.apply(x0, Zp, lsp, varp, betap, mcp, roll, H6, DT)
  with torch.no_grad():
    _, tape = roll(x0.detach(), H6, dt=DT, with_jacobians=True)
  assert cost.shape == (S, H6) and xs.shape == (H6, S, sy["nx"]) and torch.equal(cost, cost1)
  assert torch.equal(xs, roll.trajectory(tape, H6)) and xs.requires_grad
  e = enc(xs)
  loss = sum(obj(x=e[h], t=DT * (h + 1)) for h in range(H6)).mean()
  a = torch.autograd.grad(loss, params + [x0], retain_graph=True)
  b = torch.autograd.grad(loss, params + [x0], retain_graph=True)
  assert all(torch.equal(u, v) for u, v in zip(a, b)) and all(float(u.abs().max()) > 0.0 for u in a)
  # either output alone, and both: the sweep is linear in its seeds
  only_cost = torch.autograd.grad(cost.sum(), params + [x0], retain_graph=True)
  plain = torch.autograd.grad(cost1.sum(), params + [x0], retain_graph=True)
  assert all(torch.equal(u, v) for u, v in zip(only_cost, plain))
  both = torch.autograd.grad(loss + cost.sum(), params + [x0], retain_graph=True)
  for u, v, w_ in zip(both, a, only_cost):
    assert float((u - v - w_).abs().max()) <= 1e-12 * max(float(v.abs().max()), float(w_.abs().max()))
  # the states output is a copy: editing it in place does not reach the tape the backward reads
  cost2, xs2 = PolicyTrajectoryFunction.apply(x0, Zp, lsp, varp, betap, mcp, roll, H6, DT)
  with torch.no_grad():
    xs2.zero_()
  edited = torch.autograd.grad(cost2.sum(), params + [x0])
  assert all(torch.equal(u, v) for u, v in zip(edited, plain))


@pytest.mark.gpu
def test_gpu_graphed_custom_objective_replays_eager(device):
  from gpflowpilco_amd.loops import GraphedPolicyLoss, pathwise_policy_loss_closure
  sy, system, _, paths, params, x0 = _closure_case("P", 37, device)
  x0 = x0.detach()
  obj = _quadratic(sy["ne"], device)
  q_mu = params[0]
  for t in params[1:]:
    t.requires_grad_(False)
  closure = pathwise_policy_loss_closure(system, obj, lambda: x0, H6, dt=DT, paths=paths, native=True, native_actions=4,
                                         native_objective=True)
  graphed = GraphedPolicyLoss(closure, [q_mu])
  for _ in range(2):
    q_mu.grad = None
    le = closure(); le.sum().backward()
    ge = q_mu.grad.detach().clone(); le = le.detach().clone()
    lg, (gg,) = graphed.loss_and_grad()
    assert torch.allclose(lg, le, rtol=1e-12, atol=1e-14) and torch.allclose(gg, ge, rtol=1e-10, atol=1e-13)
    assert torch.allclose(graphed.loss(), le, rtol=1e-12, atol=1e-14)
    with torch.no_grad():
      q_mu.mul_(0.9)
      x0.add_(0.01)
  graphed.check()
