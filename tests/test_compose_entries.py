"""The three entry families of ``ops.ComposedRollout`` (one action, ``_nd``, ``_nd_mixed``) share one Python call path: what that
can get wrong is an argument list.  Without a GPU: every (entry, arguments) pair the wrapper assembles fits the entry's ctypes
signature and passes the loaded library's own argument checks as far as the one buffer left too small; the composed
``_lib.SIGNATURES`` equal a written-out snapshot; the two loss closures keep their fall-back texts."""
import ctypes as C
import warnings

import pytest
import torch

from gpflowpilco_amd import _lib, loops, ops
from gpflowpilco_amd import bijectors as tfb
from gpflowpilco_amd import dynamics, models as gp
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
from tests.helpers import gp_model_from_oracle, random_svgp_params

F64 = torch.float64
NX, ACTIVE, LG, B, H = 4, (1,), 3, 3, 4
MD, MP = 40, 12
FLAGS_DRIFT, FLAGS_POLICY = _lib.MM_FULL_OUTPUT_COV | _lib.MM_MODEL_UNCERTAINTY, _lib.MM_FULL_OUTPUT_COV
MM_E_WORKSPACE, MM_E_STATE = -4, -6

# ---- the signatures of the eleven composed-rollout entries, as written out before they were composed from their pieces ---------
_T = {"c_void_p": C.c_void_p, "c_size_t": C.c_size_t, "c_int": C.c_int, "c_double": C.c_double,
      "POINTER(c_int32)": C.POINTER(C.c_int32), "POINTER(c_double)": C.POINTER(C.c_double)}
SNAPSHOT = {
    "mm_rollout_composed": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_double c_double c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p "
        "c_size_t c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p"),
    "mm_rollout_composed_nd": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_int POINTER(c_double) POINTER(c_double) c_void_p c_void_p c_void_p c_void_p c_void_p "
        "c_void_p c_void_p c_void_p c_size_t c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p"),
    "mm_rollout_composed_taped": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_double c_double c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_size_t c_void_p "
        "c_size_t c_void_p c_size_t c_void_p c_void_p"),
    "mm_rollout_composed_backward": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_double c_double c_void_p c_void_p c_void_p c_size_t c_void_p c_void_p c_void_p c_void_p "
        "c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p"),
    "mm_rollout_composed_backward_seeded": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_double c_double c_void_p c_void_p c_void_p c_size_t c_void_p c_void_p c_void_p c_void_p "
        "c_void_p c_void_p c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p"),
    "mm_rollout_composed_taped_nd": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_int POINTER(c_double) POINTER(c_double) c_void_p c_void_p c_void_p c_void_p c_void_p "
        "c_void_p c_size_t c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p"),
    "mm_rollout_composed_backward_nd": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_int POINTER(c_double) POINTER(c_double) c_void_p c_void_p c_void_p c_size_t c_void_p "
        "c_void_p c_void_p c_void_p c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p"),
    "mm_rollout_composed_backward_nd_seeded": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_int POINTER(c_double) POINTER(c_double) c_void_p c_void_p c_void_p c_size_t c_void_p "
        "c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p"),
    "mm_rollout_composed_nd_mixed": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_int POINTER(c_double) POINTER(c_double) c_void_p c_void_p c_void_p c_void_p c_void_p "
        "c_void_p c_void_p c_void_p c_size_t c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p c_void_p c_void_p"),
    "mm_rollout_composed_taped_nd_mixed": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_int POINTER(c_double) POINTER(c_double) c_void_p c_void_p c_void_p c_void_p c_void_p "
        "c_void_p c_size_t c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p c_void_p c_void_p"),
    "mm_rollout_composed_backward_nd_mixed": ("c_int",
        "c_void_p c_size_t c_int c_int c_int c_void_p c_size_t c_int c_int c_int c_int c_int c_double c_int c_int "
        "POINTER(c_int32) c_int POINTER(c_double) POINTER(c_double) c_void_p c_void_p c_void_p c_size_t c_void_p "
        "c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_size_t c_void_p c_size_t c_void_p c_void_p c_void_p"),
}


def test_composed_signatures_equal_the_snapshot():
  composed = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith("mm_rollout_composed")}
  want = {k: (_T[res], [_T[t] for t in args.split()]) for k, (res, args) in SNAPSHOT.items()}
  assert len(want) == 11 and set(composed) == set(want)
  for k, (res, args) in want.items():
    assert composed[k][0] is res, k
    assert list(composed[k][1]) == args, k


# ---- argument assembly on stub packs ---------------------------------------------------------------------------------------------
ENTRIES = {
    "one": dict(forward="mm_rollout_composed", taped="mm_rollout_composed_taped", backward="mm_rollout_composed_backward",
                seeded="mm_rollout_composed_backward_seeded"),
    "nd": dict(forward="mm_rollout_composed_nd", taped="mm_rollout_composed_taped_nd", backward="mm_rollout_composed_backward_nd",
               seeded="mm_rollout_composed_backward_nd_seeded"),
    "nd_mixed": dict(forward="mm_rollout_composed_nd_mixed", taped="mm_rollout_composed_taped_nd_mixed",
                     backward="mm_rollout_composed_backward_nd_mixed", seeded="mm_rollout_composed_backward_nd_mixed"),
}
CASES = [("one", 1), ("nd", 1), ("nd", 2), ("nd_mixed", 1), ("nd_mixed", 2)]
SCALES, SHIFTS = (2.0, 1.5), (-0.5, -0.4)


class _Pack:
  """What ``ComposedRollout`` reads of a ``PackedModel``, on host memory of the packed size."""

  def __init__(self, L, M, d, with_C):
    self.L, self.M, self.d, self.with_C, self.dtype = L, M, d, with_C, F64
    self.nbytes = _lib.lib().mm_packed_model_bytes(L, M, d, _lib.MM_F64, int(with_C))
    assert self.nbytes > 0
    self.buf = torch.zeros(self.nbytes, dtype=torch.uint8)
    self.device = self.buf.device


def _rollout(family, nu):
  mixed = family == "nd_mixed"
  ne = NX + len(ACTIVE)
  drift, policy = _Pack(LG if mixed else NX, MD, ne + nu, True), _Pack(nu, MP, ne, False)
  head = dict(head_scale=SCALES[0], head_shift=SHIFTS[0]) if nu == 1 else dict(head_scale=SCALES, head_shift=SHIFTS)
  mix = dict(mix_W=torch.ones(NX, LG, dtype=F64), mix_c=torch.zeros(NX, dtype=F64)) if mixed else {}
  return ops.ComposedRollout(drift, policy, nx=NX, active_dims=ACTIVE, target=torch.zeros(ne, dtype=F64),
                             precis=torch.eye(ne, dtype=F64), **head, **mix)


def _calls(roll, family, short=None):
  """role -> (entry, arguments) as the wrapper assembles them, on host buffers of exactly the sizes the entries ask for
  (``short``: that buffer one byte smaller); and the buffers, to be kept alive over a call."""
  lib, fam, code = _lib.lib(), ops._COMPOSED[family], _lib.MM_F64
  d, p = roll.drift, roll.policy
  n = dict(wd=lib.mm_workspace_bytes(B, d.L, d.M, d.d, code, FLAGS_DRIFT), wp=lib.mm_workspace_bytes(B, p.L, p.M, p.d, code, FLAGS_POLICY),
           wc=roll._bytes(fam, "compose_ws", (B,), (code,)), tape=roll._tape_bytes(fam, B, H, code),
           wb=roll._backward_ws_bytes(fam, B, p.M))
  assert all(v > 0 for v in n.values()), n
  if short is not None:
    n[short] -= 1
  t = {k: torch.zeros(v, dtype=torch.uint8) for k, v in n.items()}
  z = lambda *shape: torch.zeros(*shape, dtype=F64)
  npar = p.M * p.d + p.M + p.d + 2
  t.update(mx=z(B, NX), Sxx=z(B, NX, NX), cost=z(H, B), tmu=z(H, B, NX), tS=z(H, B, NX, NX), g_cost=z(H, B), g_xm=z(H, B, NX),
           g_xS=z(H, B, NX, NX), g_pol=z(B, roll.nu, npar), g_m=z(B, NX), g_S=z(B, NX, NX), status=torch.zeros(4, dtype=torch.int32))
  fwd = lambda tmu, tS: roll._forward_call(fam, p, B, H, 1.0, t["mx"], t["Sxx"], t["cost"], tmu, tS, t["wd"], t["wp"], t["wc"],
                                           t["status"], None)
  sweep = lambda seeds: roll._sweep_call(fam, p, B, H, 1.0, t["tape"], t["g_cost"], seeds, t["g_pol"], t["g_m"], t["g_S"], t["wd"],
                                         t["wb"], t["status"], None)
  calls = {"forward": fwd(None, None), "forward_traj": fwd(t["tmu"], t["tS"]),
           "taped": roll._taped_call(fam, p, B, H, 1.0, t["mx"], t["Sxx"], t["cost"], t["wd"], t["wp"], t["tape"], t["status"], None),
           "backward": sweep(None), "seeded": sweep((t["g_xm"], t["g_xS"])), "null_seeds": sweep((None, None))}
  return calls, t


@pytest.mark.parametrize("family,nu", CASES)
def test_assembled_arguments_fit_the_signatures(family, nu):
  roll = _rollout(family, nu)
  calls, t = _calls(roll, family)
  names = ENTRIES[family]
  pairs = lambda *keys: tuple(v for k in keys for v in (t[k].data_ptr(), t[k].numel()))        # (pointer, bytes) per buffer
  for role, (entry, args) in calls.items():
    assert entry == names[{"forward_traj": "forward", "null_seeds": "seeded"}.get(role, role)], role
    assert entry in _lib.SIGNATURES
    argtypes = _lib.SIGNATURES[entry][1]
    assert len(args) == len(argtypes), (entry, len(args), len(argtypes))
    for i, (a, ty) in enumerate(zip(args, argtypes)):
      try:
        ty.from_param(a)
      except (TypeError, C.ArgumentError) as e:
        raise AssertionError(f"{entry}: argument {i} = {a!r} is no {ty.__name__}") from e
    # the places a suffix changes: dims, head constants, what follows g_cost, what trails
    assert args[:5] == (roll.drift.buf.data_ptr(), roll.drift.nbytes, roll.drift.L, MD, NX + len(ACTIVE) + nu)
    assert args[5:9] == (roll.policy.buf.data_ptr(), roll.policy.nbytes, MP, NX + len(ACTIVE))
    assert args[9:15] == (_lib.MM_F64, B, H, 1.0, NX, len(ACTIVE)) and list(args[15]) == list(ACTIVE)
    if family == "one":
      assert args[16:18] == (SCALES[0], SHIFTS[0])
      body = 18
    else:
      assert args[16] == nu and list(args[17]) == list(SCALES[:nu]) and list(args[18]) == list(SHIFTS[:nu])
      body = 19
    assert args[body:body + 2] == (roll.target.data_ptr(), roll.precis.data_ptr())
    mixing = (roll.mix_W.data_ptr(), roll.mix_c.data_ptr()) if family == "nd_mixed" else ()
    if role in ("backward", "seeded", "null_seeds"):
      assert args[body + 2:body + 5] == (t["tape"].data_ptr(), t["tape"].numel(), t["g_cost"].data_ptr())
      after = {"backward": (None, None) if mixing else (), "null_seeds": (None, None),
               "seeded": (t["g_xm"].data_ptr(), t["g_xS"].data_ptr())}[role]        # (the mixed sweep has the seeded signature only)
      assert args[body + 5:body + 5 + len(after)] == after
      rest = body + 5 + len(after)
      assert args[rest:rest + 3] == (t["g_pol"].data_ptr(), t["g_m"].data_ptr(), t["g_S"].data_ptr())
      assert args[rest + 3:rest + 9] == pairs("wd", "wb") + (t["status"].data_ptr(), None)
      assert args[len(args) - len(mixing[:1]):] == mixing[:1]
    else:
      assert args[body + 2:body + 5] == (t["mx"].data_ptr(), t["Sxx"].data_ptr(), t["cost"].data_ptr())
      if role == "taped":
        assert args[body + 5:body + 13] == pairs("wd", "wp", "tape") + (t["status"].data_ptr(), None)
      else:
        assert args[body + 5:body + 7] == ((t["tmu"].data_ptr(), t["tS"].data_ptr()) if role == "forward_traj" else (None, None))
        assert args[body + 7:body + 15] == pairs("wd", "wp", "wc") + (t["status"].data_ptr(), None)
      assert args[len(args) - len(mixing):] == mixing


@pytest.mark.parametrize("family,nu", CASES)
def test_library_takes_the_assembled_arguments_as_far_as_the_short_buffer(family, nu):
  """The library checks its arguments before any HIP call: with every buffer of the size its query names but one, a byte short,
  each entry gets as far as MM_E_WORKSPACE -- pointers, dtype, dims and the composition of the shapes are accepted -- and a
  drift d off by one is MM_E_STATE."""
  lib = _lib.lib()
  roll = _rollout(family, nu)
  for short, roles in (("wc", ("forward", "forward_traj")), ("tape", ("taped", "backward", "seeded", "null_seeds")),
                       ("wb", ("backward", "seeded", "null_seeds"))):
    calls, keep = _calls(roll, family, short)
    for role in roles:
      entry, args = calls[role]
      assert getattr(lib, entry)(*args) == MM_E_WORKSPACE, (entry, role, short)
      assert getattr(lib, entry)(*args[:4], args[4] + 1, *args[5:]) == MM_E_STATE, (entry, role)
    del keep


def test_the_public_methods_pick_the_families():
  one, nd, mixed = _rollout("one", 1), _rollout("nd", 2), _rollout("nd_mixed", 1)
  assert (one._family, one._nd_family) == (ops._COMPOSED["one"], ops._COMPOSED["nd"]) and not one.uses_nd
  assert nd._family is nd._nd_family is ops._COMPOSED["nd"] and nd.uses_nd
  assert mixed._family is mixed._nd_family is ops._COMPOSED["nd_mixed"] and mixed.uses_nd
  assert (one.scale, one.shift) == (SCALES[0], SHIFTS[0]) and (nd.scale, nd.shift) == (SCALES, SHIFTS)
  x, S, tape, g = torch.zeros(B, NX, dtype=F64), torch.zeros(B, NX, NX, dtype=F64), torch.zeros(8, dtype=torch.uint8), torch.zeros(H, B)
  for roll, text in ((nd, "one-action"), (mixed, "taped_nd / backward_nd")):
    with pytest.raises(NotImplementedError, match=text):
      roll.taped(x, S, H)
    with pytest.raises(NotImplementedError, match=text):
      roll.backward(tape, g, B, H)
  assert one.supports_backward() and not nd.supports_backward() and not mixed.supports_backward()
  for roll in (one, nd, mixed):                                               # the size queries need no GPU
    assert roll.backward_nd_refusal() is None and roll.supports_backward_nd()
    assert roll.tape_bytes_nd(B, H) == roll._tape_bytes(roll._nd_family, B, H, _lib.MM_F64) > 0


# ---- the loss closures' fall-back texts ------------------------------------------------------------------------------------------
def _cpu_system(scale, target_grad=False):
  ne = NX + len(ACTIVE)
  drift = gp_model_from_oracle(random_svgp_params(seed=1, L=NX, M=8, d=ne + 1, whiten=True, mean=False), "cpu")
  pol = gp_model_from_oracle(random_svgp_params(seed=2, L=1, M=6, d=ne, whiten=True, mean=False), "cpu")
  head = tfb.Chain([tfb.Scale(scale), tfb.Shift(-0.5), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=ACTIVE), solver=dynamics.MomentMatchingEuler())
  objective = GaussianObjective(target=torch.zeros(ne, dtype=F64).requires_grad_(target_grad), precis=torch.eye(ne, dtype=F64))
  return system, objective, head.bijectors


SWEEP_COVERS = "requires a gradient (the native reverse sweep covers the policy SVGP's parameters and the initial state"


def test_constants_that_require_a_gradient_keep_their_texts():
  mx = torch.zeros(B, NX, dtype=F64)
  for scale, target_grad, name in ((torch.tensor(2.0, dtype=F64, requires_grad=True), False, "the policy head's Scale.scale"),
                                   (2.0, True, "objective.target")):
    system, objective, bj = _cpu_system(scale, target_grad)
    fast = loops.native_policy_loss(system, objective, H)
    assert fast is not None
    assert fast.grad_obstacle(mx) == f"{name} {SWEEP_COVERS})"                                 # policy_loss_closure's reason
    assert loops._constants_grad_obstacle(bj, objective, False, "initial states") == f"{name} {SWEEP_COVERS}s)"    # the pathwise one
    # with native_objective the objective's own parameters are the torch part's: only the head's constants stand in the way
    assert loops._constants_grad_obstacle(bj, objective, True, "initial state") == (None if target_grad else f"{name} {SWEEP_COVERS})")
    assert loops._objective_uses_trajectory(objective, True) == target_grad and not loops._objective_uses_trajectory(objective, False)
  system, objective, bj = _cpu_system(2.0)
  assert loops._constants_grad_obstacle(bj, objective, False, "initial state") is None


@pytest.mark.parametrize("closure", ["policy_loss_closure", "pathwise_policy_loss_closure"])
def test_fallback_warns_once_with_the_closure_s_text(closure):
  warned = []
  with warnings.catch_warnings(record=True) as seen:
    warnings.simplefilter("always")
    loops._warn_fallback(warned, None, closure, "first reason")
    loops._warn_fallback(warned, True, closure, "second reason")
    loops._warn_fallback([], False, closure, "native=False says nothing")
  assert [str(w.message) for w in seen] == [f"{closure}: falling back to the torch composition of the rollout (first reason)"]
  assert seen[0].category is RuntimeWarning and warned == ["first reason"]
