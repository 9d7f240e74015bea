"""The rollout harness of ``MomentMatchingPILCO`` (``gpflow_pilco/loops/pilco.py:176-227``):
``policy_loss_closure`` builds the function whose value the policy optimiser minimises -- the
expected cost accumulated along a moment-matched rollout.  The RL orchestration around it
(data collection, checkpoints, optimisers) is out of scope."""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import contextlib
import functools
import warnings

import numpy as np
import torch

from .dynamics import DynamicalSystem, Euler, MomentMatchingEuler
from .moment_matching import GaussianMoments, moment_matching


def get_state_initializer(mean: torch.Tensor, covariance: torch.Tensor) -> Callable:
  """pilco.py:222-227: the initial state as moments with a leading batch axis."""
  mx = mean if mean.ndim > 1 else mean[None]
  Sxx = covariance if covariance.ndim > 2 else covariance[None]
  return lambda: (mx, Sxx)


def _native_parts(system: DynamicalSystem, objective: Callable, why: Optional[list], moment_solver: bool,
                  no_encoder: bool = False, any_objective: bool = False, coregionalized: bool = False):
  """The pieces the native rollouts are written for -- TrigonometricEncoder, policy = InverseLinkWrapper(KernelRegressor(SVGP with
  one latent per action, up to 4), Chain[Scale, Shift, NormalCDF]) with scale and shift a scalar or one value per action, SVGP
  drift, no diffusion, GaussianObjective (the cartpole wiring of ``examples/cartpole_swingup/swingup_loops.py:41-91``; two
  actions: the double pendulum) -- or None, with the reason appended to ``why``.  ``head_constants()`` returns two floats for
  one action and two tuples of nu floats for nu > 1.

  ``no_encoder``: also take ``encoder=None`` and ``TrigonometricEncoder(active_dims=())``, treated alike (the native entries with
  na = 0: the encoding is the identity); the encoder returned is then one without active dims.  ``any_objective``: also take an
  objective that is no ``GaussianObjective`` (the caller evaluates it on the native rollout's trajectory).  ``coregionalized``: also
  take a drift with a ``LinearCoregionalization`` kernel of no more latents than outputs (the caller mixes: ``_drift_mixing``); a
  coregionalised policy stays refused.  Without ``moment_solver`` a drift wrapped in a ``KernelRegressor`` (a mean-only drift)
  is looked through: the drift returned is the model inside."""
  from . import bijectors as tfb
  from .components import TrigonometricEncoder
  from .cost import GaussianObjective
  from .models import SVGP, InverseLinkWrapper, KernelRegressor, LinearCoregionalization, kernel_family
  enc, pol, drift = system.encoder, system.policy, system.drift
  if not moment_solver and isinstance(drift, KernelRegressor):
    # a mean-only drift under the Euler solver (the reference's model_uncertainty=False): the parts are those of the model
    # inside; the pathwise closure evaluates its mean (pathwise.MeanDrift).  The moment-matching closures keep refusing it below:
    # their native rollouts carry the model's uncertainty
    drift = drift.model

  def no(reason):
    if why is not None:
      why.append(reason)
    return None
  if system.diffusion is not None:
    return no("a diffusion term")
  if moment_solver and not isinstance(system.solver, MomentMatchingEuler):
    return no("a solver other than MomentMatchingEuler")
  if enc is None or (isinstance(enc, TrigonometricEncoder) and len(enc.active_dims) == 0):
    if not no_encoder:
      return no(f"encoder {type(enc).__name__} (the native rollout implements TrigonometricEncoder)" if enc is None else
                "a TrigonometricEncoder without active dims (native_no_encoder=True runs it natively)")
    enc = TrigonometricEncoder(active_dims=())
  if not isinstance(enc, TrigonometricEncoder):
    return no(f"encoder {type(enc).__name__} (the native rollout implements TrigonometricEncoder)")
  if not isinstance(objective, GaussianObjective) and not any_objective:
    return no(f"objective {type(objective).__name__} (the native rollout implements GaussianObjective)")
  if not isinstance(pol, InverseLinkWrapper) or not isinstance(pol.model, KernelRegressor):
    return no("the policy is not InverseLinkWrapper(KernelRegressor(SVGP))")
  pm_, head = pol.model.model, pol.invlink
  if not isinstance(pm_, SVGP) or not isinstance(drift, SVGP):
    return no("the policy or the drift is not an SVGP")
  try:
    pol_family, drift_family = kernel_family(pm_.latent_kernels), kernel_family(drift.latent_kernels)
  except (ValueError, NotImplementedError) as e:
    return no(str(e))
  if pol_family != 0:
    return no(f"a {type(pm_.latent_kernels[0]).__name__} policy (the native head kernels evaluate a SquaredExponential policy)")
  if moment_solver and drift_family != 0:
    return no(f"a {type(drift.latent_kernels[0]).__name__} drift (moment matching has closed forms for SquaredExponential only)")
  nu = int(pm_.num_latent_gps)
  if nu < 1 or nu > 4:
    return no(f"a policy with {nu} latents (the native rollout takes 1 to 4 actions)")
  if not coregionalized:
    if isinstance(pm_.kernel, LinearCoregionalization) or isinstance(drift.kernel, LinearCoregionalization):
      return no("a LinearCoregionalization kernel (its mixing stays on the host)")
  elif isinstance(pm_.kernel, LinearCoregionalization):
    return no("a coregionalised policy (a LinearCoregionalization kernel on the policy: the native mixing covers the drift only)")
  elif isinstance(drift.kernel, LinearCoregionalization):
    W = drift.kernel.W
    if W.ndim != 2 or W.shape[1] != int(drift.num_latent_gps):
      return no(f"a LinearCoregionalization drift whose W {tuple(W.shape)} does not match its {drift.num_latent_gps} latents")
    if W.shape[1] > W.shape[0]:
      return no(f"a coregionalised drift with more latents than outputs (Lg = {W.shape[1]} > nx = {W.shape[0]}: the native "
                "mixing takes Lg <= nx)")
  if any(k.active_dims is not None for k in pm_.latent_kernels + drift.latent_kernels):
    return no("a kernel with active_dims")
  bj = head.bijectors if isinstance(head, tfb.Chain) else None
  if not (bj and len(bj) == 3 and isinstance(bj[0], tfb.Scale) and isinstance(bj[1], tfb.Shift) and isinstance(bj[2], tfb.NormalCDF)):
    return no("the policy head is not Chain[Scale, Shift, NormalCDF]")

  memo = {}

  def _constant(v):
    # a tensor's values are read back once per version: the closures ask on every call, and a read-back from the device is not
    # allowed while a HIP graph is being captured (GraphedPolicyLoss warms up first)
    src = v if isinstance(v, torch.Tensor) else None
    if src is not None:
      hit = memo.get(id(src))
      if hit is not None and hit[0] is src and hit[1] == src._version:
        return hit[2]
    if isinstance(v, torch.Tensor):
      v = v.detach()
      v = float(v) if v.numel() == 1 else [float(t) for t in v.reshape(-1).tolist()]
    if nu == 1:
      out = float(v)
    else:
      out = tuple(float(t) for t in v) if isinstance(v, (list, tuple)) else (float(v),) * nu
      if len(out) != nu:
        raise ValueError("not one value per action")
    if src is not None:
      memo[id(src)] = (src, src._version, out)
    return out

  def head_constants():
    return _constant(bj[0].scale), _constant(bj[1].shift)
  try:
    head_constants()
  except (TypeError, ValueError, RuntimeError):
    return no("the policy head's scale / shift are neither scalars nor one value per action")
  return enc, pm_, drift, bj, head_constants


def _drift_mixing(drift):
  """``mixing(device) -> (W [nx, Lg], c [nx] | None)`` of a coregionalised drift as float64 device tensors, or None for any other
  drift.  The tensors are re-made when ``kernel.W`` or the Constant mean change in place (their ``_version``), as target / precision
  are re-read: a new pair makes ``native_policy_loss`` rebuild its rollout object."""
  from .models import Constant, LinearCoregionalization
  if not isinstance(drift.kernel, LinearCoregionalization):
    return None
  memo = {}

  def mixing(device):
    W = drift.kernel.W
    c = drift.mean_function.c if isinstance(drift.mean_function, Constant) else None
    key = (id(W), W._version, None if c is None else (id(c), c._version))
    hit = memo.get(str(device))
    if hit is None or hit[0] != key or hit[1] is not W:
      f64 = torch.float64
      Wd = W.detach().to(device=device, dtype=f64).clone().contiguous()
      cd = None if c is None else c.detach().to(device=device, dtype=f64).reshape(-1).clone().contiguous()
      hit = (key, W, Wd, cd)
      memo[str(device)] = hit
    return hit[2], hit[3]
  return mixing


def _pathwise_mixing_obstacle(drift, paths, grad: bool) -> Optional[str]:
  """Why the ``_mixed`` pathwise entries do not take these sample paths of a coregionalised ``drift`` (None: they do): the paths
  must carry the drift's mixing -- ``mix_W`` of W's shape, ``mix_c`` exactly when the mean is a ``Constant`` -- and, where a
  gradient is being taken (``grad``), W and the mean must be constants: the reverse sweep has no adjoint for them."""
  from .models import Constant
  W = drift.kernel.W
  c = drift.mean_function.c if isinstance(drift.mean_function, Constant) else None
  pW, pc = getattr(paths, "mix_W", None), getattr(paths, "mix_c", None)
  if pW is None:
    return "the given paths carry no mixing (mix_W) for the coregionalised drift"
  if tuple(pW.shape) != tuple(W.shape) or (pc is None) != (c is None) or (pc is not None and pc.shape[0] != W.shape[0]):
    return (f"the given paths carry a mixing of another shape than the drift's (mix_W {tuple(pW.shape)}, mix_c "
            f"{None if pc is None else tuple(pc.shape)}; the drift: W {tuple(W.shape)}, mean {None if c is None else tuple(c.shape)})")
  if grad and W.requires_grad:
    return "the drift's mixing matrix W requires a gradient (the native reverse sweep takes a frozen drift)"
  if grad and c is not None and c.requires_grad:
    return "the coregionalised drift's Constant mean requires a gradient (the native reverse sweep takes a frozen drift)"
  return None


def _objective_uses_trajectory(objective: Callable, native_objective: bool) -> bool:
  """The objective is evaluated in torch on the native rollout's trajectory (``native_objective``): one that is no
  ``GaussianObjective``, or one whose target / precision require a gradient while gradients are being taken."""
  from .cost import GaussianObjective
  if not native_objective:
    return False
  if not isinstance(objective, GaussianObjective):
    return True
  return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                         for t in (objective.target, objective.precis))


def _constants_grad_obstacle(bj, objective: Callable, native_objective: bool, state: str) -> Optional[str]:
  """The native reverse sweeps return gradients for the policy SVGP's parameters and the initial state(s) only: the head's Scale /
  Shift and the objective's target / precision enter as constants (float() / raw pointers).  -> the reason one of them that
  requires a gradient keeps the sweep out, or None.  ``state``: how the closure names what the sweep does cover ("initial state" /
  "initial states").  With ``native_objective`` the objective's own parameters are differentiated by the torch part -- and without
  it only a ``GaussianObjective`` gets this far (``_native_parts``), so .target / .precis exist; an objective of the caller's own
  has neither and is not asked for them."""
  outside = {"the policy head's Scale.scale": bj[0].scale, "the policy head's Shift.shift": bj[1].shift}
  if not native_objective:
    outside.update({"objective.target": objective.target, "objective.precis": objective.precis})
  for name, t in outside.items():
    if isinstance(t, torch.Tensor) and t.requires_grad:
      return f"{name} requires a gradient (the native reverse sweep covers the policy SVGP's parameters and the {state})"
  return None


def _warn_fallback(warned: list, native: Optional[bool], closure: str, reason: str):
  """The torch composition is about to run on GPU tensors (60 x slower than the native path at cartpole sizes): say so, once per
  closure (``warned``: its record).  Bind it with ``functools.partial`` -- no frame of its own, so the warning points where the
  closures' own helpers always pointed."""
  if native is not False and not warned:
    warned.append(reason)
    warnings.warn(f"{closure}: falling back to the torch composition of the rollout ({reason})", RuntimeWarning, stacklevel=3)


def native_policy_loss(system: DynamicalSystem, objective: Callable, num_steps: int, dt: float = 1.0,
                       why: Optional[list] = None, native_actions: int = 1, native_no_encoder: bool = False,
                       native_objective: bool = False, native_coregionalized: bool = False, native_wide: bool = False):
  """``f(mx, Sxx) -> loss [B]`` running the whole rollout in ``mm_rollout_composed`` (csrc/mm_compose.hip), or None
  when the system is not the shape that entry point implements: TrigonometricEncoder, policy =
  InverseLinkWrapper(KernelRegressor(SVGP with one latent per action), Chain[Scale, Shift, NormalCDF]), SVGP drift, no
  diffusion, MomentMatchingEuler, GaussianObjective -- the cartpole wiring of
  ``examples/cartpole_swingup/swingup_loops.py:41-91``; a policy with 2 to 4 actions runs in ``mm_rollout_composed_nd``
  (csrc/mm_compose_nd.hip).  ``f.with_grad(mx, Sxx)`` is the same loss as a differentiable op
  (native reverse sweep, csrc/mm_compose_bwd.hip) where ``f.supports_grad(mx)``: one action only by default.  ``why``: a list that
  receives the reason when None is returned.

  ``native_actions``: the largest number of actions ``with_grad`` may differentiate natively.  The default 1 keeps a policy with
  several actions forward only (``grad_obstacle`` names ``nu > 1``); with ``native_actions >= nu`` its gradient runs through the
  multi-action tape and reverse sweep (csrc/mm_compose_bwd_nd.hip, ``autodiff.ComposedRolloutFunction``) where
  ``ComposedRollout.backward_nd_refusal`` has no objection.

  ``native_no_encoder``: take a system with ``encoder=None`` (or a ``TrigonometricEncoder`` without active dims) too: the native
  entries with na = 0; the cost is the objective of the raw state (``GaussianObjective.target`` is [nx]).

  ``native_objective``: take any objective.  One that is no ``GaussianObjective``, or a ``GaussianObjective`` whose target /
  precision require a gradient, is evaluated in torch on the trajectory of the native rollout (``f.uses_trajectory(mx)``):
  ``autodiff.ComposedTrajectoryFunction`` returns the H states as differentiable outputs, the loss is the reference's accumulation
  ``objective(x = encoder match of x_t, t = t)`` over them, and the seeded reverse sweep carries its gradient back to the policy
  and the initial state; the objective's own parameters get theirs from the torch part.

  ``native_coregionalized``: take a drift with a ``LinearCoregionalization`` kernel of Lg <= nx latents too: its mixing f = W g + c
  runs on the device after every drift match (csrc/mm_mix.h) and the rollout -- one action included -- goes through the
  ``_nd_mixed`` entries, forward and gradient (``ComposedRolloutFunction`` / ``ComposedTrajectoryFunction``).  W and the Constant
  mean are constants of the frozen drift, re-read when they change in place.

  ``native_wide``: let ``with_grad`` differentiate a rollout with 8 < ne <= 16 encoded dims natively too, through the tapes of the
  ``_nd`` family and the wide reverse sweep (``mm_compose_wide_backward*``, ``ComposedRollout.backward_wide_refusal``); the other
  options keep their meaning there (``native_actions`` still decides nu > 1).  ne <= 8 is routed as without it."""
  from . import ops
  wide = bool(native_wide)
  parts = _native_parts(system, objective, why, moment_solver=True, no_encoder=bool(native_no_encoder),
                        any_objective=bool(native_objective), coregionalized=bool(native_coregionalized))
  if parts is None:
    return None
  enc, pm_, drift, bj, head_constants = parts
  mixing = _drift_mixing(drift)
  max_native = int(native_actions)
  cache = {}
  zero_cost = {}

  def cost_constants(mx, zero):
    """(target, precis) of the rollout's built-in cost: the objective's, or zeros where the trajectory route ignores that cost."""
    if not zero:
      return objective.target, objective.precis
    key = (mx.dtype, str(mx.device))
    if key not in zero_cost:
      ne = mx.shape[-1] + len(enc.active_dims)
      zero_cost[key] = (torch.zeros(ne, dtype=mx.dtype, device=mx.device), torch.zeros(ne, ne, dtype=mx.dtype, device=mx.device))
    return zero_cost[key]

  def uses_trajectory(mx=None) -> bool:
    return _objective_uses_trajectory(objective, native_objective)

  def current_roll(mx: torch.Tensor, fresh_policy: bool = True, zero: bool = False):
    # (fresh_policy=False: the caller brings its own pack of the policy's current parameters -- the differentiable
    # path -- and the rollout object only has to have the right shapes: no re-pack of the policy here)
    # Everything the rollout reads is looked up on EVERY call: ``packed()`` re-packs a model whose parameters were
    # updated in place (optimiser step, refit between episodes: _PackCache keys on the tensors' versions), and the
    # head / objective constants are read from their owners.  Only the compose workspace is kept across calls.
    # (zero: the rollout of the trajectory route, built with a zero target / precision -- its cost output is ignored)
    key = (mx.dtype, str(mx.device), bool(zero))
    ent = cache.get(key)
    roll = None if ent is None else ent[0]
    pd = drift.packed(mx.dtype, True, mx.device)
    pp = roll.policy if (roll is not None and not fresh_policy) else pm_.packed(mx.dtype, False, mx.device)
    scale, shift = head_constants()
    target, precis = cost_constants(mx, zero)
    mix_W, mix_c = mixing(mx.device) if mixing is not None else (None, None)
    if (roll is None or roll.drift is not pd or roll.policy is not pp or roll.scale != scale or roll.shift != shift
        or ent[1] is not target or ent[2] is not precis or ent[3] != (target._version, precis._version)
        or (mixing is not None and (roll.mix_W is not mix_W or roll.mix_c is not mix_c))):
      new = ops.ComposedRollout(pd, pp, nx=mx.shape[-1], active_dims=enc.active_dims, head_scale=scale, head_shift=shift,
                                target=target, precis=precis, mix_W=mix_W, mix_c=mix_c)
      if roll is not None:
        new._wsc = roll._wsc                               # same shapes: the workspace carries over
      roll = new
      cache[key] = (roll, target, precis, (target._version, precis._version))
    return roll

  def objective_of_trajectory(xm: torch.Tensor, xS: torch.Tensor):
    """pilco.py:199-205 over the states x_1 .. x_H (xm [B, H, nx], xS [B, H, nx, nx]) at the unit-spaced times 1 .. H."""
    loss = torch.zeros(xm.shape[0], dtype=xm.dtype, device=xm.device)
    for h in range(num_steps):
      x = GaussianMoments(moments=(xm[:, h], xS[:, h]), centered=True)
      if system.encoder is not None:
        x = moment_matching(x, system.encoder).y
      loss = loss + objective(x=x, t=dt * float(h + 1))
    return loss

  def run(mx: torch.Tensor, Sxx: torch.Tensor, policy=None):
    if uses_trajectory(mx):
      roll = current_roll(mx, fresh_policy=policy is None, zero=True)
      _, _, _, tm, tS = roll(mx, Sxx, num_steps, dt=dt, keep_trajectory=True, policy=policy)
      return objective_of_trajectory(tm.transpose(0, 1), tS.transpose(0, 1))
    _, _, cost = current_roll(mx, fresh_policy=policy is None)(mx, Sxx, num_steps, dt=dt, policy=policy)
    return cost.sum(1)

  def run_with_grad(mx: torch.Tensor, Sxx: torch.Tensor):
    """The same loss as a differentiable function of the policy's parameters (and of the initial state): forward =
    the taped native rollout, backward = the native reverse sweep (autodiff.ComposedRolloutFunction); the policy enters
    in packed coordinates computed from its parameters by differentiable torch ops (a 30 x 30 precompute).  The tape and
    the reverse sweep are float64; a float32 state is cast up on the way in and the loss back down (autograd carries both)."""
    from .autodiff import ComposedRolloutFunction, ComposedTrajectoryFunction
    out_dtype = mx.dtype
    if mx.dtype != torch.float64:
      mx, Sxx = mx.double(), Sxx.double()
    traj = uses_trajectory(mx)
    roll = current_roll(mx, fresh_policy=False, zero=traj)
    roll.use_wide = wide and roll.ne > 8                   # (8 < ne <= 16: the tape of the _nd family and the wide reverse sweep)
    Zp, lsp, varp, betap, _, mcp = pm_.precompute(mx.device)
    if mcp is None:
      mcp = torch.zeros(roll.nu, dtype=Zp.dtype, device=mx.device)
    if traj:
      # the objective in torch on the H returned states; the rollout's own (zero-precision) cost is not part of the loss
      _, xm, xS = ComposedTrajectoryFunction.apply(mx, Sxx, Zp, lsp, varp, betap, mcp, roll, num_steps, dt)
      return objective_of_trajectory(xm, xS).to(out_dtype)
    # (several actions: native_actions >= nu; a coregionalised drift takes the _nd family with one action too: roll.uses_nd)
    cost = ComposedRolloutFunction.apply(mx, Sxx, Zp, lsp, varp, betap, mcp, roll, num_steps, dt)
    return cost.sum(1).to(out_dtype)

  def run_from_parameters(mx: torch.Tensor, Sxx: torch.Tensor):
    """Forward only, the policy packed from its parameters on the stream (no snapshot from outside): what a HIP-graph
    capture of the loss of a trainable policy must record, so that replays follow the optimiser's in-place updates."""
    with torch.no_grad():
      Zp, lsp, varp, betap, _, mcp = pm_.precompute(mx.device)
      pol = ops.pack_model(Zp, lsp, varp, betap, None, mcp, dtype=mx.dtype, sync=False)
      return run(mx, Sxx, policy=pol)
  run.from_parameters = run_from_parameters

  def grad_obstacle(mx: torch.Tensor) -> Optional[str]:
    """None when ``with_grad`` covers everything that asks for a gradient here, else the reason it does not."""
    if mx.dtype not in (torch.float32, torch.float64):
      return f"state dtype {mx.dtype}"
    nu = int(pm_.num_latent_gps)
    if nu > 1 and max_native <= 1:
      return (f"the policy has nu = {pm_.num_latent_gps} actions (nu > 1: the native rollout is forward only, its tape and "
              "reverse sweep are one-action)")
    if nu > max(1, max_native):
      return f"the policy has nu = {nu} actions (nu > 1) and native_actions = {max_native}"
    obstacle = _constants_grad_obstacle(bj, objective, native_objective, "initial state")
    if obstacle is not None:
      return obstacle
    if any(t.requires_grad for t in drift._parameters()) or (mixing is not None and drift.kernel.W.requires_grad):
      return "the drift is being trained (the native reverse sweep takes a frozen drift)"
    mx64 = mx if mx.dtype == torch.float64 else torch.empty(mx.shape, dtype=torch.float64, device=mx.device)
    roll = current_roll(mx64, fresh_policy=False, zero=uses_trajectory(mx))
    if wide and roll.ne > 8:
      return roll.backward_wide_refusal()
    if roll.uses_nd:
      return roll.backward_nd_refusal()
    if not roll.supports_backward():
      return (f"the policy has M = {roll.policy.M} centres on {roll.ne} encoded dims (the native reverse sweep takes "
              f"M <= {ops.ComposedRollout.BACKWARD_MAX_POLICY_M}, encoded dim <= 8)")
    return None

  def supports_grad(mx: torch.Tensor) -> bool:
    return grad_obstacle(mx) is None
  run.with_grad = run_with_grad
  run.supports_grad = supports_grad
  run.grad_obstacle = grad_obstacle
  run.uses_trajectory = uses_trajectory
  return run


def policy_loss_closure(system: DynamicalSystem, objective: Callable, state_initializer: Callable,
                        num_steps: int, initial_time: float = 0.0,
                        solution_times: Optional[Sequence[float]] = None, native: Optional[bool] = None,
                        native_actions: int = 1, native_no_encoder: bool = False, native_objective: bool = False,
                        native_coregionalized: bool = False, native_wide: bool = False, **kwargs) -> Callable:
  """pilco.py:176-220.  Returns ``closure() -> loss [B]``; ``system.solver`` should be a
  ``MomentMatchingEuler`` (pilco.py:141-144).

  ``native``: None (default) runs the rollout natively whenever the system has the shape ``mm_rollout_composed``
  implements (``native_policy_loss``) and the state is on the GPU: forward only (one ``mm_rollout_composed`` call) when
  nothing requires a gradient, and as ONE differentiable op -- taped forward + native reverse sweep
  (``autodiff.ComposedRolloutFunction``) -- when the policy's parameters or the initial state do (float64, frozen
  drift, one action; with several actions a gradient takes the torch composition, which differentiates through
  ``special.bvn_cdf``); False always takes the torch composition (``forward_sde`` over ``moment_matching``); True insists on the
  native path.

  ``native_actions``: the largest number of actions whose GRADIENT may run natively (a named parameter, not a solver option).
  The default 1 is the routing described above.  With ``native_actions >= nu`` a gradient of the policy SVGP's parameters and / or
  the initial state of a policy with 2 to 4 actions runs as one differentiable op too (``autodiff.ComposedRolloutFunction``: the
  multi-action tape and reverse sweep, csrc/mm_compose_bwd_nd.hip) -- frozen drift, constant head and objective, float64 tape
  (a float32 state is cast up), inside the sweep's LDS bound; every other case falls back once and names its reason.

  ``native_no_encoder``: with the default False a system without an encoder (``encoder=None``: mountain car,
  forward_sde.py:49-68) takes the torch composition as before (``native=True`` raises); True runs it natively, forward and
  gradient, through the entries' na = 0 form -- the cost is the objective of the raw state.  With an encoder present the option
  changes nothing.

  ``native_objective``: with the default False only a constant ``GaussianObjective`` runs natively.  True also takes any other
  objective, and a ``GaussianObjective`` whose target / precision require a gradient: the rollout stays native, its trajectory
  comes back as a differentiable output (``autodiff.ComposedTrajectoryFunction``), and the objective is accumulated over the H
  states in torch, which also carries the gradient of the objective's own parameters.  Head scale / shift gradients and a
  trainable drift keep falling back.

  ``native_coregionalized``: with the default False a drift (or policy) with a ``LinearCoregionalization`` kernel takes the torch
  composition as before.  True runs a coregionalised DRIFT with Lg <= nx latents natively, forward and gradient, for 1 to 4 actions
  (``native_actions`` still governs the gradient of nu > 1): the mixing f = W g + c is one small launch per step on the device
  (``mm_rollout_composed_nd_mixed`` and its tape / reverse sweep).  A coregionalised policy, Lg > nx, a trainable drift (W and the
  mean included) and head / objective constants that require a gradient each fall back once, with a named reason.  So does a
  drift or a policy with Matern latents: moment matching has closed forms for SquaredExponential only (``native=True`` raises with
  that reason, and the torch composition meets ``moment_matching``'s own ``NotImplementedError``).

  ``native_wide``: with the default False a gradient at more than 8 encoded dims (ne = nx + na > 8) takes the torch composition, as
  before and with the same text.  True runs it as one differentiable op for 8 < ne <= 16 (``mm_compose_wide_backward*``: the wide
  reverse sweep over the ``_nd`` family's tape) -- 1 to 4 actions under ``native_actions``, with or without an encoder
  (``native_no_encoder``), any objective (``native_objective``: the seeded sweep), a coregionalised drift
  (``native_coregionalized``), and under ``GraphedPolicyLoss``.  ne = 17..24, a policy past the sweep's LDS bound, a trainable
  drift, and head / objective constants that require a gradient (without ``native_objective``) each fall back once with a named
  reason.  ne <= 8 is routed as without the option."""
  uniform = solution_times is None
  if solution_times is None:
    solution_times = np.arange(1, 1 + num_steps, dtype=np.float64)     # pilco.py:186
  encoder = system.encoder
  fast = None
  shape_reason = None
  if native is not False:
    if not uniform or float(initial_time) != 0.0:
      shape_reason = "non-uniform solution times (the native rollout takes unit steps from t = 0)"
    elif kwargs:
      shape_reason = f"solver options {sorted(kwargs)}"
    else:
      why_not = []
      fast = native_policy_loss(system, objective, num_steps, dt=1.0, why=why_not, native_actions=native_actions,
                                native_no_encoder=native_no_encoder, native_objective=native_objective,
                                native_coregionalized=native_coregionalized, native_wide=native_wide)
      if fast is None:
        shape_reason = why_not[0] if why_not else "the system is not the shape mm_rollout_composed implements"
  if native is True and fast is None:
    # (the text SquaredExponential systems have always got; a Matern drift or policy adds its named reason)
    raise ValueError("native=True: the system is not the shape mm_rollout_composed implements"
                     + (f" ({shape_reason})" if shape_reason and "SquaredExponential" in shape_reason else ""))

  def _accumulate_loss(t, state, loss):                                # pilco.py:199-205
    x = GaussianMoments(moments=state, centered=True)
    if encoder is not None:
      x = moment_matching(x, encoder).y
    return loss + objective(x=x, t=t)

  _fallback = functools.partial(_warn_fallback, [], native, "policy_loss_closure")

  def _use_native(mx, Sxx):
    if fast is None and mx.is_cuda:
      _fallback(shape_reason or "the system is not the shape mm_rollout_composed implements")
    if fast is None or not mx.is_cuda or mx.ndim != 2:
      return False
    models = [system.drift, getattr(getattr(system.policy, "model", None), "model", None)]
    trainable = any(t.requires_grad for m in models if m is not None for t in m._parameters())
    if native_coregionalized:              # (the mixing matrix of a coregionalised drift is one of its parameters here)
      W = getattr(system.drift.kernel, "W", None)
      trainable = trainable or (isinstance(W, torch.Tensor) and W.requires_grad)
    if torch.is_grad_enabled() and (trainable or mx.requires_grad or Sxx.requires_grad or fast.uses_trajectory(mx)):
      return False                       # someone differentiates: the torch composition carries the autograd graph
    if trainable and torch.cuda.is_current_stream_capturing():
      # a captured graph must evaluate a trainable model FROM its parameters, not from a packed snapshot that goes
      # stale at the next optimiser step: only the policy can be re-packed inside the graph (run.from_parameters)
      return "from_parameters" if not any(t.requires_grad for t in system.drift._parameters()) else False
    return True

  def _use_native_grad(mx, Sxx):
    """Someone differentiates, and what is differentiated is what the native reverse sweep covers: the policy's
    parameters and / or the initial state, with a frozen drift (the tape is float64; a float32 state is cast up)."""
    if native is False or not mx.is_cuda or not torch.is_grad_enabled():
      return False
    if fast is None:
      _fallback(shape_reason or "the system is not the shape mm_rollout_composed implements")
      return False
    if mx.ndim != 2:
      _fallback(f"state of rank {mx.ndim} (the native path takes mx [B, nx])")
      return False
    why = fast.grad_obstacle(mx)
    if why is not None:
      _fallback(why)
      return False
    return True

  def _closure():                                                      # pilco.py:207-217
    mx, Sxx = state_initializer()
    use = _use_native(mx, Sxx)
    if use == "from_parameters":
      return fast.from_parameters(mx, Sxx)
    if use:
      return fast(mx, Sxx)
    if _use_native_grad(mx, Sxx):
      return fast.with_grad(mx, Sxx)
    loss = torch.zeros(mx.shape[:-1], dtype=mx.dtype, device=mx.device)
    _, loss = system.solve_forward(iterator="foldl", initial_time=initial_time,
                                   initial_state=(mx, Sxx), solution_times=solution_times,
                                   callbacks_and_initializers=((_accumulate_loss, loss),), **kwargs)
    return loss

  return _closure


class GraphedPolicyLoss:
  """The policy loss closure -- and its gradient w.r.t. the policy parameters -- captured once into HIP
  graphs (``torch.cuda.CUDAGraph``) and replayed.

  The reference traces the closure once under ``tf.function`` (pilco.py:219-220); here the equivalent
  is a graph capture: at cartpole sizes one composed rollout step is several hundred small kernels
  and the eager path is bound by the host launching them (measured: 10.7 ms/step forward+backward
  eager, 2.4 ms/step replayed; 1.5 -> 0.77 ms/step forward only).

  Everything the closure reads must live in fixed tensors: the state initializer has to return the SAME
  tensors on every call (``get_state_initializer`` does; write a new initial state into them with
  ``copy_``), parameters are updated in place (optimisers do), shapes are frozen.  Replays read the
  current values of the TRAINABLE models (they are evaluated from their parameters inside the graph);
  frozen models (the drift) enter through their packed snapshot -- rebuild the object after refitting them.
  ``loss()`` / ``loss_and_grad()`` return static tensors that the next replay
  overwrites; gradients are also left in ``p.grad`` (overwritten, not accumulated).  No host-side
  checks run inside a replay: a non-PD state shows up as nan in the loss and in the packed models'
  status words (``PackedModel.check_status``); a failed Kuu factorisation of the trainable policy poisons its
  factor with NaN inside the graph and is recorded in ``linalg.capture_status`` -- ``check()`` (synchronising)
  raises for either.
  """

  def __init__(self, closure: Callable, parameters: Sequence[torch.Tensor], warmup: int = 2):
    self.closure = closure
    self.parameters = [p for p in parameters if p.requires_grad]
    if not self.parameters:
      raise ValueError("GraphedPolicyLoss needs at least one parameter with requires_grad=True")
    dev = self.parameters[0].device
    side = torch.cuda.Stream(device=dev)                 # warm-up off the capturing stream (lazy init, caches)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      for _ in range(max(1, warmup)):
        with torch.no_grad():
          closure()
        for p in self.parameters:
          p.grad = None
        closure().sum().backward()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    self._fwd = torch.cuda.CUDAGraph()
    with torch.no_grad():
      with torch.cuda.graph(self._fwd):
        self._loss_fwd = closure()
    for p in self.parameters:
      p.grad = None
    self._bwd = torch.cuda.CUDAGraph()
    with torch.cuda.graph(self._bwd):
      self._loss_bwd = closure()
      self._loss_bwd.sum().backward()
    self._grads = [p.grad for p in self.parameters]
    self._loss_bwd = self._loss_bwd.detach()
    self._device = dev

  def check(self):
    """Synchronising check of what the replays could not raise: in-graph factorisation failures."""
    from .linalg import check_capture_status
    check_capture_status(self._device)

  def loss(self) -> torch.Tensor:
    """Forward only: the per-batch-element loss [B]."""
    self._fwd.replay()
    return self._loss_fwd

  def loss_and_grad(self):
    """-> (loss [B], [d sum(loss) / d p for p in parameters]); the gradients are also in ``p.grad``."""
    self._bwd.replay()
    for p, g in zip(self.parameters, self._grads):
      p.grad = g
    return self._loss_bwd, self._grads


def pathwise_policy_loss_closure(system: DynamicalSystem, objective: Callable, state_initializer: Callable, num_steps: int,
                                 dt: float = 1.0, num_bases: int = 1024, paths=None, native: Optional[bool] = None,
                                 generator: Optional[torch.Generator] = None, native_actions: int = 1,
                                 native_inputs: int = 8, native_sampler: bool = False,
                                 native_no_encoder: bool = False, native_objective: bool = False,
                                 native_coregionalized: bool = False) -> Callable:
  """``PathwisePILCO._policy_loss_closure`` (gpflow_pilco/loops/pilco.py:263-298).  Returns ``closure() -> loss [S]``: the cost
  accumulated along one sample rollout per initial state -- per step encoder -> policy -> drift sample path -> Euler -> objective
  of the encoded state (tensor branch of ``forward_sde``, dynamics/forward_sde.py:23-31; ``Euler.step``, solvers.py:50-65).  The
  caller takes the mean and differentiates it w.r.t. the policy (examples/cartpole_swingup/train_utils.py:108-135).

  ``system.drift``: a ``pathwise.PathwiseSVGP``; ``state_initializer() -> x0 [S, nx]`` (pilco.py:300-303: ``p.sample([batch_size])``);
  ``paths``: None = new sample paths on every call (pilco.py:281-284), else a ``pathwise.Paths`` to reuse.  Unit-spaced solution
  times ``dt, 2 dt, ...`` (pilco.py:257: ``arange(1, 1 + num_steps)``).

  On the GPU, for the cartpole wiring (``_native_parts``, one action) with drift inputs of dimension <= 8, the whole closure is the native
  rollout (csrc/mm_pathwise_policy.hip): forward only when nothing requires a gradient, else ONE differentiable op
  (``pathwise.PolicyRolloutFunction``: the stream pass also emits the paths' Jacobians, the reverse sweep is one kernel).
  Otherwise -- ``native=False``, another wiring, a gradient the native sweep does not cover -- the torch composition through
  ``DynamicalSystem.solve_forward`` runs, saying so once (the paths stay on the device and are differentiable in x).

  ``native_actions``: the largest number of actions the closure may run natively.  The default 1 keeps a policy with several
  actions on the torch composition (with the "nu > 1" warning; ``native=True`` raises).  With ``native_actions >= nu`` such a
  policy runs in the same native rollout through its ``_nd`` entries (1 to 4 actions), forward and gradient, where
  nx + na + nu <= 8, the policy has <= 256 centres and -- when a gradient is asked for -- the reverse sweep takes the shape
  (``PolicyRollout.supports_backward``); every other case falls back and names its reason.

  ``native_inputs``: the largest drift input dimension nd = nx + na + nu the closure may run natively.  The default 8 is the
  routing above.  With ``native_inputs=16`` a system with 8 < nd <= 16 (the cart-double-pendulum: nx 6, two angles, one force,
  nd 9) runs in the wide entries (``PolicyRollout(wide=True)``: the Jacobian pass of the weight stream over half sample groups),
  forward and gradient, for any number of actions ``native_actions`` admits; nd > 16 or a gradient outside the reverse sweep's
  LDS bound falls back once, naming the bound (the forward stays native in the latter case).  Values above 16 behave as 16.
  The torch composition itself is differentiable for nd <= 16 (``Paths.__call__``).

  ``native_sampler``: with ``paths=None``, where the new paths of each call come from.  The default False calls
  ``drift.generate_paths`` (torch, from nothing each time: Kuu and its factor included, every tensor newly allocated, one host
  synchronisation).  True keeps one ``pathwise.PathSampler`` per (S, dtype, device) and draws from it -- on the native and on the
  torch-composition route alike: the drift's factor is cached per version of its parameters, a draw allocates and synchronises
  nothing, so a ``GraphedPolicyLoss`` of the closure captures, and each replay draws new paths (from the default generator:
  ``generator`` must be None for that).  The paths of a call live in the sampler's static buffers until the next call.  With
  ``paths`` given the option changes nothing.

  ``native_no_encoder``: with the default False a system without an encoder takes the torch composition (``native=True`` raises);
  True runs it in the native rollouts with na = 0 (the drift's inputs are (x, u), the cost that of the raw state), under the same
  ``native_actions`` / ``native_inputs`` rules.

  ``native_objective``: with the default False only a constant ``GaussianObjective`` runs natively (its cost is computed in the
  rollout's kernels).  True also takes any other objective of a tensor of states, and a ``GaussianObjective`` whose target /
  precision require a gradient: the rollout stays native with a zero built-in cost, its states x_1 .. x_H come back as a
  differentiable output (``pathwise.PolicyTrajectoryFunction``; forward only under ``no_grad`` when neither the policy nor the
  initial states require a gradient), and the loss is the reference's accumulation (pilco.py:272-275) in torch on them: the whole
  [H, S, nx] block encoded in one call, then ``objective(x=encoder(x_h), t=h dt)`` per step.  The seeded reverse sweep
  (``mm_pathwise_policy_rollout_backward[_nd|_wide]_seeded``) carries d loss / d x_h back to the policy and the initial states; the
  objective's own parameters get their gradients from the torch part.  A constant ``GaussianObjective`` keeps the in-kernel cost.
  The option composes with ``native_actions``, ``native_inputs``, ``native_no_encoder``, ``native_sampler`` and ``paths`` under their
  rules; head scale / shift gradients keep falling back.

  ``native_coregionalized``: with the default False a drift (or policy) with a ``LinearCoregionalization`` kernel takes the torch
  composition, saying so once (``native=True`` raises) -- on paths that carry the drift's mixing (``Paths.mix_W`` / ``mix_c``:
  ``generate_paths`` and ``PathSampler`` draw Lg latent paths and ``Paths.__call__`` returns W g + c), so the composition is
  correct for any Lg.  True runs a coregionalised DRIFT with Lg <= nx latents in the ``_mixed`` native entries, forward and
  gradient (csrc/mm_pathwise_policy.hip: a latent-sized tape, the mixing inside the head kernel and the reverse sweep), for
  1 to 4 actions and nd <= 16 under the ``native_actions`` / ``native_inputs`` rules; it composes with ``native_no_encoder``,
  ``native_objective``, ``native_sampler`` and ``paths=``.  W and the Constant mean are constants of the frozen drift, taken from
  the paths of the call.  A coregionalised policy, Lg > nx, given ``paths`` that carry no mixing or one of another shape than the
  drift's, and a W or a mean that requires a gradient each fall back once, with a named reason.

  A drift with ``models.Matern32`` / ``Matern52`` latents (one family for the whole model) runs natively under the same rules and
  options, with no flag of its own: its paths carry ``Paths.kernel`` and ``PolicyRollout`` calls
  ``mm_pathwise_policy_rollout_kern`` for every shape; the torch composition (``native=False``) works too, because
  ``Paths.__call__`` routes on the family.  A Matern POLICY falls back once, by name (``native=True`` raises): the native head
  kernels evaluate a SquaredExponential policy; its torch composition is ``SVGP.predict_mean`` with the family's Gram matrix.

  A MEAN-ONLY drift -- ``system.drift`` a ``KernelRegressor`` around an ``SVGP`` / ``PathwiseSVGP``, what the reference's
  ``build_dynamics(..., model_uncertainty=False)`` builds (pilco.py:45-79) -- steps every sample with the posterior mean.  Nothing
  is drawn: ``paths``, ``num_bases``, ``generator`` and ``native_sampler`` are ignored, as ``KernelRegressor.__call__`` ignores the
  paths.  The torch composition is the same Euler fold (``drift(eu)`` is ``predict_mean``); on the GPU the native route runs under
  the rules and options above, with no flag of its own, on a ``pathwise.MeanDrift`` of the model (cached per version of its
  parameters; ``mm_pathwise_policy_rollout_mean``: the shared weights through LDS instead of a weight stream).  A drift whose
  parameters require a gradient falls back once, by name: the torch composition differentiates ``predict_mean``.  With
  ``native=True`` an obstacle met at a call (nd > 16, more actions than ``native_actions``, a trainable drift, ...) raises with the
  reason the fallback would have named."""
  from . import ops
  from .components import TrigonometricEncoder
  from .linalg import index_tensor
  from .models import SVGP, KernelRegressor, LinearCoregionalization
  from .pathwise import MeanDrift, PathSampler, PathwiseSVGP, PolicyRollout, PolicyRolloutFunction, PolicyTrajectoryFunction
  drift = system.drift
  mean_only = isinstance(drift, KernelRegressor) and isinstance(drift.model, SVGP)
  if mean_only:
    drift = drift.model                                        # (system.drift keeps the wrapper: system.forward evaluates the mean)
  elif not isinstance(drift, PathwiseSVGP):
    raise TypeError("pathwise_policy_loss_closure needs a PathwiseSVGP drift (gpflow_pilco/loops/pilco.py:230-236)")
  H = int(num_steps)
  why_not: list = []
  parts = None if native is False else _native_parts(system, objective, why_not, moment_solver=False,
                                                     no_encoder=bool(native_no_encoder),
                                                     any_objective=bool(native_objective),
                                                     coregionalized=bool(native_coregionalized))
  if native is True and parts is None:
    raise ValueError(f"native=True: {why_not[0] if why_not else 'the system is not the shape the native rollout implements'}")
  max_native = int(native_actions)
  max_nd = min(16, int(native_inputs))
  if native is True and parts[1].num_latent_gps > max(1, max_native):
    raise ValueError("native=True: the native pathwise rollout is one-action" if max_native <= 1 else
                     f"native=True: the policy has {parts[1].num_latent_gps} actions, native_actions={max_native}")
  _fallback = functools.partial(_warn_fallback, [], native, "pathwise_policy_loss_closure")
  if mean_only and native is True:
    # a mean-only drift had no route before this one: native=True holds at every call too (a sampled drift keeps its warning)
    def _fallback(reason):
      raise ValueError(f"native=True: {reason}")

  def _torch_loss(x0, pth):
    times = dt * np.arange(1, 1 + H, dtype=np.float64)
    enc = system.encoder

    def _accumulate_loss(t, state, loss):                              # pilco.py:272-275
      return loss + objective(x=state if enc is None else enc(state), t=t)
    loss0 = torch.zeros(x0.shape[:-1], dtype=x0.dtype, device=x0.device)
    solver = Euler()
    # (a mean-only drift reads no paths: system.drift(eu) is KernelRegressor.__call__ = predict_mean)
    with (contextlib.nullcontext() if mean_only else drift.set_temporary_paths(pth)):
      _, loss = solver(func=system.forward, initial_time=0.0, initial_state=x0, solution_times=times,
                       callbacks_and_initializers=((_accumulate_loss, loss0),), iterator="foldl")
    return loss

  samplers = {}

  def _new_paths(x0):
    if not native_sampler:
      return drift.generate_paths(x0.shape[0], num_bases, dtype=x0.dtype, device=x0.device, generator=generator)
    key = (x0.shape[0], x0.dtype, str(x0.device))
    if key not in samplers:
      samplers[key] = PathSampler(drift, x0.shape[0], num_bases, dtype=x0.dtype, device=x0.device)
    return samplers[key].draw(generator=generator)

  def _encode(xs):
    """``system.encoder(xs)``.  A plain ``TrigonometricEncoder`` is evaluated by its own transform on columns selected with cached
    device index tensors (``linalg.index_tensor``): ``Encoder.__call__`` indexes with a Python list, which uploads the indices on
    every call -- a copy a HIP-graph capture of the closure refuses.  A subclass keeps its own ``__call__``."""
    enc = system.encoder
    if enc is None:
      return xs
    if type(enc) is not TrigonometricEncoder:
      return enc(xs)
    active, inactive = enc.get_partition_indices(ndims=xs.shape[-1])
    if not active:
      return xs
    ret = enc.transform(xs.index_select(-1, index_tensor(active, xs.device)))
    return torch.cat([ret, xs.index_select(-1, index_tensor(inactive, xs.device))], dim=-1) if inactive else ret

  def _objective_of_states(xs):
    """pilco.py:272-275 over the states x_1 .. x_H (xs [H, S, nx]) at the times dt, 2 dt, ..: one encoder call for the block."""
    e = _encode(xs)
    loss = torch.zeros(xs.shape[1], dtype=xs.dtype, device=xs.device)
    for h in range(H):
      loss = loss + objective(x=e[h], t=dt * float(h + 1))
    return loss

  def _closure():
    x0 = state_initializer()
    # (a mean-only drift: nothing is drawn and given paths are not read, as KernelRegressor.__call__ ignores them)
    pth = None if mean_only else paths if paths is not None else _new_paths(x0)
    if parts is None or not x0.is_cuda or x0.ndim != 2:
      if x0.is_cuda and native is not False:
        _fallback(why_not[0] if why_not else f"state of rank {x0.ndim}")
      return _torch_loss(x0, pth)
    enc, pm_, _, bj, head_constants = parts
    nx, na = x0.shape[-1], len(enc.active_dims)
    nu = int(pm_.num_latent_gps)
    if nu > max(1, max_native):
      _fallback(f"the policy has nu = {nu} actions (nu > 1: the native pathwise rollout is one-action)" if max_native <= 1 else
                f"the policy has nu = {nu} actions (nu > 1) and native_actions = {max_native}")
      return _torch_loss(x0, pth)
    pol_M = max(iv.Z.shape[0] for iv in pm_.inducing_variable.inducing_variables[:nu])
    nd = nx + na + nu
    if max_nd > 8:
      if nd > max_nd or pol_M > 256:
        _fallback(f"drift inputs of dimension nx + na + nu = {nd} > {max_nd} or a policy of more than 256 centres ({pol_M})")
        return _torch_loss(x0, pth)
    elif nu == 1:
      if nd > 8 or pol_M > 256:
        _fallback("drift inputs of dimension > 8 or a policy of more than 256 centres")
        return _torch_loss(x0, pth)
    elif nd > 8 or pol_M > 256:
      _fallback(f"drift inputs of dimension nx + na + nu = {nd} > 8 or a policy of more than 256 centres ({pol_M})")
      return _torch_loss(x0, pth)
    traj = _objective_uses_trajectory(objective, native_objective)
    grad = torch.is_grad_enabled()
    if mean_only:
      frozen = list(drift._parameters()) + ([drift.kernel.W] if isinstance(drift.kernel, LinearCoregionalization) else [])
      if grad and any(isinstance(t, torch.Tensor) and t.requires_grad for t in frozen):
        _fallback("the mean-only drift's parameters require a gradient (the native rollout takes a frozen drift; the torch "
                  "composition differentiates predict_mean)")
        return _torch_loss(x0, pth)
      pth = MeanDrift.from_model(drift, x0.dtype, x0.device)   # cached per version of the drift's parameters
    if isinstance(drift.kernel, LinearCoregionalization):      # (native_coregionalized: _native_parts refused it otherwise)
      obstacle = _pathwise_mixing_obstacle(drift, pth, grad)
      if obstacle is not None:
        _fallback(obstacle)
        return _torch_loss(x0, pth)
    obstacle = _constants_grad_obstacle(bj, objective, native_objective, "initial states") if grad else None
    if obstacle is not None:
      _fallback(obstacle)
      return _torch_loss(x0, pth)
    scale, shift = head_constants()
    pol_pack = pm_.packed(torch.float64, False, x0.device)
    # (the trajectory route: a zero built-in cost, its output ignored)
    # (a Matern drift: PolicyRollout routes on pth.kernel -- the one _kern entry, for every shape admitted above)
    roll = PolicyRollout(pth, pol_pack, nx=nx, active_dims=enc.active_dims, head_scale=scale, head_shift=shift,
                         target=None if traj else objective.target, precis=None if traj else objective.precis, wide=nd > 8,
                         num_samples=x0.shape[0] if mean_only else None)
    needs = grad and (x0.requires_grad or any(t.requires_grad for t in pm_._parameters()))
    if needs and not roll.supports_backward():
      _fallback(f"the native reverse sweep does not take nu = {nu} actions with {pol_M} centres on {nx + na} inputs (its LDS bound)")
      return _torch_loss(x0, pth)
    if not needs:
      with torch.no_grad():
        pol = None
        if traj and torch.cuda.is_current_stream_capturing() and any(t.requires_grad for t in pm_._parameters()):
          # a captured forward of a trainable policy packs it FROM its parameters inside the graph, so that replays follow the
          # optimiser's in-place updates (the cached pack is a snapshot: native_policy_loss's run.from_parameters).  Only on
          # the trajectory route, which is new: the built-in-cost branch below is deliberately left as it was -- a captured
          # forward-only graph of it keeps reading the snapshot taken at capture (its loss_and_grad graph packs from the
          # parameters already) -- so that nothing changes with the option off; treating both alike is a change of its own
          Zp, lsp, varp, betap, _, mcp = pm_.precompute(x0.device)
          pol = ops.pack_model(Zp, lsp, varp, betap, None, mcp, dtype=torch.float64, sync=False)
        cost, tape = roll(x0, H, dt=dt, policy=pol)
      # (the trajectory route: the states are constants here; an objective parameter that requires a gradient still gets it)
      return _objective_of_states(roll.trajectory(tape, H)) if traj else cost.sum(0)
    Zp, lsp, varp, betap, _, mcp = pm_.precompute(x0.device)
    if mcp is None:
      mcp = torch.zeros(nu, dtype=Zp.dtype, device=x0.device)
    if traj:
      _, xs = PolicyTrajectoryFunction.apply(x0, Zp, lsp, varp, betap, mcp, roll, H, dt)
      return _objective_of_states(xs).to(x0.dtype)
    return PolicyRolloutFunction.apply(x0, Zp, lsp, varp, betap, mcp, roll, H, dt).sum(1).to(x0.dtype)

  return _closure
