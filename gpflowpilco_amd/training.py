"""Fitting an ``SVGP`` drift to data: the reference's ``update_dynamics`` -- L-BFGS on the negative of
``SVGP.maximum_log_likelihood_objective`` (the ELBO plus the model's prior).

The parameters of ``models`` are plain tensors, so the constraints gpflow attaches to its ``Parameter``s live here: ``fit_svgp``
optimises unconstrained leaves -- softplus for the kernel variances and the noise variance, a sigmoid onto ``lengthscale_bounds``
for the lengthscales, the lower triangle of ``q_sqrt``, everything else as it is -- and evaluates the loss with the constrained
values standing in for the model's own tensors.  After the fit the values are copied INTO those tensors in place, so their
``_version`` moves and the model's pack cache (``models._PackCache``) repacks on the next ``packed()``.
"""
from __future__ import annotations

import contextlib
from typing import Callable, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import models as gp

__all__ = ("fit_svgp",)


def _inv_softplus(y: torch.Tensor) -> torch.Tensor:
  return y + torch.log(-torch.expm1(-y))


class _Slot:
  """One tensor attribute of the model (``owner.name``), its unconstrained leaf and the map between the two."""

  def __init__(self, owner, name: str, forward: Callable, inverse: Callable, trainable: bool = True):
    self.owner, self.name, self.forward = owner, name, forward
    self.original = getattr(owner, name)
    self.leaf = inverse(self.original.detach().clone()).requires_grad_(trainable)
    self.trainable = trainable

  def value(self) -> torch.Tensor:
    return self.forward(self.leaf) if self.trainable else self.original


def _identity(t):
  return t


def _slots(model, train_inducing: bool, bounds: Tuple[float, float], mean_only: bool, collapsed: bool = False) -> List[_Slot]:
  lo, hi = (float(b) for b in bounds)
  eps = 1e-9 * (hi - lo)
  to_ls = lambda r: lo + (hi - lo) * torch.sigmoid(r)
  from_ls = lambda v: torch.logit((v.clamp(lo + eps, hi - eps) - lo) / (hi - lo))
  kernels, Zs = gp.unpack_multioutput(model.kernel, model.inducing_variable, model.num_latent_gps)
  slots, seen = [], set()
  for k in kernels:                                              # a SharedIndependent kernel is one object: one pair of leaves
    if id(k) not in seen:
      seen.add(id(k))
      slots.append(_Slot(k, "variance", F.softplus, _inv_softplus, trainable=not mean_only))
      slots.append(_Slot(k, "lengthscales", to_ls, from_ls))
  ivs = getattr(model.inducing_variable, "inducing_variables", [model.inducing_variable])
  for iv in ivs:
    if id(iv) not in seen:
      seen.add(id(iv))
      slots.append(_Slot(iv, "Z", _identity, _identity, trainable=train_inducing))
  slots.append(_Slot(model.likelihood, "variance", F.softplus, _inv_softplus))
  slots.append(_Slot(model, "q_mu", _identity, _identity, trainable=not collapsed))
  M = model.q_sqrt.shape[-1]
  rows, cols = torch.tril_indices(M, M, device=model.q_sqrt.device)
  slots.append(_Slot(model, "q_sqrt", lambda v: _scatter_tril(v, rows, cols, M), lambda S: S[:, rows, cols],
                     trainable=not (mean_only or collapsed)))
  if isinstance(model.mean_function, gp.Constant):
    slots.append(_Slot(model.mean_function, "c", _identity, _identity))
  if isinstance(model.kernel, gp.LinearCoregionalization):
    slots.append(_Slot(model.kernel, "W", _identity, _identity))
  return slots


def _scatter_tril(v: torch.Tensor, rows: torch.Tensor, cols: torch.Tensor, M: int) -> torch.Tensor:
  S = torch.zeros(v.shape[0], M, M, dtype=v.dtype, device=v.device)
  S[:, rows, cols] = v
  return S


@contextlib.contextmanager
def _substituted(slots: List[_Slot], values: List[torch.Tensor]):
  """The model with ``values`` in the place of its own tensors (same attributes, other objects), restored on exit."""
  try:
    for s, v in zip(slots, values):
      setattr(s.owner, s.name, v)
    yield
  finally:
    for s in slots:
      setattr(s.owner, s.name, s.original)


def fit_svgp(model, data, max_iter: int = 100, train_inducing: Optional[bool] = None,
             lengthscale_bounds: Tuple[float, float] = (0.01, 100.0), native: Optional[bool] = None,
             history: Optional[list] = None, collapsed: bool = False) -> list:
  """Fit ``model`` (an ``SVGP`` / ``PathwiseSVGP``, or a ``KernelRegressor`` around one) to ``data = (X, Y)`` by at most
  ``max_iter`` iterations of ``torch.optim.LBFGS`` (strong-Wolfe line search) on ``model.training_loss(data, native)``.

  ``train_inducing=None`` is the reference's rule (loops/pilco.py:67-68): the inducing points are frozen when M >= N.  A
  ``KernelRegressor`` is fitted as the reference's ``model_uncertainty=False`` drift (pilco.py:70-74): ``q_sqrt`` and the
  kernel variances stay as they are.  The fitted values are written into the model's own tensors in place.

  ``collapsed=True`` fits the hyper-parameters alone, on ``model.collapsed_training_loss`` (the bound at the optimal q(u), which
  a Gaussian likelihood gives in closed form): ``q_mu`` and ``q_sqrt`` are no leaves of the optimiser, and after the last
  iteration ``model.set_optimal_q`` writes the optimum at the fitted hyper-parameters, so that ``model.training_loss`` there is the
  final history entry.  Independent latents only; a ``KernelRegressor`` and a coregionalised kernel raise ``NotImplementedError``.

  Returns the loss history: the loss before each iteration and the final loss (appended to ``history`` when one is given)."""
  mean_only = isinstance(model, gp.KernelRegressor)
  if collapsed and mean_only:
    raise NotImplementedError("fit_svgp(collapsed=True): a KernelRegressor keeps its q_sqrt frozen, so its objective differs from "
                              "the collapsed bound by a term that depends on the lengthscales; fit it with collapsed=False")
  if isinstance(model, gp.GPModelWrapper):
    model = model.model
  if not isinstance(model, gp.SVGP):
    raise TypeError(f"fit_svgp fits an SVGP (or a KernelRegressor around one), got {type(model).__name__}")
  if not isinstance(model.likelihood, gp.GaussianLikelihood):
    raise NotImplementedError("fit_svgp: Gaussian likelihood only")
  if collapsed and isinstance(model.kernel, gp.LinearCoregionalization):
    raise NotImplementedError("fit_svgp(collapsed=True): a LinearCoregionalization kernel couples the latents through W (the "
                              "collapsed bound needs cross-latent statistics); fit it with collapsed=False")
  model_loss = model.collapsed_training_loss if collapsed else model.training_loss
  X = data[0]
  if train_inducing is None:
    train_inducing = model.q_mu.shape[-2] < X.shape[0]
  slots = _slots(model, bool(train_inducing), lengthscale_bounds, mean_only, bool(collapsed))
  leaves = [s.leaf for s in slots if s.trainable]
  history = [] if history is None else history
  # one iteration per step() call (the curvature pairs persist in the optimiser's state), so that the history is per iteration;
  # max_eval bounds the line search of that iteration (its default, 5/4 max_iter = 1, would end the search after one point)
  opt = torch.optim.LBFGS(leaves, max_iter=1, max_eval=32, line_search_fn="strong_wolfe")

  def loss_value() -> torch.Tensor:
    with _substituted(slots, [s.value() for s in slots]):
      return model_loss(data, native=native)

  def plain_closure():
    opt.zero_grad()
    loss = loss_value()
    loss.backward()
    return loss

  reference = []

  def collapsed_closure():
    # a trial point of the line search whose I + AAT is singular to rounding (a noise variance of 1e-18 on the first,
    # extrapolating, search) is rejected with a large finite loss and no gradient, so that the search brackets and backs off; an
    # iterate is never such a point, and a failure of Kuu + jitter I, or any failure at the starting point, is raised as it is
    try:
      loss = plain_closure()
    except gp.SingularCollapsedBound:
      if not reference:
        raise
      opt.zero_grad()
      return leaves[0].new_tensor(1e10 * max(1.0, reference[0]))
    if not reference:
      reference.append(abs(float(loss.detach())))              # the loss at the starting point: the scale of a rejection
    return loss

  closure = collapsed_closure if collapsed else plain_closure

  for _ in range(int(max_iter)):
    loss = float(opt.step(closure).detach())                   # the loss at the iterate this iteration starts from
    history.append(loss)
    if loss != loss or abs(loss) == float("inf"):
      break
    if len(history) > 1 and abs(history[-2] - loss) <= 1e-9 * max(1.0, abs(loss)):
      break
  with torch.no_grad():
    values = [s.value() for s in slots]
    with _substituted(slots, values):
      history.append(float(model_loss(data, native=native)))
    if history[-1] != history[-1] or abs(history[-1]) == float("inf"):
      raise FloatingPointError(f"fit_svgp: the loss became {history[-1]} (history {history}); the model is left as it was")
    for s, v in zip(slots, values):
      if s.trainable:
        s.original.copy_(v)
    if collapsed:
      model.set_optimal_q(data, native=native)
  return history
