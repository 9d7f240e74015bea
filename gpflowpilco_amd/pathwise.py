"""Pathwise (decoupled-sampling) GP paths and sample rollouts -- SURVEY.md row f-3.

Mirrors the surface the reference uses from ``gpflow_sampling`` (un-vendored third party):
``PathwiseSVGP.generate_paths(num_samples, num_bases, sample_axis=0)``,
``set_temporary_paths`` and ``predict_f_samples`` / ``__call__``
(``gpflow_pilco/models/svgp.py:124-130``, ``loops/pilco.py:263-303``).  Path *generation*
(sampling weights, one Cholesky solve per latent) runs on EVERY call of a rollout closure that
is not handed paths (``loops/pilco.py:281-284``: new paths per optimiser step).
``generate_paths`` is torch plumbing that starts from nothing each time (Kuu and its factor
included); ``PathSampler`` keeps what does not change between draws, draws into preallocated
buffers and does the reformatting in two kernels (``csrc/mm_pathwise_sample.hip``), so that a
draw neither allocates nor synchronises and can be captured in a HIP graph.  Path *evaluation*
-- the per-step hot loop -- runs in ``mm_pathwise_eval`` / ``mm_pathwise_rollout``
(``csrc/mm_pathwise.hip``).  Parity with gpflow_sampling is unpinned (see
``oracle/pathwise_oracle.py``).

The latents of a model are ``SquaredExponential``, ``Matern32`` or ``Matern52`` (one family per model: ``models.kernel_family``).
The family changes three things -- the distribution of the random-Fourier frequencies (``spectral_frequencies``), the Gram matrix
the update weights are solved with, and the basis value of the stream pass's update half (``Paths.kernel``: the ``_kern`` entries
of the C ABI) -- and nothing else: layouts, tapes and reverse sweeps are shared.
"""
from __future__ import annotations

import contextlib
import math
from dataclasses import dataclass
from typing import Optional

import torch

from .linalg import cholesky

from . import _lib
from .models import (DEFAULT_FLOAT, DEFAULT_JITTER, KERNEL_NAMES, KERNEL_SE, SVGP, Constant, LinearCoregionalization, Zero,
                     _scaled_sqdist, _stack_kernel_params, kernel_family, stationary_profile, unpack_multioutput)
from .ops import _dtype_code, _ptr, _require_device, _stream, check


BOUND_ULPS = 8.0      # Paths.eval_with_bound: rounding bound = BOUND_ULPS x unit roundoff x the sum of the absolute terms


def _kernel_code(kernel) -> int:
  """"se" | "matern32" | "matern52" (or the code 0 | 1 | 2) -> the C ABI's kernel argument."""
  if isinstance(kernel, str):
    if kernel not in KERNEL_NAMES:
      raise ValueError(f"kernel {kernel!r}: expected one of {KERNEL_NAMES}")
    return KERNEL_NAMES.index(kernel)
  if int(kernel) not in range(len(KERNEL_NAMES)):
    raise ValueError(f"kernel code {kernel}: expected 0 (se), 1 (matern32) or 2 (matern52)")
  return int(kernel)


def spectral_frequencies(n: torch.Tensor, ls: torch.Tensor, family: int, chi: Optional[torch.Tensor] = None) -> torch.Tensor:
  """The random-Fourier frequencies of a kernel family from standard normals: n [L, K, d], lengthscales ls [L, d] ->
  omega [L, K, d].  SquaredExponential: n / ls (its spectral density is Gaussian).  Matern-nu: a multivariate Student-t with
  2 nu degrees of freedom, omega = (n / ls) sqrt(2 nu / chi2) with one chi2_{2 nu} per (latent, basis function) -- the sum of
  the squares of the 2 nu (3 or 5) standard normals ``chi`` [L, K, 2 nu].  Plain torch: runs on any device."""
  if family == KERNEL_SE:
    return n / ls[:, None, :]
  dof = 3 if family == 1 else 5
  if chi is None or chi.shape != n.shape[:2] + (dof,):
    raise ValueError(f"a Matern draw needs chi [L, K, {dof}] standard normals")
  # (scale first, then the lengthscales: the order of PathSampler, whose basis kernel does the division)
  return (n * (chi * chi).sum(-1).reciprocal().mul(float(dof)).sqrt()[:, :, None]) / ls[:, None, :]


def _gram(Z: torch.Tensor, ls: torch.Tensor, var: torch.Tensor, family: int) -> torch.Tensor:
  """Kuu + jitter [L, M, M] of the family (SquaredExponential: the expression the samplers have always used)."""
  A = Z / ls[:, None, :]
  M = Z.shape[1]
  if family == KERNEL_SE:
    d2 = (A * A).sum(-1)[:, :, None] + (A * A).sum(-1)[:, None, :] - 2.0 * A @ A.transpose(1, 2)
    prof = torch.exp(-0.5 * d2.clamp_min(0.0))
  else:
    prof = stationary_profile(_scaled_sqdist(A, A), family)
  return var[:, None, None] * prof + DEFAULT_JITTER * torch.eye(M, dtype=DEFAULT_FLOAT, device=Z.device)


def _pad_last(t: torch.Tensor, mult: int) -> torch.Tensor:
  n = t.shape[-1]
  pad = (-n) % mult
  return t if pad == 0 else torch.nn.functional.pad(t, (0, pad))


@dataclass
class Paths:
  """S sample paths of L latent GPs (device tensors, element type ``dtype``).

  ``mix_W`` [nx, Lg] (with ``mix_c`` [nx] or None; both float64): the paths of a coregionalised model, f = W g + c -- L = Lg latent
  paths mixed to nx outputs, the constant added after the mixing as gpflow does (``mean_c`` is then None).  ``__call__``,
  ``eval_jac`` and ``eval_with_bound`` return the MIXED quantities (f [S, nx], J = W J_g [S, nx, d], bound |W| err_g): the latent
  values from the entries below with L = Lg, the mixing as a few float64 torch ops -- the route of the torch composition; the
  native policy rollout mixes in its own kernels (``PolicyRollout``)."""
  omega: torch.Tensor      # [L, d, Kp]   omega^T / 2 pi  (revolutions, k-major)
  phase: torch.Tensor      # [L, Kp]      b / 2 pi
  zs: torch.Tensor         # [L, d, Mp]   (Z * x_scale)^T, x_scale = sqrt(log2 e) / lengthscales
  hz: torch.Tensor         # [L, Mp]      |zs|^2 / 2
  wb: torch.Tensor         # [G, L, NB, 4, BT] blocked weight stream (prior blocks, then update blocks)
  num_samples: int
  lengthscales: torch.Tensor   # [L, d] f64: x_scale = sqrt(log2 e) / lengthscales
  prior_scale: torch.Tensor    # [L] f64  sqrt(2 var / K)
  variance: torch.Tensor       # [L] f64
  mean_c: Optional[torch.Tensor]  # [L] f64 or None
  mix_W: Optional[torch.Tensor] = None   # [nx, Lg] f64: f = W g + c (None: the latents are the outputs)
  mix_c: Optional[torch.Tensor] = None   # [nx] f64 or None
  kernel: int = 0                        # the latents' family: 0 SquaredExponential, 1 Matern-3/2, 2 Matern-5/2 (every entry routes on it)

  @property
  def dtype(self):
    return self.wb.dtype

  def _dims(self):
    L, d, Kp = self.omega.shape
    return self.num_samples, L, self.zs.shape[-1], Kp, d

  def _mixed_values(self, g: torch.Tensor) -> torch.Tensor:
    """g [S, Lg] -> W g + c [S, nx] (float64 arithmetic, this dtype's result)."""
    f = g.to(DEFAULT_FLOAT) @ self.mix_W.T
    return (f if self.mix_c is None else f + self.mix_c).to(self.dtype)

  def __call__(self, x: torch.Tensor) -> torch.Tensor:
    """f_s(x_s): x [S, d] -> [S, L] (mixed paths: [S, nx]).  Differentiable in x where the Jacobian pass exists (d <= 16): the torch
    composition of a sample rollout (``loops.pathwise_policy_loss_closure``'s fallback) then carries gradients through the paths."""
    if torch.is_grad_enabled() and x.requires_grad:
      return _PathsEval.apply(x, self)
    g = self._latent_values(x)
    return g if self.mix_W is None else self._mixed_values(g)

  def _operands(self):
    """((S, L, Mp, Kp, d), the nine drift operands omega_t .. wb): sizes and pointers in the order every entry of the C ABI lists
    them.  The one place this list is written: the sample entries (``_run``) and ``PolicyRollout`` both take it from here."""
    return self._dims(), (self.omega.data_ptr(), self.phase.data_ptr(), self.zs.data_ptr(), self.hz.data_ptr(),
                          self.lengthscales.data_ptr(), self.prior_scale.data_ptr(), self.variance.data_ptr(),
                          _ptr(self.mean_c), self.wb.data_ptr())

  def _run(self, stem: str, ins, outs, steps=()):
    """One call of a sample entry -- ``stem``: mm_pathwise_eval | _eval_jac | _eval_bound | _rollout; SquaredExponential paths call
    the entries they always have, Matern paths the ``_kern`` siblings with the family appended.  The argument list: sizes, dtype,
    ``steps`` (the rollout's H, dt), the buffers ``ins`` (x [S, d] first), the drift operands, the buffers ``outs`` (None: NULL),
    stream."""
    x = ins[0]
    _require_device(x, self.wb)
    sizes, drift = self._operands()
    S, d = sizes[0], sizes[-1]
    if x.shape != (S, d) or x.dtype != self.dtype:
      raise ValueError(f"expected x [{S},{d}] of {self.dtype}, got {tuple(x.shape)} {x.dtype}")
    entry, kern = (stem, ()) if self.kernel == 0 else (stem + "_kern", (int(self.kernel),))
    ins = [t.contiguous() for t in ins]                      # (kept until the call is made)
    rc = getattr(_lib.lib(), entry)(*sizes, _dtype_code(self.dtype), *steps, *(t.data_ptr() for t in ins), *drift,
                                    *(_ptr(t) for t in outs), _stream(x.device), *kern)
    check(rc, entry)

  def _empty(self, x: torch.Tensor, *tail) -> torch.Tensor:
    """An output [S, L, *tail] beside x."""
    return torch.empty(self.num_samples, self.omega.shape[0], *tail, dtype=self.dtype, device=x.device)

  def _latent_values(self, x: torch.Tensor) -> torch.Tensor:
    out = self._empty(x)
    self._run("mm_pathwise_eval", (x,), (out,))
    return out

  def eval_jac(self, x: torch.Tensor):
    """f_s(x_s) and its Jacobian: x [S, d] -> (f [S, L], d f / d x [S, L, d]) from ONE pass over the weight stream (d <= 16; for
    d > 8 a wave takes the four samples of a group two at a time).  f is bit-equal to ``__call__``'s.  Mixed paths: (W g + c, W J_g)."""
    g, jac = self._latent_jac(x)
    if self.mix_W is None:
      return g, jac
    return self._mixed_values(g), torch.einsum('il,sld->sid', self.mix_W, jac.to(DEFAULT_FLOAT)).to(self.dtype)

  def _latent_jac(self, x: torch.Tensor):
    out, jac = self._empty(x), self._empty(x, self.omega.shape[1])
    self._run("mm_pathwise_eval_jac", (x,), (out, jac))
    return out, jac

  def eval_with_bound(self, x: torch.Tensor):
    """f_s(x_s) and a bound on what this dtype's rounding did to it: x [S, d] -> (f [S, L], err [S, L]) from ONE pass over the
    weight stream (``mm_pathwise_eval_bound``).  err = BOUND_ULPS u (scale sum_k |w cos| + var sum_m |v k|): the update weights
    v = Kuu^-1 (u - Phi w) cancel 1e5 .. 1e7-fold in sum_m v_m k(x, z_m) at M = 2000, so a float32 sample's value can have lost
    its digits (C5 shard: ~2e-2 of max |f|) -- this is where the caller sees it; float64 paths are the accurate mode.  Mixed paths:
    (W g + c, |W| err_g)."""
    g, err = self._latent_bound(x)
    if self.mix_W is None:
      return g, err
    return self._mixed_values(g), (err.to(DEFAULT_FLOAT) @ self.mix_W.abs().T).to(self.dtype)

  def _latent_bound(self, x: torch.Tensor):
    out, ab = self._empty(x), self._empty(x)
    self._run("mm_pathwise_eval_bound", (x,), (out, ab))
    # unit roundoff u = finfo.eps / 2; v and the basis value each carry ~u, the exponent's own rounding (|arg| up to ~20 at the
    # C5 shape) a few u more: BOUND_ULPS u covers the measured worst case with a factor ~2 in hand (tests/test_pathwise.py)
    return out, ab * (BOUND_ULPS * 0.5 * torch.finfo(self.dtype).eps)

  def flagged(self, x: torch.Tensor, tol: float):
    """(f, mask [S, L], count): the (sample, latent) values whose rounding bound exceeds ``tol`` x max |f| of the batch."""
    f, err = self.eval_with_bound(x)
    mask = err > tol * f.abs().amax()
    return f, mask, int(mask.sum().item())

  def rollout(self, x0: torch.Tensor, num_steps: int, dt: float = 1.0, keep_trajectory: bool = False):
    """Drift-only Euler rollout of all S paths (d == L): x <- x + dt f(x), H steps in one ABI call."""
    if self.mix_W is not None:
      raise ValueError("Paths.rollout: the drift-only rollout does not mix (these paths carry mix_W: f = W g + c); step "
                       "x + dt paths(x) in torch, or use PolicyRollout")
    x = x0.contiguous().clone()
    tmp = torch.empty_like(x)
    traj = torch.empty(num_steps, *x.shape, dtype=self.dtype, device=x.device) if keep_trajectory else None
    self._run("mm_pathwise_rollout", (x, tmp), (traj,), steps=(int(num_steps), float(dt)))
    return (x, traj) if keep_trajectory else x


class _PathsEval(torch.autograd.Function):
  """f = paths(x) with d f / d x from the same weight-stream pass (``mm_pathwise_eval_jac``)."""

  @staticmethod
  def forward(ctx, x, paths):
    f, jac = paths.eval_jac(x.detach())
    ctx.save_for_backward(jac)
    return f

  @staticmethod
  def backward(ctx, g):
    (jac,) = ctx.saved_tensors
    return torch.einsum('sl,sld->sd', g, jac), None


def paths_from_arrays(omega, phase, w, v, Z, lengthscales, variance, mean_c=None, dtype=torch.float32,
                      device="cuda", mix_W=None, mix_c=None, kernel="se") -> Paths:
  """Build ``Paths`` from explicit arrays (omega [L,K,d], phase [L,K], w [S,L,K], v [S,L,M], Z [L,M,d]).  ``mix_W`` [nx, L] (and
  ``mix_c`` [nx] or None): the mixing of a coregionalised model; the latents then have no mean of their own.  ``kernel``: the
  family of every latent, "se" | "matern32" | "matern52" (or its code)."""
  kernel = _kernel_code(kernel)
  t64 = lambda a: torch.as_tensor(a, dtype=DEFAULT_FLOAT, device=device)
  if mix_W is None and mix_c is not None:
    raise ValueError("mix_c without mix_W")
  if mix_W is not None:
    if mean_c is not None:
      raise ValueError("mixed paths carry no latent mean: the constant is mix_c, added after the mixing")
    mix_W = t64(mix_W).contiguous()
    mix_c = None if mix_c is None else t64(mix_c).reshape(-1).contiguous()
    if mix_W.ndim != 2 or mix_W.shape[1] != omega.shape[0] or (mix_c is not None and mix_c.shape[0] != mix_W.shape[0]):
      raise ValueError(f"mix_W must be [nx, L = {omega.shape[0]}] and mix_c [nx], got {tuple(mix_W.shape)} and "
                       f"{None if mix_c is None else tuple(mix_c.shape)}")
  mult = 128 if dtype == torch.float64 else 256          # BT: terms per block of the weight stream
  xscale = math.sqrt(math.log2(math.e)) / t64(lengthscales)                    # [L, d]
  zs = t64(Z) * xscale[:, None, :]
  hz = 0.5 * (zs * zs).sum(-1)
  K = omega.shape[1]
  tt = lambda a: a.to(dtype).contiguous()
  padk = lambda a: tt(_pad_last(t64(a), mult))
  two_pi = 2.0 * math.pi
  omega_p = tt(_pad_last(t64(omega).transpose(1, 2) / two_pi, mult))           # [L, d, Kp]
  zs_p = tt(_pad_last(zs.transpose(1, 2), mult))                                # [L, d, Mp]
  var = t64(variance)
  # blocked weight stream [G, L, NB, 4, BT]
  wp, vp = _pad_last(t64(w), mult), _pad_last(t64(v), mult)
  S, L = wp.shape[:2]
  G = (S + 3) // 4
  allw = torch.cat([wp, vp], dim=-1)                                              # [S, L, Kp + Mp]
  if G * 4 != S:
    allw = torch.cat([allw, torch.zeros(G * 4 - S, L, allw.shape[-1], dtype=DEFAULT_FLOAT, device=device)], 0)
  NB = allw.shape[-1] // mult
  wb = allw.reshape(G, 4, L, NB, mult).permute(0, 2, 3, 1, 4).to(dtype).contiguous()
  return Paths(omega=omega_p, phase=padk(t64(phase) / two_pi), zs=zs_p, hz=padk(hz), wb=wb, num_samples=S,
               lengthscales=xscale.contiguous(), prior_scale=torch.sqrt(2.0 * var / K).contiguous(),
               variance=var.contiguous(), mean_c=None if mean_c is None else t64(mean_c).contiguous(), mix_W=mix_W, mix_c=mix_c,
               kernel=kernel)


def _mean_and_mixing(model: SVGP, L: int, device):
  """-> (mean_c [L] | None, mix_W [nx, Lg] | None, mix_c [nx] | None), float64 on ``device``: a ``LinearCoregionalization`` kernel
  mixes its L = Lg latent paths with W and adds the Constant mean (nx entries, or one value for all) afterwards."""
  c = None
  if isinstance(model.mean_function, Constant):
    c = model.mean_function.c.detach().to(device=device, dtype=DEFAULT_FLOAT)
  elif not isinstance(model.mean_function, Zero):
    raise NotImplementedError
  if not isinstance(model.kernel, LinearCoregionalization):
    return (None if c is None else c.expand(L).contiguous()), None, None
  W = model.kernel.W.detach().to(device=device, dtype=DEFAULT_FLOAT).clone().contiguous()
  if W.ndim != 2 or W.shape[1] != L:
    raise ValueError(f"LinearCoregionalization: W {tuple(W.shape)} does not match the {L} latent kernels")
  return None, W, (None if c is None else c.expand(W.shape[0]).clone().contiguous())


@dataclass
class MeanDrift:
  """The posterior MEAN of a frozen model as the native entries take it: what a drift wrapped in a ``KernelRegressor`` (the
  reference's ``build_dynamics(..., model_uncertainty=False)``, gpflow_pilco/loops/pilco.py:45-79) evaluates for every sample
  under the Euler solver.  The operands are ``Paths``' update half with ONE weight vector per latent, beta = Kuu^-1 u
  (``SVGP._mean_weights``), in place of the per-sample stream: no prior half, no sample axis -- ``__call__`` and ``eval_jac`` take
  any number of rows.  ``mix_W`` / ``mix_c`` as in ``Paths``: the mean of a coregionalised model, W g + c.  Evaluation runs in
  ``mm_pathwise_mean_eval`` (csrc/mm_pathwise_mean.hip: the operands staged through LDS, nothing of size S M in memory);
  ``PolicyRollout`` takes a ``MeanDrift`` in place of ``Paths``."""
  zs: torch.Tensor             # [L, d, Mp]   (Z * x_scale)^T, x_scale = sqrt(log2 e) / lengthscales
  hz: torch.Tensor             # [L, Mp]      |zs|^2 / 2
  beta: torch.Tensor           # [L, Mp] f64  Kuu^-1 u, zero beyond M
  lengthscales: torch.Tensor   # [L, d] f64: x_scale, as in Paths
  variance: torch.Tensor       # [L] f64
  mean_c: Optional[torch.Tensor]  # [L] f64 or None
  mix_W: Optional[torch.Tensor] = None   # [nx, Lg] f64
  mix_c: Optional[torch.Tensor] = None   # [nx] f64 or None
  kernel: int = 0
  num_centres: int = 0                   # M: the centres before padding

  PAD = 32                               # Mp is a multiple of it (the entry itself takes any M)

  @property
  def dtype(self):
    return self.zs.dtype

  @property
  def device(self):
    return self.zs.device

  def _dims(self):
    L, d, Mp = self.zs.shape
    return L, Mp, d

  @classmethod
  def from_arrays(cls, Z, lengthscales, variance, beta, mean_c=None, dtype=torch.float32, device="cuda", mix_W=None, mix_c=None,
                  kernel="se") -> "MeanDrift":
    """Z [L, M, d], lengthscales [L, d], variance [L], beta [L, M] (and mean_c [L], or the mixing of a coregionalised model):
    the expressions of ``paths_from_arrays`` for the operands the two share."""
    kernel = _kernel_code(kernel)
    t64 = lambda a: torch.as_tensor(a, dtype=DEFAULT_FLOAT, device=device).detach()
    if mix_W is None and mix_c is not None:
      raise ValueError("mix_c without mix_W")
    if mix_W is not None and mean_c is not None:
      raise ValueError("a mixed mean carries no latent mean: the constant is mix_c, added after the mixing")
    xscale = math.sqrt(math.log2(math.e)) / t64(lengthscales)
    zs = t64(Z) * xscale[:, None, :]
    hz = 0.5 * (zs * zs).sum(-1)
    tt = lambda a: a.to(dtype).contiguous()
    beta = t64(beta)
    if beta.shape != zs.shape[:2]:
      raise ValueError(f"beta must be [L, M] = {tuple(zs.shape[:2])}, got {tuple(beta.shape)}")
    return cls(zs=tt(_pad_last(zs.transpose(1, 2), cls.PAD)), hz=tt(_pad_last(hz, cls.PAD)),
               beta=_pad_last(beta, cls.PAD).contiguous(), lengthscales=xscale.contiguous(), variance=t64(variance).contiguous(),
               mean_c=None if mean_c is None else t64(mean_c).contiguous(),
               mix_W=None if mix_W is None else t64(mix_W).contiguous(),
               mix_c=None if mix_c is None else t64(mix_c).reshape(-1).contiguous(), kernel=kernel, num_centres=int(Z.shape[1]))

  @classmethod
  def from_model(cls, model, dtype=torch.float32, device="cuda") -> "MeanDrift":
    """The mean of an ``SVGP`` / ``PathwiseSVGP`` (or of a ``KernelRegressor`` around one), SquaredExponential or Matern.  Cached
    on the model per (dtype, device) and per version of its parameters, like its packs: an in-place update makes the next call
    rebuild it; a cache hit reads nothing from the device (a HIP-graph capture of a closure that calls this is fine once warm)."""
    from .models import GPModelWrapper
    while isinstance(model, GPModelWrapper):
      model = model.model
    if not isinstance(model, SVGP):
      raise TypeError(f"MeanDrift.from_model takes an SVGP (or a KernelRegressor around one), got {type(model).__name__}")
    device = torch.device(device)
    params = list(model._parameters())
    if isinstance(model.kernel, LinearCoregionalization):
      params.append(model.kernel.W)
    family = kernel_family(model.latent_kernels)
    key = tuple((id(t), t._version, t.device) for t in params) + (family,)
    cache = model.__dict__.setdefault("_mean_drift_cache", {})
    slot = (dtype, str(device))
    hit = cache.get(slot)
    if hit is not None and hit[0] == key:
      return hit[1]
    with torch.no_grad():
      Z, ls, var, beta, _ = model._mean_weights(device, family)
      mean_c, mix_W, mix_c = _mean_and_mixing(model, Z.shape[0], device)
      out = cls.from_arrays(Z, ls, var, beta, mean_c, dtype=dtype, device=device, mix_W=mix_W, mix_c=mix_c, kernel=family)
    cache[slot] = (key, out)
    return out

  def _mixed_values(self, g: torch.Tensor) -> torch.Tensor:
    f = g.to(DEFAULT_FLOAT) @ self.mix_W.T
    return (f if self.mix_c is None else f + self.mix_c).to(self.dtype)

  def _operands(self):
    """((L, Mp, d), the six drift operands zs_t .. beta) in the order of the C ABI: ``Paths._operands`` for a mean-only drift."""
    return self._dims(), (self.zs.data_ptr(), self.hz.data_ptr(), self.lengthscales.data_ptr(), self.variance.data_ptr(),
                          _ptr(self.mean_c), self.beta.data_ptr())

  def _eval(self, x: torch.Tensor, jac: bool):
    _require_device(x, self.zs)
    (L, Mp, d), drift = self._operands()
    if x.ndim != 2 or x.shape[1] != d or x.dtype != self.dtype:
      raise ValueError(f"expected x [S,{d}] of {self.dtype}, got {tuple(x.shape)} {x.dtype}")
    x = x.contiguous()
    S = x.shape[0]
    out = torch.empty(S, L, dtype=self.dtype, device=x.device)
    J = torch.empty(S, L, d, dtype=self.dtype, device=x.device) if jac else None
    rc = _lib.lib().mm_pathwise_mean_eval(S, L, Mp, d, _dtype_code(self.dtype), x.data_ptr(), *drift, out.data_ptr(), _ptr(J),
                                          _stream(x.device), int(self.kernel))
    check(rc, "mm_pathwise_mean_eval")
    return out, J

  def __call__(self, x: torch.Tensor) -> torch.Tensor:
    """x [S, d] -> the mean [S, L] (mixed: [S, nx]); differentiable in x through the Jacobian of the same pass."""
    if torch.is_grad_enabled() and x.requires_grad:
      return _PathsEval.apply(x, self)
    g = self._eval(x, False)[0]
    return g if self.mix_W is None else self._mixed_values(g)

  def eval_jac(self, x: torch.Tensor):
    """-> (f [S, L], d f / d x [S, L, d]) from one pass; mixed: (W g + c, W J_g).  f is bit-equal to ``__call__``'s."""
    g, jac = self._eval(x, True)
    if self.mix_W is None:
      return g, jac
    return self._mixed_values(g), torch.einsum('il,sld->sid', self.mix_W, jac.to(DEFAULT_FLOAT)).to(self.dtype)


def generate_paths(model: SVGP, num_samples: int, num_bases: int = 1024, dtype=torch.float32,
                   device="cuda", generator: Optional[torch.Generator] = None) -> Paths:
  """Draw S decoupled sample paths of an SVGP: random-Fourier prior + inducing-point update
  (gpflow_sampling's decoupled sampler; ``loops/pilco.py:281-284``)."""
  kernels, Zs = unpack_multioutput(model.kernel, model.inducing_variable, model.num_latent_gps)
  family = kernel_family(kernels)
  Z, ls, var = _stack_kernel_params(kernels, Zs, device)
  L, M, d = Z.shape
  S, K = num_samples, num_bases
  rn = lambda *shape: torch.randn(*shape, dtype=DEFAULT_FLOAT, device=device, generator=generator)
  n = rn(L, K, d)
  phase = 2.0 * math.pi * torch.rand(L, K, dtype=DEFAULT_FLOAT, device=device, generator=generator)
  w = rn(S, L, K)
  Luu = cholesky(_gram(Z, ls, var, family))
  q_mu = model.q_mu.to(device=device, dtype=DEFAULT_FLOAT).T                       # [L, M]
  q_sqrt = torch.tril(model.q_sqrt.to(device=device, dtype=DEFAULT_FLOAT))          # [L, M, M]
  eps = rn(S, L, M)
  # a Matern model's chi2 normals come AFTER every draw a SquaredExponential model makes: SE draws from a generator state are
  # what they always were, and PathSampler draws in the same order
  omega = spectral_frequencies(n, ls, family, None if family == KERNEL_SE else rn(L, K, 3 if family == 1 else 5))
  u = q_mu[None] + torch.einsum('slm,lnm->sln', eps, q_sqrt)                       # samples of q(u)
  if model.whiten:
    u = torch.einsum('lnm,slm->sln', Luu, u)
  Phi_Z = torch.sqrt(2.0 * var / K)[:, None, None] * torch.cos(Z @ omega.transpose(1, 2) + phase[:, None, :])  # [L,M,K]
  resid = u - torch.einsum('lmk,slk->slm', Phi_Z, w)
  v = torch.cholesky_solve(resid.permute(1, 2, 0), Luu).permute(2, 0, 1)             # [S, L, M]
  mean_c, mix_W, mix_c = _mean_and_mixing(model, L, device)
  return paths_from_arrays(omega, phase, w, v, Z, ls, var, mean_c, dtype=dtype, device=device, mix_W=mix_W, mix_c=mix_c,
                           kernel=family)


class PathSampler:
  """Draws sample paths of ONE model over and over (``PathwisePILCO``: new paths on every optimiser step) without redoing what
  does not depend on the draw.

  Cached per version of the model's parameters (keyed on the tensors' ``_version`` like ``models._PackCache``; rebuilt lazily by the
  next ``draw`` after an in-place update): the stacked Z, lengthscales and variances, ``Luu = chol(Kuu + jitter)`` (one
  ``linalg.cholesky`` with its check), ``q(u)``'s mean and factor -- mapped through ``Luu`` for a whitened model, so that
  u = c + T eps is one batched GEMM -- and the model-constant operands of ``Paths`` (``zs``, ``hz``, ``lengthscales``, ``prior_scale``,
  ``variance``, ``mean_c``, and for a coregionalised model ``mix_W``, ``mix_c``: the torch expressions of ``paths_from_arrays``).  Preallocated once: the float64 draw buffers
  ``n [L,K,d]``, ``b [L,K]``, ``w [S,L,K]``, ``eps [S,L,M]``, ``Phi_Z [L,M,K]``, the right-hand side ``[L,M,S]`` the two triangular
  solves run in place on, and the outputs ``omega``, ``phase``, ``wb`` in the stream dtype.

  ``draw()``: RNG fills in ``generate_paths``'s order (the same generator state gives the same numbers) -> ``mm_pathwise_basis`` ->
  u and u - Phi_Z w as two batched GEMMs into ``[L,M,S]`` -> two triangular solves with the cached factor ->
  ``mm_pathwise_pack_stream``, all on the current stream.  After the first call a draw performs no host synchronisation and keeps
  no new memory, and it can be captured in a HIP graph (``generator=None`` only; draw once eagerly first: a stale cache cannot be
  rebuilt under capture, its factorisation check reads the device)."""

  def __init__(self, model: SVGP, num_samples: int, num_bases: int = 1024, dtype=torch.float32, device="cuda"):
    self.model, self.S, self.K = model, int(num_samples), int(num_bases)
    self.dtype, self.device = dtype, torch.device(device)
    self._code = _dtype_code(dtype)
    if self.S <= 0 or self.K <= 0:
      raise ValueError("PathSampler needs num_samples >= 1 and num_bases >= 1")
    if not self.device.type == "cuda":
      raise RuntimeError("gpflowpilco_amd kernels run on the GPU only (no CPU fallback): PathSampler on " + str(self.device))
    self._key = None
    self._bufs = None

  # -- what depends on the model alone ------------------------------------------------------------------------------------------
  def _refresh(self):
    model, dev = self.model, self.device
    params = list(model._parameters())                       # (the Constant mean's tensor is one of them)
    if isinstance(model.kernel, LinearCoregionalization):
      params.append(model.kernel.W)
    family = kernel_family(model.latent_kernels)
    key = tuple((id(t), t._version, t.device) for t in params) + (family,)
    if key == self._key:
      return
    if torch.cuda.is_current_stream_capturing():
      raise RuntimeError("PathSampler: the model changed since the last draw (or nothing was drawn yet); draw() once outside the "
                         "graph capture first")
    with torch.no_grad():
      kernels, Zs = unpack_multioutput(model.kernel, model.inducing_variable, model.num_latent_gps)
      Z, ls, var = _stack_kernel_params(kernels, Zs, dev)
      L, M, d = Z.shape
      if d > _lib.MM_DMAX:
        raise ValueError(f"PathSampler: input dimension {d} exceeds MM_DMAX = {_lib.MM_DMAX}")
      Luu = cholesky(_gram(Z, ls, var, family))
      q_mu = model.q_mu.to(device=dev, dtype=DEFAULT_FLOAT).T                        # [L, M]
      q_sqrt = torch.tril(model.q_sqrt.to(device=dev, dtype=DEFAULT_FLOAT))           # [L, M, M]
      c, T = q_mu.unsqueeze(-1), q_sqrt
      if model.whiten:                                                                # u = Luu (q_mu + q_sqrt eps)
        c, T = Luu @ c, Luu @ T
      mean_c, mix_W, mix_c = _mean_and_mixing(model, L, dev)
      # the model-constant operands of Paths, by the expressions of paths_from_arrays
      mult = 128 if self.dtype == torch.float64 else 256
      tt = lambda a: a.to(self.dtype).contiguous()
      xscale = math.sqrt(math.log2(math.e)) / ls
      zs = Z * xscale[:, None, :]
      hz = 0.5 * (zs * zs).sum(-1)
      self._const = dict(zs=tt(_pad_last(zs.transpose(1, 2), mult)), hz=tt(_pad_last(hz, mult)), lengthscales=xscale.contiguous(),
                         prior_scale=torch.sqrt(2.0 * var / self.K).contiguous(), variance=var.contiguous(), mean_c=mean_c,
                         mix_W=mix_W, mix_c=mix_c, kernel=family)
      self._Z, self._ls, self._var = Z.contiguous(), ls.contiguous(), var.contiguous()
      self._Luu, self._LuuT = Luu.contiguous(), Luu.transpose(1, 2)
      self._c, self._T = c.contiguous(), T.contiguous()
    dof = 0 if family == KERNEL_SE else 3 if family == 1 else 5
    if self._bufs is None or self._dims != (L, M, d) or self._dof != dof:
      self._dims, self._dof = (L, M, d), dof
      S, K = self.S, self.K
      f64 = lambda *shape: torch.empty(*shape, dtype=DEFAULT_FLOAT, device=dev)
      Kp, Mp, G = K + (-K) % mult, M + (-M) % mult, (S + 3) // 4
      out = lambda *shape: torch.empty(*shape, dtype=self.dtype, device=dev)
      self._bufs = dict(n=f64(L, K, d), b=f64(L, K), w=f64(S, L, K), eps=f64(S, L, M), phiZ=f64(L, M, K), rhs=f64(L, M, S),
                        omega=out(L, d, Kp), phase=out(L, Kp), wb=out(G, L, (Kp + Mp) // mult, 4, mult))
      if dof:                                                # the chi2 normals of a Matern draw and the scale they give
        self._bufs.update(chi=f64(L, K, dof), tscale=f64(L, K))
    self._key = key

  @property
  def buffers(self):
    """The static buffers of the last draw (``n``, ``b``, ``w``, ``eps``, ``phiZ``, ``rhs`` = the update weights v as [L,M,S],
    ``omega``, ``phase``, ``wb``); the next ``draw`` overwrites them."""
    return self._bufs

  def draw(self, generator: Optional[torch.Generator] = None, clone: bool = False) -> Paths:
    """New sample paths.  The returned ``Paths`` holds the sampler's STATIC buffers: the next ``draw`` (or the replay of a graph
    that captured one) overwrites them; ``clone=True`` returns an independent copy."""
    if generator is not None and torch.cuda.is_current_stream_capturing():
      raise RuntimeError("PathSampler.draw: under graph capture only generator=None (the default generator, which the capture "
                         "registers) is supported")
    self._refresh()
    B, (L, M, d), S, K = self._bufs, self._dims, self.S, self.K
    with torch.no_grad():
      B["n"].normal_(generator=generator)
      B["b"].uniform_(generator=generator).mul_(2.0 * math.pi)
      B["w"].normal_(generator=generator)
      B["eps"].normal_(generator=generator)
      if self._dof:
        # Matern: n <- n sqrt(2 nu / chi2) in place (spectral_frequencies' expressions, into preallocated buffers), drawn after
        # everything else as generate_paths does; mm_pathwise_basis then divides by the lengthscales as for any family
        B["chi"].normal_(generator=generator)
        torch.mul(B["chi"], B["chi"], out=B["chi"])
        torch.sum(B["chi"], dim=-1, out=B["tscale"])
        B["tscale"].reciprocal_().mul_(float(self._dof)).sqrt_()
        B["n"].mul_(B["tscale"].unsqueeze(-1))
      lib, stream = _lib.lib(), _stream(self.device)
      check(lib.mm_pathwise_basis(L, K, M, d, self._code, B["n"].data_ptr(), B["b"].data_ptr(), self._Z.data_ptr(),
                                  self._ls.data_ptr(), self._var.data_ptr(), B["omega"].data_ptr(), B["phase"].data_ptr(),
                                  B["phiZ"].data_ptr(), stream), "mm_pathwise_basis")
      rhs = B["rhs"]
      torch.baddbmm(self._c.expand(L, M, S), self._T, B["eps"].permute(1, 2, 0), out=rhs)        # u = c + T eps      [L, M, S]
      rhs.baddbmm_(B["phiZ"], B["w"].permute(1, 2, 0), alpha=-1.0)                               # u - Phi_Z w
      torch.linalg.solve_triangular(self._Luu, rhs, upper=False, out=rhs)
      torch.linalg.solve_triangular(self._LuuT, rhs, upper=True, out=rhs)                        # v = Kuu^-1 (u - Phi_Z w)
      check(lib.mm_pathwise_pack_stream(S, L, K, M, self._code, B["w"].data_ptr(), rhs.data_ptr(), B["wb"].data_ptr(), stream),
            "mm_pathwise_pack_stream")
      cp = (lambda t: t.clone() if isinstance(t, torch.Tensor) else t) if clone else (lambda t: t)
      return Paths(omega=cp(B["omega"]), phase=cp(B["phase"]), wb=cp(B["wb"]), num_samples=S,
                   **{k: cp(v) for k, v in self._const.items()})


class PathwiseSVGP(SVGP):
  """``gpflow_pilco.models.PathwiseSVGP`` (models/svgp.py:124-130): an SVGP whose ``__call__``
  evaluates the currently attached sample paths."""

  _paths: Optional[Paths] = None

  def generate_paths(self, num_samples: int, num_bases: int = 1024, sample_axis: int = 0,
                     dtype=torch.float32, device="cuda", generator=None) -> Paths:
    assert sample_axis == 0
    return generate_paths(self, num_samples, num_bases, dtype=dtype, device=device, generator=generator)

  def path_sampler(self, num_samples: int, num_bases: int = 1024, dtype=torch.float32, device="cuda") -> PathSampler:
    """A ``PathSampler`` of this model: ``.draw()`` is ``generate_paths`` for repeated use."""
    return PathSampler(self, num_samples, num_bases, dtype=dtype, device=device)

  @contextlib.contextmanager
  def set_temporary_paths(self, paths: Paths):
    prev, self._paths = self._paths, paths
    try:
      yield
    finally:
      self._paths = prev

  def predict_f_samples(self, x: torch.Tensor, **kwargs) -> torch.Tensor:
    if self._paths is None:
      raise RuntimeError("no sample paths attached: use generate_paths / set_temporary_paths")
    return self._paths(x)

  def __call__(self, x, **kwargs):
    return self.predict_f_samples(x, **kwargs)


class PolicyRollout:
  """The pathwise policy rollout on the device (csrc/mm_pathwise_policy.hip: ``mm_pathwise_policy_rollout``; several actions:
  ``mm_pathwise_policy_rollout_nd``, the same kernels): per sample path encoder -> policy mean through
  Chain[Scale, Shift, NormalCDF] -> drift sample -> Euler -> cost -- the body of ``PathwisePILCO._policy_loss_closure``
  (gpflow_pilco/loops/pilco.py:263-298).

  ``paths``: the drift's sample paths (nx latents on nd = nx + na + nu inputs, nd <= 8; ``wide=True``: nd <= 16); ``policy``: an ``ops.PackedModel`` with
  one latent per action (nu = 1 .. 4) on ne = nx + na inputs (any dtype: only its float64 blocks are read); ``head_scale`` /
  ``head_shift``: a float, or one value per action.  The actions follow the encoding in latent order.  A one-latent pack with
  float head constants runs the one-action entries (wrappers of the ``_nd`` ones: nu = 1, head constants by value, ``g_policy``
  without the latent axis); nu > 1 (or ``nd_entries=True``) the ``_nd`` entries.  ``wide=True``: the
  ``_wide`` entries (same signatures and results, any nu), which take nd <= 16.
  ``__call__(x0, H)`` -> ``(cost [H, S], tape)``; ``backward(tape, g_cost)`` -> ``(g_policy, g_x0 [S, nx] | None)`` with
  g_policy [M ne + M + ne + 2] from the one-action entries and [nu, M ne + M + ne + 2] from the ``_nd`` ones (per latent dZ,
  dbeta, d ls^2, dvar, dmean).  ``supports_backward()``: whether the reverse sweep takes this shape (its LDS bound:
  include/gpflowpilco_mm.h).

  ``target`` / ``precis`` None: a zero target and a zero precision of the right size (the entries need the pointers); the cost
  output is then meaningless -- the rollout of a caller whose loss is its own function of the states: ``trajectory(tape, H)`` gives
  x_1 .. x_H, and ``backward(..., g_states=...)`` (the ``_seeded`` entries) carries d loss / d x_1 .. x_H back to the policy and
  to x_0, with or without a ``g_cost`` of the built-in cost beside it.

  Paths with ``mix_W`` (a coregionalised drift: Lg latents mixed to nx outputs, Lg <= nx) run the ``_mixed`` entries -- nd <= 16,
  1 to 4 actions, the ``_nd`` shapes of ``g_policy``; ``wide`` and ``nd_entries`` are then ignored.  The tape's sample slot and
  Jacobian block are latent-sized (``mm_pathwise_tape_bytes_mixed``); the mixing happens in the head kernel and the reverse sweep.

  Paths of a Matern drift (``paths.kernel`` 1 or 2) run the one forward entry ``mm_pathwise_policy_rollout_kern`` for every shape --
  one action included -- with the ``_wide`` signatures, tape and reverse sweeps (mixed paths: the ``_mixed`` ones): ``wide`` and
  ``nd_entries`` are then ignored and ``g_policy`` has the ``_nd`` shape.  The policy stays SquaredExponential.

  A ``MeanDrift`` in place of ``paths`` (a mean-only drift: every sample steps with the posterior mean) runs the one forward entry
  ``mm_pathwise_policy_rollout_mean`` under the same rules as a Matern drift -- the ``_wide`` / ``_mixed`` tape and sweeps, the
  ``_nd`` shape of ``g_policy``, any family, with or without mixing.  It has no sample axis: ``num_samples`` (the rows of the x0
  this rollout will be called with) is then required."""

  def __init__(self, paths, policy, nx: int, active_dims, head_scale, head_shift,
               target: Optional[torch.Tensor] = None, precis: Optional[torch.Tensor] = None, nd_entries: Optional[bool] = None,
               wide: bool = False, num_samples: Optional[int] = None):
    self.mean = isinstance(paths, MeanDrift)
    if self.mean:
      if num_samples is None or int(num_samples) < 1:
        raise ValueError("a MeanDrift has no sample axis: pass num_samples (the rows of x0)")
      (L, Mp, d), S = paths._dims(), int(num_samples)
      wide, nd_entries = True, True
    else:
      S, L, Mp, Kp, d = paths._dims()
      if num_samples is not None and int(num_samples) != S:
        raise ValueError(f"num_samples = {num_samples}, but the paths hold {S} samples")
    self.S = int(S)
    self.paths, self.policy = paths, policy
    self.nx, self.active = int(nx), tuple(int(i) for i in active_dims)
    self.na = len(self.active)
    self.nu = int(policy.L)
    self.ne, self.nd = self.nx + self.na, self.nx + self.na + self.nu
    if not 1 <= self.nu <= 4:
      raise ValueError(f"the pathwise policy rollout takes policies with 1 to 4 latents (one per action), got {self.nu}")
    mix_W = getattr(paths, "mix_W", None)
    self.kernel = int(getattr(paths, "kernel", 0))
    if self.kernel:                                            # a Matern drift: the one _kern entry (the _wide signatures and tape)
      wide, nd_entries = True, True
    self.mixed = mix_W is not None
    self.Lg = int(L) if self.mixed else 0
    if self.mixed:
      if mix_W.ndim != 2 or mix_W.shape[0] != self.nx or mix_W.shape[1] != L:
        raise ValueError(f"shapes do not compose: mix_W {tuple(mix_W.shape)} (want [nx = {self.nx}, Lg = {L}]: one row per state, "
                         "one column per latent path)")
      if L > self.nx:
        raise ValueError(f"the mixed pathwise policy rollout takes Lg <= nx latents, got Lg = {L} > nx = {self.nx}")
      mix_c = getattr(paths, "mix_c", None)
      if mix_c is not None and tuple(mix_c.shape) != (self.nx,):
        raise ValueError(f"shapes do not compose: mix_c {tuple(mix_c.shape)} (want [nx = {self.nx}])")
      wide, nd_entries = True, True
    if (not self.mixed and L != self.nx) or d != self.nd or policy.d != self.ne:
      raise ValueError(f"shapes do not compose: paths L={L} d={d} (want {self.nx}, {self.nd}), policy L={policy.L} d={policy.d} "
                       f"(want {self.nu}, {self.ne})")
    self.wide = bool(wide)
    if self.nd > (16 if self.wide else 8) or policy.M > 256:
      raise ValueError(f"the pathwise policy rollout takes drift inputs of dimension <= {16 if self.wide else 8} and policies of "
                       "<= 256 centres")

    def per_action(v, what):
      if isinstance(v, torch.Tensor):
        v = v.detach().reshape(-1).tolist()
      vals = tuple(float(t) for t in v) if isinstance(v, (list, tuple)) else (float(v),) * self.nu
      if len(vals) == 1 and self.nu > 1:
        vals = vals * self.nu
      if len(vals) != self.nu:
        raise ValueError(f"{what}: expected a float or one value per action ({self.nu}), got {len(vals)}")
      return vals
    scales, shifts = per_action(head_scale, "head_scale"), per_action(head_shift, "head_shift")
    self.nd_entries = (self.nu > 1 or self.wide) if nd_entries is None else bool(nd_entries)
    if self.wide and not self.nd_entries:
      raise ValueError("nd_entries=False: the wide entries have the _nd signatures")
    if self.nu > 1 and not self.nd_entries:
      raise ValueError("nd_entries=False: the one-action entries take one-latent policies")
    if self.nd_entries:
      self.scale, self.shift = scales, shifts
      self._scale_c, self._shift_c = (_lib.C.c_double * self.nu)(*scales), (_lib.C.c_double * self.nu)(*shifts)
    else:
      self.scale, self.shift = scales[0], shifts[0]
    dev = paths.zs.device
    self.target = (torch.zeros(self.ne, dtype=paths.dtype, device=dev) if target is None else
                   target.to(dtype=paths.dtype, device=dev).contiguous())
    self.precis = (torch.zeros(self.ne, self.ne, dtype=paths.dtype, device=dev) if precis is None else
                   precis.to(dtype=paths.dtype, device=dev).contiguous())
    self._act = (_lib.C.c_int32 * self.na)(*self.active)
    if self.mixed:
      self._mix_W = mix_W.detach().to(dtype=torch.float64, device=dev).contiguous()
      self._mix_c = None if mix_c is None else mix_c.detach().to(dtype=torch.float64, device=dev).contiguous()
    # which entries this rollout calls and what its argument lists carry besides the buffers, decided here once.  The one-action
    # entries take no action count and their head constants by value; the others the count and one array per constant.
    sfx = "wide" if self.wide else "nd"                        # which set of entries with the _nd signatures
    stem = "mm_pathwise_policy_rollout"
    self._bounded_scratch_query = f"mm_pathwise_backward_scratch_bytes_{sfx}"      # (the mixed sweep's query is the _wide one)
    mixing = (self.Lg, self._mix_W.data_ptr(), _ptr(self._mix_c)) if self.mixed else ()
    if self.nd_entries:
      self._forward = f"{stem}_" + ("mean" if self.mean else "kern" if self.kernel else "mixed" if self.mixed else sfx)
      self._tape_query = "mm_pathwise_tape_bytes_" + ("mixed" if self.mixed else "nd")
      self._scratch_query = self._bounded_scratch_query
      # (unseeded, seeded): the mixed sweep is one entry with the seeded signature
      self._sweeps = (f"{stem}_backward_mixed",) * 2 if self.mixed else (f"{stem}_backward_{sfx}", f"{stem}_backward_{sfx}_seeded")
      self._nu, self._head = (self.nu,), (self._scale_c, self._shift_c)
      # the _kern and _mean entries always take the mixing (none: 0, NULL, NULL) and the family after it
      self._forward_tail = (mixing or (0, None, None)) + (self.kernel,) if self.kernel or self.mean else mixing
    else:
      self._forward, self._tape_query, self._scratch_query = stem, "mm_pathwise_tape_bytes", "mm_pathwise_backward_scratch_bytes"
      self._sweeps = (f"{stem}_backward", f"{stem}_backward_seeded")
      self._nu, self._head, self._forward_tail = (), (self.scale, self.shift), ()
    self._tape_Lg, self._sweep_tail = mixing[:1], mixing[:2]

  def _policy(self, policy):
    pol = self.policy if policy is None else policy
    if (pol.L, pol.M, pol.d) != (self.policy.L, self.policy.M, self.policy.d):
      raise ValueError("the policy pack does not have the shape this rollout was built for")
    return pol

  def supports_backward(self) -> bool:
    """False where the reverse sweep's per-workgroup LDS (the nu policy blocks + four gradient slabs) exceeds 160 KiB."""
    return getattr(_lib.lib(), self._bounded_scratch_query)(self.S, self.policy.M, self.ne, self.nu) > 0

  def __call__(self, x0: torch.Tensor, num_steps: int, dt: float = 1.0, with_jacobians: bool = False, policy=None):
    pol = self._policy(policy)
    P = self.paths
    S = self.S
    _require_device(x0, P.zs)
    if x0.shape != (S, self.nx) or x0.dtype != P.dtype:
      raise ValueError(f"expected x0 [{S},{self.nx}] of {P.dtype}, got {tuple(x0.shape)} {x0.dtype}")
    H, code = int(num_steps), _dtype_code(P.dtype)
    lib = _lib.lib()
    n = getattr(lib, self._tape_query)(S, H, self.nx, self.na, *self._nu, *self._tape_Lg, code, int(with_jacobians))
    if n == 0:
      raise ValueError("mm_pathwise_tape_bytes rejected the shape")
    tape = torch.empty(n, dtype=torch.uint8, device=x0.device)
    cost = torch.empty(H, S, dtype=P.dtype, device=x0.device)
    x0 = x0.contiguous()
    dims, drift = P._operands()
    # a mean-only drift has shared weights: no K, no prior half, beta in the stream's place
    sizes = (S, dims[1]) if self.mean else (S, dims[2], dims[3])
    rc = getattr(lib, self._forward)(*sizes, code, H, float(dt), self.nx, self.na, self._act, *self._nu, *drift,
                                     pol.buf.data_ptr(), pol.nbytes, pol.M, *self._head,
                                     self.target.data_ptr(), self.precis.data_ptr(), x0.data_ptr(), cost.data_ptr(),
                                     tape.data_ptr(), tape.numel(), int(with_jacobians), _stream(x0.device), *self._forward_tail)
    check(rc, self._forward)
    return cost, tape

  def states(self, tape: torch.Tensor, num_steps: int) -> torch.Tensor:
    """x_0 .. x_H [H + 1, S, nx] (a view of the tape)."""
    S = self.S
    es = 8 if self.paths.dtype == torch.float64 else 4
    n = (num_steps + 1) * S * self.nx
    return tape[:n * es].view(self.paths.dtype).view(num_steps + 1, S, self.nx)

  def trajectory(self, tape: torch.Tensor, num_steps: int) -> torch.Tensor:
    """x_1 .. x_H [H, S, nx] (a view of the tape): the states the per-step objective is evaluated on."""
    return self.states(tape, num_steps)[1:]

  def backward(self, tape: torch.Tensor, g_cost: Optional[torch.Tensor], num_steps: int, dt: float = 1.0, policy=None,
               want_state_grad: bool = False, g_states: Optional[torch.Tensor] = None):
    """``g_states`` [H, S, nx] (any float dtype): block h = d loss / d x_{h+1}, the gradient w.r.t. ``trajectory(tape, H)`` -- the
    ``_seeded`` entries; ``g_cost`` may then be None (the built-in cost is not part of the loss).  Without ``g_states``: the
    unseeded entries."""
    pol = self._policy(policy)
    S, H = self.S, int(num_steps)
    if g_cost is None and g_states is None:
      raise ValueError("g_cost may be None only when g_states is given")
    if g_cost is not None:
      g_cost = g_cost.to(torch.float64).contiguous()
      if g_cost.shape != (H, S):
        raise ValueError(f"g_cost must be [H={H}, S={S}]")
    if g_states is not None:
      g_states = g_states.to(torch.float64).contiguous()
      if g_states.shape != (H, S, self.nx):
        raise ValueError(f"g_states must be [H={H}, S={S}, nx={self.nx}]")
      _require_device(g_states, tape)
    return self._sweep(pol, tape, g_cost, g_states, H, float(dt), want_state_grad, seeded=g_states is not None)

  def _sweep(self, pol, tape, g_cost, g_states, H, dt, want_state_grad, seeded):
    """One reverse sweep: the unseeded entry of this rollout's family (one action, ``_nd``, ``_wide``), or -- ``seeded`` -- its
    ``_seeded`` sibling, which takes ``g_x`` after ``g_cost`` (either may be None -> NULL).  g_cost [H, S], g_states [H, S, nx]:
    contiguous f64.  Mixed paths: the one ``_mixed`` entry, which has the seeded signature."""
    S, code, dev = self.S, _dtype_code(self.paths.dtype), tape.device
    npar = pol.M * self.ne + pol.M + self.ne + 2
    g_x0 = torch.empty(S, self.nx, dtype=torch.float64, device=dev) if want_state_grad else None
    seeded = seeded or self.mixed
    seeds = (_ptr(g_cost), _ptr(g_states)) if seeded else (g_cost.data_ptr(),)
    lib = _lib.lib()
    ns = getattr(lib, self._scratch_query)(S, pol.M, self.ne, *self._nu)
    if ns == 0:
      raise ValueError(f"the reverse sweep does not take nu={self.nu}, M={pol.M}, ne={self.ne}: its policy blocks and gradient "
                       "slabs exceed 160 KiB of LDS (see supports_backward)")
    g_pol = torch.empty(*self._nu, npar, dtype=torch.float64, device=dev)
    scratch = torch.empty(ns, dtype=torch.uint8, device=dev)
    entry = self._sweeps[bool(seeded)]
    rc = getattr(lib, entry)(S, code, H, dt, self.nx, self.na, self._act, *self._nu, pol.buf.data_ptr(), pol.nbytes, pol.M,
                             *self._head, self.target.data_ptr(), self.precis.data_ptr(), tape.data_ptr(), tape.numel(), *seeds,
                             g_pol.data_ptr(), _ptr(g_x0), scratch.data_ptr(), scratch.numel(), _stream(dev), *self._sweep_tail)
    check(rc, entry)
    return g_pol, g_x0


def _taped_policy_rollout(ctx, x0, Z, ls, var, beta, mean_c, roll, num_steps, dt):
  """The forward of the two autograd functions below: pack the policy from its packed coordinates, run the taped rollout, keep what
  the backward needs on ``ctx``.  -> (cost [H, S], tape)."""
  from . import ops
  f64 = torch.float64
  det = lambda t: t.detach().to(f64)
  pol = ops.pack_model(det(Z), det(ls), det(var), det(beta), None, det(mean_c), dtype=f64, sync=False)
  cost, tape = roll(x0.detach(), num_steps, dt=dt, with_jacobians=True, policy=pol)
  ctx.roll, ctx.pol, ctx.tape, ctx.H, ctx.dt = roll, pol, tape, int(num_steps), float(dt)
  ctx.save_for_backward(ls)
  ctx.need_state = x0.requires_grad
  ctx.shapes = (Z.shape, ls.shape, var.shape, beta.shape, mean_c.shape)
  ctx.x_dtype = x0.dtype
  return cost, tape


def _policy_rollout_gradients(ctx, g_cost, g_states=None):
  """The backward of the two autograd functions below: one reverse sweep, its packed gradient split per input."""
  (ls,) = ctx.saved_tensors
  g, g_x0 = ctx.roll.backward(ctx.tape, None if g_cost is None else g_cost.T.contiguous(), ctx.H, dt=ctx.dt, policy=ctx.pol,
                              want_state_grad=ctx.need_state, g_states=g_states)
  M, d = ctx.pol.M, ctx.pol.d
  zs, lss, vs, bs, ms = ctx.shapes
  g = g.reshape(ctx.pol.L, -1)                                                           # per latent: dZ, dbeta, d ls^2, dvar, dmean
  gZ = g[:, :M * d].reshape(zs)
  gbeta = g[:, M * d:M * d + M].reshape(bs)
  gls = (2.0 * ls.detach().reshape(-1, d) * g[:, M * d + M:M * d + M + d]).reshape(lss)  # d/d ls = 2 ls d/d ls^2
  gvar = g[:, M * d + M + d].reshape(vs)
  gmean = g[:, M * d + M + d + 1].reshape(ms)
  return (None if g_x0 is None else g_x0.to(ctx.x_dtype)), gZ, gls, gvar, gbeta, gmean, None, None, None


class PolicyRolloutFunction(torch.autograd.Function):
  """The pathwise policy loss as ONE differentiable op: forward = ``mm_pathwise_policy_rollout`` with the Jacobian tape,
  backward = ``mm_pathwise_policy_rollout_backward`` (several actions: the ``_nd`` entries).  The policy enters in packed
  coordinates with a leading latent axis (Z [nu,M,ne], lengthscales [nu,ne], variance [nu], beta [nu,M], mean_c [nu]) computed from
  its parameters by differentiable torch ops, as in ``autodiff.ComposedRolloutFunction``.  Output: cost [S, H]."""

  @staticmethod
  def forward(ctx, x0, Z, ls, var, beta, mean_c, roll, num_steps, dt):
    cost, _ = _taped_policy_rollout(ctx, x0, Z, ls, var, beta, mean_c, roll, num_steps, dt)
    return cost.T.contiguous()

  @staticmethod
  def backward(ctx, g_cost):
    return _policy_rollout_gradients(ctx, g_cost)


class PolicyTrajectoryFunction(torch.autograd.Function):
  """``PolicyRolloutFunction`` with the STATES as a second differentiable output, for a loss the caller evaluates on the sample
  trajectory (a caller-defined objective: ``loops.pathwise_policy_loss_closure(native_objective=True)``) -- the pathwise analogue
  of ``autodiff.ComposedTrajectoryFunction``.  Same inputs; outputs ``(cost [S, H], states [H, S, nx])``: the built-in cost (of
  ``roll``'s target / precision; meaningless when those are zero) and x_1 .. x_H, a copy of the tape's block (the caller may edit
  it in place; the backward reads the tape).  Backward: whichever of the two output gradients arrived goes into the seeded reverse
  sweep (``mm_pathwise_policy_rollout_backward[_nd|_wide]_seeded``), NULL for the one autograd did not produce."""

  @staticmethod
  def forward(ctx, x0, Z, ls, var, beta, mean_c, roll, num_steps, dt):
    cost, tape = _taped_policy_rollout(ctx, x0, Z, ls, var, beta, mean_c, roll, num_steps, dt)
    ctx.set_materialize_grads(False)                       # an output the loss does not use arrives as None, not as zeros
    return cost.T.contiguous(), roll.trajectory(tape, num_steps).clone()

  @staticmethod
  def backward(ctx, g_cost, g_states):
    if g_cost is None and g_states is None:
      return (None,) * 9
    return _policy_rollout_gradients(ctx, g_cost, g_states)    # (g_states None: the built-in cost alone, the unseeded sweep)
