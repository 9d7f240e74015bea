"""Parameter containers for the moment-matching handlers.

Minimal torch equivalents of the gpflow / gpflow_pilco objects the hot path
reads (fields, plus what trains an ``SVGP`` from data: ``SVGP.elbo``, ``SVGP.initialize``, ``PilcoPenaltySNR``; the
optimiser is ``training.fit_svgp``):

* kernels: ``SquaredExponential``, ``Matern32`` / ``Matern52`` (pathwise sampling only) and the multi-output ``SeparateIndependent`` /
  ``SharedIndependent`` / ``LinearCoregionalization`` (gpflow.kernels), read at
  ``gpflow_pilco/moment_matching/models.py:205-212,279-286,331-354``;
* inducing variables (gpflow.inducing_variables), read at ``utils/kernel_expectation.py:41-69``;
* mean functions ``Zero`` / ``Constant`` (``gpflow_pilco/models/mean_functions.py:24-38``);
* ``SVGP`` / ``GPR`` (``gpflow_pilco/models/svgp.py:32-45``, ``gpr.py:26-37``) and the wrappers
  ``KernelRegressor`` / ``InverseLinkWrapper`` (``gpflow_pilco/models/core.py:30-71``).

``model.precompute()`` does, once per (frozen) model, what the reference redoes every
call at ``moment_matching/models.py:216-235``: Kuu + jitter, its Cholesky, and from it
``beta = Kuu^-1 u`` and ``C = Kuu^-1 S Kuu^-1 - Kuu^-1`` (float64, torch/rocSOLVER).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch

from .linalg import CholeskyError, cholesky

DEFAULT_JITTER = 1e-6  # gpflow.config.default_jitter()
DEFAULT_FLOAT = torch.float64  # gpflow.config.default_float()


def _as_param(x, device=None) -> torch.Tensor:
  t = x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=DEFAULT_FLOAT)
  t = t.to(DEFAULT_FLOAT)
  return t.to(device) if device is not None else t


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------
class Kernel:
  pass


class Stationary(Kernel):
  """The fields and helpers of a stationary ARD kernel (gpflow.kernels.Stationary): variance, lengthscales, active_dims."""

  def __init__(self, variance=1.0, lengthscales=1.0, active_dims: Optional[Sequence[int]] = None):
    self.variance = _as_param(variance)
    self.lengthscales = _as_param(lengthscales)
    self.active_dims = None if active_dims is None else tuple(int(i) for i in active_dims)

  @property
  def ard(self) -> bool:
    return self.lengthscales.ndim > 0

  def slice(self, X: torch.Tensor) -> torch.Tensor:
    if self.active_dims is None:
      return X
    return X[..., list(self.active_dims)]

  def slice_cov(self, cov: torch.Tensor) -> torch.Tensor:
    if self.active_dims is None:
      return cov
    idx = list(self.active_dims)
    return cov[..., idx, :][..., :, idx]

  def lengthscales_vector(self, ndims: int) -> torch.Tensor:
    ls = self.lengthscales
    return ls if ls.ndim > 0 else ls.expand(ndims)


class SquaredExponential(Stationary):
  """gpflow.kernels.SquaredExponential: variance * exp(-0.5 |(x - x')/lengthscales|^2)."""

  def K(self, X: torch.Tensor, X2: Optional[torch.Tensor] = None) -> torch.Tensor:
    X = self.slice(X)
    ls = self.lengthscales_vector(X.shape[-1]).to(X)
    A = X / ls
    B = A if X2 is None else self.slice(X2) / ls
    d2 = (A * A).sum(-1)[:, None] + (B * B).sum(-1)[None, :] - 2.0 * A @ B.T
    return self.variance.to(X) * torch.exp(-0.5 * d2.clamp_min(0.0))


def _scaled_sqdist(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
  """r^2 [..., n, m] between the rows of A [..., n, d] and B [..., m, d] (inputs already divided by the lengthscales), expanded
  form, clamped at 0."""
  d2 = (A * A).sum(-1)[..., :, None] + (B * B).sum(-1)[..., None, :] - 2.0 * A @ B.transpose(-1, -2)
  return d2.clamp_min(0.0)


# kernel families: the codes of the C ABI's ``kernel`` argument (include/gpflowpilco_mm.h, the _kern entries)
KERNEL_SE, KERNEL_MATERN32, KERNEL_MATERN52 = 0, 1, 2
KERNEL_NAMES = ("se", "matern32", "matern52")


def stationary_profile(r2: torch.Tensor, family: int) -> torch.Tensor:
  """k(r) / variance of a kernel family as a function of r^2 (gpflow's parametrisation)."""
  if family == KERNEL_SE:
    return torch.exp(-0.5 * r2)
  if family not in (KERNEL_MATERN32, KERNEL_MATERN52):
    raise ValueError(f"kernel family {family}: expected 0 (SquaredExponential), 1 (Matern32) or 2 (Matern52)")
  # (the derivative of sqrt at 0 is infinite: clamp where autograd must pass through r = 0; k itself is smooth there)
  s = torch.sqrt((3.0 if family == KERNEL_MATERN32 else 5.0) * r2.clamp_min(1e-36))
  if family == KERNEL_MATERN32:
    return (1.0 + s) * torch.exp(-s)
  return (1.0 + s + s * s / 3.0) * torch.exp(-s)


class _Matern(Stationary):
  """A Matern kernel with ``SquaredExponential``'s fields and methods (gpflow.kernels.Matern32 / Matern52); only ``K`` differs.
  Sampled by the pathwise solver (``pathwise.generate_paths``); moment matching has closed forms for SquaredExponential only."""
  family = None

  def K(self, X: torch.Tensor, X2: Optional[torch.Tensor] = None) -> torch.Tensor:
    X = self.slice(X)
    ls = self.lengthscales_vector(X.shape[-1]).to(X)
    A = X / ls
    B = A if X2 is None else self.slice(X2) / ls
    return self.variance.to(X) * stationary_profile(_scaled_sqdist(A, B), self.family)


class Matern32(_Matern):
  """gpflow.kernels.Matern32: variance (1 + sqrt3 r) exp(-sqrt3 r), r = |(x - x') / lengthscales|."""
  family = KERNEL_MATERN32


class Matern52(_Matern):
  """gpflow.kernels.Matern52: variance (1 + sqrt5 r + 5 r^2 / 3) exp(-sqrt5 r), r = |(x - x') / lengthscales|."""
  family = KERNEL_MATERN52


def kernel_family(kernels) -> int:
  """The family shared by a list of latent kernels: 0 SquaredExponential, 1 Matern32, 2 Matern52.  Raises ``ValueError`` naming the
  latents when they differ (one weight-stream pass evaluates one family), ``NotImplementedError`` for any other kernel class."""
  fams = []
  for i, k in enumerate(kernels):
    if isinstance(k, _Matern):
      fams.append(k.family)
    elif isinstance(k, SquaredExponential):
      fams.append(KERNEL_SE)
    else:
      raise NotImplementedError(f"latent {i}: kernel {type(k).__name__} (SquaredExponential, Matern32 and Matern52 are implemented)")
  if any(f != fams[0] for f in fams):
    raise ValueError("the latent kernels of one model must be of one family, got "
                     + ", ".join(f"latent {i}: {type(k).__name__}" for i, k in enumerate(kernels)))
  return fams[0] if fams else KERNEL_SE


def require_squared_exponential(kernels, what: str):
  fam = kernel_family(kernels)
  if fam != KERNEL_SE:
    raise NotImplementedError(f"{what}: moment matching has closed forms for SquaredExponential only (the kernel expectations "
                              f"of utils/kernel_expectation.py), not for {type(kernels[0]).__name__}; a Matern model is evaluated "
                              "by SVGP.predict_mean and sampled by the pathwise solver")


class MultioutputKernel(Kernel):
  kernels: List[SquaredExponential]

  @property
  def num_latent_gps(self) -> int:
    return len(self.kernels)


class SeparateIndependent(MultioutputKernel):
  def __init__(self, kernels: Sequence[SquaredExponential]):
    self.kernels = list(kernels)


class SharedIndependent(MultioutputKernel):
  def __init__(self, kernel: SquaredExponential, output_dim: int):
    self.kernel = kernel
    self.kernels = [kernel] * output_dim


class LinearCoregionalization(MultioutputKernel):
  def __init__(self, kernels: Sequence[SquaredExponential], W):
    self.kernels = list(kernels)
    self.W = _as_param(W)  # [P, L]


# ---------------------------------------------------------------------------
# inducing variables, mean functions, likelihood
# ---------------------------------------------------------------------------
class InducingPoints:
  def __init__(self, Z):
    self.Z = _as_param(Z)


class SeparateIndependentInducingVariables:
  def __init__(self, inducing_variable_list: Sequence[InducingPoints]):
    self.inducing_variables = list(inducing_variable_list)


class SharedIndependentInducingVariables:
  def __init__(self, inducing_variable: InducingPoints):
    self.inducing_variable = inducing_variable
    self.inducing_variables = [inducing_variable]


class Zero:
  def __call__(self, X):
    return torch.zeros_like(X[..., :1])


class Constant:
  def __init__(self, c):
    self.c = _as_param(c).reshape(-1)

  def __call__(self, X):
    return self.c.to(X).expand(X.shape[:-1] + self.c.shape)


class GaussianLikelihood:
  def __init__(self, variance=1.0):
    self.variance = _as_param(variance)


def unpack_multioutput(kernel, inducing_variable, num_latent: Optional[int] = None):
  """``unpack_multioutput`` (utils/kernel_expectation.py:41-69) -> (kernels, [Z_a])."""
  if isinstance(kernel, MultioutputKernel):
    kernels = list(kernel.kernels)
  else:
    kernels = [kernel] * (num_latent or 1)
  L = len(kernels)
  if isinstance(inducing_variable, SeparateIndependentInducingVariables):
    ivs = list(inducing_variable.inducing_variables)
    assert len(ivs) == L
  elif isinstance(inducing_variable, SharedIndependentInducingVariables):
    ivs = L * list(inducing_variable.inducing_variables)
  elif isinstance(inducing_variable, InducingPoints):
    ivs = L * [inducing_variable]
  else:
    raise NotImplementedError(type(inducing_variable))
  return kernels, [iv.Z for iv in ivs]


# ---------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------
class _PackCache:
  """Caches the precompute and the packed device model per (dtype, with_C); keyed on the
  parameter tensors' versions so an in-place update (training step) invalidates it."""

  def __init__(self):
    self._key = None
    self._pre = None
    self._packed = {}

  def pre(self, model, device):
    """The cached ``model.precompute(device)`` tuple (Z, ls, var, beta, C, mean_c), nothing packed: a second call on an unchanged
    model factors nothing."""
    key = tuple((id(t), t._version, t.device) for t in model._parameters()) + (str(device),)
    if key != self._key:
      self._key, self._pre, self._packed = key, None, {}
    if self._pre is None:
      self._pre = model.precompute(device)
    return self._pre

  def get(self, model, dtype, with_C, device):
    self.pre(model, device)
    slot = (dtype, bool(with_C))
    if slot not in self._packed:
      from . import ops
      Z, ls, var, beta, C, mean_c = self._pre
      capturing = Z.is_cuda and torch.cuda.is_current_stream_capturing()
      det = lambda t: None if t is None else t.detach()
      self._packed[slot] = ops.pack_model(det(Z), det(ls), det(var), det(beta), det(C) if with_C else None, det(mean_c),
                                          dtype=dtype, sync=not capturing)
    return self._packed[slot]


# lengthscale given to an input dimension a latent kernel does NOT act on (per-latent ``active_dims``): the SE kernel
# with lengthscale l -> infinity on a dimension is the kernel that ignores it; 1e6 perturbs every expectation by
# O(Sigma_kk / 1e12) relative
INACTIVE_LENGTHSCALE = 1.0e6


def kernel_input_dims(kernels, ndims: Optional[int] = None):
  """Sorted union of the latent kernels' ``active_dims`` (None if every kernel acts on all inputs), and whether
  the kernels differ in what they act on."""
  if all(k.active_dims is None for k in kernels):
    return None, False
  if any(k.active_dims is None for k in kernels):
    if ndims is None:
      raise ValueError("mixing sliced and unsliced latent kernels needs the input dimension")
    union = tuple(range(ndims))
  else:
    union = tuple(sorted(set(i for k in kernels for i in k.active_dims)))
  differ = any((k.active_dims if k.active_dims is not None else union) != kernels[0].active_dims for k in kernels) \
      or kernels[0].active_dims is None
  return union, differ


def _stack_kernel_params(kernels, Zs, device):
  """-> Z [L,M,d], lengthscales [L,d], variance [L] on the kernels' common input dimensions.

  Kernels with the same ``active_dims`` (the reference's assumption, utils/kernel_expectation.py:98-100): sliced
  as the reference slices.  Kernels acting on DIFFERENT subsets (moment_matching/models.py:264-270 slices per
  kernel): every latent is embedded into the sorted union of the active dimensions with the lengthscale
  ``INACTIVE_LENGTHSCALE`` (and inducing coordinate 0) on the dimensions it ignores -- the kernels, their
  expectations under any (dense or diagonal) Gaussian and all pair terms are then exact to ~1e-12, including the
  product shortcut of disjoint kernels under a diagonal Gaussian (utils/kernel_expectation.py:85-89), which is the
  special case G = 0 of the general pair term."""
  union, differ = kernel_input_dims(kernels, Zs[0].shape[-1])
  if not differ:
    d = Zs[0].shape[-1] if kernels[0].active_dims is None else len(kernels[0].active_dims)
    Z = torch.stack([k.slice(z.to(device=device, dtype=DEFAULT_FLOAT)) for k, z in zip(kernels, Zs)])
    ls = torch.stack([k.lengthscales_vector(d).to(device=device, dtype=DEFAULT_FLOAT) for k in kernels])
  else:
    d = len(union)
    pos = {u: i for i, u in enumerate(union)}
    Zl, lsl = [], []
    for k, z in zip(kernels, Zs):
      act = union if k.active_dims is None else k.active_dims
      zf = torch.zeros(z.shape[0], d, dtype=DEFAULT_FLOAT, device=device)
      lf = torch.full((d,), INACTIVE_LENGTHSCALE, dtype=DEFAULT_FLOAT, device=device)
      idx = torch.tensor([pos[u] for u in act], device=device)
      zf[:, idx] = k.slice(z.to(device=device, dtype=DEFAULT_FLOAT))
      lf[idx] = k.lengthscales_vector(len(act)).to(device=device, dtype=DEFAULT_FLOAT)
      Zl.append(zf); lsl.append(lf)
    Z, ls = torch.stack(Zl), torch.stack(lsl)
  var = torch.stack([k.variance.to(device=device, dtype=DEFAULT_FLOAT).reshape(()) for k in kernels])
  return Z, ls, var


PREDICT_CHUNK_BYTES = 256 * 2 ** 20  # the torch route of predict_f keeps every intermediate below about this size
# the native route of the collapsed bound takes the streamed statistics kernel (mm_gram_stats_se) up to this many inducing points
# and the composition of existing parts (chunked mm_gram_se, batched GEMM, mm_gram_se_backward) above it.  Origin: the sweep of
# tools/bench_svgp_collapsed.py (profiles/svgp_collapsed_bench.json; L 8, d 8, statistics + adjoint, streamed / composed):
# M 256 is the largest swept size at which the streamed kernel is the faster one at both N -- 0.87 at N 4000, 0.38 at N 65 536;
# M 320: 1.10 / 0.51, M 384: 1.29 / 0.62, M 512: 1.76 / 1.16 (it re-forms a K tile for every block pair that uses it).  Sizes
# between the swept ones (steps of 64) are not measured.
STATS_STREAMED_MAX_M = 256


def _native_predict_refusal(model, X, kernels, family: int, d: int, differ: bool) -> Optional[str]:
  """Why ``predict_f`` of this model at these points does not take the HIP kernel (None: it does)."""
  if not X.is_cuda:
    return f"the points are on {X.device} (the HIP predictive kernel runs on the GPU)"
  if family != KERNEL_SE:
    return f"the native predict_f is SquaredExponential only, the latents are {type(kernels[0]).__name__} (torch route)"
  if differ:
    return "the latent kernels act on differing active_dims (torch route)"
  if d > 32:
    return f"input dimension {d} exceeds MM_DMAX = 32"
  if torch.is_grad_enabled() and (X.requires_grad or any(t.requires_grad for t in model._parameters())):
    return "a gradient is being recorded (the native predict_f is not differentiable: torch route, or torch.no_grad())"
  return None


def _predict_y_from_f(model, who: str, mean, var, full_output_cov: bool):
  """Adds the Gaussian likelihood's variance to the latent marginals (on the diagonal under ``full_output_cov``)."""
  if not isinstance(model.likelihood, GaussianLikelihood):
    raise NotImplementedError(f"{who}: Gaussian likelihood only, got {type(model.likelihood).__name__}")
  s2 = model.likelihood.variance.to(var)
  if full_output_cov:
    return mean, var + torch.diag_embed(s2.expand(var.shape[-1]))
  return mean, var + s2


def _gaussian_log_density(Y, mean, var):
  import math
  return -0.5 * (torch.log(2.0 * math.pi * var) + (Y - mean) ** 2 / var)


class SingularCollapsedBound(CholeskyError):
  """``I + Lu^-1 Phi Lu^-T / s2`` of the collapsed bound could not be factorised: its condition grows as N var / s2."""


class SVGP:
  """``gpflow_pilco.models.SVGP`` fields: kernel, inducing_variable, q_mu [M,L], q_sqrt [L,M,M],
  whiten, mean_function, likelihood, num_latent_gps."""

  def __init__(self, kernel, inducing_variable, q_mu, q_sqrt, whiten: bool = True,
               mean_function=None, likelihood=None, num_latent_gps: Optional[int] = None,
               prior: Optional[Callable] = None):
    self.kernel = kernel
    self.inducing_variable = (InducingPoints(inducing_variable)
                              if isinstance(inducing_variable, torch.Tensor) else inducing_variable)
    self.q_mu = _as_param(q_mu)
    self.q_sqrt = _as_param(q_sqrt)
    self.whiten = bool(whiten)
    self.mean_function = Zero() if mean_function is None else mean_function
    self.likelihood = likelihood
    self.num_latent_gps = num_latent_gps or self.q_mu.shape[-1]
    self.prior = prior
    self._cache = _PackCache()

  def predict_mean(self, x: torch.Tensor) -> torch.Tensor:
    """Posterior mean at deterministic inputs x [..., D]: K(x, Z) Kuu^-1 u (+ mean function), i.e. the
    mean half of gpflow's ``predict_f``; what ``KernelRegressor.__call__`` returns (models/core.py:60-62).
    Plain torch (policy evaluation on real states; not on the moment-matching hot path)."""
    kernels = self.latent_kernels
    family = kernel_family(kernels)
    Z, ls, var, beta, mean_c = self._mean_weights(x.device, family)
    union, differ = kernel_input_dims(kernels, x.shape[-1])
    xs = (x[..., list(union)] if differ else kernels[0].slice(x)).to(DEFAULT_FLOAT)
    lead = xs.shape[:-1]
    xs2 = xs.reshape(-1, xs.shape[-1])
    A = xs2[None] / ls[:, None, :]                              # [L, n, d]
    Bz = Z / ls[:, None, :]                                     # [L, M, d]
    if family == KERNEL_SE:
      d2 = (A * A).sum(-1)[:, :, None] + (Bz * Bz).sum(-1)[:, None, :] - 2.0 * A @ Bz.transpose(1, 2)
      Kxz = var[:, None, None] * torch.exp(-0.5 * d2.clamp_min(0.0))
    else:
      Kxz = var[:, None, None] * stationary_profile(_scaled_sqdist(A, Bz), family)
    g = (Kxz @ beta.unsqueeze(-1)).squeeze(-1).T                # [n, L]
    if isinstance(self.kernel, LinearCoregionalization):
      g = g @ self.kernel.W.to(g).T
      if isinstance(self.mean_function, Constant):
        g = g + self.mean_function.c.to(g)
    elif mean_c is not None:
      g = g + mean_c
    return g.reshape(lead + g.shape[-1:]).to(x.dtype)

  def __call__(self, x, **kwargs):
    if isinstance(x, torch.Tensor):
      return self.predict_mean(x)
    raise NotImplementedError("SVGP.__call__ takes a tensor of inputs")

  # -- helpers used by the handlers ---------------------------------------
  def _parameters(self):
    kernels, Zs = unpack_multioutput(self.kernel, self.inducing_variable, self.num_latent_gps)
    out = [self.q_mu, self.q_sqrt] + list(Zs)
    for k in kernels:
      out += [k.variance, k.lengthscales]
    if isinstance(self.mean_function, Constant):
      out.append(self.mean_function.c)
    return out

  @property
  def latent_kernels(self):
    return unpack_multioutput(self.kernel, self.inducing_variable, self.num_latent_gps)[0]

  def _mean_weights(self, device, family: int):
    """-> Z, ls, var, beta = Kuu^-1 u, mean_c: what ``predict_mean`` needs.  SquaredExponential: ``precompute``'s; a Matern model
    (which ``precompute`` refuses) from its own Gram matrix."""
    if family == KERNEL_SE:
      Z, ls, var, beta, _, mean_c = self.precompute(device)
      return Z, ls, var, beta, mean_c
    kernels, Zs = unpack_multioutput(self.kernel, self.inducing_variable, self.num_latent_gps)
    Z, ls, var = _stack_kernel_params(kernels, Zs, device)
    L, M, d = Z.shape
    A = Z / ls[:, None, :]
    Kuu = var[:, None, None] * stationary_profile(_scaled_sqdist(A, A), family)
    Luu = cholesky(Kuu + DEFAULT_JITTER * torch.eye(M, dtype=DEFAULT_FLOAT, device=device))
    v = self.q_mu.to(device=device, dtype=DEFAULT_FLOAT).T.unsqueeze(-1)
    if not self.whiten:
      v = torch.linalg.solve_triangular(Luu, v, upper=False)
    beta = torch.linalg.solve_triangular(Luu.transpose(1, 2), v, upper=True).squeeze(-1)
    mean_c = None
    if isinstance(self.mean_function, Constant):
      if not isinstance(self.kernel, LinearCoregionalization):
        mean_c = self.mean_function.c.to(device=device, dtype=DEFAULT_FLOAT).expand(L).contiguous()
    elif not isinstance(self.mean_function, Zero):
      raise NotImplementedError
    return Z, ls, var, beta, mean_c

  def precompute(self, device):
    """-> Z [L,M,d], ls [L,d], var [L], beta [L,M], C [L,M,M], mean_c [L]|None (float64, device).  SquaredExponential latents
    only: what is computed here feeds the moment-matching kernels."""
    kernels, Zs = unpack_multioutput(self.kernel, self.inducing_variable, self.num_latent_gps)
    require_squared_exponential(kernels, "SVGP.precompute")
    Z, ls, var = _stack_kernel_params(kernels, Zs, device)
    L, M, d = Z.shape
    A = Z / ls[:, None, :]
    d2 = (A * A).sum(-1)[:, :, None] + (A * A).sum(-1)[:, None, :] - 2.0 * A @ A.transpose(1, 2)
    Kuu = var[:, None, None] * torch.exp(-0.5 * d2.clamp_min(0.0))
    Kuu = Kuu + DEFAULT_JITTER * torch.eye(M, dtype=DEFAULT_FLOAT, device=device)  # models.py:216
    Luu = cholesky(Kuu)                                                # :217
    v = self.q_mu.to(device=device, dtype=DEFAULT_FLOAT).T.unsqueeze(-1)            # [L,M,1]  :228
    S = torch.tril(self.q_sqrt.to(device=device, dtype=DEFAULT_FLOAT))              # :229
    if not self.whiten:                                                             # :230-232
      v = torch.linalg.solve_triangular(Luu, v, upper=False)
      S = torch.linalg.solve_triangular(Luu, S, upper=False)
    LuuT = Luu.transpose(1, 2)
    beta = torch.linalg.solve_triangular(LuuT, v, upper=True).squeeze(-1)           # :235
    Acov = S @ S.transpose(1, 2) - torch.eye(M, dtype=DEFAULT_FLOAT, device=device)
    X = torch.linalg.solve_triangular(LuuT, Acov, upper=True)                       # L^-T (A - I)
    C = torch.linalg.solve_triangular(LuuT, X.transpose(1, 2), upper=True)          # L^-T (A - I) L^-1
    C = 0.5 * (C + C.transpose(1, 2))
    mean_c = None
    if isinstance(self.mean_function, Constant):
      if isinstance(self.kernel, LinearCoregionalization):
        mean_c = None            # added after the W mixing, on the host
      else:
        mean_c = self.mean_function.c.to(device=device, dtype=DEFAULT_FLOAT).expand(L).contiguous()
    elif not isinstance(self.mean_function, Zero):
      raise NotImplementedError                                                     # :291
    return Z, ls, var, beta, C, mean_c

  def packed(self, dtype, with_C: bool, device):
    """(A Matern model is refused by ``precompute``, which every cache miss runs: nothing is checked per call.)"""
    return self._cache.get(self, dtype, with_C, device)

  # -- prediction at deterministic points (gpflow's predict_f / predict_y / predict_log_density) ---------------------------------
  def _latent_marginals_torch(self, X2, kernels, Zs, family: int):
    """mean_g, var_g [n, L] of the latents at X2 [n, d]: gpflow's conditional (Lu^-1 Kuf, whitened or not -- the algebra of
    ``elbo``), differentiable, any kernel family, any device; n in chunks that keep [L, M, chunk] below PREDICT_CHUNK_BYTES."""
    device = X2.device
    Z, ls, var = _stack_kernel_params(kernels, Zs, device)
    L, M, d = Z.shape
    Az = Z / ls[:, None, :]
    Kuu = var[:, None, None] * stationary_profile(_scaled_sqdist(Az, Az), family)
    Lu = cholesky(Kuu + DEFAULT_JITTER * torch.eye(M, dtype=DEFAULT_FLOAT, device=device))
    qm = self.q_mu.to(device=device, dtype=DEFAULT_FLOAT).T                       # [L,M]
    S = torch.tril(self.q_sqrt.to(device=device, dtype=DEFAULT_FLOAT))            # [L,M,M]
    chunk = max(1, PREDICT_CHUNK_BYTES // (8 * L * M))
    means, variances = [], []
    for start in range(0, X2.shape[0], chunk):
      Ax = X2[None, start:start + chunk] / ls[:, None, :]
      Kuf = var[:, None, None] * stationary_profile(_scaled_sqdist(Az, Ax), family)
      A = torch.linalg.solve_triangular(Lu, Kuf, upper=False)                     # [L,M,n]
      Aq = A if self.whiten else torch.linalg.solve_triangular(Lu.transpose(1, 2), A, upper=True)
      SA = S.transpose(1, 2) @ Aq
      means.append((Aq * qm[:, :, None]).sum(1).T)
      variances.append((var[:, None] - (A * A).sum(1) + (SA * SA).sum(1)).T)
    if not means:
      empty = X2.new_zeros(0, L)
      return empty, empty
    return torch.cat(means), torch.cat(variances)

  def predict_f(self, Xnew: torch.Tensor, full_cov: bool = False, full_output_cov: bool = False, native: Optional[bool] = None):
    """gpflow's ``predict_f`` at deterministic points Xnew [..., D]: (mean [..., P], var [..., P]), or the output covariance
    [..., P, P] with ``full_output_cov``.  Independent latents: mean_g + c and var_g (``diag_embed`` of it); a
    ``LinearCoregionalization``: W mean_g + c and var_g (W o W)^T (W diag(var_g) W^T), mixed in torch on the [n, L] marginals.
    ``full_cov=True`` (covariances between points) is not implemented.

    ``native=None`` takes the HIP kernel (``ops.predict_se``: mean_g = k^T beta, var_g = var + k^T C k from the cached
    ``precompute``, K never materialised) for SquaredExponential latents with equal ``active_dims`` and d <= 32 at points on a GPU
    when no gradient is being recorded (grad mode off, or neither a parameter nor Xnew requires one), and torch otherwise;
    ``native=False`` always torch (the conditional of ``elbo``; differentiable, CPU and Matern families too, chunked over the
    points); ``native=True`` raises ``ValueError`` with the reason where the native route does not apply."""
    if full_cov:
      raise NotImplementedError("SVGP.predict_f: full_cov=True is not implemented (marginals per point only)")
    kernels, Zs = unpack_multioutput(self.kernel, self.inducing_variable, self.num_latent_gps)
    family = kernel_family(kernels)
    union, differ = kernel_input_dims(kernels, Xnew.shape[-1])
    Xs = (Xnew[..., list(union)] if differ else kernels[0].slice(Xnew)).to(DEFAULT_FLOAT)
    lead, d = Xs.shape[:-1], Xs.shape[-1]
    X2 = Xs.reshape(-1, d)
    coreg = isinstance(self.kernel, LinearCoregionalization)
    if not isinstance(self.mean_function, (Zero, Constant)):
      raise NotImplementedError(f"SVGP.predict_f: mean function {type(self.mean_function).__name__}")
    refusal = _native_predict_refusal(self, X2, kernels, family, d, differ)
    if native and refusal is not None:
      raise ValueError(f"SVGP.predict_f(native=True): {refusal}")
    if native is not False and refusal is None:
      from . import ops
      Z, ls, var, beta, C, mean_c = (None if t is None else t.detach() for t in self._cache.pre(self, X2.device))
      mean_g, var_g = ops.predict_se(X2.detach(), Z, ls, var, beta, C, None)
    else:
      mean_g, var_g = self._latent_marginals_torch(X2, kernels, Zs, family)
    if coreg:
      W = self.kernel.W.to(mean_g)                                                # [P,L]
      mean = mean_g @ W.T
      var = torch.einsum("pl,nl,ql->npq", W, var_g, W) if full_output_cov else var_g @ (W * W).T
    else:
      mean, var = mean_g, (torch.diag_embed(var_g) if full_output_cov else var_g)
    if isinstance(self.mean_function, Constant):
      mean = mean + self.mean_function.c.to(mean)
    return mean.reshape(lead + mean.shape[1:]).to(Xnew.dtype), var.reshape(lead + var.shape[1:]).to(Xnew.dtype)

  def predict_y(self, Xnew: torch.Tensor, full_cov: bool = False, full_output_cov: bool = False, native: Optional[bool] = None):
    """``predict_f`` plus ``likelihood.variance`` (on the diagonal under ``full_output_cov``); Gaussian likelihood only."""
    mean, var = self.predict_f(Xnew, full_cov=full_cov, full_output_cov=full_output_cov, native=native)
    return _predict_y_from_f(self, "SVGP.predict_y", mean, var, full_output_cov)

  def predict_log_density(self, data, native: Optional[bool] = None) -> torch.Tensor:
    """log N(Y | predict_y(X)) per point and output, [N, P], for ``data = (X, Y)``; Gaussian likelihood only."""
    X, Y = data
    if not isinstance(self.likelihood, GaussianLikelihood):
      raise NotImplementedError(f"SVGP.predict_log_density: Gaussian likelihood only, got {type(self.likelihood).__name__}")
    mean, var = self.predict_y(X, native=native)
    return _gaussian_log_density(Y.to(mean), mean, var)

  # -- training: the ELBO, its objective and the initialiser (gpflow's SVGP.elbo; models/svgp.py:41-121) --------------------------
  def _native_gram_refusal(self, X, kernels, family: int, d: int, differ: bool) -> Optional[str]:
    """Why the ELBO of this model on these data does not take the HIP Gram (None: it does)."""
    if not X.is_cuda:
      return f"the data are on {X.device} (the HIP Gram kernel runs on the GPU)"
    if family != KERNEL_SE:
      return f"the native Gram is SquaredExponential only, the latents are {type(kernels[0]).__name__} (torch Gram)"
    if differ:
      return "the latent kernels act on differing active_dims (torch Gram)"
    if d > 32:
      return f"input dimension {d} exceeds MM_DMAX = 32"
    return None

  def elbo(self, data, native: Optional[bool] = None) -> torch.Tensor:
    """gpflow's ``SVGP.elbo`` on the full batch ``data = (X [N,d], Y [N,P])``, Gaussian likelihood: expected log-likelihood under
    the marginals of q(f) minus KL(q(u) || p(u)), differentiable in every parameter (kernel variances and lengthscales, Z, q_mu,
    q_sqrt, the Constant mean, ``kernel.W``, ``likelihood.variance``).

    Per latent: Kuu = k(Z, Z) + jitter I = Lu Lu^T, A = Lu^-1 Kuf; whitened, mean_g = A^T q_mu and
    var_g = var - colsum(A^2) + colsum((tril(q_sqrt)^T A)^2); not whitened, the two q terms with Lu^-T A.  The two Gram matrices
    are the only [L,M,N]-sized elementwise work: ``native=None`` takes them from the HIP kernel (``autodiff.GramSEFunction`` /
    ``GramSESelfFunction``) on a GPU for SquaredExponential latents with d <= 32 and from torch otherwise (CPU data, a Matern
    family, latents on differing ``active_dims``); ``native=False`` always from torch; ``native=True`` raises with the reason where
    the native route does not apply.  The factorisation, the solves and the products are torch's on both routes."""
    import math
    X, Y = data
    if not isinstance(self.likelihood, GaussianLikelihood):
      raise NotImplementedError(f"SVGP.elbo: Gaussian likelihood only, got {type(self.likelihood).__name__}")
    kernels, Zs = unpack_multioutput(self.kernel, self.inducing_variable, self.num_latent_gps)
    family = kernel_family(kernels)
    device = X.device
    Z, ls, var = _stack_kernel_params(kernels, Zs, device)
    L, M, d = Z.shape
    union, differ = kernel_input_dims(kernels, X.shape[-1])
    Xs = (X[..., list(union)] if differ else kernels[0].slice(X)).to(DEFAULT_FLOAT)
    Y = Y.to(device=device, dtype=DEFAULT_FLOAT)
    N = Xs.shape[0]
    refusal = self._native_gram_refusal(Xs, kernels, family, d, differ)
    if native and refusal is not None:
      raise ValueError(f"SVGP.elbo(native=True): {refusal}")
    if native is not False and refusal is None:
      from .autodiff import GramSEFunction, GramSESelfFunction
      Kuf = GramSEFunction.apply(Xs.detach(), Z, ls, var)
      Kuu = GramSESelfFunction.apply(Z, ls, var)
    else:
      Az, Ax = Z / ls[:, None, :], Xs[None] / ls[:, None, :]
      Kuf = var[:, None, None] * stationary_profile(_scaled_sqdist(Az, Ax), family)
      Kuu = var[:, None, None] * stationary_profile(_scaled_sqdist(Az, Az), family)
    eye = torch.eye(M, dtype=DEFAULT_FLOAT, device=device)
    Lu = cholesky(Kuu + DEFAULT_JITTER * eye)
    A = torch.linalg.solve_triangular(Lu, Kuf, upper=False)                       # [L,M,N]
    qm = self.q_mu.to(device=device, dtype=DEFAULT_FLOAT).T                       # [L,M]
    S = torch.tril(self.q_sqrt.to(device=device, dtype=DEFAULT_FLOAT))            # [L,M,M]
    log_qdiag = torch.log(torch.diagonal(S, dim1=-2, dim2=-1).abs()).sum()
    if self.whiten:
      Aq = A
      kl = 0.5 * ((qm * qm).sum() + (S * S).sum() - L * M) - log_qdiag
    else:
      Aq = torch.linalg.solve_triangular(Lu.transpose(1, 2), A, upper=True)       # Lu^-T A = Kuu^-1 Kuf
      Lm = torch.linalg.solve_triangular(Lu, qm.unsqueeze(-1), upper=False)
      LS = torch.linalg.solve_triangular(Lu, S, upper=False)
      log_udiag = torch.log(torch.diagonal(Lu, dim1=-2, dim2=-1)).sum()
      kl = 0.5 * ((Lm * Lm).sum() + (LS * LS).sum() - L * M) + log_udiag - log_qdiag
    mean_g = (Aq * qm[:, :, None]).sum(1)                                         # [L,N]
    SA = S.transpose(1, 2) @ Aq
    var_g = var[:, None] - (A * A).sum(1) + (SA * SA).sum(1)                      # [L,N]
    if isinstance(self.kernel, LinearCoregionalization):
      W = self.kernel.W.to(device=device, dtype=DEFAULT_FLOAT)                    # [P,L]
      f_mean, f_var = mean_g.T @ W.T, var_g.T @ (W * W).T
    else:
      f_mean, f_var = mean_g.T, var_g.T
    if isinstance(self.mean_function, Constant):
      f_mean = f_mean + self.mean_function.c.to(device=device, dtype=DEFAULT_FLOAT)
    elif not isinstance(self.mean_function, Zero):
      raise NotImplementedError(f"SVGP.elbo: mean function {type(self.mean_function).__name__}")
    if Y.shape != f_mean.shape:
      raise ValueError(f"SVGP.elbo: Y {tuple(Y.shape)} against {tuple(f_mean.shape)} model outputs")
    s2 = self.likelihood.variance.to(device=device, dtype=DEFAULT_FLOAT)
    fit = (-0.5 * torch.log(2.0 * math.pi * s2) - ((Y - f_mean) ** 2 + f_var) / (2.0 * s2)).sum()
    return fit - kl

  def maximum_log_likelihood_objective(self, data, native: Optional[bool] = None) -> torch.Tensor:
    """``elbo + prior(self)`` (models/svgp.py:41-45)."""
    objective = self.elbo(data, native=native)
    if self.prior is not None:
      objective = objective + self.prior(self)
    return objective

  def training_loss(self, data, native: Optional[bool] = None) -> torch.Tensor:
    return -self.maximum_log_likelihood_objective(data, native=native)

  def training_loss_closure(self, data, native: Optional[bool] = None) -> Callable[[], torch.Tensor]:
    """Zero-argument callable of the training loss: the reference's ``dynamics_loss_closure`` (loops/pilco.py:173-174)."""
    return lambda: self.training_loss(data, native=native)

  # -- collapsed (SGPR) training: the bound at the optimal q(u), from the Gram statistics Phi = Kuf Kuf^T and Psi = Kuf [Y, 1] ------
  def _native_stats_refusal(self, X, kernels, family: int, d: int, differ: bool, Q: int) -> Optional[str]:
    """Why the collapsed bound of this model on these data does not take the HIP statistics (None: it does)."""
    if not X.is_cuda:
      return f"the data are on {X.device} (the HIP statistics kernel runs on the GPU)"
    if family != KERNEL_SE:
      return f"the native statistics are SquaredExponential only, the latents are {type(kernels[0]).__name__} (torch route)"
    if differ:
      return "the latent kernels act on differing active_dims (torch route)"
    if d > 32:
      return f"input dimension {d} exceeds MM_DMAX = 32"
    if Q > 33:
      return f"{Q - 1} outputs exceed the 32 the statistics kernel takes"
    return None

  def _collapsed_factors(self, data, native: Optional[bool], who: str):
    """What the collapsed bound and the optimal q(u) share, per latent: Lu, LB = chol(I + AAT), c = LB^-1 Lu^-1 psi / s2, AAT, the
    residual sums r^T r [L], the kernel variances [L], s2 and N."""
    X, Y = data
    if not isinstance(self.likelihood, GaussianLikelihood):
      raise NotImplementedError(f"{who}: Gaussian likelihood only, got {type(self.likelihood).__name__}")
    if isinstance(self.kernel, LinearCoregionalization):
      raise NotImplementedError(f"{who}: a LinearCoregionalization kernel couples the latents through W (the optimal q(u) is "
                                "joint over the latents and needs cross-latent statistics); elbo / fit_svgp remain for it")
    if not isinstance(self.mean_function, (Zero, Constant)):
      raise NotImplementedError(f"{who}: mean function {type(self.mean_function).__name__}")
    kernels, Zs = unpack_multioutput(self.kernel, self.inducing_variable, self.num_latent_gps)
    family = kernel_family(kernels)
    device = X.device
    Z, ls, var = _stack_kernel_params(kernels, Zs, device)
    L, M, d = Z.shape
    union, differ = kernel_input_dims(kernels, X.shape[-1])
    Xs = (X[..., list(union)] if differ else kernels[0].slice(X)).to(DEFAULT_FLOAT)
    Y = Y.to(device=device, dtype=DEFAULT_FLOAT)
    N = Xs.shape[0]
    if Y.shape != (N, L):
      raise ValueError(f"{who}: Y {tuple(Y.shape)} against {(N, L)} model outputs")
    R = torch.cat([Y, torch.ones(N, 1, dtype=DEFAULT_FLOAT, device=device)], dim=1)           # [N, Q], Q = P + 1
    refusal = self._native_stats_refusal(Xs, kernels, family, d, differ, L + 1)
    if native and refusal is not None:
      raise ValueError(f"{who}(native=True): {refusal}")
    if native is not False and refusal is None:
      from .autodiff import GramSESelfFunction, GramStatsComposedFunction, GramStatsSEFunction
      if M <= STATS_STREAMED_MAX_M:
        Phi, Psi = GramStatsSEFunction.apply(Xs.detach(), R.detach(), Z, ls, var)
      else:
        Phi, Psi = GramStatsComposedFunction.apply(Xs.detach(), R.detach(), Z, ls, var, PREDICT_CHUNK_BYTES)
      Kuu = GramSESelfFunction.apply(Z, ls, var)
    else:
      Az = Z / ls[:, None, :]
      Kuu = var[:, None, None] * stationary_profile(_scaled_sqdist(Az, Az), family)
      Phi = torch.zeros(L, M, M, dtype=DEFAULT_FLOAT, device=device)
      Psi = torch.zeros(L, M, L + 1, dtype=DEFAULT_FLOAT, device=device)
      chunk = max(1, PREDICT_CHUNK_BYTES // (8 * L * M))
      for start in range(0, N, chunk):
        Ax = Xs[None, start:start + chunk] / ls[:, None, :]
        Kuf = var[:, None, None] * stationary_profile(_scaled_sqdist(Az, Ax), family)          # [L, M, chunk]
        Phi = Phi + Kuf @ Kuf.transpose(1, 2)
        Psi = Psi + Kuf @ R[start:start + chunk]
    s2 = self.likelihood.variance.to(device=device, dtype=DEFAULT_FLOAT)
    if isinstance(self.mean_function, Constant):
      mc = self.mean_function.c.to(device=device, dtype=DEFAULT_FLOAT).expand(L)
    else:
      mc = torch.zeros(L, dtype=DEFAULT_FLOAT, device=device)
    eye = torch.eye(M, dtype=DEFAULT_FLOAT, device=device)
    Lu = cholesky(Kuu + DEFAULT_JITTER * eye)
    T = torch.linalg.solve_triangular(Lu, Phi, upper=False)                                    # Lu^-1 Phi
    AAT = torch.linalg.solve_triangular(Lu, T.transpose(1, 2), upper=False) / s2              # Lu^-1 Phi Lu^-T / s2
    AAT = 0.5 * (AAT + AAT.transpose(1, 2))
    try:
      LB = cholesky(eye + AAT)
    except CholeskyError as e:                                  # (Kuu + jitter I above raises the plain CholeskyError)
      raise SingularCollapsedBound(f"{who}: I + AAT is singular to rounding (noise variance {float(s2.detach()):.3e}): {e}") from e
    idx = torch.arange(L, device=device)
    psi = Psi[idx, :, idx] - mc[:, None] * Psi[:, :, L]                                        # [L, M]: Kuf_l (y_l - c_l)
    c = torch.linalg.solve_triangular(LB, torch.linalg.solve_triangular(Lu, psi.unsqueeze(-1), upper=False), upper=False) / s2
    rr = ((Y - mc) ** 2).sum(0)                                                                # [L]
    return Lu, LB, c.squeeze(-1), AAT, rr, var, s2, N

  def collapsed_elbo(self, data, native: Optional[bool] = None) -> torch.Tensor:
    """The ELBO at the optimal q(u) (Titsias' collapsed bound, gpflow's ``SGPR.elbo``) on the full batch ``data = (X [N,d], Y [N,P])``:
    sum over the latents of log N(y_l | c_l, Qff_l + s2 I) - tr(Kff_l - Qff_l) / (2 s2).  Independent latents (P = L outputs, one
    Gaussian noise s2) with a ``Zero`` or ``Constant`` mean; ``q_mu`` and ``q_sqrt`` are not read.  Differentiable in the kernel
    variances and lengthscales, Z, ``likelihood.variance`` and the Constant mean.

    The data enter through Phi_l = Kuf_l Kuf_l^T [M,M], Psi_l = Kuf_l [Y, 1] [M,P+1] and sums over Y alone; everything after that
    is M x M algebra.  ``native=None`` takes Phi and Psi from HIP on a GPU for SquaredExponential latents with equal ``active_dims``,
    d <= 32 and P <= 32 -- up to ``STATS_STREAMED_MAX_M`` inducing points from the streamed kernel
    (``autodiff.GramStatsSEFunction``: Kuf is never stored, on either pass), above it from the composition that is faster there
    (``autodiff.GramStatsComposedFunction``: chunked ``mm_gram_se``, batched GEMMs, ``mm_gram_se_backward``; memory bounded by
    ``PREDICT_CHUNK_BYTES``) -- and from torch otherwise; ``native=False`` always from torch; ``native=True`` raises ``ValueError`` with the reason where the native route does
    not apply.  The torch route forms the statistics in chunks of N that keep [L, M, chunk] below ``PREDICT_CHUNK_BYTES`` and lets
    autograd keep the chunks: it is the CPU / Matern route, not the fast one."""
    import math
    Lu, LB, c, AAT, rr, var, s2, N = self._collapsed_factors(data, native, "SVGP.collapsed_elbo")
    L = c.shape[0]
    bound = -0.5 * N * L * math.log(2.0 * math.pi) - torch.log(torch.diagonal(LB, dim1=-2, dim2=-1)).sum()
    bound = bound - 0.5 * N * L * torch.log(s2) - rr.sum() / (2.0 * s2) + 0.5 * (c * c).sum()
    bound = bound - N * var.sum() / (2.0 * s2) + 0.5 * torch.diagonal(AAT, dim1=-2, dim2=-1).sum()
    return bound

  def optimal_q(self, data, native: Optional[bool] = None):
    """-> (q_mu [M,L], q_sqrt [L,M,M]) of the q(u) that maximises ``elbo`` at the present hyper-parameters (Titsias 2009, eq. 10),
    in the model's own parametrisation: whitened, q_mu_l = LB^-T c and q_sqrt_l = chol((I + AAT)^-1); not whitened, Lu times the
    mean and chol(Lu (I + AAT)^-1 Lu^T).  Runs under ``torch.no_grad()``; routing as ``collapsed_elbo``."""
    with torch.no_grad():
      Lu, LB, c, AAT, rr, var, s2, N = self._collapsed_factors(data, native, "SVGP.optimal_q")
      M = Lu.shape[-1]
      mu = torch.linalg.solve_triangular(LB.transpose(1, 2), c.unsqueeze(-1), upper=True)      # [L, M, 1]
      LBinv = torch.linalg.solve_triangular(LB, torch.eye(M, dtype=DEFAULT_FLOAT, device=Lu.device).expand_as(LB), upper=False)
      if not self.whiten:
        mu = Lu @ mu
        LBinv = LBinv @ Lu.transpose(1, 2)                                                     # cov = (LB^-1 Lu^T)^T (LB^-1 Lu^T)
      cov = LBinv.transpose(1, 2) @ LBinv
      q_sqrt = cholesky(0.5 * (cov + cov.transpose(1, 2)))
      return mu.squeeze(-1).T.contiguous(), q_sqrt

  def set_optimal_q(self, data, native: Optional[bool] = None):
    """Writes ``optimal_q(data)`` into ``q_mu`` and ``q_sqrt`` in place (their ``_version`` moves: the pack cache repacks)."""
    q_mu, q_sqrt = self.optimal_q(data, native=native)
    with torch.no_grad():
      self.q_mu.copy_(q_mu.to(self.q_mu))
      self.q_sqrt.copy_(q_sqrt.to(self.q_sqrt))

  def collapsed_training_loss(self, data, native: Optional[bool] = None) -> torch.Tensor:
    """-(``collapsed_elbo`` + prior(self)): ``training_loss`` with q(u) at its optimum."""
    objective = self.collapsed_elbo(data, native=native)
    if self.prior is not None:
      objective = objective + self.prior(self)
    return -objective

  @classmethod
  def initialize(cls, data, num_inducing: int, likelihood=None, mean_function="default", kernels=None,
                 coregionalize: Optional[bool] = None, num_latent_gps: Optional[int] = None, max_corr: float = 1.0,
                 seed: Optional[int] = None, **kwargs):
    """A model to start ``training.fit_svgp`` from (models/svgp.py:47-121, models/initializers.py): SquaredExponential latents
    with median-heuristic lengthscales, inducing points by k-means (the data themselves when N <= num_inducing; one draw shared
    by every latent when ``max_corr == 1``, else per distinct kernel with overly correlated points replaced), a ``Constant`` zero
    mean, q_mu = 0 and q_sqrt = I, and -- when the latent count differs from the output count, or on request -- a
    ``LinearCoregionalization`` with row-normalised random ``W``.  ``likelihood=None`` is ``GaussianLikelihood()``; ``seed`` seeds
    the k-means, the replacements and ``W``."""
    X, Y = (_as_param(t) for t in data)
    P = Y.shape[-1]
    L = P if num_latent_gps is None else int(num_latent_gps)
    if coregionalize is None:
      coregionalize = P != L
    if isinstance(mean_function, str) and mean_function == "default":
      mean_function = Constant(torch.zeros(P, dtype=DEFAULT_FLOAT))
    if kernels is None:
      kernels = [SquaredExponential(lengthscales=lengthscales_median(X)) for _ in range(L)]
    gen = None if seed is None else torch.Generator().manual_seed(int(seed))
    cache, points = {}, []
    for kern in kernels:
      key = None if max_corr == 1 else (type(kern), tuple(kern.variance.reshape(-1).tolist()),
                                        tuple(kern.lengthscales.reshape(-1).tolist()))
      if key not in cache:
        cache[key] = inducing_points_kmeans(X, num_inducing, kernel_and_tol=(kern, max_corr), generator=gen)
      points.append(InducingPoints(cache[key].clone()))
    if coregionalize:
      if P == L:
        W = torch.eye(P, dtype=DEFAULT_FLOAT)
      else:
        W = torch.randn(P, L, dtype=DEFAULT_FLOAT, generator=gen)
        W = W / W.norm(dim=-1, keepdim=True)
      kernel = LinearCoregionalization(kernels, W)
    else:
      if P != L:
        raise ValueError(f"{L} independent latents for {P} outputs: coregionalize")
      kernel = SeparateIndependent(kernels)
    M = points[0].Z.shape[0]
    kwargs.setdefault("q_mu", torch.zeros(M, L, dtype=DEFAULT_FLOAT))
    kwargs.setdefault("q_sqrt", torch.eye(M, dtype=DEFAULT_FLOAT).repeat(L, 1, 1))
    return cls(kernel=kernel, inducing_variable=SeparateIndependentInducingVariables(points),
               likelihood=GaussianLikelihood() if likelihood is None else likelihood, mean_function=mean_function,
               num_latent_gps=L, **kwargs)


# ---------------------------------------------------------------------------
# initialisers (models/initializers.py) and the signal-to-noise prior (models/priors.py)
# ---------------------------------------------------------------------------
def lengthscales_median(X: torch.Tensor, lower: float = 0.01, upper: float = 100.0) -> torch.Tensor:
  """Median heuristic: sqrt(1/2) x the median pairwise distance on every dimension, clipped to [1.1 lower, 0.9 upper]."""
  dist = torch.pdist(_as_param(X))
  if dist.numel() == 0:
    med = torch.ones((), dtype=DEFAULT_FLOAT)
  else:
    n = dist.numel()
    med = 0.5 * (dist.kthvalue((n - 1) // 2 + 1).values + dist.kthvalue(n // 2 + 1).values)
  return torch.full((X.shape[-1],), float((0.5 ** 0.5 * med).clamp(1.1 * lower, 0.9 * upper)), dtype=DEFAULT_FLOAT)


def _kmeans(X: torch.Tensor, k: int, generator=None, iterations: int = 50) -> torch.Tensor:
  """k-means++ seeding and Lloyd iterations.  Every centre is a data point or the mean of data points, so it lies inside the
  data's bounding box; a cluster that empties keeps its centre."""
  N = X.shape[0]
  centres = X[torch.randint(N, (1,), generator=generator)]
  d2 = ((X - centres[0]) ** 2).sum(-1)
  for _ in range(1, k):
    if float(d2.sum()) > 0.0:
      i = torch.multinomial(d2 / d2.sum(), 1, generator=generator)
    else:                                                       # fewer distinct points than centres
      i = torch.randint(N, (1,), generator=generator)
    centres = torch.cat([centres, X[i]])
    d2 = torch.minimum(d2, ((X - X[i]) ** 2).sum(-1))
  assign = None
  for _ in range(iterations):
    new = torch.cdist(X, centres).argmin(-1)
    if assign is not None and torch.equal(new, assign):
      break
    assign = new
    sums = torch.zeros_like(centres).index_add_(0, assign, X)
    counts = torch.zeros(k, dtype=X.dtype).index_add_(0, assign, torch.ones(N, dtype=X.dtype))
    centres = torch.where(counts[:, None] > 0, sums / counts.clamp_min(1.0)[:, None], centres)
  return centres


def inducing_points_kmeans(X: torch.Tensor, num_inducing: int, kernel_and_tol=None, generator=None) -> torch.Tensor:
  """Z [min(N, num_inducing), d]: the data when N <= num_inducing, else k-means centres; with ``kernel_and_tol = (kernel, tol)``
  and tol < 1, points correlated above tol are replaced (``replace_duplicates``)."""
  X = _as_param(X).detach().cpu()
  if X.ndim != 2:
    raise ValueError(f"X [N,d] expected, got {tuple(X.shape)}")
  points = X.clone() if X.shape[0] <= num_inducing else _kmeans(X, int(num_inducing), generator)
  if kernel_and_tol is not None and kernel_and_tol[1] < 1:
    points = replace_duplicates(points, *kernel_and_tol, generator=generator)
  return points


def replace_duplicates(points: torch.Tensor, kernel, tol: float, num_attempts: int = 32, generator=None) -> torch.Tensor:
  """Perturb the points whose correlation k(z, z') / variance with another point exceeds ``tol``: the most entangled first, by
  growing Gaussian steps (1e-3 x 1.1^attempt), until no correlation reaches ``tol``; a point that cannot be moved is left."""
  if tol == 1:
    return points
  if not 0 < tol < 1:
    raise ValueError(f"max_corr {tol}: expected a value in (0, 1]")
  import warnings
  points = points.clone()
  with torch.no_grad():
    corr = kernel.K(points) / kernel.variance
    corr.fill_diagonal_(-float("inf"))
    while True:
      hits = (corr > tol).sum(-1)
      if not bool((hits > 0).any()):
        return points
      i = int(hits.argmax())
      for attempt in range(num_attempts):
        alt = points[i] + 1e-3 * 1.1 ** attempt * torch.randn(points.shape[-1], dtype=points.dtype, generator=generator)
        xorr = (kernel.K(points, alt[None]) / kernel.variance).squeeze(-1)
        xorr[i] = -float("inf")
        if not bool((xorr >= tol).any()):
          points[i] = alt
          corr[i, :] = xorr
          corr[:, i] = xorr
          break
      else:
        warnings.warn("failed to replace an overly correlated inducing point; continuing")
        corr[i, :] = -float("inf")
        corr[:, i] = -float("inf")


class AbstractSNR:
  """log signal-to-noise ratio per output of a model with a Gaussian likelihood (models/priors.py:22-44)."""

  def get_log_snr(self, model) -> torch.Tensor:
    if not isinstance(model.likelihood, GaussianLikelihood):
      raise NotImplementedError("the signal-to-noise prior needs a Gaussian likelihood")
    kernel = model.kernel
    log_noise = torch.log(model.likelihood.variance)
    if isinstance(kernel, SharedIndependent):
      log_signals = torch.log(kernel.kernel.variance).expand(model.num_latent_gps)
    elif isinstance(kernel, SeparateIndependent):
      log_signals = torch.log(torch.stack([k.variance for k in kernel.kernels]))
    elif isinstance(kernel, LinearCoregionalization):
      variances = torch.stack([k.variance for k in kernel.kernels])
      log_signals = torch.log((kernel.W ** 2) @ variances.to(kernel.W))
    else:
      log_signals = torch.log(kernel.variance)
    return log_signals - log_noise.to(log_signals)

  def __call__(self, model) -> torch.Tensor:
    raise NotImplementedError


class PilcoPenaltySNR(AbstractSNR):
  """PILCO's penalty on large signal-to-noise ratios: -sum (log snr / log threshold)^power (models/priors.py:47-55)."""

  def __init__(self, threshold: float, power: float):
    self.threshold = threshold
    self.power = power

  def __call__(self, model) -> torch.Tensor:
    import math
    log_snr = self.get_log_snr(model)
    return -((log_snr / math.log(self.threshold)) ** self.power).sum()


class GPR:
  """``gpflow_pilco.models.GPR`` fields: kernel, data=(X, Y), likelihood.variance, mean_function."""

  def __init__(self, data: Tuple, kernel: SquaredExponential, mean_function=None,
               noise_variance=1.0, prior: Optional[Callable] = None):
    X, Y = data
    self.data = (_as_param(X), _as_param(Y))
    self.kernel = kernel
    self.mean_function = Zero() if mean_function is None else mean_function
    self.likelihood = GaussianLikelihood(noise_variance)
    self.prior = prior
    self._cache = _PackCache()

  def __call__(self, x, **kwargs):
    raise NotImplementedError("GPR.predict_f is outside the accelerated path")

  def _parameters(self):
    out = [self.data[0], self.data[1], self.kernel.variance, self.kernel.lengthscales,
           self.likelihood.variance]
    if isinstance(self.mean_function, Constant):
      out.append(self.mean_function.c)
    return out

  @property
  def latent_kernels(self):
    return [self.kernel]

  def precompute(self, device):
    X, Y = (t.to(device=device, dtype=DEFAULT_FLOAT) for t in self.data)
    if Y.shape[-1] != 1:
      raise NotImplementedError("GPR moment matching is single-output (models.py:44-111)")
    c = None
    if isinstance(self.mean_function, Constant):                                    # models.py:53-54
      c = self.mean_function.c.to(device=device, dtype=DEFAULT_FLOAT).reshape(1)
      Y = Y - c
    elif not isinstance(self.mean_function, Zero):
      raise NotImplementedError
    require_squared_exponential([self.kernel], "GPR.precompute")
    Z, ls, var = _stack_kernel_params([self.kernel], [X], device)
    N = X.shape[0]
    Kyy = self.kernel.K(X) + self.likelihood.variance.to(X) * torch.eye(N, dtype=DEFAULT_FLOAT, device=device)
    Lyy = cholesky(Kyy)                                                # :66-68
    beta = torch.cholesky_solve(Y, Lyy).T.contiguous()                              # [1,N]   :75
    C = -torch.cholesky_inverse(Lyy).unsqueeze(0)                                   # -(K + s2 I)^-1  (:86-88)
    return Z, ls, var, beta, C, c

  def packed(self, dtype, with_C: bool, device):
    return self._cache.get(self, dtype, with_C, device)

  # -- prediction at deterministic points ------------------------------------------------------------------------------------
  def predict_f(self, Xnew: torch.Tensor, full_cov: bool = False, full_output_cov: bool = False, native: Optional[bool] = None):
    """gpflow's ``GPR.predict_f`` at Xnew [..., D], single-output as ``precompute``: (mean [..., 1], var [..., 1]), or the
    [..., 1, 1] covariance with ``full_output_cov``.  ``native`` as ``SVGP.predict_f``: the HIP kernel on ``precompute``'s tuple
    (Z = X, beta = (K + s2 I)^-1 (Y - c), C = -(K + s2 I)^-1), or torch (Ly^-1 Kxf; differentiable, any device and family)."""
    if full_cov:
      raise NotImplementedError("GPR.predict_f: full_cov=True is not implemented (marginals per point only)")
    family = kernel_family([self.kernel])
    Xs = self.kernel.slice(Xnew).to(DEFAULT_FLOAT)
    lead, d = Xs.shape[:-1], Xs.shape[-1]
    X2 = Xs.reshape(-1, d)
    refusal = _native_predict_refusal(self, X2, [self.kernel], family, d, False)
    if native and refusal is not None:
      raise ValueError(f"GPR.predict_f(native=True): {refusal}")
    if native is not False and refusal is None:
      from . import ops
      Z, ls, var, beta, C, c = (None if t is None else t.detach() for t in self._cache.pre(self, X2.device))
      mean, var = ops.predict_se(X2.detach(), Z, ls, var, beta, C, c)
    else:
      device = X2.device
      X, Y = (t.to(device=device, dtype=DEFAULT_FLOAT) for t in self.data)
      if Y.shape[-1] != 1:
        raise NotImplementedError("GPR.predict_f is single-output")
      c = None
      if isinstance(self.mean_function, Constant):
        c = self.mean_function.c.to(device=device, dtype=DEFAULT_FLOAT).reshape(1)
        Y = Y - c
      elif not isinstance(self.mean_function, Zero):
        raise NotImplementedError(f"GPR.predict_f: mean function {type(self.mean_function).__name__}")
      n = X.shape[0]
      Ly = cholesky(self.kernel.K(X) + self.likelihood.variance.to(X) * torch.eye(n, dtype=DEFAULT_FLOAT, device=device))
      alpha = torch.linalg.solve_triangular(Ly, Y, upper=False)                   # [n,1]
      chunk = max(1, PREDICT_CHUNK_BYTES // (8 * n))
      means, variances = [], []
      for start in range(0, X2.shape[0], chunk):
        A = torch.linalg.solve_triangular(Ly, self.kernel.K(X, Xnew.reshape(-1, Xnew.shape[-1])[start:start + chunk].to(DEFAULT_FLOAT)),
                                          upper=False)
        means.append(A.T @ alpha)
        variances.append((self.kernel.variance.to(A) - (A * A).sum(0))[:, None])
      mean = torch.cat(means) if means else X2.new_zeros(0, 1)
      var = torch.cat(variances) if variances else X2.new_zeros(0, 1)
      if c is not None:
        mean = mean + c
    if full_output_cov:
      var = var[..., None]
    return mean.reshape(lead + mean.shape[1:]).to(Xnew.dtype), var.reshape(lead + var.shape[1:]).to(Xnew.dtype)

  def predict_y(self, Xnew: torch.Tensor, full_cov: bool = False, full_output_cov: bool = False, native: Optional[bool] = None):
    """``predict_f`` plus the noise variance."""
    mean, var = self.predict_f(Xnew, full_cov=full_cov, full_output_cov=full_output_cov, native=native)
    return _predict_y_from_f(self, "GPR.predict_y", mean, var, full_output_cov)

  def predict_log_density(self, data, native: Optional[bool] = None) -> torch.Tensor:
    """log N(Y | predict_y(X)) per point, [N, 1], for ``data = (X, Y)``."""
    X, Y = data
    mean, var = self.predict_y(X, native=native)
    return _gaussian_log_density(Y.to(mean), mean, var)


class GPModelWrapper:
  """``gpflow_pilco.models.core.GPModelWrapper``: attribute access falls through to the model."""

  def __init__(self, model, **attrs):
    self.__dict__["_model"] = model
    self.__dict__.update(attrs)

  def __getattr__(self, name):
    return getattr(self.__dict__["_model"], name)

  @property
  def model(self):
    return self.__dict__["_model"]


class KernelRegressor(GPModelWrapper):
  """Mean-only view of a model (no predictive uncertainty); models/core.py:60-62."""

  def __call__(self, x, **kwargs):
    return self.model.predict_mean(x)


class InverseLinkWrapper(GPModelWrapper):
  """model followed by an inverse link (bijector chain); models/core.py:65-71."""

  def __init__(self, model, invlink):
    super().__init__(model=model, invlink=invlink)

  def __call__(self, *args, **kwargs):
    return self.invlink(self.model(*args, **kwargs))
