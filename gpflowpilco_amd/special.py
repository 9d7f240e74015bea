"""Special functions used by the NormalCDF moment match (moment_matching/bijectors.py:39-69):
``ndtr`` (utils/bvn.py:38-42), Owen's T (tensorflow_probability ``owens_t``, third party) and the bivariate
normal CDF of the n-D branch (bijectors.py:59-63)."""
from __future__ import annotations

import math

import numpy as np
import torch

_GL_X, _GL_W = np.polynomial.legendre.leggauss(48)


_GL_CACHE = {}


def ndtr(x: torch.Tensor) -> torch.Tensor:
  return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def owens_t(h: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
  """T(h, a) = 1/(2 pi) int_0^a exp(-h^2 (1 + x^2) / 2) / (1 + x^2) dx for 0 <= a <= 1
  (the only range bijectors.py:58 needs: a = rsqrt(1 + 2 v)), by 48-point Gauss-Legendre."""
  key = (h.dtype, str(h.device))
  if key not in _GL_CACHE:                                     # uploaded once per (dtype, device)
    _GL_CACHE[key] = (torch.as_tensor(_GL_X, dtype=h.dtype, device=h.device),
                      torch.as_tensor(_GL_W, dtype=h.dtype, device=h.device))
  xs, ws = _GL_CACHE[key]
  t = 0.5 * a.unsqueeze(-1) * (xs + 1.0)                       # nodes on [0, a]
  f = torch.exp(-0.5 * h.unsqueeze(-1) ** 2 * (1.0 + t * t)) / (1.0 + t * t)
  return (0.5 * a) * (f * ws).sum(-1) / (2.0 * math.pi)


BVN_PANELS = 4                                                 # equal 48-point panels on [0, asin rho] (csrc/mm_compose_nd.hip too)


def _bvn_forward(h: torch.Tensor, k: torch.Tensor, rho: torch.Tensor) -> torch.Tensor:
  key = ("bvn", h.dtype, str(h.device))
  if key not in _GL_CACHE:
    x01 = np.concatenate([(p + 0.5 * (_GL_X + 1.0)) / BVN_PANELS for p in range(BVN_PANELS)])
    w01 = np.tile(0.5 * _GL_W / BVN_PANELS, BVN_PANELS)
    _GL_CACHE[key] = (torch.as_tensor(x01, dtype=h.dtype, device=h.device),
                      torch.as_tensor(w01, dtype=h.dtype, device=h.device))
  xs, ws = _GL_CACHE[key]
  a = torch.asin(rho.clamp(-1.0, 1.0))
  t = a.unsqueeze(-1) * xs                                     # nodes on [0, asin rho]
  st, c2 = torch.sin(t), torch.cos(t) ** 2
  hh, kk = h.unsqueeze(-1), k.unsqueeze(-1)
  f = torch.exp(-(hh * hh + kk * kk - 2.0 * hh * kk * st) / (2.0 * c2))
  ph, pk = ndtr(h), ndtr(k)
  out = ph * pk + a * (f * ws).sum(-1) / (2.0 * math.pi)
  # Frechet bounds max(0, Phi(h) + Phi(k) - 1) <= Phi2 <= min(Phi(h), Phi(k)): keeps the quadrature's error out of the tails
  return torch.minimum(torch.maximum(out, (ph + pk - 1.0).clamp_min(0.0)), torch.minimum(ph, pk))


class _BvnCdf(torch.autograd.Function):

  @staticmethod
  def forward(ctx, h, k, rho):
    ctx.shapes = (h.shape, k.shape, rho.shape)
    h, k, rho = torch.broadcast_tensors(h, k, rho)
    ctx.save_for_backward(h, k, rho)
    return _bvn_forward(h, k, rho)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, g):
    h, k, rho = ctx.saved_tensors
    s2 = 1.0 - rho * rho
    s = torch.sqrt(s2)
    phi = lambda x: torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    gh = g * phi(h) * ndtr((k - rho * h) / s) if ctx.needs_input_grad[0] else None
    gk = g * phi(k) * ndtr((h - rho * k) / s) if ctx.needs_input_grad[1] else None
    gr = (g * torch.exp(-(h * h - 2.0 * rho * h * k + k * k) / (2.0 * s2)) / (2.0 * math.pi * s)
          if ctx.needs_input_grad[2] else None)
    return tuple(None if t is None else t.sum_to_size(shape) for t, shape in zip((gh, gk, gr), ctx.shapes))


def bvn_cdf(h: torch.Tensor, k: torch.Tensor, rho: torch.Tensor) -> torch.Tensor:
  """Phi2(h, k; rho) = P(X <= h, Y <= k) of a standard bivariate normal with correlation rho (|rho| <= 1), broadcasting.

  Plackett's integral Phi(h) Phi(k) + 1/(2 pi) int_0^{asin rho} exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)) dt by
  Gauss-Legendre on four equal 48-point panels (the nodes ``owens_t`` uses).  float64 error against the Owen's-T identity
  on |h|, |k| <= 6: <= 1.3e-15 for |rho| <= 0.9999, 1.4e-8 at |rho| = 0.999999 (the integrand's width shrinks like
  sqrt(1 - rho^2)).

  The gradient is the closed form -- dPhi2/dh = phi(h) Phi((k - rho h) / sqrt(1 - rho^2)), the same in k, dPhi2/drho =
  the bivariate density -- not the derivative of the quadrature (first order only; it needs |rho| < 1).  The lower
  limit is -inf: the reference integrates from -9 because the gradient of ITS quadrature becomes unstable
  (bijectors.py:59-60), which the closed form does not; the two differ by less than 2 Phi(-9) = 2.3e-19."""
  ref = next((t for t in (h, k, rho) if isinstance(t, torch.Tensor)), None)
  if ref is None:
    ref = torch.zeros((), dtype=torch.get_default_dtype())
  h, k, rho = (t if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=ref.dtype, device=ref.device)
               for t in (h, k, rho))
  return _BvnCdf.apply(h, k, rho)
