"""Moment matching through the policy head's bijectors
(``gpflow_pilco/moment_matching/bijectors.py:21-69``)."""
from __future__ import annotations

import math

import torch

from .. import bijectors as tfb
from ..special import bvn_cdf, ndtr, owens_t
from .core import Chain, LinearOperatorDiag, Moments, dispatcher, moment_matching
from .gaussian import GaussianMatch, GaussianMoments


class HeadNormalCDF(tfb.NormalCDF):
  """``NormalCDF`` as a member of a policy head: the form whose moment match answers n-D inputs (``_mm_gauss_ndtr_head``).
  The bare bijector on an n-D state keeps raising NotImplementedError, as it always has here (that call is pinned by
  tests/test_compose.py); ``tfb.Chain`` and ``InverseLinkWrapper`` -- every way a policy reaches the head -- go through
  ``head_member``."""


def head_member(bijector):
  return HeadNormalCDF() if type(bijector) is tfb.NormalCDF else bijector


@dispatcher.register(Moments, tfb.Chain)
def _mm_chain(x: Moments, bijector: tfb.Chain, /, **kwargs):
  return moment_matching(x, Chain(*(head_member(b) for b in bijector.bijectors)), **kwargs)


@dispatcher.register(Moments, tfb.Shift)
def _mm_shift(x: Moments, bijector: tfb.Shift, /, **kwargs):
  return moment_matching(x, torch.add, bijector.shift, **kwargs)


@dispatcher.register(Moments, tfb.Scale)
def _mm_scale(x: Moments, bijector: tfb.Scale, /, **kwargs):
  return moment_matching(x, torch.mul, bijector.scale, **kwargs)


@dispatcher.register(GaussianMoments, tfb.NormalCDF)
def _mm_gauss_ndtr(x: GaussianMoments, _):
  """bijectors.py:39-58, the 1-D branch (Owen's T).  An n-D state is answered for the members of a policy head
  (``_mm_gauss_ndtr_head``); for the bare bijector it is refused, as before."""
  if x.ndim != 1:
    raise NotImplementedError("NormalCDF moment matching of an n-D input: wrap the bijector in a Chain (the policy head), "
                              "whose members use the bivariate normal CDF")
  return _ndtr_match(x)


@dispatcher.register(GaussianMoments, HeadNormalCDF)
def _mm_gauss_ndtr_head(x: GaussianMoments, _):
  """bijectors.py:39-69 with the n-D branch (:59-63)."""
  return _ndtr_match(x)


def _ndtr_match(x: GaussianMoments):
  """E[Phi(x_i) Phi(x_j)] = P(w_i <= 0, w_j <= 0), w = z - x.

  1-D: Owen's T (:57-58).  n-D (:59-63): y2_ij = Phi2(z_i, z_j; rho_ij), rho_ij = Sxx_ij / sqrt((1 + vx_i)(1 + vx_j)),
  by ``special.bvn_cdf`` (Plackett's integral with closed-form gradients; the reference's Genz BVN of ``utils/bvn.py``
  integrates from -9, see there); the diagonal keeps Owen's T.  The reference returns the 1-D
  second moment with shape [N, 1], which is only consistent for N == 1 (it always uses one
  input distribution); here it is [N, 1, 1] so that batches work."""
  x1 = x.mean()
  Sxx = x.covariance(dense=True)
  vx = torch.diagonal(Sxx, dim1=-2, dim2=-1)
  isq_vw = torch.rsqrt(vx + 1.0)
  z = isq_vw * x1
  y1 = ndtr(z)
  if x.ndim == 1:
    y2 = (y1 - 2.0 * owens_t(z, torch.rsqrt(1.0 + 2.0 * vx))).unsqueeze(-1)
  else:
    n = x.ndim
    iu = torch.triu_indices(n, n, 1, device=x1.device)
    rho = (Sxx * isq_vw.unsqueeze(-1) * isq_vw.unsqueeze(-2))[..., iu[0], iu[1]]
    pair = bvn_cdf(z[..., iu[0]], z[..., iu[1]], rho.clamp(-1.0, 1.0))
    y2 = torch.diag_embed(y1 - 2.0 * owens_t(z, torch.rsqrt(1.0 + 2.0 * vx)))
    y2[..., iu[0], iu[1]] = pair
    y2[..., iu[1], iu[0]] = pair
  vxy = isq_vw * vx * ((2.0 * math.pi) ** -0.5) * torch.exp(-0.5 * z * z)
  y = GaussianMoments(moments=(y1, y2), centered=False)
  return GaussianMatch(x=x, y=y, cross=(LinearOperatorDiag(vxy / vx), True))
