"""numpy references of the multi-action policy head (TEST INFRASTRUCTURE ONLY): the bivariate normal CDF by the
Owen's-T identity on ``scipy.special.owens_t``, the n-D NormalCDF moment match (bijectors.py:48-69), a vector Scale,
and the policy functions the rollout oracle (oracle.mm_compose_oracle) takes as ``policy_fn``."""
import numpy as np
from scipy.special import owens_t

from oracle import mm_compose_oracle as co


def bvn_ref(h, k, rho):
  """Phi2(h, k; rho) = (Phi(h) + Phi(k)) / 2 - T(h, (k - rho h) / (h s)) - T(k, (h - rho k) / (k s)) - delta,
  s = sqrt(1 - rho^2), delta = 0 if h k > 0 or (h k = 0 and h + k >= 0) else 1/2 (Owen 1956).  h = 0 or k = 0 by the
  limits: Phi2(0, k) = Phi(k) / 2 + T(k, rho / s), Phi2(0, 0) = 1/4 + asin(rho) / (2 pi)."""
  h, k, rho = np.broadcast_arrays(np.asarray(h, float), np.asarray(k, float), np.asarray(rho, float))
  s = np.sqrt(1.0 - rho * rho)
  with np.errstate(divide="ignore", invalid="ignore"):
    hs = np.where(h == 0.0, 1.0, h); ks = np.where(k == 0.0, 1.0, k)
    gen = (0.5 * (co.ndtr(h) + co.ndtr(k)) - owens_t(h, (k - rho * h) / (hs * s)) - owens_t(k, (h - rho * k) / (ks * s))
           - np.where((h * k > 0.0) | ((h * k == 0.0) & (h + k >= 0.0)), 0.0, 0.5))
    h0 = 0.5 * co.ndtr(k) + owens_t(k, rho / s)
    k0 = 0.5 * co.ndtr(h) + owens_t(h, rho / s)
  both = 0.25 + np.arcsin(rho) / (2.0 * np.pi)
  return np.where((h == 0.0) & (k == 0.0), both, np.where(h == 0.0, h0, np.where(k == 0.0, k0, gen)))


def mm_ndtr_nd(x, pair=bvn_ref):
  """bijectors.py:48-69 for any number of dims: y1_i = Phi(z_i), y2_ij = Phi2(z_i, z_j; rho_ij) (Owen's T on the
  diagonal, as the 1-D branch), pre-inverted diagonal cross.  ``pair``: the bivariate term (``product_pair`` gives the
  head that ignores the correlation between the latents)."""
  x1 = x[0]; Sxx = co.covariance(x)
  n = x1.shape[-1]
  vx = np.diagonal(Sxx, axis1=-2, axis2=-1)
  isq = 1.0 / np.sqrt(vx + 1.0)
  z = isq * x1
  y1 = co.ndtr(z)
  rho = Sxx * isq[..., :, None] * isq[..., None, :]
  y2 = pair(z[..., :, None], z[..., None, :], np.clip(rho, -1.0, 1.0) * (1.0 - np.eye(n)))
  dg = y1 - 2.0 * owens_t(z, 1.0 / np.sqrt(1.0 + 2.0 * vx))
  y2 = y2 * (1.0 - np.eye(n)) + dg[..., :, None] * np.eye(n)
  vxy = isq * vx * (2.0 * np.pi) ** -0.5 * np.exp(-0.5 * z ** 2)
  return dict(x=x, y=(y1, y2, False), cross=(("diag", vxy / vx), True))


def product_pair(h, k, rho):
  return co.ndtr(h) * co.ndtr(k) + 0.0 * rho


def mm_mul(x, c):
  """maths.py:62-79 with a vector c: the second moment scales by the outer product."""
  c = np.asarray(c, float)
  y = (c * x[0], (c[:, None] * c[None, :]) * x[1], x[2])
  return dict(x=x, y=y, cross=(("diag", np.broadcast_to(c, x[0].shape).copy()), True))


def mm_head_nd(x, scale, shift, pair=bvn_ref):
  """Chain[Scale(vec), Shift(vec), NormalCDF] on a Gaussian."""
  return co.mm_chain(x, [lambda s: mm_mul(s, scale), lambda s: co.mm_add(s, np.asarray(shift, float)),
                         lambda s: mm_ndtr_nd(s, pair)])


def mm_policy_nd(x, model, scale, shift, pair=bvn_ref):
  """u = scale * (Phi(f(e)) + shift) with a multi-latent, mean-only regressor (models.py:27-41)."""
  ops = [lambda s: mm_mul(s, scale), lambda s: co.mm_add(s, np.asarray(shift, float)), lambda s: mm_ndtr_nd(s, pair),
         lambda s: co.mm_svgp(s, model, model_uncertainty=False)]
  return co.mm_chain(x, ops)
