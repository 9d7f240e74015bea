"""Monte Carlo estimate of what ``moment_matching(x, model)`` computes in closed form: the reference's acceptance check
(``tests/test_moment_matching.py:57-84``) as a public function, on the model's own ``predict_f``."""
from __future__ import annotations

from typing import Optional

import torch

from .gaussian import GaussianMatch, GaussianMoments

__all__ = ("sampled_moments",)


def sampled_moments(x: GaussianMoments, model, num_samples: int = 10 ** 6, generator: Optional[torch.Generator] = None,
                    samples: Optional[torch.Tensor] = None, model_uncertainty: bool = True, chunk: int = 2 ** 18) -> GaussianMatch:
  """Draw X [S, B, d] ~ N(mean, cov) of ``x`` (Cholesky factor times ``torch.randn`` under ``generator``; or the caller's ``samples``
  [S, B, d]), evaluate ``model.predict_f(X, full_output_cov=True)`` chunk by chunk (``chunk`` draws of every batch element at a
  time) and accumulate sum f, sum f f^T, sum F_cov and sum x f^T in float64:

    y     = N(mean f, Cov(F_mu) + E[F_cov])      (``model_uncertainty=False``: without E[F_cov])
    cross = (Cov(x, f), False)                   (not pre-inverted)

  With the native ``predict_f`` a model's closed-form match can be checked at 10^6 draws; the error of the estimate is the
  reference's ``10 / sqrt(S)`` for moments of order one."""
  mean = x.mean().to(torch.float64)
  cov = x.covariance(dense=True).to(torch.float64)
  B, d = mean.shape
  if samples is None:
    S = int(num_samples)
    sqrt = torch.linalg.cholesky(cov)
  else:
    if samples.ndim != 3 or samples.shape[1:] != (B, d):
      raise ValueError(f"sampled_moments: samples [S,{B},{d}] expected, got {tuple(samples.shape)}")
    S = samples.shape[0]
  if S <= 0 or chunk <= 0:
    raise ValueError(f"sampled_moments: {S} samples in chunks of {chunk}")
  s_f = s_ff = s_var = s_xf = None
  for start in range(0, S, chunk):
    n = min(chunk, S - start)
    if samples is None:
      rvs = torch.randn(n, B, d, dtype=torch.float64, device=mean.device, generator=generator)
      X = mean + torch.einsum("bij,sbj->sbi", sqrt, rvs)
    else:
      X = samples[start:start + n].to(mean)
    F_mu, F_cov = model.predict_f(X.reshape(n * B, d), full_output_cov=True)
    P = F_mu.shape[-1]
    F_mu = F_mu.to(torch.float64).reshape(n, B, P)
    F_cov = F_cov.to(torch.float64).reshape(n, B, P, P)
    parts = (F_mu.sum(0), torch.einsum("sbi,sbj->bij", F_mu, F_mu), F_cov.sum(0), torch.einsum("sbi,sbj->bij", X, F_mu))
    if s_f is None:
      s_f, s_ff, s_var, s_xf = parts
    else:
      s_f, s_ff, s_var, s_xf = s_f + parts[0], s_ff + parts[1], s_var + parts[2], s_xf + parts[3]
  mf = s_f / S
  Sff = s_ff / S - mf[:, :, None] * mf[:, None, :]
  if model_uncertainty:
    Sff = Sff + s_var / S
  Sxf = s_xf / S - mean[:, :, None] * mf[:, None, :]
  return GaussianMatch(x=x, y=GaussianMoments(moments=(mf, Sff), centered=True), cross=(Sxf, False))
