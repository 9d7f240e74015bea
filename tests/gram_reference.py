"""Reference of the SE-ARD Gram matrix and its adjoint for tests/test_gram_host.py and tests/test_gpu_gram.py: the difference-form
Gram in float64 torch on the CPU, its gradients by autograd, and -- the scale the tolerances of the adjoint are stated in -- the sum
of the ABSOLUTE values of the terms of every output (the same expressions with |G| and |x - z|)."""
import functools

import torch

F64 = torch.float64


@functools.lru_cache(maxsize=None)
def make_case(L, M, N, d, seed=0):
  """X [N,d], Z [L,M,d], ls [L,d], var [L] and a random G [L,M,N] (and Gs [L,M,M], not symmetric, for the self mode)."""
  g = torch.Generator().manual_seed(1000 * seed + 17 * L + 5 * M + 3 * N + d)
  X = torch.randn(N, d, dtype=F64, generator=g)
  Z = torch.randn(L, M, d, dtype=F64, generator=g)
  ls = (0.4 + 0.6 * torch.rand(L, d, dtype=F64, generator=g)) * d ** 0.5
  var = 0.5 + torch.rand(L, dtype=F64, generator=g)
  G = torch.randn(L, M, N, dtype=F64, generator=g)
  Gs = torch.randn(L, M, M, dtype=F64, generator=g)
  return X, Z, ls, var, G, Gs


def _diff(X, Z):
  """[L,M,N,d]: x_n - z_lm; X None: z_ln - z_lm (both slots are Z)."""
  return (Z[:, None, :, :] if X is None else X[None, None, :, :]) - Z[:, :, None, :]


def gram(X, Z, ls, var):
  """K [L,M,N] = var exp(-1/2 sum_k ((x_nk - z_lmk) / ls_lk)^2), from differences."""
  r = _diff(X, Z) / ls[:, None, None, :]
  return var[:, None, None] * torch.exp(-0.5 * (r * r).sum(-1))


@functools.lru_cache(maxsize=None)
def reference(L, M, N, d, self_mode=False, seed=0):
  """-> dict(K, gZ, gls, gvar, sZ, sls, svar): the Gram matrix, autograd's gradients of sum(G K), and the absolute-term sums."""
  X, Z, ls, var, G, Gs = make_case(L, M, N, d, seed)
  return reference_of(None, Z, ls, var, Gs) if self_mode else reference_of(X, Z, ls, var, G)


def reference_of(X, Z, ls, var, G):
  """The same for given CPU operands; X None: the self mode, G [L,M,M] any matrix."""
  self_mode = X is None
  Zr, lr, vr = (t.clone().requires_grad_(True) for t in (Z, ls, var))
  K = gram(X, Zr, lr, vr)
  gZ, gls, gvar = torch.autograd.grad((G * K).sum(), (Zr, lr, vr))
  K = K.detach()
  diff = _diff(X, Z).abs()
  t = G.abs() * K
  tz = (G.abs() + G.abs().transpose(1, 2)) * K if self_mode else t
  return dict(K=K, gZ=gZ, gls=gls, gvar=gvar,
              sZ=(tz[..., None] * diff).sum(2) / ls[:, None, :] ** 2,
              sls=(t[..., None] * diff ** 2).sum((1, 2)) / ls ** 3,
              svar=t.sum((1, 2)) / var)
