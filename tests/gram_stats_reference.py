"""Reference of the streamed Gram statistics Phi = K K^T, Psi = K R and of their adjoint for tests/test_gram_stats_host.py and
tests/test_gpu_gram_stats.py: float64 torch on the CPU from coordinate differences (tests/gram_reference.py's Gram), the gradients
of sum(GPhi Phi) + sum(GPsi Psi) by autograd, and -- the scale every tolerance is stated in -- each output's sum of the ABSOLUTE
values of its terms: the same expressions with |GPhi + GPhi^T| K + |GPsi| |R|^T for the adjoint of K (K >= 0), |R| and |x - z|."""
import functools

import torch

from tests.gram_reference import _diff, gram, make_case as _gram_case

F64 = torch.float64

# (L, M, N, d, Q): one point, block and chunk edges on both sides of 64, d and Q at their limits, two and three blocks
SHAPES = [(1, 1, 1, 1, 0), (2, 63, 65, 9, 3), (1, 64, 64, 32, 1), (2, 65, 63, 9, 33), (1, 129, 130, 4, 2), (3, 37, 1, 3, 1),
          (2, 130, 257, 17, 3), (1, 16, 128, 16, 1)]


@functools.lru_cache(maxsize=None)
def make_case(L, M, N, d, Q, seed=0):
  """X [N,d], R [N,Q] (None when Q = 0), Z [L,M,d], ls [L,d], var [L], GPhi [L,M,M] (not symmetric), GPsi [L,M,Q] (None)."""
  X, Z, ls, var, _, GPhi = _gram_case(L, M, N, d, seed)
  g = torch.Generator().manual_seed(77 + 1000 * seed + 13 * L + 7 * M + 5 * N + 3 * d + Q)
  R = torch.randn(N, Q, dtype=F64, generator=g) if Q else None
  GPsi = torch.randn(L, M, Q, dtype=F64, generator=g) if Q else None
  return X, R, Z, ls, var, GPhi, GPsi


@functools.lru_cache(maxsize=None)
def reference(L, M, N, d, Q, seed=0):
  return reference_of(*make_case(L, M, N, d, Q, seed))


def reference_of(X, R, Z, ls, var, GPhi, GPsi):
  """-> dict(Phi, Psi, gZ, gls, gvar, sPhi, sPsi, sZ, sls, svar); Psi and sPsi None without R."""
  Zr, lr, vr = (t.clone().requires_grad_(True) for t in (Z, ls, var))
  K = gram(X, Zr, lr, vr)
  Phi = K @ K.transpose(1, 2)
  Psi = None if R is None else K @ R
  loss = (GPhi * Phi).sum() + (0.0 if R is None else (GPsi * Psi).sum())
  gZ, gls, gvar = torch.autograd.grad(loss, (Zr, lr, vr))
  K = K.detach()
  GK = (GPhi + GPhi.transpose(1, 2)).abs() @ K
  if R is not None:
    GK = GK + GPsi.abs() @ R.abs().T
  t = GK * K
  diff = _diff(X, Z).abs()
  return dict(Phi=Phi.detach(), Psi=None if R is None else Psi.detach(), gZ=gZ, gls=gls, gvar=gvar,
              sPhi=Phi.detach(), sPsi=None if R is None else K @ R.abs(),
              sZ=(t[..., None] * diff).sum(2) / ls[:, None, :] ** 2,
              sls=(t[..., None] * diff ** 2).sum((1, 2)) / ls ** 3,
              svar=t.sum((1, 2)) / var)


def assert_close(got, ref, tol, names=("Phi", "Psi", "gZ", "gls", "gvar"), tols=None):
  """|got - ref| <= tol x the output's absolute-term sum, entry by entry; prints every figure before it asserts."""
  scale = dict(Phi="sPhi", Psi="sPsi", gZ="sZ", gls="sls", gvar="svar")
  worst = {}
  for name in names:
    if ref[name] is None:
      assert got[name] is None
      continue
    worst[name] = float(((got[name] - ref[name]).abs() / ref[scale[name]].clamp_min(1e-300)).max())
  print("error / absolute-term sum:", worst)
  for name, w in worst.items():
    bound = tol if tols is None else tols.get(name, tol)
    assert w <= bound, (name, w, bound)
