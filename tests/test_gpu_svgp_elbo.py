"""``SVGP.elbo`` on the GPU: the native route (HIP Gram and adjoint, csrc/mm_gram.hip) against the torch route on the same device, in
the value and in the gradient of every parameter.

Tolerance 10 cond(Kuu) 4e-13 -- values relative, gradients relative to each tensor's largest entry; cond(Kuu) is measured here.  The
two routes differ only in the Gram entries, at the 1e-14 var level of tests/test_gpu_gram.py, and the factorisation amplifies that
difference by the conditioning of Kuu."""
import pytest
import torch

from gpflowpilco_amd import models as gp
from gpflowpilco_amd.training import fit_svgp

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _model(device, N=257, M=65, d=9, L=3, whiten=True, coreg=False, matern=False, seed=0):
  """A model with every parameter a leaf on ``device``, its data, and the named leaves."""
  g = torch.Generator().manual_seed(300 + seed)
  r = lambda *s: torch.rand(*s, dtype=F64, generator=g)
  n = lambda *s: torch.randn(*s, dtype=F64, generator=g)
  P = 4 if coreg else L
  leaf = lambda t: t.to(device).requires_grad_(True)
  p = {}
  cls = gp.Matern32 if matern else gp.SquaredExponential
  kernels = []
  for l in range(L):
    p[f"variance{l}"], p[f"lengthscales{l}"] = leaf(0.6 + r(())), leaf(1.5 + r(d))
    kernels.append(cls(p[f"variance{l}"], p[f"lengthscales{l}"]))
  ivs = []
  for l in range(L):
    p[f"Z{l}"] = leaf(n(M, d))
    ivs.append(gp.InducingPoints(p[f"Z{l}"]))
  p["q_mu"], p["q_sqrt"] = leaf(n(M, L)), leaf(torch.tril(0.2 * n(L, M, M)) + 0.8 * torch.eye(M, dtype=F64))
  p["c"], p["noise"] = leaf(n(P)), leaf(torch.tensor(0.2, dtype=F64))
  if coreg:
    p["W"] = leaf(n(P, L))
    kernel = gp.LinearCoregionalization(kernels, p["W"])
  else:
    kernel = gp.SeparateIndependent(kernels)
  model = gp.SVGP(kernel, gp.SeparateIndependentInducingVariables(ivs), p["q_mu"], p["q_sqrt"], whiten=whiten,
                  mean_function=gp.Constant(p["c"]), likelihood=gp.GaussianLikelihood(p["noise"]), num_latent_gps=L)
  return model, (n(N, d).to(device), n(N, P).to(device)), p


def _cond(model):
  with torch.no_grad():
    return max(float(torch.linalg.cond(k.K(iv.Z).cpu() + gp.DEFAULT_JITTER * torch.eye(iv.Z.shape[0], dtype=F64)))
               for k, iv in zip(model.kernel.kernels, model.inducing_variable.inducing_variables))


def _compare_routes(model, data, p):
  tol = 10.0 * _cond(model) * 4e-13
  out = {}
  for native in (None, False):
    value = model.elbo(data, native=native)
    out[native] = (float(value.detach()), torch.autograd.grad(value, list(p.values())))
  (v1, g1), (v0, g0) = out[None], out[False]
  assert abs(v1 - v0) <= tol * abs(v0), (v1, v0, tol)
  for name, a, b in zip(p, g1, g0):
    assert float((a - b).abs().max()) <= tol * float(b.abs().max()), (name, float((a - b).abs().max() / b.abs().max()), tol)
  return tol


@pytest.mark.parametrize("coreg", [False, True], ids=["independent", "coregionalized"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "not_whitened"])
def test_native_route_matches_torch_route(device, whiten, coreg):
  model, data, p = _model(device, whiten=whiten, coreg=coreg)
  tol = _compare_routes(model, data, p)
  assert tol < 1e-7                                              # the inducing points are well separated: the comparison is sharp


def test_native_route_past_the_blocked_factorisation(device):
  """M = 300 > linalg's 256 block: the blocked Cholesky carries the gradient, and hands the self-mode adjoint a matrix that is
  not symmetric."""
  model, data, p = _model(device, M=300, L=1, seed=1)
  _compare_routes(model, data, p)


def test_native_true_refuses_a_matern_model(device):
  model, data, _ = _model(device, N=20, M=6, d=3, L=2, matern=True)
  with pytest.raises(ValueError, match="SquaredExponential only.*Matern32"):
    model.elbo(data, native=True)
  assert float(model.elbo(data)) == float(model.elbo(data, native=False))       # native=None: the torch Gram


def test_native_route_is_taken(device, monkeypatch):
  """``native=None`` on a GPU reaches the HIP Gram entries (it does not quietly build the Gram in torch)."""
  from gpflowpilco_amd import ops
  calls = []
  for name in ("gram_se", "gram_se_backward"):
    monkeypatch.setattr(ops, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(getattr(ops, name), name))
  model, data, p = _model(device, N=40, M=17, d=4, L=2)
  model.elbo(data).backward()
  assert calls.count("gram_se") == 2 and calls.count("gram_se_backward") == 2   # Kuf and Kuu, forward and adjoint
  calls.clear()
  model.elbo(data, native=False).backward()
  assert not calls


def test_fit_on_the_gpu(device):
  g = torch.Generator().manual_seed(11)
  X = 4.0 * torch.rand(150, 2, dtype=F64, generator=g) - 2.0
  Y = torch.stack([torch.sin(1.5 * X[:, 0]) + 0.5 * X[:, 1], torch.cos(X[:, 0]) * torch.tanh(X[:, 1])], -1)
  Y = Y + 0.05 * torch.randn(Y.shape, dtype=F64, generator=g)
  model = gp.SVGP.initialize((X, Y), 20, seed=2)
  versions = [t._version for t in model._parameters()]
  history = fit_svgp(model, (X.to(device), Y.to(device)), max_iter=3)
  assert 2 <= len(history) <= 4 and all(h == h and abs(h) != float("inf") for h in history)
  assert history[-1] < history[0]
  assert all(t._version > v for t, v in zip(model._parameters(), versions))
