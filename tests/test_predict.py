"""``SVGP.predict_f`` / ``predict_y`` / ``predict_log_density`` and their ``GPR`` counterparts without a GPU: the torch route against
``oracle.pin_oracle.svgp_predict_f`` / ``gpr_predict_f`` at 1e-10 x the absolute-term sum of each output (tests/predict_reference.py),
its gradients, the routing of ``native``, and the argument validation of ``mm_predict_se``, which answers before any HIP call."""
import ctypes
import math

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, models as gp
from oracle import mm_oracle as mo, pin_oracle
from tests.helpers import gp_model_from_oracle
from tests.predict_reference import model_case, model_reference, sums

F64 = torch.float64


def _close(got, want, scale, tol=1e-10):
  err = (got - want).abs()
  assert bool((err <= tol * scale).all()), float((err / scale.clamp_min(1e-300)).max())


@pytest.mark.parametrize("coreg", [False, True], ids=["independent", "coregionalized"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
def test_torch_route_against_oracle(whiten, coreg):
  p, X = model_case(whiten, coreg)
  model = gp_model_from_oracle(p, "cpu")
  ref = model_reference(p, X, model)
  Xt = torch.from_numpy(X)
  mean, cov = model.predict_f(Xt, full_output_cov=True)
  P = 3 if coreg else 2
  assert mean.shape == (X.shape[0], P) and cov.shape == (X.shape[0], P, P)
  _close(mean, ref["mean"], ref["smean"])
  _close(cov, ref["cov"], ref["scov"])
  mean2, var = model.predict_f(Xt, native=False)
  assert var.shape == (X.shape[0], P)
  _close(mean2, ref["mean"], ref["smean"])
  _close(var, torch.diagonal(ref["cov"], dim1=-2, dim2=-1), torch.diagonal(ref["scov"], dim1=-2, dim2=-1))
  # leading dimensions are kept, and the chunked evaluation is the unchunked one
  mean3, cov3 = model.predict_f(Xt.reshape(7, 10, -1), full_output_cov=True)
  assert mean3.shape == (7, 10, P) and torch.equal(mean3.reshape(-1, P), mean) and torch.equal(cov3.reshape(-1, P, P), cov)
  old = gp.PREDICT_CHUNK_BYTES
  try:
    gp.PREDICT_CHUNK_BYTES = 8 * 2 * 40 * 16                  # 16 points a chunk
    mean4, var4 = model.predict_f(Xt)
  finally:
    gp.PREDICT_CHUNK_BYTES = old
  _close(mean4, mean2, ref["smean"], 1e-13)
  _close(var4, var, torch.diagonal(ref["scov"], dim1=-2, dim2=-1), 1e-13)


def _gpr_case():
  rng = np.random.default_rng(21)
  n, d = 30, 3
  X, ls = rng.uniform(size=(n, d)), np.exp(rng.uniform(np.log(0.3), np.log(3.0), size=d))
  Y = np.sin(3.0 * X[:, :1]) + 0.1 * rng.standard_normal((n, 1))
  p = mo.GPRParams(X=X, Y=Y, lengthscales=ls, variance=0.89 ** 2, noise_variance=0.05, mean_c=0.3)
  model = gp.GPR((torch.from_numpy(X), torch.from_numpy(Y)), gp.SquaredExponential(variance=p.variance, lengthscales=torch.from_numpy(ls)),
                 mean_function=gp.Constant(torch.tensor([p.mean_c], dtype=F64)), noise_variance=p.noise_variance)
  return p, model, rng.uniform(-0.2, 1.2, size=(50, d))


def test_gpr_against_oracle():
  p, model, Xnew = _gpr_case()
  mean_o, cov_o = (torch.from_numpy(a) for a in pin_oracle.gpr_predict_f(Xnew, p))
  s = sums(torch.from_numpy(Xnew), *model.precompute("cpu"))
  mean, var = model.predict_f(torch.from_numpy(Xnew))
  assert mean.shape == var.shape == (50, 1)
  _close(mean, mean_o.reshape(50, 1), s["smean"])
  _close(var, cov_o.reshape(50, 1), s["svar"])
  _, cov = model.predict_f(torch.from_numpy(Xnew), full_output_cov=True)
  assert cov.shape == (50, 1, 1) and torch.equal(cov[..., 0], var)
  # predict_y and predict_log_density: the closed form
  Y = torch.from_numpy(np.random.default_rng(3).standard_normal((50, 1)))
  _, yvar = model.predict_y(torch.from_numpy(Xnew))
  assert torch.equal(yvar, var + 0.05)
  want = -0.5 * (math.log(2.0 * math.pi) + torch.log(var + 0.05) + (Y - mean) ** 2 / (var + 0.05))
  assert float((model.predict_log_density((torch.from_numpy(Xnew), Y)) - want).abs().max()) < 1e-12
  with pytest.raises(NotImplementedError, match="full_cov"):
    model.predict_f(torch.from_numpy(Xnew), full_cov=True)
  with pytest.raises(ValueError, match="cpu"):
    model.predict_f(torch.from_numpy(Xnew), native=True)


def test_predict_y_and_log_density_closed_form():
  p, X = model_case(True, True)
  model = gp_model_from_oracle(p, "cpu")
  Xt = torch.from_numpy(X)
  with pytest.raises(NotImplementedError, match="Gaussian likelihood only, got NoneType"):
    model.predict_y(Xt)
  with pytest.raises(NotImplementedError, match="Gaussian likelihood only, got NoneType"):
    model.predict_log_density((Xt, torch.zeros(X.shape[0], 3, dtype=F64)))
  s2 = torch.tensor(0.07, dtype=F64)
  model.likelihood = gp.GaussianLikelihood(s2)
  mean, var = model.predict_f(Xt)
  _, cov = model.predict_f(Xt, full_output_cov=True)
  ymean, yvar = model.predict_y(Xt)
  assert torch.equal(ymean, mean) and torch.equal(yvar, var + s2)
  _, ycov = model.predict_y(Xt, full_output_cov=True)
  assert torch.equal(ycov, cov + s2 * torch.eye(3, dtype=F64))
  Y = torch.from_numpy(np.random.default_rng(4).standard_normal((X.shape[0], 3)))
  want = -0.5 * math.log(2.0 * math.pi) - 0.5 * torch.log(var + s2) - 0.5 * (Y - mean) ** 2 / (var + s2)
  got = model.predict_log_density((Xt, Y))
  assert got.shape == (X.shape[0], 3) and float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
def test_torch_route_is_differentiable(whiten):
  p, _ = model_case(whiten, True, 2, 5, 2, 3)
  model = gp_model_from_oracle(p, "cpu")
  X0 = torch.from_numpy(np.random.default_rng(8).uniform(size=(3, 2)))
  kern = model.kernel.kernels[0]

  def f(X, q_mu, q_sqrt, ls, W):
    model.q_mu, model.q_sqrt, kern.lengthscales, model.kernel.W = q_mu, q_sqrt, ls, W
    mean, cov = model.predict_f(X, full_output_cov=True)
    return mean, cov

  args = tuple(t.clone().requires_grad_(True) for t in (X0, model.q_mu, model.q_sqrt, kern.lengthscales, model.kernel.W))
  assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)
  mean, _ = f(*args)
  assert mean.requires_grad


def test_routing():
  p, X = model_case(True, False)
  model = gp_model_from_oracle(p, "cpu")
  Xt = torch.from_numpy(X)
  with pytest.raises(ValueError, match=r"native=True\): the points are on cpu"):
    model.predict_f(Xt, native=True)
  with pytest.raises(NotImplementedError, match="full_cov=True"):
    model.predict_f(Xt, full_cov=True)
  # a wrapper forwards
  mean, var = model.predict_f(Xt)
  wmean, wvar = gp.KernelRegressor(model).predict_f(Xt)
  assert torch.equal(wmean, mean) and torch.equal(wvar, var)
  # a Matern model takes torch: its own conditional, with the Matern Gram
  t = lambda a: torch.tensor(np.asarray(a), dtype=F64)
  kernels = [gp.Matern52(variance=t(p.variance[a]), lengthscales=t(p.lengthscales[a])) for a in range(2)]
  matern = gp.SVGP(kernel=gp.SeparateIndependent(kernels), inducing_variable=gp.InducingPoints(t(p.Z[0])), q_mu=t(p.q_mu),
                   q_sqrt=t(p.q_sqrt), whiten=True, num_latent_gps=2)
  mmean, mvar = matern.predict_f(Xt)
  for a in range(2):
    Kuu = kernels[a].K(t(p.Z[0])) + gp.DEFAULT_JITTER * torch.eye(40, dtype=F64)
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(Kuu), kernels[a].K(t(p.Z[0]), Xt), upper=False)
    S = torch.tril(t(p.q_sqrt[a]))
    assert float((mmean[:, a] - A.T @ t(p.q_mu[:, a])).abs().max()) < 1e-9
    assert float((mvar[:, a] - (kernels[a].variance - (A * A).sum(0) + ((S.T @ A) ** 2).sum(0))).abs().max()) < 1e-9
  assert float((mmean - mean).abs().max()) > 1e-4            # ... and not the SquaredExponential one
  with pytest.raises(ValueError, match="native=True"):
    matern.predict_f(Xt, native=True)


def test_abi_validation_without_a_gpu():
  """-1 / -2 / -4 before any HIP call (the pointers are never dereferenced), and a size query that ignores N."""
  lib = _lib.lib()
  one = ctypes.c_void_p(8)
  ok = [one] * 5                                               # X Z ls var beta
  call = lambda L, M, N, d, ptrs, C, mean, fvar, ws, nbytes: lib.mm_predict_se(L, M, N, d, *ptrs, C, None, mean, fvar, ws, nbytes, None)
  big = lib.mm_predict_workspace_bytes(2, 17, 5, 3)
  assert big > 0
  for missing in range(5):
    ptrs = [None if i == missing else one for i in range(5)]
    assert call(2, 17, 5, 3, ptrs, one, one, one, one, big) == -1
  assert call(2, 17, 5, 3, ok, one, None, one, one, big) == -1                 # no mean
  assert call(2, 17, 5, 3, ok, one, one, one, None, big) == -1                 # no workspace
  assert call(2, 17, 5, 3, ok, one, one, None, one, big) == -1                 # C without fvar
  assert call(2, 17, 5, 3, ok, None, one, one, one, big) == -1                 # fvar without C
  assert call(2, 17, 5, 33, ok, one, one, one, one, big) == -2                 # d > MM_DMAX
  for L, M, N, d in ((0, 17, 5, 3), (2, 0, 5, 3), (2, 17, 0, 3), (2, 17, 5, 0), (2, 2 ** 20 + 1, 5, 3), (2 ** 16, 17, 2 ** 31 - 1, 3)):
    assert call(L, M, N, d, ok, one, one, one, one, big) == -2
    assert lib.mm_predict_workspace_bytes(L, M, N, d) == 0
  assert call(2, 17, 5, 3, ok, one, one, one, one, big - 1) == -4
  assert call(2, 17, 5, 3, ok, None, one, None, one, big - 1) == -4            # the mean alone asks for the same workspace
  assert lib.mm_predict_workspace_bytes(8, 2000, 2 ** 20, 8) == lib.mm_predict_workspace_bytes(8, 2000, 2 ** 24, 8) > 0
  assert lib.mm_predict_workspace_bytes(1, 1, 1, 1) > 0
  assert lib.mm_predict_workspace_bytes(2, 17, 5, 33) == 0
  assert lib.mm_abi_version() == 2
