"""``SVGP.collapsed_elbo`` / ``optimal_q`` / ``set_optimal_q`` (torch route, CPU, float64) and ``fit_svgp(collapsed=True)``.

* The collapsed bound against its dense statement, sum_l log N(y_l | c_l, Qff_l + s2 I) - tr(Kff_l - Qff_l) / (2 s2) with the
  determinant from ``slogdet``; numpy, Gram matrices from coordinate differences (``tests/test_svgp_elbo.py``'s helpers and design:
  cond(Kuu) <= 1e3, asserted, and that file's tolerance 1e-9 for the same reason).
* The optimal q(u): after ``set_optimal_q`` the ELBO equals the collapsed bound, and every perturbation of q lowers it.  The
  second-order drop of a perturbation of size 1e-3 is of order 1e-6 M against rounding of order 1e-11: no tolerance is involved.
"""
import math

import numpy as np
import pytest
import torch

from gpflowpilco_amd import models as gp
from gpflowpilco_amd import training
from gpflowpilco_amd.training import fit_svgp
from gpflowpilco_amd.linalg import CholeskyError
from tests.test_svgp_elbo import JITTER, _gram_np, _kuu, make_model
from tests.test_svgp_fit import _data

F64 = torch.float64


def dense_collapsed(model, data, max_cond=1e3):
  X, Y = (t.numpy() for t in data)
  N = X.shape[0]
  s2 = float(model.likelihood.variance)
  kernels, Zs = gp.unpack_multioutput(model.kernel, model.inducing_variable, model.num_latent_gps)
  c = model.mean_function.c.detach().numpy() if isinstance(model.mean_function, gp.Constant) else np.zeros(len(kernels))
  c = np.broadcast_to(c, (len(kernels),))
  want = 0.0
  for l, (k, Z) in enumerate(zip(kernels, Zs)):
    Z = Z.numpy()
    Kuu, Kuf = _gram_np(k, Z, Z) + JITTER * np.eye(Z.shape[0]), _gram_np(k, Z, X)
    assert np.linalg.cond(Kuu) <= max_cond
    r = Y[:, l] - c[l]
    Qff = Kuf.T @ np.linalg.solve(Kuu, Kuf)
    C = Qff + s2 * np.eye(N)
    want += (-0.5 * (N * math.log(2.0 * math.pi) + np.linalg.slogdet(C)[1] + r @ np.linalg.solve(C, r))
             - (N * float(k.variance) - np.trace(Qff)) / (2.0 * s2))
  return want


def _shared_model():
  """A ``SharedIndependent`` kernel on shared inducing points, three outputs, on the grid design."""
  base, (X, _) = make_model(seed=5)
  g = torch.Generator().manual_seed(11)
  kernel = gp.SharedIndependent(base.kernel.kernels[0], 3)
  iv = gp.SharedIndependentInducingVariables(base.inducing_variable.inducing_variables[0])
  M = iv.inducing_variable.Z.shape[0]
  model = gp.SVGP(kernel, iv, torch.zeros(M, 3, dtype=F64), torch.eye(M, dtype=F64).repeat(3, 1, 1),
                  mean_function=gp.Constant(torch.randn(3, dtype=F64, generator=g)), likelihood=gp.GaussianLikelihood(0.2),
                  num_latent_gps=3)
  return model, (X, torch.randn(X.shape[0], 3, dtype=F64, generator=g))


CASES = {"whitened": dict(whiten=True), "not_whitened": dict(whiten=False), "constant_mean": dict(whiten=True, const=True),
         "constant_mean_not_whitened": dict(whiten=False, const=True, seed=3), "matern32": dict(whiten=True, matern=True, const=True)}


@pytest.mark.parametrize("case", sorted(CASES) + ["shared"])
def test_collapsed_elbo_against_the_dense_statement(case):
  model, data = _shared_model() if case == "shared" else make_model(**CASES[case])
  got, want = float(model.collapsed_elbo(data)), dense_collapsed(model, data)
  assert abs(got - want) <= 1e-9 * abs(want), (got, want)
  assert float(model.collapsed_elbo(data, native=False)) == got            # on the CPU both requests take the torch route


def test_collapsed_elbo_chunks_the_points(monkeypatch):
  model, data = make_model(const=True)
  want = float(model.collapsed_elbo(data))
  monkeypatch.setattr(gp, "PREDICT_CHUNK_BYTES", 8 * 2 * 12 * 7)            # chunks of 7 of the 50 points
  got = float(model.collapsed_elbo(data))
  assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("whiten", [True, False])
def test_elbo_at_the_optimal_q_is_the_collapsed_bound(whiten):
  model, data = make_model(whiten=whiten, const=True, seed=3)
  before = (model.q_mu, model.q_sqrt, model.q_mu._version, model.q_sqrt._version)
  assert abs(float(model.elbo(data)) - float(model.collapsed_elbo(data))) > 1.0      # the random q is far from the optimum
  q_mu, q_sqrt = model.optimal_q(data)
  assert q_mu.shape == model.q_mu.shape and q_sqrt.shape == model.q_sqrt.shape and not q_mu.requires_grad
  assert torch.equal(q_sqrt, torch.tril(q_sqrt))
  model.set_optimal_q(data)
  assert model.q_mu is before[0] and model.q_sqrt is before[1]
  assert model.q_mu._version > before[2] and model.q_sqrt._version > before[3]
  assert torch.equal(model.q_mu, q_mu) and torch.equal(model.q_sqrt, q_sqrt)
  got, want = float(model.elbo(data)), float(model.collapsed_elbo(data))
  assert abs(got - want) <= 1e-9 * abs(want), (got, want)


@pytest.mark.parametrize("whiten", [True, False])
def test_every_perturbation_of_the_optimal_q_lowers_the_elbo(whiten):
  model, data = make_model(whiten=whiten, const=True, seed=3)
  model.set_optimal_q(data)
  best = float(model.elbo(data))
  q_mu, q_sqrt = model.q_mu.clone(), model.q_sqrt.clone()
  g = torch.Generator().manual_seed(17)
  for _ in range(5):
    d_mu = torch.randn(q_mu.shape, dtype=F64, generator=g)
    d_sq = torch.tril(torch.randn(q_sqrt.shape, dtype=F64, generator=g))
    for dm, ds in ((d_mu, 0.0 * d_sq), (0.0 * d_mu, d_sq)):                 # q_mu alone, then tril(q_sqrt) alone
      model.q_mu, model.q_sqrt = q_mu + 1e-3 * dm, q_sqrt + 1e-3 * ds
      assert float(model.elbo(data)) < best


@pytest.mark.parametrize("whiten", [True, False])
def test_collapsed_elbo_gradients(whiten):
  """``torch.autograd.gradcheck`` in every hyper-parameter at N 10, M 5, d 2, L 2 (the settings of ``test_elbo_gradients``)."""
  n, m, d, L = 10, 5, 2, 2
  g = torch.Generator().manual_seed(7)
  X, Y = torch.rand(n, d, dtype=F64, generator=g) * 2.0, torch.randn(n, L, dtype=F64, generator=g)
  params = dict(var=0.6 + torch.rand(L, dtype=F64, generator=g), ls=0.7 + 0.3 * torch.rand(L, d, dtype=F64, generator=g),
                Z=torch.rand(L, m, d, dtype=F64, generator=g) * 2.0, c=torch.randn(L, dtype=F64, generator=g),
                s2=torch.tensor(0.3, dtype=F64))
  names = sorted(params)

  def f(*values):
    p = dict(zip(names, values))
    kernels = [gp.SquaredExponential(p["var"][l], p["ls"][l]) for l in range(L)]
    iv = gp.SeparateIndependentInducingVariables([gp.InducingPoints(p["Z"][l]) for l in range(L)])
    model = gp.SVGP(gp.SeparateIndependent(kernels), iv, torch.zeros(m, L, dtype=F64), torch.eye(m, dtype=F64).repeat(L, 1, 1),
                    whiten=whiten, mean_function=gp.Constant(p["c"]), likelihood=gp.GaussianLikelihood(p["s2"]), num_latent_gps=L)
    return model.collapsed_elbo((X, Y))

  inputs = tuple(params[k].clone().requires_grad_(True) for k in names)
  assert torch.autograd.gradcheck(f, inputs, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_collapsed_elbo_does_not_read_q():
  model, data = make_model(const=True)
  want = float(model.collapsed_elbo(data))
  model.q_mu, model.q_sqrt = None, None
  assert float(model.collapsed_elbo(data)) == want


def test_collapsed_training_loss_is_minus_bound_plus_prior():
  model, data = make_model(const=True)
  model.prior = gp.PilcoPenaltySNR(1000.0, 30.0)
  assert float(model.collapsed_training_loss(data)) == -float(model.collapsed_elbo(data) + model.prior(model))


def test_collapsed_refusals():
  model, data = make_model()
  with pytest.raises(ValueError, match="native=True.*cpu"):
    model.collapsed_elbo(data, native=True)
  coreg, cdata = make_model(coreg=True)
  for call in (coreg.collapsed_elbo, coreg.optimal_q, coreg.set_optimal_q, coreg.collapsed_training_loss):
    with pytest.raises(NotImplementedError, match="couples the latents through W.*elbo / fit_svgp remain"):
      call(cdata)
  with pytest.raises(NotImplementedError, match="couples the latents through W"):
    fit_svgp(coreg, cdata, collapsed=True)
  model.likelihood = object()
  with pytest.raises(NotImplementedError, match="Gaussian"):
    model.collapsed_elbo(data)
  with pytest.raises(NotImplementedError, match="Gaussian"):
    fit_svgp(model, data, collapsed=True)


def test_collapsed_fit(monkeypatch):
  """N 150, M 20, d 2, L 2: the design of ``tests/test_svgp_fit.py``."""
  X, Y, _ = _data(150)
  model = gp.SVGP.initialize((X, Y), 20, seed=1, prior=gp.PilcoPenaltySNR(1000.0, 30.0))
  tensors = model._parameters() + [model.likelihood.variance]
  versions = [t._version for t in tensors]
  start = float(model.collapsed_training_loss((X, Y)))
  seen = []
  lbfgs = torch.optim.LBFGS
  monkeypatch.setattr(training.torch.optim, "LBFGS", lambda params, **kw: (seen.extend(params), lbfgs(seen, **kw))[1])
  history = fit_svgp(model, (X, Y), max_iter=25, collapsed=True)
  monkeypatch.undo()
  assert 2 <= len(history) <= 26
  assert all(h == h and abs(h) != float("inf") for h in history)
  assert history[0] == pytest.approx(start, rel=1e-12)             # (the leaves are the constraints' inverses: a rounding apart)
  assert all(b <= a for a, b in zip(history, history[1:])) and history[-1] < history[0]
  # the hyper-parameters alone are optimised: 2 x (variance, lengthscales, Z), the noise, the constant mean
  M, L = model.q_mu.shape
  d = X.shape[1]
  assert sorted(tuple(p.shape) for p in seen) == sorted(2 * [(), (d,), (M, d)] + [(), (L,)])
  assert not any(p.shape == (L, M * (M + 1) // 2) for p in seen)             # (q_mu [M, L] has Z's shape here: counted above)
  assert all(t._version > v for t, v in zip(tensors, versions))
  assert all(a is b for a, b in zip(tensors, model._parameters()))
  # the model's q is the optimum at the fitted hyper-parameters
  assert float(model.training_loss((X, Y))) == pytest.approx(history[-1], rel=1e-8)
  assert float(model.collapsed_training_loss((X, Y))) == pytest.approx(history[-1], rel=1e-12)


def test_collapsed_fit_refuses_a_kernel_regressor():
  X, Y, _ = _data(40)
  model = gp.SVGP.initialize((X, Y), 8, seed=5)
  with pytest.raises(NotImplementedError, match="KernelRegressor.*q_sqrt frozen.*lengthscales"):
    fit_svgp(gp.KernelRegressor(model), (X, Y), collapsed=True)


def _fit_with_a_failing_call(failing_call, error):
  """``fit_svgp(collapsed=True)`` whose ``failing_call``-th loss evaluation raises ``error`` -> (history, evaluations made)."""
  X, Y, _ = _data(60)
  model = gp.SVGP.initialize((X, Y), 10, seed=5)
  loss, calls = model.collapsed_training_loss, []

  def flaky(data, native=None):
    calls.append(len(calls))
    if len(calls) == failing_call:
      raise error
    return loss(data, native=native)
  model.collapsed_training_loss = flaky
  return fit_svgp(model, (X, Y), max_iter=4, collapsed=True), len(calls)


def test_collapsed_fit_rejects_a_trial_point_with_a_singular_bound():
  """The second evaluation is the first trial point of the first line search: rejected, the search backs off and the fit goes on."""
  clean, n_clean = _fit_with_a_failing_call(0, None)
  history, n = _fit_with_a_failing_call(2, gp.SingularCollapsedBound("I + AAT"))
  assert n > 2 and all(h == h and abs(h) < 1e9 for h in history)
  assert history[0] == clean[0] and history[-1] < history[0] and all(b <= a for a, b in zip(history, history[1:]))


def test_collapsed_fit_raises_every_other_failure():
  with pytest.raises(gp.SingularCollapsedBound):                    # at the starting point nothing can be rejected
    _fit_with_a_failing_call(1, gp.SingularCollapsedBound("I + AAT"))
  with pytest.raises(CholeskyError, match="Kuu"):                   # a failure of Kuu + jitter I is not the bound's
    _fit_with_a_failing_call(2, CholeskyError("Kuu"))


def test_a_singular_bound_has_its_own_error():
  model, (X, Y) = make_model(const=True)
  data = (X[:5], Y[:5])                                             # 5 points against 12 inducing points: AAT has rank 5,
  model.likelihood.variance = torch.tensor(1e-30, dtype=F64)        # and at this noise the identity is lost to rounding
  with pytest.raises(gp.SingularCollapsedBound, match="I \\+ AAT is singular.*1.000e-30"):
    model.collapsed_elbo(data)
  assert issubclass(gp.SingularCollapsedBound, CholeskyError)
