"""``SVGP.initialize`` and ``training.fit_svgp`` on the CPU (torch route of the ELBO)."""
import functools

import pytest
import torch

from gpflowpilco_amd import models as gp
from gpflowpilco_amd.training import fit_svgp

F64 = torch.float64


def _data(N, d=2, P=2, seed=0, noise=0.05):
  """A known smooth function of x in [-2, 2]^d plus noise."""
  g = torch.Generator().manual_seed(200 + seed)
  X = 4.0 * torch.rand(N, d, dtype=F64, generator=g) - 2.0
  F = torch.stack([torch.sin(1.5 * X[:, 0]) + 0.5 * X[:, 1], torch.cos(X[:, 0]) * torch.tanh(X[:, 1]) + 0.3], -1)[:, :P]
  return X, F + noise * torch.randn(N, P, dtype=F64, generator=g), F


# ---- initialize -------------------------------------------------------------------------------------------------------------
def test_initialize_shapes_and_lengthscales():
  X, Y, _ = _data(120)
  model = gp.SVGP.initialize((X, Y), 15, seed=1)
  assert isinstance(model.kernel, gp.SeparateIndependent) and model.num_latent_gps == 2
  assert model.q_mu.shape == (15, 2) and model.q_sqrt.shape == (2, 15, 15) and model.whiten
  assert isinstance(model.mean_function, gp.Constant) and torch.equal(model.mean_function.c, torch.zeros(2, dtype=F64))
  assert isinstance(model.likelihood, gp.GaussianLikelihood)
  Zs = [iv.Z for iv in model.inducing_variable.inducing_variables]
  assert len(Zs) == 2 and all(z.shape == (15, 2) for z in Zs)
  assert torch.equal(Zs[0], Zs[1]) and Zs[0].data_ptr() != Zs[1].data_ptr()       # max_corr = 1: one draw, a tensor per latent
  # every k-means centre lies inside the data's bounding box
  assert bool((Zs[0] >= X.min(0).values).all()) and bool((Zs[0] <= X.max(0).values).all())
  for k in model.kernel.kernels:
    assert k.lengthscales.shape == (2,)
    assert bool((k.lengthscales >= 1.1 * 0.01).all()) and bool((k.lengthscales <= 0.9 * 100.0).all())
  # the median heuristic itself
  want = 0.5 ** 0.5 * float(torch.pdist(X).quantile(0.5))
  assert abs(float(model.kernel.kernels[0].lengthscales[0]) - want) <= 1e-12 * want
  assert torch.isfinite(model.elbo((X, Y)))


def test_initialize_clips_the_lengthscales():
  X, Y, _ = _data(30)
  assert float(gp.lengthscales_median(1e-4 * X)[0]) == pytest.approx(1.1 * 0.01, rel=1e-15)
  assert float(gp.lengthscales_median(1e4 * X)[0]) == pytest.approx(0.9 * 100.0, rel=1e-15)


def test_initialize_returns_the_data_when_there_are_few():
  X, Y, _ = _data(10)
  for num in (10, 25):
    model = gp.SVGP.initialize((X, Y), num)
    assert all(torch.equal(iv.Z, X) for iv in model.inducing_variable.inducing_variables)
    assert model.q_mu.shape == (10, 2)


def test_initialize_is_seeded():
  X, Y, _ = _data(120)
  Z = lambda seed: gp.SVGP.initialize((X, Y), 15, seed=seed).inducing_variable.inducing_variables[0].Z
  assert torch.equal(Z(5), Z(5))
  assert not torch.equal(Z(5), Z(6))


def test_initialize_coregionalizes_when_the_latent_count_differs():
  X, Y, _ = _data(60)
  model = gp.SVGP.initialize((X, Y), 8, num_latent_gps=3, seed=2)
  assert isinstance(model.kernel, gp.LinearCoregionalization)
  assert model.kernel.W.shape == (2, 3) and model.q_mu.shape == (8, 3)
  assert torch.allclose(model.kernel.W.norm(dim=-1), torch.ones(2, dtype=F64), rtol=1e-14, atol=0)
  assert torch.isfinite(model.elbo((X, Y)))
  same = gp.SVGP.initialize((X, Y), 8, coregionalize=True, seed=2)
  assert isinstance(same.kernel, gp.LinearCoregionalization) and torch.equal(same.kernel.W, torch.eye(2, dtype=F64))


def test_initialize_replaces_overly_correlated_points():
  X, Y, _ = _data(40)
  X = torch.cat([X, X[:5] + 1e-9])                               # five near-duplicates
  Y = torch.cat([Y, Y[:5]])
  model = gp.SVGP.initialize((X, Y), 45, max_corr=0.99999, seed=3)      # (the steps reach 0.02: ~1e-2 lengthscales)
  for k, iv in zip(model.kernel.kernels, model.inducing_variable.inducing_variables):
    corr = k.K(iv.Z) / k.variance
    corr.fill_diagonal_(0.0)
    assert float(corr.max()) < 0.99999


# ---- fit_svgp ---------------------------------------------------------------------------------------------------------------
BOUNDS = (0.05, 20.0)


@functools.lru_cache(maxsize=None)
def _fitted():
  """One fit on N 120, M 15, d 2, L 2 shared by the tests below: (model, before, history, train, held-out)."""
  X, Y, _ = _data(120)
  Xt, _, Ft = _data(200, seed=9)
  model = gp.SVGP.initialize((X, Y), 15, seed=1, prior=gp.PilcoPenaltySNR(1000.0, 30.0))
  before = dict(rmse=float(((model.predict_mean(Xt) - Ft) ** 2).mean().sqrt()),
                tensors=[(t, id(t), t._version, t.clone()) for t in model._parameters() + [model.likelihood.variance]],
                loss=float(model.training_loss((X, Y))))
  record = []
  history = fit_svgp(model, (X, Y), max_iter=40, lengthscale_bounds=BOUNDS, history=record)
  assert history is record
  return model, before, history, (X, Y), (Xt, Ft)


def test_fit_lowers_the_loss():
  model, before, history, data, _ = _fitted()
  assert 2 <= len(history) <= 41
  assert all(h == h and abs(h) != float("inf") for h in history)
  assert history[0] == before["loss"]
  assert history[-1] < history[0]
  assert float(model.training_loss(data)) == pytest.approx(history[-1], rel=1e-12)      # the written-back model IS the fitted one


def test_fit_improves_the_held_out_error():
  model, before, _, _, (Xt, Ft) = _fitted()
  rmse = float(((model.predict_mean(Xt) - Ft) ** 2).mean().sqrt())
  assert rmse < before["rmse"]
  assert rmse < 0.15                                               # the function has unit scale, the noise 0.05


def test_fit_keeps_the_constraints():
  model = _fitted()[0]
  for k in model.kernel.kernels:
    assert float(k.variance) > 0.0
    assert bool((k.lengthscales > BOUNDS[0]).all()) and bool((k.lengthscales < BOUNDS[1]).all())
  assert float(model.likelihood.variance) > 0.0
  assert torch.equal(model.q_sqrt, torch.tril(model.q_sqrt))


def test_fit_writes_back_in_place():
  model, before, _, _, _ = _fitted()
  now = model._parameters() + [model.likelihood.variance]
  assert len(now) == len(before["tensors"])
  for t, (t0, ident, version, value) in zip(now, before["tensors"]):
    assert t is t0 and id(t) == ident                              # the same tensor objects ...
    assert t._version > version                                    # ... updated in place: the pack cache's key moves
    assert not torch.equal(t, value)


@pytest.mark.parametrize("N,frozen", [(8, True), (10, True), (30, False)])
def test_fit_freezes_the_inducing_points_when_there_are_no_more_data(N, frozen):
  X, Y, _ = _data(N)
  model = gp.SVGP.initialize((X, Y), 10, seed=4)
  M = model.q_mu.shape[0]
  assert (M >= N) == frozen
  Z0 = [iv.Z.clone() for iv in model.inducing_variable.inducing_variables]
  history = fit_svgp(model, (X, Y), max_iter=3)
  assert history[-1] < history[0]
  same = [torch.equal(iv.Z, z) for iv, z in zip(model.inducing_variable.inducing_variables, Z0)]
  assert all(same) if frozen else not any(same)
  if frozen:                                                       # ... and asking for it trains them
    fit_svgp(model, (X, Y), max_iter=2, train_inducing=True)
    assert not any(torch.equal(iv.Z, z) for iv, z in zip(model.inducing_variable.inducing_variables, Z0))


def test_fit_of_a_kernel_regressor_freezes_the_uncertainty():
  X, Y, _ = _data(60)
  model = gp.SVGP.initialize((X, Y), 10, seed=5)
  q_sqrt, variances = model.q_sqrt.clone(), [k.variance.clone() for k in model.kernel.kernels]
  ls = [k.lengthscales.clone() for k in model.kernel.kernels]
  history = fit_svgp(gp.KernelRegressor(model), (X, Y), max_iter=5)
  assert history[-1] < history[0]
  assert torch.equal(model.q_sqrt, q_sqrt) and all(torch.equal(k.variance, v) for k, v in zip(model.kernel.kernels, variances))
  assert not any(torch.equal(k.lengthscales, l) for k, l in zip(model.kernel.kernels, ls))
  with pytest.raises(TypeError, match="SVGP"):
    fit_svgp(object(), (X, Y))
