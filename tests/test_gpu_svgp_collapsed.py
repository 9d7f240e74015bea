"""``SVGP.collapsed_elbo`` on the GPU: the native route (streamed Gram statistics, csrc/mm_gram_stats.hip) against the torch route on
the same device, in the value and in the gradient of every hyper-parameter, and ``fit_svgp(collapsed=True)`` there.

Tolerance ``max(1e-9, 100 gap)`` -- values relative, gradients relative to each tensor's largest entry.  ``gap`` is the relative
difference, measured here on the CPU, between the torch route and the dense numpy statement of the bound on the same model: two
float64 formulations of one quantity set the floor, and the factor 100 covers the Gram entries' 1e-14 carried through the
conditioning of Kuu (the rule of tests/test_gpu_f64_reference.py).  Both figures are printed."""
import pytest
import torch

from gpflowpilco_amd import models as gp
from gpflowpilco_amd.training import fit_svgp
from tests.test_gpu_svgp_elbo import _model
from tests.test_svgp_collapsed import dense_collapsed

pytestmark = pytest.mark.gpu

F64 = torch.float64
HYPER = lambda p: {k: v for k, v in p.items() if k not in ("q_mu", "q_sqrt")}


def _compare_routes(device, **design):
  cpu_model, cpu_data, cpu_p = _model("cpu", **design)
  for t in cpu_p.values():
    t.requires_grad_(False)                                       # (the dense statement is numpy's)
  with torch.no_grad():
    dense = dense_collapsed(cpu_model, cpu_data, max_cond=float("inf"))
    gap = abs(float(cpu_model.collapsed_elbo(cpu_data)) - dense) / abs(dense)
  tol = max(1e-9, 100.0 * gap)
  model, data, p = _model(device, **design)
  p = HYPER(p)
  out = {}
  for native in (None, False):
    value = model.collapsed_elbo(data, native=native)
    out[native] = (float(value.detach()), torch.autograd.grad(value, list(p.values())))
  (v1, g1), (v0, g0) = out[None], out[False]
  worst = {name: float((a - b).abs().max() / b.abs().max()) for name, a, b in zip(p, g1, g0)}
  print(f"gap {gap:.3e} tol {tol:.3e} value difference {abs(v1 - v0) / abs(v0):.3e} gradient differences {worst}")
  assert abs(v1 - v0) <= tol * abs(v0), (v1, v0, tol)
  for name, w in worst.items():
    assert w <= tol, (name, w, tol)
  assert abs(v1 - dense) <= tol * abs(dense)


# the native route's two ways to the statistics, each forced on every design: the streamed kernel (M <= STATS_STREAMED_MAX_M) and
# the composition of mm_gram_se, batched GEMMs and mm_gram_se_backward (above it)
ROUTES = {"streamed": 10 ** 6, "composed": 0}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "not_whitened"])
def test_native_route_matches_torch_route(device, monkeypatch, whiten, route):
  monkeypatch.setattr(gp, "STATS_STREAMED_MAX_M", ROUTES[route])
  _compare_routes(device, whiten=whiten)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_native_route_past_the_blocked_factorisation(device, monkeypatch, route):
  monkeypatch.setattr(gp, "STATS_STREAMED_MAX_M", ROUTES[route])
  _compare_routes(device, M=300, L=1, seed=1)


def test_native_route_is_taken(device, monkeypatch):
  """``native=None`` on a GPU reaches the HIP statistics (it does not quietly form them in torch)."""
  from gpflowpilco_amd import ops
  calls = []
  for name in ("gram_stats_se", "gram_stats_se_backward"):
    monkeypatch.setattr(ops, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(getattr(ops, name), name))
  model, data, p = _model(device, N=40, M=17, d=4, L=2)
  model.collapsed_elbo(data).backward()
  assert calls.count("gram_stats_se") == 1 and calls.count("gram_stats_se_backward") == 1
  calls.clear()
  model.collapsed_elbo(data, native=False).backward()
  assert not calls
  # past the measured threshold the statistics come from the existing Gram entries and batched GEMMs
  monkeypatch.setattr(gp, "STATS_STREAMED_MAX_M", 16)
  for name in ("gram_se", "gram_se_backward"):
    monkeypatch.setattr(ops, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(getattr(ops, name), name))
  model.collapsed_elbo(data).backward()
  assert not any(c.startswith("gram_stats") for c in calls)
  assert calls.count("gram_se") == 3 and calls.count("gram_se_backward") == 2     # Kuf forward and adjoint passes, and Kuu
  matern, mdata, _ = _model(device, N=20, M=6, d=3, L=2, matern=True)
  with pytest.raises(ValueError, match="SquaredExponential only.*Matern32"):
    matern.collapsed_elbo(mdata, native=True)
  assert float(matern.collapsed_elbo(mdata)) == float(matern.collapsed_elbo(mdata, native=False))      # native=None: torch


def test_collapsed_fit_on_the_gpu(device):
  g = torch.Generator().manual_seed(11)
  X = 4.0 * torch.rand(150, 2, dtype=F64, generator=g) - 2.0
  Y = torch.stack([torch.sin(1.5 * X[:, 0]) + 0.5 * X[:, 1], torch.cos(X[:, 0]) * torch.tanh(X[:, 1])], -1)
  Y = Y + 0.05 * torch.randn(Y.shape, dtype=F64, generator=g)
  model = gp.SVGP.initialize((X, Y), 20, seed=2)
  tensors = model._parameters() + [model.likelihood.variance]
  versions = [t._version for t in tensors]
  data = (X.to(device), Y.to(device))
  history = fit_svgp(model, data, max_iter=3, collapsed=True)
  assert 2 <= len(history) <= 4 and all(h == h and abs(h) != float("inf") for h in history)
  assert history[-1] < history[0]
  assert all(t._version > v for t, v in zip(tensors, versions))
  assert -float(model.elbo(data)) == pytest.approx(history[-1], rel=1e-8)      # the model's q is the optimum (no prior here)
