"""The reference's acceptance test (``tests/test_moment_matching.py:57-84,199-264``) end to end on the device: ``sampled_moments`` at
10^6 seeded draws through the native ``predict_f`` against the native ``moment_matching``, float64, at the reference's
``10 / sqrt(S)`` = 1e-2 absolute -- mean, covariance and cross-covariance.  Designs and their condition: tests/test_sampled_moments.py."""
import pytest
import torch

from gpflowpilco_amd.moment_matching import GaussianMoments, moment_matching, sampled_moments
from oracle import pin_oracle
from tests.helpers import gp_model_from_oracle
from tests.test_sampled_moments import DESIGNS, _case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,whiten", DESIGNS)
def test_sampled_moments_against_native_moment_matching(device, seed, whiten):
  p, _, mu, Sigma, _ = _case(seed, whiten)
  model = gp_model_from_oracle(p, device)
  x = GaussianMoments(moments=(torch.from_numpy(mu).to(device), torch.from_numpy(Sigma).to(device)), centered=True)
  S = 10 ** 6
  tol = pin_oracle.mc_tol(S)
  assert tol == 1e-2
  calls = []
  native = model.predict_f
  model.predict_f = lambda X, **kw: (calls.append(X.shape[0]), native(X, native=True, **kw))[1]     # the native route, by name
  mc = sampled_moments(x, model, num_samples=S, generator=torch.Generator(device=device).manual_seed(7 + seed))
  assert sum(calls) == 2 * S and len(calls) == 4                      # chunks of 2^18 draws of both batch elements
  del model.predict_f
  mm = moment_matching(x, model)
  assert float((mc.y.mean() - mm.y.mean()).abs().max()) < tol
  assert float((mc.y.covariance() - mm.y.covariance()).abs().max()) < tol
  assert float((mc.cross_covariance() - mm.cross_covariance()).abs().max()) < tol
