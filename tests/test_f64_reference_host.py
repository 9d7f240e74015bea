"""The reference the f64 pack is pinned to (tests/test_gpu_f64_reference.py) earns the name here, on the CPU and without any
kernel: tests.helpers.materialised_reference -- autodiff.moment_match_torch, the materialised [P, M, M] evaluation, and its
float64 autograd, fed with the model's own precompute() operands -- against the numpy oracle (values, and central differences
for the gradient), and its own conditioning floor on every draw of the GPU table."""
import numpy as np
import pytest
import torch

from gpflowpilco_amd.synthetic import make_inputs, make_svgp
from oracle import mm_oracle as mo
from tests.helpers import REFERENCE_DRAWS, materialised_reference, oracle_params, reference_draw, scale_err


def _cotangents(B, L, d, seed):
  g = torch.Generator(device="cpu").manual_seed(seed)
  return tuple(torch.randn(s, generator=g, dtype=torch.float64) for s in ((B, L), (B, L, L), (B, d, L)))


@pytest.mark.parametrize("shape", [(2, 40, 3, (0.7, 3.0)), (3, 100, 4, (0.7, 3.0)), (2, 70, 31, (2.5, 5.0))],
                         ids=["L2M40d3", "L3M100d4", "L2M70d31"])
def test_reference_values_equal_the_oracle(shape):
  """1e-8 of each output's scale: the oracle re-derives beta and C through its own Cholesky of Kuu, the reference takes them
  from precompute(); what separates them is that conditioning noise (3e-10 at worst on these draws)."""
  L, M, d, ls_bounds = shape
  B = 2
  syn = make_svgp(L, M, d, seed=60 + L + d, ls_bounds=ls_bounds, mean_c=True)
  mu, S = make_inputs(B, d, seed=9, scale=0.2, lo=0.3, hi=0.7)
  g = _cotangents(B, L, d, 2)
  (f1, Sff, cross, _, _), _ = materialised_reference(syn.to_model("cpu"), mu, S, True, True, *g, floor_trials=0)
  want = mo.mm_gauss_svgp_mo(mu, S, oracle_params(syn), True, True, 0.0)
  errs = [scale_err(a_, b_) for a_, b_ in zip((f1, Sff, cross), want)]
  print("reference vs oracle (f1, Sff, cross):", errs)
  assert max(errs) <= 1e-8, errs
  # without the model's uncertainty and with a diagonal output covariance: C = None, P = L
  (f1, Sd, cross, _, _), _ = materialised_reference(syn.to_model("cpu"), mu, S, False, False, g[0], g[0], g[2], floor_trials=0)
  want = mo.mm_gauss_svgp_mo(mu, S, oracle_params(syn), False, False, 0.0)
  errs = [scale_err(a_, b_) for a_, b_ in zip((f1, Sd, cross), want)]
  assert max(errs) <= 1e-8, errs


def test_reference_gradient_matches_central_differences_of_the_oracle():
  """The step and the bar of tests/test_gpu_backward.py::test_gradients_match_finite_differences, which differences the HIP
  path: here the reference's autograd is what is differenced against."""
  L, M, d, B = 3, 20, 4, 2
  syn = make_svgp(L, M, d, seed=60 + L + d, ls_bounds=(0.7, 3.0), mean_c=True)
  p = oracle_params(syn)
  mu, S = make_inputs(B, d, seed=9, scale=0.2, lo=0.3, hi=0.7)
  g = _cotangents(B, L, d, 2)
  A1, A2, A3 = (t.numpy() for t in g)

  def loss(mu_, S_):
    f1, Sff, cr = mo.mm_gauss_svgp_mo(mu_, S_, p, True, True, 0.0)
    return (A1 * f1).sum() + (A2 * Sff).sum() + (A3 * cr).sum()

  (_, _, _, gmu, gS), _ = materialised_reference(syn.to_model("cpu"), mu, S, True, True, *g, floor_trials=0)
  gmu, gS = gmu.numpy(), gS.numpy()
  eps = 1e-4   # the oracle carries ~1e-10 of cond(Kuu) noise: larger steps keep noise/eps small
  for b in range(B):
    for k in range(d):
      mp, mm = mu.copy(), mu.copy(); mp[b, k] += eps; mm[b, k] -= eps
      fd = (loss(mp, S) - loss(mm, S)) / (2 * eps)
      assert abs(fd - gmu[b, k]) < 3e-5 * max(1.0, abs(fd)), (b, k, fd, gmu[b, k])
    for i in range(d):
      for j in range(i, d):
        D = np.zeros((d, d)); D[i, j] = D[j, i] = 1.0
        Sp, Sm = S.copy(), S.copy(); Sp[b] += eps * D; Sm[b] -= eps * D
        fd = (loss(mu, Sp) - loss(mu, Sm)) / (2 * eps)
        an = gS[b, i, j] + gS[b, j, i] if i != j else gS[b, i, i]
        assert abs(fd - an) < 3e-5 * max(1.0, abs(fd)), (b, i, j, fd, an)


@pytest.mark.parametrize("name", list(REFERENCE_DRAWS))
def test_reference_floor_is_below_1e_10_on_every_gpu_draw(name):
  """A condition on the draws, not a measurement: the GPU bar is max(1e-9, 100 x floor), so with every floor <= 1e-10 no bar
  exceeds 1e-8.  A draw that misses it is replaced by another of the same branch."""
  syn, mu, S, g, full, unc = reference_draw(name)
  _, floors = materialised_reference(syn.to_model("cpu"), mu, S, full, unc, *g, floor_trials=4)
  print(name, "floors (f1, Sff, cross, g_mu, g_Sigma):", floors)
  assert max(floors) <= 1e-10, floors
