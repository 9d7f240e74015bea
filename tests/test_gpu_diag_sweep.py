"""Edges of the diagonal pairs' f64 sweep (mm_f64.hip, ``mmq_f64_body``): the per-batch-element operands go through a
two-slot LDS ring, one batch element per barrier, and the partial sums of up to 16 batch elements are flushed together.
Every case runs against the oracle at the tolerances of the parity tests:
  * M below 64 and not a multiple of 64 (padded tile rows and columns);
  * B = 1, B odd, B not a multiple of 16, and B large enough for more than one batch chunk per tile (the ring restarts
    per chunk, the last flush of a chunk is partial);
  * d not a multiple of 4 (ring rows past d hold the gamma row against a zero A operand) and d > 8 (KS4 = 3);
  * with and without model uncertainty (the fused D = C + beta beta^T sum or the weights alone);
  * the f32 model (LOWP tiers) and the f64 model, whose small cases run diagonal and off-diagonal pairs in one launch
    (``k_qred_f64_both``) and whose larger ones take two launches;
  * the MM_FORCE_WORST_TIER bit (every wave tile through the range-reduced e^x) and wide input covariances (wave tiles
    spread over the Taylor tiers)."""
import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib, ops
from gpflowpilco_amd.synthetic import make_inputs, make_svgp
from oracle import mm_oracle as mo
from tests.helpers import oracle_params, to_dev

pytestmark = pytest.mark.gpu

# (L, M, d, B, input std)
SHAPES = [
  (2, 40, 8, 1, 0.1),        # M < 64, B = 1
  (3, 130, 8, 37, 0.1),      # M % 64 != 0, two batch chunks of 19 and 18
  (2, 96, 5, 17, 0.3),       # d % 4 != 0, B % 16 == 1
  (1, 70, 3, 33, 0.5),       # one latent (no off-diagonal pairs), KS4 = 1, two chunks
  (2, 64, 12, 5, 0.2),       # KS4 = 3
]
IDS = ["M40B1", "M130B37", "d5B17", "L1d3B33", "d12B5"]


def _run(shape, dtype, unc, device, extra_flags=0, ls_bounds=(0.3, 3.0), seed=41):
  L, M, d, B, scale = shape
  syn = make_svgp(L, M, d, seed=seed + 7 * L + d, device=str(device), ls_bounds=ls_bounds)
  model = syn.to_model(device)
  mu, S = make_inputs(B, d, seed=seed, scale=scale, lo=0.2, hi=0.8)
  pm = model.packed(dtype, unc, device)
  f1, Sff, cross = ops.moment_match(pm, to_dev(mu, device, dtype), to_dev(S, device, dtype), True, unc,
                                    extra_flags=extra_flags)
  pm.check_status(B)
  o1, oS, oc = mo.mm_gauss_svgp_mo(mu, S, oracle_params(syn), full_output_cov=True, model_uncertainty=unc)
  return (f1, Sff, cross), (o1, oS, oc)


def _check(got, want, dtype):
  tol = 1e-6 if dtype == torch.float64 else 2e-5
  for g, w in zip(got, want):
    g = g.double().cpu().numpy()
    assert np.isfinite(g).all()
    err = np.abs(g - w).max()
    assert err <= tol * max(np.abs(w).max(), 1e-30), (err, np.abs(w).max())


@pytest.mark.parametrize("unc", [True, False], ids=["unc", "no_unc"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_diagonal_sweep_edges_against_the_oracle(shape, dtype, unc, device):
  got, want = _run(shape, dtype, unc, device)
  _check(got, want, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=[IDS[1], IDS[2]])
def test_worst_tier_bit_matches_the_oracle_and_the_tiers(shape, dtype, device):
  got, want = _run(shape, dtype, True, device, extra_flags=_lib.MM_FORCE_WORST_TIER)
  _check(got, want, dtype)
  tiers, _ = _run(shape, dtype, True, device)
  scale = float(tiers[1].abs().max())
  tol = 1e-9 if dtype == torch.float64 else 2e-6      # the Taylor tiers against the any-argument e^x (C amplifies ~1e6)
  assert float((got[1] - tiers[1]).abs().max()) <= tol * scale


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_wide_inputs_spread_over_the_tiers(dtype, device):
  # short lengthscales and a wide input covariance: the wave tiles' max |b| ranges over every tier and past the last one
  got, want = _run((3, 150, 6, 21, 1.0), dtype, True, device, ls_bounds=(0.2, 1.0), seed=5)
  _check(got, want, dtype)


def test_f64_model_in_two_launches(device):
  # L = 5, M = 600: diagonal + off-diagonal work items exceed the one-launch limit of k_qred_f64_both
  got, want = _run((5, 600, 4, 2, 0.2), torch.float64, True, device)
  _check(got, want, torch.float64)
