"""Seeded random sweep over shapes and flags: HIP path (through the dispatcher and the C ABI) vs the fp64 CPU oracle.

Complements the hand-picked cases of test_gpu_parity.py: every draw combines a shape (L, M, d, B -- M and B not
multiples of anything, d on both sides of the d <= 8 / d > 8 kernel families), a dtype, the two flags of the handler
(full_output_cov, model_uncertainty), whitening, a Constant mean, an optional LinearCoregionalization mixing and an
input width.  Tolerances as in test_gpu_parity.py (max abs error / max abs value per tensor).

Beside the seeded list, fixed draws with MANY latents on wide inputs (``WIDE``: the drift shapes of the wide composed rollouts,
tests/test_gpu_compose_wide.py -- the seeded list reaches d = 17 with L <= 4 only), and one closed rollout at L = d = 12."""
import dataclasses

import numpy as np
import pytest
import torch

from gpflowpilco_amd.moment_matching import GaussianMoments, moment_matching
from gpflowpilco_amd.synthetic import generate_covariance
from oracle import mm_fused_ref as fr
from oracle import mm_oracle as mo
from tests.helpers import gp_model_from_oracle, random_svgp_params, scale_err, to_dev

pytestmark = pytest.mark.gpu


def _draws(n):
  rng = np.random.default_rng(20240607)
  out = []
  for i in range(n):
    d = int(rng.choice([1, 2, 3, 5, 7, 8, 9, 12, 17]))
    L = int(rng.integers(1, 5))
    M = int(rng.integers(3, 260))
    # many points on a line (or in a square) at these lengthscales make Kuu + 1e-6 I singular to working precision:
    # with whiten=False |C| reaches 1e12 and the two fp64 CPU routes (literal oracle, fused restatement) already differ
    # by O(1) on Sff (first version of this sweep: d = 1, M = 138 and 218) -- not a question the GPU can answer
    B = int(rng.integers(1, 9))
    c = dict(seed=1000 + i, L=L, M=M, d=d, B=B, f32=bool(rng.integers(0, 2)), full=bool(rng.integers(0, 2)),
             unc=bool(rng.integers(0, 2)), whiten=bool(rng.integers(0, 2)), mean=bool(rng.integers(0, 2)),
             mix=bool(rng.integers(0, 3) == 0), scale=float(rng.choice([0.02, 0.1, 0.3])))
    # (a non-whitened q_sqrt goes through Kuu^-1 twice: only where random points stay apart, d >= 3, and fewer of them)
    c["whiten"] = c["whiten"] or d <= 2
    cap = {1: 40, 2: 120} if c["whiten"] else {3: 100}
    c["M"] = min(M, cap.get(d, M if c["whiten"] else 180))
    # f32 models are specified for states narrower than the lengthscales (|b| < 1; beyond it the
    # exp2 branch is covered by test_large_delta_slow_path_f32 and the wide-Sigma case of test_gpu_fullsize.py at
    # their own tolerances): the d <= 2 draws use lengthscales of 0.15-0.45, so their f32 variants keep std 0.02
    if c["f32"] and d <= 2:
      c["scale"] = 0.02
    out.append(c)
  return out


DRAWS = _draws(24)


def _ids(draws):
  return [f"{i}-L{c['L']}M{c['M']}d{c['d']}B{c['B']}{'f32' if c['f32'] else 'f64'}" for i, c in enumerate(draws)]


# (L, M, d, B): 136 and 78 pairs on the d > 8 kernel families, full covariance, with model uncertainty, both dtypes
WIDE = [dict(seed=2000 + i, L=L, M=M, d=d, B=B, f32=f32, full=True, unc=True, whiten=True, mean=True, mix=False, scale=0.1)
        for i, (L, M, d, B) in enumerate([(16, 40, 25, 3), (12, 40, 17, 2)]) for f32 in (False, True)]


@pytest.mark.parametrize("c", DRAWS, ids=_ids(DRAWS))
def test_random_shape_and_flags(c, device):
  _check_draw(c, device)


@pytest.mark.parametrize("c", WIDE, ids=_ids(WIDE))
def test_many_latents_on_wide_inputs(c, device):
  _check_draw(c, device)


def _check_draw(c, device):
  dtype = torch.float32 if c["f32"] else torch.float64
  # lengthscales grow with d so that the kernel expectations stay away from underflow (tests/test_kernel_expectation.py:61-62)
  # (and short in one or two dimensions, where long lengthscales make Kuu numerically rank-deficient)
  lo = 0.15 if c["d"] <= 2 else 0.5 * max(1.0, np.sqrt(c["d"] / 4.0))
  p = random_svgp_params(seed=c["seed"], L=c["L"], M=c["M"], d=c["d"], whiten=c["whiten"], ls_bounds=(lo, 3.0 * lo),
                         mean=c["mean"], W_rows=(c["L"] + 1 if c["mix"] and c["L"] > 1 else None))
  rng = np.random.default_rng(c["seed"] + 7)
  mu = rng.uniform(0.2, 0.8, size=(c["B"], c["d"]))
  Sigma = generate_covariance(rng, c["d"], (c["B"],), c["scale"])
  f1o, Sffo, cro = mo.mm_gauss_svgp_mo(mu, Sigma, p, full_output_cov=c["full"], model_uncertainty=c["unc"])
  tol = dict(f1=2e-6, Sff=5e-5, cross=2e-6) if c["f32"] else dict(f1=1e-9, Sff=1e-6, cross=1e-9)
  # the draw must be well posed in fp64: the literal oracle and the algorithm-matched restatement agree on the CPU
  # (both in latent space: the restatement stops before the LinearCoregionalization mixing)
  p_lat = dataclasses.replace(p, W=None, mean_c=None)
  _, Slit, _ = mo.mm_gauss_svgp_mo(mu, Sigma, p_lat, full_output_cov=True, model_uncertainty=c["unc"])
  _, Sfus, _ = fr.moment_match(mu, Sigma, p_lat, *fr.precompute(p_lat), model_uncertainty=c["unc"])
  assert np.abs(Sfus - Slit).max() < 0.1 * tol["Sff"] * np.abs(Slit).max(), "ill-conditioned draw: fix the generator, not the tolerance"
  model = gp_model_from_oracle(p, device)
  x = GaussianMoments((to_dev(mu, device, dtype), to_dev(Sigma, device, dtype)), centered=True)
  m = moment_matching(x, model, full_output_cov=c["full"], model_uncertainty=c["unc"])
  cov = m.y.covariance()
  cov = cov.diag_part() if not c["full"] else cov
  errs = dict(f1=scale_err(m.y.mean(), f1o), Sff=scale_err(cov, Sffo), cross=scale_err(m.cross[0], cro))
  assert all(errs[k] < tol[k] for k in tol), (c, errs)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_closed_rollout_at_twelve_dims(dtype, device):
  """``ops.rollout_closed`` at L = d = 12 (M = 40, B = 3, H = 3) against ``mo.rollout_closed``, bars of
  tests/test_gpu_parity.py::test_euler_and_rollout: k_euler's loops over d * d = 144 entries make three trips (every other test
  of it has d * d <= 64)."""
  from gpflowpilco_amd import ops
  from gpflowpilco_amd.synthetic import make_inputs, make_svgp
  from tests.helpers import oracle_params
  L = d = 12
  H, B = 3, 3
  lo = 0.5 * np.sqrt(d / 4.0)
  syn = make_svgp(L, 40, d, seed=2100, ls_bounds=(lo, 3.0 * lo))
  mu, Sigma = make_inputs(B, d, seed=2101, scale=0.1, lo=0.3, hi=0.7)
  _, _, traj = mo.rollout_closed(mu, Sigma, oracle_params(syn), H, dt=1.0, keep=True)
  assert min(np.linalg.eigvalsh(S).min() for _, S in traj) > 1e-4 and max(np.abs(m).max() for m, _ in traj) < 2.0
  pm = syn.to_model(device).packed(dtype, True, device)
  m1, S1, tmu, tS = ops.rollout_closed(pm, to_dev(mu, device, dtype), to_dev(Sigma, device, dtype), H, dt=1.0, keep_trajectory=True)
  pm.check_status(B)
  tol = 1e-6 if dtype == torch.float64 else 2e-5
  errs = [max(scale_err(tmu[h], traj[h][0]), scale_err(tS[h], traj[h][1])) for h in range(H)]
  print(f"closed rollout L = d = 12 {dtype}: worst error per step {errs}")
  assert max(errs) < tol, errs
  assert torch.equal(m1, tmu[-1]) and torch.equal(S1, tS[-1])
