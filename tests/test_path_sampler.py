"""pathwise.PathSampler: the cached, capturable path sampler and its two kernels (csrc/mm_pathwise_sample.hip).

``generate_paths`` -> ``paths_from_arrays`` (torch, unchanged) is the reference throughout: the pack kernel and the basis kernel's
omega / phase are bit-equal to it from the same numbers, a draw from the same generator state gives the same paths to the
project's f64 pathwise bar (1e-9 of max |f|: the sampler maps q(u) through the cached factor and solves in [L,M,S], so v differs
by rounding, amplified by cond(Kuu) <= 4.4e7 on these shapes), the statistics of the draws match the SVGP's predictive moments, the
cache follows in-place updates of the parameters, a draw keeps no memory and captures in a HIP graph, and the closure option
``native_sampler`` computes what the closure computes on a clone of the same draw, bit for bit."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib
from gpflowpilco_amd.pathwise import PathSampler, PathwiseSVGP, generate_paths, paths_from_arrays
from gpflowpilco_amd.synthetic import make_svgp
from oracle.pin_oracle import svgp_predict_f
from tests.helpers import gp_model_from_oracle, random_svgp_params

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mm_pathwise_basis", "mm_pathwise_pack_stream")
F64_BAR = 1e-9                        # the project's f64 pathwise bar: |f - f_ref| <= 1e-9 max |f_ref|


def _code(dtype):
  return _lib.MM_F64 if dtype == F64 else _lib.MM_F32


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_the_abi_version_is_unchanged():
  header = open(os.path.join(ROOT, "include", "gpflowpilco_mm.h")).read()
  lib = _lib.lib()
  for name in NEW:
    assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert name in _lib.SIGNATURES and getattr(lib, name) is not None
  assert lib.mm_abi_version() == 2


def test_argument_validation_refuses_before_any_device_work():
  lib = _lib.lib()
  E_DIM = -2
  for code in (_lib.MM_F32, _lib.MM_F64):
    basis = lambda L=2, K=8, M=4, d=3: lib.mm_pathwise_basis(L, K, M, d, code, *([None] * 9))
    pack = lambda S=4, L=2, K=8, M=4: lib.mm_pathwise_pack_stream(S, L, K, M, code, *([None] * 4))
    assert basis(d=33) == E_DIM and basis(K=0) == E_DIM and basis(M=0) == E_DIM and basis(d=0) == E_DIM and basis(L=0) == E_DIM
    assert pack(S=0) == E_DIM and pack(K=0) == E_DIM and pack(M=0) == E_DIM and pack(L=0) == E_DIM
    assert basis() == -1 and pack() == -1                      # sizes fine, pointers NULL: MM_E_ARG, still nothing launched
  assert lib.mm_pathwise_basis(2, 8, 4, 3, 7, *([None] * 9)) == -3 and lib.mm_pathwise_pack_stream(4, 2, 8, 4, 7, *([None] * 4)) == -3


def _wb_by_formula(w, v, dtype):
  """The index formula of include/gpflowpilco_mm.h restated in numpy: w [S,L,K], v [L,M,S] -> wb [G,L,NB,4,BT]."""
  S, L, K = w.shape
  M = v.shape[1]
  BT = 128 if dtype == F64 else 256
  Kp, Mp, G = -(-K // BT) * BT, -(-M // BT) * BT, -(-S // 4)
  nbK, NB = Kp // BT, (Kp + Mp) // BT
  wb = np.full((G, L, NB, 4, BT), np.nan)
  for g in range(G):
    for sl in range(4):
      s = 4 * g + sl
      for l in range(L):
        for nb in range(NB):
          for t in range(BT):
            if nb < nbK:
              k = nb * BT + t
              wb[g, l, nb, sl, t] = w[s, l, k] if (s < S and k < K) else 0.0
            else:
              m = (nb - nbK) * BT + t
              wb[g, l, nb, sl, t] = v[l, m, s] if (s < S and m < M) else 0.0
  return wb.astype(np.float64 if dtype == F64 else np.float32)


def _dummy_paths(w, v_slm, dtype, device):
  """paths_from_arrays on (w, v) with one-dimensional placeholder operands: only ``wb`` is looked at."""
  S, L, K = w.shape
  M = v_slm.shape[-1]
  one = lambda *s: torch.ones(*s, dtype=F64, device=device)
  return paths_from_arrays(one(L, K, 1), one(L, K), w, v_slm, one(L, M, 1), one(L, 1), one(L), None, dtype=dtype, device=device)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_wb_index_formula_restates_paths_from_arrays(dtype):
  S, L, K, M = 5, 2, 300, 130
  rng = np.random.default_rng(11)
  w, v = rng.standard_normal((S, L, K)), rng.standard_normal((S, L, M))
  ref = _dummy_paths(torch.tensor(w), torch.tensor(v), dtype, "cpu").wb.numpy()
  got = _wb_by_formula(w, np.ascontiguousarray(v.transpose(1, 2, 0)), dtype)
  assert got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(got, ref)


def _cartpole(device, S=37, seed=3, grads=True):
  """The cartpole-shaped wiring of tests/test_pathwise.py: nx 4, one angle, one action, policy of 12 centres."""
  from gpflowpilco_amd import bijectors as tfb, dynamics, models as gp
  from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder
  base = make_svgp(4, 48, 6, seed=31, ls_bounds=(0.9, 3.0)).to_model(device)
  drift = PathwiseSVGP(kernel=base.kernel, inducing_variable=base.inducing_variable, q_mu=base.q_mu, q_sqrt=base.q_sqrt, whiten=True,
                       num_latent_gps=4)
  pol_o = random_svgp_params(seed=32, L=1, M=12, d=5, whiten=True, ls_bounds=(0.9, 2.0), mean=False)
  pol_o.q_mu = 0.2 * pol_o.q_mu
  pol = gp_model_from_oracle(pol_o, device)
  kern = pol.kernel.kernels[0]
  params = [pol.q_mu, pol.inducing_variable.inducing_variables[0].Z, kern.lengthscales, kern.variance]
  if grads:
    for t in params:
      t.requires_grad_(True)
  policy = gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=tfb.Chain([tfb.Scale(2.0), tfb.Shift(-0.5), tfb.NormalCDF()]))
  system = dynamics.DynamicalSystem(drift=drift, policy=policy, encoder=TrigonometricEncoder(active_dims=(1,)), solver=dynamics.Euler())
  target = torch.tensor([0.0, 1.0, 0.2, 0.0, 0.1], dtype=F64, device=device)
  objective = GaussianObjective(target=target, precis=2.0 * torch.eye(5, dtype=F64, device=device))
  g = torch.Generator(device=device).manual_seed(seed)
  x0 = 0.2 + 0.6 * torch.rand(S, 4, dtype=F64, device=device, generator=g)
  return system, objective, drift, params, x0


def test_closure_with_given_paths_ignores_the_sampler():
  """``native_sampler=True`` with ``paths`` given: no sampler is built, nothing is drawn -- the closure evaluates the paths it was
  handed (on the CPU the sampler would refuse: it has no CPU path)."""
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure

  class Sentinel(Exception):
    pass

  class Handed:                                                      # stands for a Paths: the torch composition only calls it
    def __call__(self, x):
      raise Sentinel
  system, objective, drift, _, x0 = _cartpole("cpu", grads=False)
  drift.generate_paths = None                                        # neither route of "new paths" may be taken
  closure = pathwise_policy_loss_closure(system, objective, lambda: x0, 2, dt=0.5, paths=Handed(), native=False, native_sampler=True)
  with pytest.raises(Sentinel):
    closure()


# ---- GPU: the pack kernel ---------------------------------------------------------------------------------------------------------
def _pack(S, L, K, M, dtype, w, v_lms, wb):
  rc = _lib.lib().mm_pathwise_pack_stream(S, L, K, M, _code(dtype), w.data_ptr(), v_lms.data_ptr(), wb.data_ptr(),
                                          torch.cuda.current_stream(w.device).cuda_stream)
  assert rc == 0, rc


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_gpu_pack_stream_is_bit_equal_to_paths_from_arrays_and_writes_every_element(dtype, device):
  """Partial sample groups (S 1, 5, 37), both pad edges of both block sizes (K 255, 256, 300; M 127, 128, 130, 257), one-element
  extremes; the output buffer is filled with NaN first and written twice."""
  g = torch.Generator(device=device).manual_seed(5)
  for S in (1, 5, 37):
    for L in (1, 3):
      for K in (1, 255, 256, 300):
        for M in (1, 127, 128, 130, 257):
          w = torch.randn(S, L, K, dtype=F64, device=device, generator=g)
          v = torch.randn(S, L, M, dtype=F64, device=device, generator=g)
          ref = _dummy_paths(w, v, dtype, device).wb
          v_lms = v.permute(1, 2, 0).contiguous()
          wb = torch.full_like(ref, float("nan"))
          _pack(S, L, K, M, dtype, w, v_lms, wb)
          first = wb.clone()
          _pack(S, L, K, M, dtype, w, v_lms, wb)
          case = (S, L, K, M)
          assert not torch.isnan(first).any(), case
          assert torch.equal(first, ref), case
          assert torch.equal(wb, first), case


# ---- GPU: the basis kernel --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(L, M, d, mean):
  return make_svgp(L, M, d, seed=7, mean_c=mean)


def _model(L, M, d, device, whiten=True, mean=False):
  syn = _synthetic(L, M, d, mean)
  base = syn.to_model(device)
  return PathwiseSVGP(kernel=base.kernel, inducing_variable=base.inducing_variable, q_mu=base.q_mu, q_sqrt=base.q_sqrt,
                      whiten=whiten, mean_function=base.mean_function, num_latent_gps=L)


def _stacked(model, device):
  from gpflowpilco_amd.models import _stack_kernel_params, unpack_multioutput
  kernels, Zs = unpack_multioutput(model.kernel, model.inducing_variable, model.num_latent_gps)
  return _stack_kernel_params(kernels, Zs, device)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [1, 6, 9, 16])
def test_gpu_basis_omega_and_phase_bit_equal_and_phi_within_its_rounding_bound(d, dtype, device):
  L, M, K, S = 2, 37, 300, 5
  model = _model(L, M, d, device)
  seed = lambda: torch.Generator(device=device).manual_seed(21)
  ref = generate_paths(model, S, K, dtype=dtype, device=device, generator=seed())
  g = seed()
  n = torch.randn(L, K, d, dtype=F64, device=device, generator=g)            # generate_paths's first two draws
  b = 2.0 * math.pi * torch.rand(L, K, dtype=F64, device=device, generator=g)
  Z, ls, var = (t.contiguous() for t in _stacked(model, device))
  omega = torch.full_like(ref.omega, float("nan"))
  phase = torch.full_like(ref.phase, float("nan"))
  phi = torch.full((L, M, K), float("nan"), dtype=F64, device=device)
  rc = _lib.lib().mm_pathwise_basis(L, K, M, d, _code(dtype), n.data_ptr(), b.data_ptr(), Z.data_ptr(), ls.data_ptr(),
                                    var.data_ptr(), omega.data_ptr(), phase.data_ptr(), phi.data_ptr(),
                                    torch.cuda.current_stream(device).cuda_stream)
  assert rc == 0
  assert torch.equal(omega, ref.omega) and torch.equal(phase, ref.phase)
  om = n / ls[:, None, :]
  amp = torch.sqrt(2.0 * var / K)[:, None, None]
  want = amp * torch.cos(Z @ om.transpose(1, 2) + b[:, None, :])
  mag = 1.0 + torch.einsum('lmj,lkj->lmk', Z.abs(), om.abs()) + b.abs()[:, None, :]
  bound = amp * (d + 4) * 2.2e-16 * mag
  excess = ((phi - want).abs() / bound).max()
  print(f"basis d={d}: max |dPhi| / bound = {float(excess):.3f}")
  assert torch.isfinite(phi).all() and float(excess) <= 1.0


# ---- GPU: same draws, same paths --------------------------------------------------------------------------------------------------
SHAPES = [(3, 100, 6, 256, 37), (3, 300, 6, 256, 37), (2, 130, 9, 300, 37)]          # (L, M, d, K, S)


@pytest.mark.gpu
@pytest.mark.parametrize("mean", [False, True], ids=["zero-mean", "const-mean"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "L{}M{}d{}K{}S{}".format(*s))
def test_gpu_draw_from_the_same_generator_state_gives_the_same_paths(shape, whiten, mean, device):
  L, M, d, K, S = shape
  model = _model(L, M, d, device, whiten=whiten, mean=mean)
  seed = lambda: torch.Generator(device=device).manual_seed(9)
  x = torch.rand(S, d, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(10))
  ref = generate_paths(model, S, K, dtype=F64, device=device, generator=seed())
  got = model.path_sampler(S, K, dtype=F64, device=device).draw(seed())
  for name in ("zs", "hz", "omega", "phase", "lengthscales", "prior_scale", "variance"):
    assert torch.equal(getattr(got, name), getattr(ref, name)), name
  assert (got.mean_c is None) == (ref.mean_c is None) == (not mean)
  if mean:
    assert torch.equal(got.mean_c, ref.mean_c)
  assert got.wb.shape == ref.wb.shape and got.num_samples == S
  nbK = got.omega.shape[-1] // 128
  assert torch.equal(got.wb[:, :, :nbK], ref.wb[:, :, :nbK])                      # the prior weights are the draws themselves
  f_ref, f_got = ref(x), got(x)
  err = float((f_got - f_ref).abs().max() / f_ref.abs().max())
  print(f"same draws {shape} whiten={whiten} mean={mean}: |df| / max|f| = {err:.2e}")
  assert err <= F64_BAR
  # f32: both routes cast their own f64 v once -- at most one f32 ulp of max |v| apart per element
  ref32 = generate_paths(model, S, K, dtype=F32, device=device, generator=seed())
  got32 = model.path_sampler(S, K, dtype=F32, device=device).draw(seed())
  nbK32 = got32.omega.shape[-1] // 256
  vmax = float(ref.wb[:, :, nbK:].abs().max())
  ulp = 2.0 ** (math.floor(math.log2(vmax)) - 23)
  assert torch.equal(got32.wb[:, :, :nbK32], ref32.wb[:, :, :nbK32])
  dv = float((got32.wb[:, :, nbK32:].double() - ref32.wb[:, :, nbK32:].double()).abs().max())
  print(f"  f32 stream: max |dv| = {dv:.3e}, one ulp of max |v| = {ulp:.3e}")
  assert dv <= ulp
  for name in ("zs", "hz", "omega", "phase"):
    assert torch.equal(getattr(got32, name), getattr(ref32, name)), name


# ---- GPU: statistics, freshness, staleness ----------------------------------------------------------------------------------------
def _stat_model(device):
  p = random_svgp_params(seed=4, L=2, M=20, d=2, whiten=True, ls_bounds=(0.5, 2.0))
  base = gp_model_from_oracle(p, device)
  return p, PathwiseSVGP(kernel=base.kernel, inducing_variable=base.inducing_variable, q_mu=base.q_mu, q_sqrt=base.q_sqrt,
                         whiten=True, mean_function=base.mean_function, num_latent_gps=2)


@pytest.mark.gpu
def test_gpu_sampler_statistics_and_model_surface(device):
  """The recipe and the bounds of tests/test_pathwise.py::test_generated_paths_statistics_and_model_surface, with the sampler."""
  p, model = _stat_model(device)
  S = 8192
  g = torch.Generator(device=device).manual_seed(0)
  paths = model.path_sampler(S, 2048, dtype=F64, device=device).draw(g)
  x0 = np.array([0.3, 0.6])
  mean, cov = svgp_predict_f(x0[None], p)
  with model.set_temporary_paths(paths):
    f = model(torch.tensor(np.broadcast_to(x0, (S, 2)).copy(), device=device))
  fm, fv = f.mean(0).cpu().numpy(), f.var(0).cpu().numpy()
  se = np.sqrt(np.diagonal(cov[0]) / S)
  assert np.all(np.abs(fm - mean[0]) < 6 * se + 2e-2)
  assert np.all(np.abs(fv - np.diagonal(cov[0])) < 0.1 * np.diagonal(cov[0]) + 2e-2)


@pytest.mark.gpu
def test_gpu_draws_are_fresh_follow_in_place_updates_and_keep_no_memory(device):
  import copy
  p, model = _stat_model(device)
  S = 8192
  sampler = model.path_sampler(S, 2048, dtype=F64, device=device)
  g = torch.Generator(device=device).manual_seed(1)
  x0 = np.array([0.3, 0.6])
  x = torch.tensor(np.broadcast_to(x0, (S, 2)).copy(), device=device)
  first = sampler.draw(g, clone=True)
  second = sampler.draw(g)
  assert not torch.equal(first.wb, second.wb) and not torch.equal(first.omega, second.omega)
  assert first.wb.data_ptr() != second.wb.data_ptr() and second.wb.data_ptr() == sampler.buffers["wb"].data_ptr()
  mean_old, cov = svgp_predict_f(x0[None], p)
  se = np.sqrt(np.diagonal(cov[0]) / S)
  tol = 6 * se + 2e-2                                               # the statistics test's bound on a sample mean
  assert np.all(np.abs(second(x).mean(0).cpu().numpy() - mean_old[0]) < tol)
  # an in-place update (what an optimiser or a refit does): the version-keyed cache must notice
  shift = np.array([1.5, -2.0])
  with torch.no_grad():
    model.q_mu.add_(torch.tensor(shift, device=device))
  p_new = copy.deepcopy(p)
  p_new.q_mu = p.q_mu + shift
  mean_new, _ = svgp_predict_f(x0[None], p_new)
  assert np.all(np.abs(mean_new[0] - mean_old[0]) > 4 * tol)         # the update moves the mean far outside the bound
  torch.cuda.synchronize(device)
  third = sampler.draw(g)
  assert np.all(np.abs(third(x).mean(0).cpu().numpy() - mean_new[0]) < tol)
  # steady state: a draw leaves the allocator where it found it
  torch.cuda.synchronize(device)
  before = torch.cuda.memory_allocated(device)
  paths = sampler.draw(g)
  torch.cuda.synchronize(device)
  assert torch.cuda.memory_allocated(device) == before
  assert paths.wb.data_ptr() == third.wb.data_ptr()


# ---- GPU: capture -----------------------------------------------------------------------------------------------------------------
def _paths_from_draw_buffers(model, sampler, device):
  """generate_paths's own arithmetic (torch, unchanged order) on the numbers in the sampler's draw buffers."""
  from gpflowpilco_amd.linalg import cholesky
  from gpflowpilco_amd.models import DEFAULT_JITTER
  B = sampler.buffers
  Z, ls, var = _stacked(model, device)
  L, M, d = Z.shape
  K = B["n"].shape[1]
  omega, phase, w, eps = B["n"] / ls[:, None, :], B["b"], B["w"], B["eps"]
  A = Z / ls[:, None, :]
  d2 = (A * A).sum(-1)[:, :, None] + (A * A).sum(-1)[:, None, :] - 2.0 * A @ A.transpose(1, 2)
  Luu = cholesky(var[:, None, None] * torch.exp(-0.5 * d2.clamp_min(0.0)) + DEFAULT_JITTER * torch.eye(M, dtype=F64, device=device))
  u = model.q_mu.T[None] + torch.einsum('slm,lnm->sln', eps, torch.tril(model.q_sqrt))
  if model.whiten:
    u = torch.einsum('lnm,slm->sln', Luu, u)
  Phi_Z = torch.sqrt(2.0 * var / K)[:, None, None] * torch.cos(Z @ omega.transpose(1, 2) + phase[:, None, :])
  resid = u - torch.einsum('lmk,slk->slm', Phi_Z, w)
  v = torch.cholesky_solve(resid.permute(1, 2, 0), Luu).permute(2, 0, 1)
  return paths_from_arrays(omega, phase, w, v, Z, ls, var, None, dtype=F64, device=device)


@pytest.mark.gpu
def test_gpu_draw_captures_in_a_graph_and_every_replay_draws_new_paths(device):
  L, M, d, K, S = SHAPES[0]
  model = _model(L, M, d, device)
  sampler = model.path_sampler(S, K, dtype=F64, device=device)
  x = torch.rand(S, d, dtype=F64, device=device, generator=torch.Generator(device=device).manual_seed(10))
  with pytest.raises(RuntimeError, match="draw\\(\\) once outside"):
    stale = model.path_sampler(S, K, dtype=F64, device=device)
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
      stale.draw()
  side = torch.cuda.Stream(device=device)                            # warm-up off the capturing stream, as GraphedPolicyLoss does
  side.wait_stream(torch.cuda.current_stream(device))
  with torch.cuda.stream(side):
    sampler.draw()
  torch.cuda.current_stream(device).wait_stream(side)
  torch.cuda.synchronize(device)
  own = torch.Generator(device=device).manual_seed(1)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):                                      # a draw that synchronised would fail here
    paths = sampler.draw()
    with pytest.raises(RuntimeError, match="generator=None"):
      sampler.draw(own)
  graph.replay()
  torch.cuda.synchronize(device)
  wb1 = paths.wb.clone()
  graph.replay()
  torch.cuda.synchronize(device)
  assert torch.isfinite(paths.wb).all() and not torch.equal(paths.wb, wb1)
  ref = _paths_from_draw_buffers(model, sampler, device)
  assert torch.equal(paths.omega, ref.omega) and torch.equal(paths.phase, ref.phase)
  f_ref, f_got = ref(x), paths(x)
  err = float((f_got - f_ref).abs().max() / f_ref.abs().max())
  print(f"replayed draw against its own draw buffers: |df| / max|f| = {err:.2e}")
  assert err <= F64_BAR


# ---- GPU: the closure -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_closure_with_native_sampler_equals_the_closure_on_a_clone_of_the_same_draw(device):
  import warnings
  from gpflowpilco_amd.loops import pathwise_policy_loss_closure
  S, H, K = 37, 6, 256
  system, objective, drift, params, x0 = _cartpole(device, S=S)
  seed = lambda: torch.Generator(device=device).manual_seed(17)

  def run(closure):
    for t in params:
      t.grad = None
    loss = closure()
    loss.mean().backward()
    return loss.detach().clone(), [t.grad.detach().clone() for t in params]
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)                   # the native route, no fallback
    la, ga = run(pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.5, num_bases=K, generator=seed(),
                                              native_sampler=True))
    given = PathSampler(drift, S, K, dtype=F64, device=device).draw(seed(), clone=True)
    lb, gb = run(pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.5, paths=given, native_sampler=True))
  assert la.shape == (S,) and torch.isfinite(la).all() and torch.equal(la, lb)
  for a_, b_ in zip(ga, gb):
    assert float(a_.abs().max()) > 0.0 and torch.equal(a_, b_)
  # the torch composition draws from the sampler too
  lt, _ = run(pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.5, num_bases=K, generator=seed(), native=False,
                                           native_sampler=True))
  assert float((lt - la).abs().max()) < 1e-10
  # off (the default): generate_paths from the caller's generator, as before
  lo, go = run(pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.5, num_bases=K, generator=seed()))
  lr, gr = run(pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.5,
                                            paths=drift.generate_paths(S, K, dtype=F64, device=device, generator=seed())))
  assert torch.equal(lo, lr) and all(torch.equal(a_, b_) for a_, b_ in zip(go, gr))
  print(f"generate_paths against the sampler, same seed: max |dloss| = {float((lo - la).abs().max()):.2e}")
  # the same paths to rounding: f within 1e-9 of max |f| per step, 6 Euler steps of dt 0.5 and a cost with O(1) slope
  assert float((lo - la).abs().max()) < 1e-7 * float(lo.abs().max())


@pytest.mark.gpu
def test_gpu_graphed_policy_loss_replays_with_new_paths_each_time(device):
  from gpflowpilco_amd.loops import GraphedPolicyLoss, pathwise_policy_loss_closure
  S, H, K = 37, 6, 256
  system, objective, drift, params, x0 = _cartpole(device, S=S)
  closure = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.5, num_bases=K, native_sampler=True)
  graphed = GraphedPolicyLoss(closure, params)
  l1, g1 = graphed.loss_and_grad()
  l1, g1 = l1.clone(), [g.clone() for g in g1]
  l2, g2 = graphed.loss_and_grad()
  torch.cuda.synchronize(device)
  graphed.check()
  assert torch.isfinite(l1).all() and torch.isfinite(l2).all() and not torch.equal(l1, l2)
  assert all(torch.isfinite(g).all() for g in g1 + list(g2)) and not torch.equal(g1[0], g2[0])
  with torch.no_grad():                                              # an optimiser's in-place step is followed
    params[0].add_(0.5)
  l3, _ = graphed.loss_and_grad()
  torch.cuda.synchronize(device)
  assert torch.isfinite(l3).all() and abs(float(l3.mean()) - float(l1.mean())) > 0.0
