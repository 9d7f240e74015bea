"""``mm_predict_se`` (csrc/mm_predict.hip) and the native route of ``predict_f`` on the GPU.

The kernel against the float64 CPU sums of tests/predict_reference.py at 1e-11 x each output's absolute-term sum (the convention of
tests/test_gpu_gram.py; the worst-case sequential bound for M^2 + M <= 66 306 terms is 7.4e-12, so M <= 257 here), on designs whose
variance bound is at most 1e-6 var (asserted by the reference).  Shapes sit on both sides of the 64-row block (M = 1, 17, 63, 64, 65,
130, 257), of the 64-point tile (N = 1, 63, 129, 130, 257) and of the 512-workgroup grid cap (N = 40 000 at L = 2: 1250 work items,
so workgroups loop).  Whole models against ``oracle.pin_oracle.svgp_predict_f`` with the gap between the two CPU formulations --
the quadratic form and the oracle's triangular solves, measured here reference against reference -- added to that bound."""
import numpy as np
import pytest
import torch

from gpflowpilco_amd import models as gp, ops
from oracle import pin_oracle
from tests.helpers import gp_model_from_oracle
from tests.predict_reference import design, model_case, model_reference, reference, sums
from tests.test_predict import _gpr_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (3, 130, 257, 9), (2, 257, 63, 4), (1, 65, 130, 17), (2, 17, 129, 32), (2, 63, 65, 9), (1, 64, 64, 32),
          (2, 17, 40000, 32)]


def _dev(device, L, M, N, d):
  _, X, ops6 = design(L, M, N, d)
  return tuple(None if t is None else t.to(device) for t in (X,) + ops6)


def _close(got, want, scale, extra=0.0, tol=1e-11):
  err = (got.cpu() - want).abs()
  assert bool((err <= tol * scale + extra).all()), float(((err - extra) / scale.clamp_min(1e-300)).max())


@pytest.mark.parametrize("L,M,N,d", SHAPES)
def test_kernel_against_cpu_sums(device, L, M, N, d):
  X, Z, ls, var, beta, C, mean_c = _dev(device, L, M, N, d)
  ref = reference(L, M, N, d)
  mean, fvar = ops.predict_se(X, Z, ls, var, beta, C, mean_c)
  assert mean.shape == fvar.shape == (N, L)
  _close(mean, ref["mean"], ref["smean"])
  _close(fvar, ref["fvar"], ref["svar"])
  # deterministic: a second call is bit-equal
  mean2, fvar2 = ops.predict_se(X, Z, ls, var, beta, C, mean_c)
  assert torch.equal(mean, mean2) and torch.equal(fvar, fvar2)
  # the mean alone: no variance, the same mean to the bit; and without the constant
  mean3, none = ops.predict_se(X, Z, ls, var, beta)
  assert none is None
  _close(mean3, ref["mean"] - mean_c.cpu(), ref["smean"])
  assert torch.equal(ops.predict_se(X, Z, ls, var, beta, None, mean_c)[0], mean)


def test_binding_errors(device):
  X, Z, ls, var, beta, C, mean_c = _dev(device, 2, 17, 129, 32)
  with pytest.raises(ValueError, match="MM_E_DTYPE"):
    ops.predict_se(X.float(), Z, ls, var, beta, C)
  with pytest.raises(ValueError, match=r"X \[N,32\]"):
    ops.predict_se(X[:, :5], Z, ls, var, beta, C)
  with pytest.raises(ValueError, match=r"C \[2,17,17\]"):
    ops.predict_se(X, Z, ls, var, beta, C[:, :5])
  big = torch.zeros(1, 4, 33, dtype=torch.float64, device=device)
  with pytest.raises(ValueError, match="MM_E_DIM"):
    ops.predict_se(torch.zeros(5, 33, dtype=torch.float64, device=device), big, torch.ones(1, 33, dtype=torch.float64, device=device),
                   torch.ones(1, dtype=torch.float64, device=device), torch.zeros(1, 4, dtype=torch.float64, device=device))
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.predict_se(X.cpu(), Z, ls, var, beta, C)


@pytest.mark.parametrize("coreg", [False, True], ids=["independent", "coregionalized"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
def test_native_predict_f_against_oracle(device, whiten, coreg):
  p, X = model_case(whiten, coreg)
  ref = model_reference(p, X, gp_model_from_oracle(p, "cpu"))
  model = gp_model_from_oracle(p, device)
  Xd = torch.from_numpy(X).to(device)
  mean, cov = model.predict_f(Xd, full_output_cov=True, native=True)
  _close(mean, ref["mean"], ref["smean"], ref["gap_mean"])
  _close(cov, ref["cov"], ref["scov"], ref["gap_cov"])
  mean2, var = model.predict_f(Xd, native=True)
  assert torch.equal(mean2, mean)
  _close(var, torch.diagonal(ref["cov"], dim1=-2, dim2=-1), torch.diagonal(ref["scov"], dim1=-2, dim2=-1),
         torch.diagonal(ref["gap_cov"], dim1=-2, dim2=-1))
  # the torch route on the device computes the same thing
  tmean, tvar = model.predict_f(Xd, native=False)
  _close(tmean, ref["mean"], ref["smean"], tol=1e-10)
  _close(tvar, torch.diagonal(ref["cov"], dim1=-2, dim2=-1), torch.diagonal(ref["scov"], dim1=-2, dim2=-1), tol=1e-10)


def test_native_gpr_against_oracle(device):
  p, cpu_model, Xnew = _gpr_case()
  mean_o, cov_o = (torch.from_numpy(a).reshape(-1, 1) for a in pin_oracle.gpr_predict_f(Xnew, p))
  s = sums(torch.from_numpy(Xnew), *cpu_model.precompute("cpu"))
  assert float((1e-11 * s["svar"] / p.variance).max()) <= 1e-6
  gap_mean, gap_var = (s["mean"] - mean_o).abs(), (s["fvar"] - cov_o).abs()
  model = gp.GPR(tuple(t.to(device) for t in cpu_model.data), gp.SquaredExponential(variance=p.variance, lengthscales=torch.from_numpy(p.lengthscales)),
                 mean_function=gp.Constant(torch.tensor([p.mean_c], dtype=torch.float64)), noise_variance=p.noise_variance)
  Xd = torch.from_numpy(Xnew).to(device)
  mean, var = model.predict_f(Xd, native=True)
  assert mean.shape == var.shape == (50, 1)
  _close(mean, mean_o, s["smean"], gap_mean)
  _close(var, cov_o, s["svar"], gap_var)
  _, yvar = model.predict_y(Xd)
  assert torch.equal(yvar, var + p.noise_variance)


def test_routing_by_grad_mode(device):
  p, X = model_case(True, True)
  ref = model_reference(p, X, gp_model_from_oracle(p, "cpu"))
  model = gp_model_from_oracle(p, device)
  Xd = torch.from_numpy(X).to(device)
  native = model.predict_f(Xd, native=True)
  model.q_mu.requires_grad_(True)
  with torch.no_grad():
    got = model.predict_f(Xd)                       # native=None under no_grad: the kernel, to the bit
  assert torch.equal(got[0], native[0]) and torch.equal(got[1], native[1]) and not got[0].requires_grad
  got = model.predict_f(Xd)                         # a parameter records a gradient: the torch route
  assert got[0].requires_grad
  _close(got[0].detach(), ref["mean"], ref["smean"], tol=1e-10)
  _close(got[1].detach(), torch.diagonal(ref["cov"], dim1=-2, dim2=-1), torch.diagonal(ref["scov"], dim1=-2, dim2=-1), tol=1e-10)
  with pytest.raises(ValueError, match="gradient"):
    model.predict_f(Xd, native=True)
  # an unchanged model factors nothing on the next call: the cached precompute is the same object
  with torch.no_grad():
    pre = model._cache.pre(model, Xd.device)
    model.predict_f(Xd)
    assert model._cache.pre(model, Xd.device) is pre


def test_graph_capture_replays_to_the_same_bits(device):
  p, X = model_case(False, True)
  model = gp_model_from_oracle(p, device)
  Xd = torch.from_numpy(X).to(device)
  eager = model.predict_f(Xd, full_output_cov=True, native=True)       # (also the warm-up: precompute and workspace are cached)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    model.predict_f(Xd, full_output_cov=True, native=True)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = model.predict_f(Xd, full_output_cov=True, native=True)
  for _ in range(2):
    out[0].zero_(); out[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
