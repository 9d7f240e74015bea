"""The streamed Gram statistics on the GPU (``ops.gram_stats_se`` / ``gram_stats_se_backward``, csrc/mm_gram_stats.hip) against
float64 torch from coordinate differences on the CPU (tests/gram_stats_reference.py).

Tolerance 1e-11 of each output's absolute-term sum, tests/test_gpu_gram.py's figure: the sums of the small shapes have at most
M N <= 33 410 terms around inner sums of M + Q <= 163, (M + Q + M N) eps <= 3.7e-12.  The large case (N 40 000, several splits
and more chunks than workgroups) keeps 1e-11 for Phi, Psi and gZ, which are N-term sums (40 000 eps = 4.4e-12), and takes 1e-9 for
gls and gvar, sums of M N = 2.6e6 terms (2.9e-10)."""
import pytest
import torch

from gpflowpilco_amd import ops
from gpflowpilco_amd._lib import lib
from gpflowpilco_amd.autodiff import GramStatsSEFunction
from tests.gram_stats_reference import SHAPES, assert_close, make_case, reference

pytestmark = pytest.mark.gpu

LARGE = (2, 65, 40000, 3, 2)


def _device_stats(case, device):
  X, R, Z, ls, var, GPhi, GPsi = (None if t is None else t.to(device) for t in case)
  Phi, Psi = ops.gram_stats_se(X, R, Z, ls, var)
  gZ, gls, gvar = ops.gram_stats_se_backward(GPhi, GPsi, X, R, Z, ls, var)
  return dict(Phi=Phi, Psi=Psi, gZ=gZ, gls=gls, gvar=gvar)


def _cpu(out):
  return {k: None if v is None else v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_statistics_and_adjoint_against_torch(device, shape):
  a = _device_stats(make_case(*shape), device)
  assert_close(_cpu(a), reference(*shape), 1e-11)
  assert torch.equal(a["Phi"], a["Phi"].transpose(1, 2))                      # symmetric to the bit
  b = _device_stats(make_case(*shape), device)
  for name in a:
    assert (a[name] is None and b[name] is None) or torch.equal(a[name], b[name])      # two calls are bit-equal


def test_many_chunks_and_splits(device):
  a = _device_stats(make_case(*LARGE), device)
  assert_close(_cpu(a), reference(*LARGE), 1e-11, tols=dict(gls=1e-9, gvar=1e-9))
  assert torch.equal(a["Phi"], a["Phi"].transpose(1, 2))
  b = _device_stats(make_case(*LARGE), device)
  assert all(torch.equal(a[name], b[name]) for name in a)


def test_function_hands_the_gradients_to_autograd(device):
  shape = (2, 65, 63, 9, 3)
  X, R, Z, ls, var, GPhi, GPsi = (t.to(device) for t in make_case(*shape))
  ref = reference(*shape)
  leaves = [t.clone().requires_grad_(True) for t in (Z, ls, var)]
  Phi, Psi = GramStatsSEFunction.apply(X, R, *leaves)
  got = torch.autograd.grad((GPhi * Phi).sum() + (GPsi * Psi).sum(), leaves)
  assert_close(dict(zip(("gZ", "gls", "gvar"), (g.cpu() for g in got))), ref, 1e-11, names=("gZ", "gls", "gvar"))
  # a missing output gradient counts as zeros
  Phi, Psi = GramStatsSEFunction.apply(X, R, *leaves)
  only_psi = torch.autograd.grad((GPsi * Psi).sum(), leaves)
  want = ops.gram_stats_se_backward(torch.zeros_like(GPhi), GPsi, X, R, Z, ls, var)
  assert all(torch.equal(a, b) for a, b in zip(only_psi, want))
  for bad in ((X.clone().requires_grad_(True), R), (X, R.clone().requires_grad_(True))):
    with pytest.raises(ValueError, match="constants"):
      ops.gram_stats_se(*bad, Z, ls, var)
    with pytest.raises(ValueError, match="constants"):
      ops.gram_stats_se_backward(GPhi, GPsi, *bad, Z, ls, var)


def test_refused_shapes(device):
  f = lambda *s: torch.ones(*s, dtype=torch.float64, device=device)
  with pytest.raises(ValueError, match="MM_E_DIM"):
    ops.gram_stats_se(f(5, 33), f(5, 2), f(2, 7, 33), f(2, 33), f(2))
  with pytest.raises(ValueError, match="MM_E_DIM"):
    ops.gram_stats_se(f(5, 3), f(5, 34), f(2, 7, 3), f(2, 3), f(2))
  with pytest.raises(ValueError, match="MM_E_DIM"):
    ops.gram_stats_se_backward(f(2, 7, 7), f(2, 7, 34), f(5, 3), f(5, 34), f(2, 7, 3), f(2, 3), f(2))
  size = lib().mm_gram_stats_workspace_bytes
  assert size(2, 7, 5, 33, 2) == 0 and size(2, 7, 5, 3, 34) == 0
  assert size(8, 512, 2 ** 20, 8, 9) == size(8, 512, 2 ** 24, 8, 9) > 0
