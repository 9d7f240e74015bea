"""``mm_gram_se`` / ``mm_gram_se_backward`` (csrc/mm_gram.hip) on the GPU against the difference-form Gram and its autograd gradients in
float64 on the CPU (tests/gram_reference.py).

Forward tolerance 1e-14 var: the exponent carries (d + 2) eps relative error and a e^-a <= 1/e, which with mm_exp_f64's 1e-15 is at
most 2.4e-15 at d = 32.  Backward tolerance 1e-11 x the sum of the absolute values of each output's terms (at most 33 410 terms:
sequential bound 3.7e-12).  Shapes sit at the edges of the kernel's 16-row tile and 128-column chunk, and on each side of d = 16,
where a tile's 16 d (row, dimension) pairs reach the workgroup's 256 threads and the column slices of the adjoint's second phase end."""
import pytest
import torch

from gpflowpilco_amd import _lib, ops
from gpflowpilco_amd.autodiff import GramSEFunction, GramSESelfFunction
from tests.gram_reference import make_case, reference, reference_of

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (1, 63, 64, 8), (3, 65, 257, 9), (2, 130, 63, 17), (1, 64, 130, 32), (3, 37, 1, 3),
          (1, 15, 127, 4), (1, 16, 128, 16), (2, 17, 129, 15)]          # ... and the tile / chunk / slice edges
SELF_M = [1, 65, 130]


def _dev(device, L, M, N, d):
  return tuple(t.to(device) for t in make_case(L, M, N, d))


def _check_backward(got, ref):
  for g, want, scale in zip(got, ("gZ", "gls", "gvar"), ("sZ", "sls", "svar")):
    err = (g.cpu() - ref[want]).abs()
    assert bool((err <= 1e-11 * ref[scale]).all()), (want, float((err / ref[scale].clamp_min(1e-300)).max()))


@pytest.mark.parametrize("L,M,N,d", SHAPES)
def test_forward_and_backward(device, L, M, N, d):
  X, Z, ls, var, G, _ = _dev(device, L, M, N, d)
  ref = reference(L, M, N, d)
  K = ops.gram_se(X, Z, ls, var)
  assert K.shape == (L, M, N)
  assert bool(((K.cpu() - ref["K"]).abs() <= 1e-14 * var.cpu()[:, None, None]).all())
  got = ops.gram_se_backward(G, X, Z, ls, var)
  _check_backward(got, ref)
  # deterministic: a second call is bit-equal
  assert torch.equal(K, ops.gram_se(X, Z, ls, var))
  assert all(torch.equal(a, b) for a, b in zip(got, ops.gram_se_backward(G, X, Z, ls, var)))


@pytest.mark.parametrize("M", SELF_M)
def test_self_mode(device, M):
  L, d = 2, 5
  _, Z, ls, var, _, Gs = _dev(device, L, M, M, d)
  ref = reference(L, M, M, d, True)
  K = ops.gram_se_self(Z, ls, var)
  assert torch.equal(torch.diagonal(K, dim1=1, dim2=2), var[:, None].expand(L, M))        # exactly var
  assert torch.equal(K, K.transpose(1, 2))                                                # symmetric to the bit
  assert bool(((K.cpu() - ref["K"]).abs() <= 1e-14 * var.cpu()[:, None, None]).all())
  assert not torch.equal(Gs, Gs.transpose(1, 2)) or M == 1
  got = ops.gram_se_backward(Gs, None, Z, ls, var)
  _check_backward(got, ref)
  assert all(torch.equal(a, b) for a, b in zip(got, ops.gram_se_backward(Gs, None, Z, ls, var)))


def test_autograd_functions(device):
  """The two ``autograd.Function``s hand the kernel's gradients to autograd, and X takes none."""
  L, M, N, d = 3, 65, 257, 9
  X, Z, ls, var, G, Gs = _dev(device, L, M, N, d)
  Zr, lr, vr = (t.clone().requires_grad_(True) for t in (Z, ls, var))
  (G * GramSEFunction.apply(X, Zr, lr, vr)).sum().backward()
  _check_backward((Zr.grad, lr.grad, vr.grad), reference(L, M, N, d))
  Zr, lr, vr = (t.clone().requires_grad_(True) for t in (Z, ls, var))
  (Gs * GramSESelfFunction.apply(Zr, lr, vr)).sum().backward()
  _check_backward((Zr.grad, lr.grad, vr.grad), reference_of(None, Z.cpu(), ls.cpu(), var.cpu(), Gs.cpu()))
  with pytest.raises(ValueError, match="constants"):
    ops.gram_se(X.clone().requires_grad_(True), Z, ls, var)


def test_dimension_limit(device):
  """d = 33 is MM_E_DIM through the binding, before any launch; the size query answers 0."""
  L, M, N, d = 1, 4, 5, 33
  X, Z = torch.zeros(N, d, dtype=torch.float64, device=device), torch.zeros(L, M, d, dtype=torch.float64, device=device)
  ls, var = torch.ones(L, d, dtype=torch.float64, device=device), torch.ones(L, dtype=torch.float64, device=device)
  with pytest.raises(ValueError, match="MM_E_DIM"):
    ops.gram_se(X, Z, ls, var)
  with pytest.raises(ValueError, match="MM_E_DIM"):
    ops.gram_se_backward(torch.zeros(L, M, N, dtype=torch.float64, device=device), X, Z, ls, var)
  assert _lib.lib().mm_gram_workspace_bytes(L, M, N, d) == 0
