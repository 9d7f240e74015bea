"""The per-entry arithmetic of csrc/mm_gram.h (SE-ARD Gram matrix and its adjoint) on the CPU build of tests/hostcheck, against
float64 torch autograd of the difference-form Gram (tests/gram_reference.py).  Tolerance: 1e-12 of each output's absolute-term sum
(``var`` for an entry of K) -- float64 evaluations of sums of at most 11 x 7 x 32 terms, whose rounding is ~1e-14 of that sum."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.gram_reference import make_case, reference

HOSTCHECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
HOSTLIB = os.path.join(HOSTCHECK, "libmm_gram_host.so")
M, N = 7, 11


@functools.lru_cache(maxsize=None)
def _lib():
  """tests/hostcheck/libmm_gram_host.so, built by ``__graft_entry__.build()``; rebuilt here when it is missing or older than its
  sources, as tests/test_coregionalized.py does for its library."""
  deps = [os.path.join(HOSTCHECK, "mm_gram_host.hip"),
          os.path.join(HOSTCHECK, os.pardir, os.pardir, "gpflowpilco_amd", "csrc", "mm_gram.h")]
  if not os.path.exists(HOSTLIB) or os.path.getmtime(HOSTLIB) < max(os.path.getmtime(p) for p in deps):
    subprocess.run(["bash", os.path.join(HOSTCHECK, "build_gram.sh")], check=True)
  lib = ctypes.CDLL(HOSTLIB)
  P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
  lib.hc_gram_fwd.argtypes = [I, I, I, P, P, P, D, P]
  lib.hc_gram_bwd.argtypes = [I, I, I, P, P, P, P, D, P, P, P]
  lib.hc_gram_fwd.restype = lib.hc_gram_bwd.restype = None
  return lib


def _ptr(a):
  return None if a is None else a.ctypes.data


def _host(L, d, self_mode):
  """K, gZ, gls, gvar of the host build, latent by latent."""
  n = M if self_mode else N
  X, Z, ls, var, G, Gs = (t.numpy().copy() for t in make_case(L, M, n, d))
  if self_mode:
    X, G = None, Gs
  K, gZ, gls, gvar = np.empty((L, M, n)), np.empty((L, M, d)), np.empty((L, d)), np.empty(L)
  for l in range(L):
    Zl, Gl, Kl, gZl, glsl, gv = np.ascontiguousarray(Z[l]), np.ascontiguousarray(G[l]), np.empty((M, n)), np.empty((M, d)), np.empty(d), np.empty(1)
    _lib().hc_gram_fwd(M, n, d, _ptr(X), Zl.ctypes.data, ls[l].ctypes.data, float(var[l]), Kl.ctypes.data)
    _lib().hc_gram_bwd(M, n, d, Gl.ctypes.data, _ptr(X), Zl.ctypes.data, ls[l].ctypes.data, float(var[l]), gZl.ctypes.data,
                       glsl.ctypes.data, gv.ctypes.data)
    K[l], gZ[l], gls[l], gvar[l] = Kl, gZl, glsl, gv[0]
  return tuple(torch.from_numpy(a) for a in (K, gZ, gls, gvar))


@pytest.mark.parametrize("self_mode", [False, True], ids=["cross", "self"])
@pytest.mark.parametrize("d", [1, 9, 32])
def test_host_arithmetic_against_autograd(d, self_mode):
  L = 2
  ref = reference(L, M, M if self_mode else N, d, self_mode)
  var = make_case(L, M, M if self_mode else N, d)[3]
  K, gZ, gls, gvar = _host(L, d, self_mode)
  assert bool(((K - ref["K"]).abs() <= 1e-12 * var[:, None, None]).all())
  for got, want, scale in ((gZ, "gZ", "sZ"), (gls, "gls", "sls"), (gvar, "gvar", "svar")):
    err = (got - ref[want]).abs()
    assert bool((err <= 1e-12 * ref[scale]).all()), (want, float((err / ref[scale].clamp_min(1e-300)).max()))


def test_self_mode_diagonal_and_symmetry():
  L, d = 2, 9
  var = make_case(L, M, M, d)[3]
  K = _host(L, d, True)[0]
  assert torch.equal(torch.diagonal(K, dim1=1, dim2=2), var[:, None].expand(L, M))
  assert torch.equal(K, K.transpose(1, 2))
