"""The schedule of csrc/mm_gram_stats.h (streamed Gram statistics Phi = K K^T, Psi = K R and their adjoint) on the CPU build of
tests/hostcheck, against float64 torch from coordinate differences (tests/gram_stats_reference.py), and the refusals of the
library's entries, which need no GPU.

Tolerance: 1e-12 of each output's absolute-term sum, as tests/test_gram_host.py and tests/test_predict_host.py.  Every shape has
M N <= 33 410 terms in its longest sums (gls, gvar), whose inner sums add at most M + Q <= 163 terms: rounding of order 1e-14 of the
absolute-term sum at the most."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from gpflowpilco_amd import _lib
from tests.gram_stats_reference import SHAPES, assert_close, make_case, reference, reference_of

HOSTCHECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
HOSTLIB = os.path.join(HOSTCHECK, "libmm_gram_stats_host.so")
CSRC = os.path.join(HOSTCHECK, os.pardir, os.pardir, "gpflowpilco_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _host():
  """tests/hostcheck/libmm_gram_stats_host.so, built by ``__graft_entry__.build()``; rebuilt here when it is missing or older than
  its sources, as tests/test_gram_host.py does for its library."""
  deps = [os.path.join(HOSTCHECK, "mm_gram_stats_host.hip"), os.path.join(CSRC, "mm_gram_stats.h"), os.path.join(CSRC, "mm_gram.h")]
  if not os.path.exists(HOSTLIB) or os.path.getmtime(HOSTLIB) < max(os.path.getmtime(p) for p in deps):
    subprocess.run(["bash", os.path.join(HOSTCHECK, "build_gram_stats.sh")], check=True)
  lib = ctypes.CDLL(HOSTLIB)
  P, I = ctypes.c_void_p, ctypes.c_int
  lib.hc_stats_splits.argtypes, lib.hc_stats_splits.restype = [I] * 3, I
  lib.hc_stats_schedule.argtypes, lib.hc_stats_schedule.restype = [I] * 3 + [P], None
  lib.hc_stats_fwd.argtypes, lib.hc_stats_fwd.restype = [I] * 5 + [P] * 7, None
  lib.hc_stats_bwd.argtypes, lib.hc_stats_bwd.restype = [I] * 5 + [P] * 10, None
  return lib


def _ptr(a):
  return None if a is None else a.ctypes.data


def host_stats(L, M, N, d, Q, case):
  X, R, Z, ls, var, GPhi, GPsi = (None if t is None else np.ascontiguousarray(t.numpy()) for t in case)
  Phi, Psi = np.full((L, M, M), np.nan), (np.full((L, M, Q), np.nan) if Q else None)
  gZ, gls, gvar = np.full((L, M, d), np.nan), np.full((L, d), np.nan), np.full(L, np.nan)
  _host().hc_stats_fwd(L, M, N, d, Q, _ptr(X), _ptr(R), _ptr(Z), _ptr(ls), _ptr(var), _ptr(Phi), _ptr(Psi))
  _host().hc_stats_bwd(L, M, N, d, Q, _ptr(GPhi), _ptr(GPsi), _ptr(X), _ptr(R), _ptr(Z), _ptr(ls), _ptr(var), _ptr(gZ), _ptr(gls),
                       _ptr(gvar))
  out = dict(Phi=Phi, Psi=Psi, gZ=gZ, gls=gls, gvar=gvar)
  return {k: None if v is None else torch.from_numpy(v) for k, v in out.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_schedule_against_torch(shape):
  got = host_stats(*shape, make_case(*shape))
  assert_close(got, reference(*shape), 1e-12)
  assert torch.equal(got["Phi"], got["Phi"].transpose(1, 2))                  # symmetric to the bit


def test_a_general_gphi_gives_the_gradient_of_the_symmetrised_one():
  shape = (2, 65, 63, 9, 3)
  X, R, Z, ls, var, GPhi, GPsi = make_case(*shape)
  assert not torch.equal(GPhi, GPhi.transpose(1, 2))
  sym = 0.5 * (GPhi + GPhi.transpose(1, 2))
  a, b = host_stats(*shape, (X, R, Z, ls, var, GPhi, GPsi)), host_stats(*shape, (X, R, Z, ls, var, sym, GPsi))
  ref = reference_of(X, R, Z, ls, var, sym, GPsi)
  for name in ("gZ", "gls", "gvar"):
    assert torch.equal(a[name], b[name])                                       # GPhi + GPhi^T is the same matrix, to the bit
  assert_close(a, ref, 1e-12, names=("gZ", "gls", "gvar"))


@pytest.mark.parametrize("L,M,N", [(1, 1, 1), (1, 16, 128), (1, 16, 40000), (1, 16, 2 ** 16 + 5), (2, 65, 257), (2, 130, 40000),
                                   (8, 512, 4000), (40, 300, 1000), (600, 10, 200)])
def test_every_block_and_point_is_visited_once(L, M, N):
  """The forward's items (latent, block pair, split) cover every point once per pair, for split counts from 1 to the target."""
  nb = (M + 63) // 64
  pairs = nb * (nb + 1) // 2
  visits = np.zeros((L, pairs, N), dtype=np.int32)
  _host().hc_stats_schedule(L, M, N, visits.ctypes.data)
  assert (visits == 1).all()
  S = _host().hc_stats_splits(L, M, N)
  print("splits", S)
  assert 1 <= S <= max(1, -(-512 // (L * pairs))) and S <= (N + 63) // 64


def test_split_counts_cover_one_to_the_target():
  S = lambda L, M, N: _host().hc_stats_splits(L, M, N)
  assert S(8, 512, 4000) == 2 and S(40, 300, 1000) == 1 and S(1, 16, 128) == 2 and S(1, 16, 40000) == 313 and S(600, 10, 200) == 1


def test_abi_validation_without_a_gpu():
  """-1 / -2 / -4 before any HIP call (the pointers are never dereferenced), and a size query that ignores N."""
  lib = _lib.lib()
  one = ctypes.c_void_p(8)
  size = lib.mm_gram_stats_workspace_bytes
  big = size(2, 17, 5, 3, 2)
  assert big > 0

  def fwd(L, M, N, d, Q, X=one, R=one, Z=one, ls=one, var=one, Phi=one, Psi=one, ws=one, nbytes=big):
    return lib.mm_gram_stats_se(L, M, N, d, Q, X, R, Z, ls, var, Phi, Psi, ws, nbytes, None)

  def bwd(L, M, N, d, Q, GPhi=one, GPsi=one, X=one, R=one, Z=one, ls=one, var=one, gZ=one, gls=one, gvar=one, ws=one, nbytes=big):
    return lib.mm_gram_stats_se_backward(L, M, N, d, Q, GPhi, GPsi, X, R, Z, ls, var, gZ, gls, gvar, ws, nbytes, None)

  for name in ("X", "Z", "ls", "var", "Phi", "ws"):
    assert fwd(2, 17, 5, 3, 2, **{name: None}) == -1
  for name in ("GPhi", "X", "Z", "ls", "var", "gZ", "gls", "gvar", "ws"):
    assert bwd(2, 17, 5, 3, 2, **{name: None}) == -1
  # Psi / R and GPsi / R are NULL together, with Q = 0
  assert fwd(2, 17, 5, 3, 2, R=None) == -1 and fwd(2, 17, 5, 3, 2, Psi=None) == -1 and fwd(2, 17, 5, 3, 0) == -1
  assert fwd(2, 17, 5, 3, 0, R=None) == -1 and fwd(2, 17, 5, 3, 0, Psi=None) == -1
  assert bwd(2, 17, 5, 3, 2, R=None) == -1 and bwd(2, 17, 5, 3, 2, GPsi=None) == -1 and bwd(2, 17, 5, 3, 0, GPsi=None) == -1
  for shape in ((2, 17, 5, 33, 2), (2, 17, 5, 3, 34), (2, 17, 5, 3, -1), (0, 17, 5, 3, 2), (2, 0, 5, 3, 2), (2, 17, 0, 3, 2),
                (2, 17, 5, 0, 2), (2, 2 ** 15 + 1, 5, 3, 2)):
    assert fwd(*shape) == -2 and bwd(*shape) == -2 and size(*shape) == 0
  assert fwd(2, 17, 5, 3, 2, nbytes=big - 1) == -4 and bwd(2, 17, 5, 3, 2, nbytes=big - 1) == -4
  assert size(8, 512, 2 ** 20, 8, 9) == size(8, 512, 2 ** 24, 8, 9) == size(8, 512, 1, 8, 9) > 0
  assert size(1, 1, 1, 1, 0) > 0
  assert lib.mm_abi_version() == 2
