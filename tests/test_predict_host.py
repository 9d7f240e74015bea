"""The block schedule of csrc/mm_predict.h (predictive mean and variance) on the CPU build of tests/hostcheck, against the float64 torch
sums of tests/predict_reference.py.  Tolerance 1e-12 x each output's absolute-term sum, as tests/test_gram_host.py: float64
evaluations of at most 129^2 + 129 terms, whose rounding is ~1e-14 of that sum.  M sits on both sides of every edge of the 64-row
block (1, 63, 64, 65, 129) and N on both sides of the 64-point tile."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.predict_reference import design, reference

HOSTCHECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
HOSTLIB = os.path.join(HOSTCHECK, "libmm_predict_host.so")
BLOCK, TILE = 64, 64                      # MMP_B, MMP_TN of csrc/mm_predict.h
SHAPES = [(1, 1, 1, 1), (2, 63, 65, 9), (1, 64, 64, 32), (2, 65, 63, 9), (1, 129, 130, 4), (1, 5, 70, 1), (2, 65, 65, 32)]


@functools.lru_cache(maxsize=None)
def _lib():
  """tests/hostcheck/libmm_predict_host.so, built by ``__graft_entry__.build()``; rebuilt here when it is missing or older than its
  sources, as tests/test_gram_host.py does for its library."""
  csrc = os.path.join(HOSTCHECK, os.pardir, os.pardir, "gpflowpilco_amd", "csrc")
  deps = [os.path.join(HOSTCHECK, "mm_predict_host.hip"), os.path.join(csrc, "mm_predict.h"), os.path.join(csrc, "mm_gram.h")]
  if not os.path.exists(HOSTLIB) or os.path.getmtime(HOSTLIB) < max(os.path.getmtime(p) for p in deps):
    subprocess.run(["bash", os.path.join(HOSTCHECK, "build_predict.sh")], check=True)
  lib = ctypes.CDLL(HOSTLIB)
  P, I = ctypes.c_void_p, ctypes.c_int
  lib.hc_predict_se.argtypes = [I] * 4 + [P] * 9
  lib.hc_predict_se.restype = I
  lib.hc_predict_schedule.argtypes = [I, I, P, P, P]
  lib.hc_predict_schedule.restype = ctypes.c_longlong
  return lib


def _host(L, M, N, d, with_C=True, fill=np.nan):
  """mean, fvar [N, L] of the host build on ``design(L, M, N, d)``; the outputs start as ``fill``."""
  _, X, ops6 = design(L, M, N, d)
  X, Z, ls, var, beta, C, mean_c = (None if t is None else t.numpy().copy() for t in (X,) + ops6)
  mean, fvar = np.full((N, L), fill), np.full((N, L), fill)
  ptr = lambda a: None if a is None else a.ctypes.data
  rc = _lib().hc_predict_se(L, M, N, d, ptr(X), ptr(Z), ptr(ls), ptr(var), ptr(beta), ptr(C) if with_C else None, ptr(mean_c),
                            ptr(mean), ptr(fvar) if with_C else None)
  assert rc == 0
  return torch.from_numpy(mean), torch.from_numpy(fvar)


@pytest.mark.parametrize("L,M,N,d", SHAPES)
def test_host_schedule_against_torch(L, M, N, d):
  ref = reference(L, M, N, d)
  mean, fvar = _host(L, M, N, d)
  for got, want, scale in ((mean, "mean", "smean"), (fvar, "fvar", "svar")):
    err = (got - ref[want]).abs()
    assert bool((err <= 1e-12 * ref[scale]).all()), (want, float((err / ref[scale]).max()))


def test_mean_only_writes_no_variance():
  L, M, N, d = 2, 65, 63, 9
  ref = reference(L, M, N, d)
  mean, fvar = _host(L, M, N, d, with_C=False, fill=-7.0)
  assert bool(((mean - ref["mean"]).abs() <= 1e-12 * ref["smean"]).all())
  assert bool((fvar == -7.0).all())
  # ... and one of the two alone is refused
  assert _lib().hc_predict_se(1, 1, 1, 1, None, None, None, None, None, None, None, None, ctypes.c_void_p(8)) == -1


@pytest.mark.parametrize("M", [1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, 5 * BLOCK])
def test_schedule_visits_every_lower_block_once(M):
  nb = (M + BLOCK - 1) // BLOCK
  cap = nb * (nb + 1) // 2 + 4
  ib, jb, w = np.full(cap, -1, dtype=np.int32), np.full(cap, -1, dtype=np.int32), np.zeros(cap)
  n = _lib().hc_predict_schedule(M, cap, ib.ctypes.data, jb.ctypes.data, w.ctypes.data)
  assert n == nb * (nb + 1) // 2
  visits = list(zip(ib[:n].tolist(), jb[:n].tolist()))
  assert sorted(visits) == [(i, j) for i in range(nb) for j in range(i + 1)]          # each (i, j <= i) exactly once
  assert all(wt == (1.0 if i == j else 2.0) for (i, j), wt in zip(visits, w[:n]))
  # a row's diagonal block is its last visit (the row's accumulator is doubled there, then the epilogue runs)
  assert all(visits[k + 1][0] == i + 1 and visits[k + 1][1] == 0 for k, (i, j) in enumerate(visits[:-1]) if i == j)
  # weights of the visited blocks cover the full M x M matrix once
  assert sum(wt for wt in w[:n]) == nb * nb
