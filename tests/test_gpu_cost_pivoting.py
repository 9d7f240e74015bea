"""``mm_expected_cost`` (csrc/mm_cost.h) on inputs whose elimination PIVOTS, against Gaussian elimination with partial pivoting in
``np.longdouble``.

tests/test_gpu_parity.py::test_expected_cost_kernel (d = 5) performs no row exchange in any of its 37 elements, so the swap
branch of the register elimination (d <= 8: a wave-shuffle row permutation of the matrix and the right-hand side, and the sign of
the determinant) and the swap loop of the LDS elimination (d > 8) never ran against a reference.  Here cov = D R D with a
near-rank-one correlation R and scales D over 1.6 decades, sorted ascending in the first half of the batch (large rows below the
pivot: swaps) and descending in the second half (almost none); d covers the register path and its edges (1 .. 8) and the LDS
path (9: its first size; 17 and above: more than 64 entries per row sweep; 32: MM_DMAX).

The comparison is per element and relative: the costs span 1e-8 .. 0.8 over the batch at d = 32, a per-tensor scale would hide
the small ones.  Bars: those of test_expected_cost_kernel, 1e-12 (f64) and 1e-5 (f32).  The conditions the inputs must satisfy
(who swaps, where; the float64 replay against the longdouble reference) are asserted on the CPU."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import to_dev

DS8 = (1, 2, 3, 5, 7, 8)            # the register elimination (mm_expected_cost_body8)
DSL = (9, 12, 17, 24, 32)           # the LDS elimination
N = 37
F64_BAR, F32_BAR = 1e-12, 1e-5


def gen(d, N=N, seed=None):
  rng = np.random.default_rng(100 + d if seed is None else seed)
  Q = rng.standard_normal((N, d, d))
  R0 = Q @ Q.transpose(0, 2, 1) / d + 0.02 * np.eye(d)
  r = np.sqrt(np.einsum('nii->ni', R0))
  R0 = R0 / r[:, :, None] / r[:, None, :]
  sg = rng.choice([-1.0, 1.0], size=(N, d))
  R = 0.1 * R0 + 0.9 * sg[:, :, None] * sg[:, None, :]
  s = np.sort(10.0 ** rng.uniform(-1.6, 0.0, size=(N, d)), axis=1)
  s[N // 2:] = s[N // 2:, ::-1]
  cov = R * s[:, :, None] * s[:, None, :]
  A = rng.standard_normal((d, d))
  W = (A @ A.T / d + np.eye(d)) * 100.0
  target = rng.uniform(size=d)
  mean = target + 0.3 / np.sqrt(100.0 * d) * rng.standard_normal((N, d))
  return mean, cov, target, W


def eliminate_system(A, R, ft=np.longdouble, mutation=None):
  """A X = R (A [n, n], R [n, nr]) by Gaussian elimination with partial pivoting on [A | R] in ``ft``: the pivot of step k is the
  first largest |entry| of column k in rows k .. n-1.  -> (X [n, nr], det(A) with its sign, rows [n] int: the row exchanged with
  row k at step k, k itself where none was).  ``mutation``: a wrong swap branch -- "no_exchange" (the branch never taken),
  "rhs_stays" (the matrix rows move, the right-hand side does not), "no_sign" (the determinant's sign is not flipped)."""
  d = A.shape[0]
  A = np.concatenate([np.asarray(A, dtype=ft), np.asarray(R, dtype=ft)], axis=1)
  nr = A.shape[1] - d
  det = ft(1.0)
  rows = np.arange(d)
  for k in range(d):
    p = k + int(np.argmax(np.abs(A[k:, k])))                          # (argmax: the first largest, as the kernel's strict >)
    if p != k and mutation != "no_exchange":
      cols = d if mutation == "rhs_stays" else d + nr
      A[[k, p], :cols] = A[[p, k], :cols]
      if mutation != "no_sign":
        det = -det
      rows[k] = p
    det = det * A[k, k]
    for i in range(k + 1, d):
      A[i, k:] = A[i, k:] - (A[i, k] / A[k, k]) * A[k, k:]
  X = np.zeros((d, nr), dtype=ft)
  for r in range(nr):
    y = np.zeros(d, dtype=ft)
    for i in range(d - 1, -1, -1):
      y[i] = (A[i, d + r] - A[i, i + 1:d] @ y[i + 1:]) / A[i, i]
    X[:, r] = y
  return X, det, rows


def eliminate(mean, cov, target, W, ft=np.longdouble, mutation=None):
  """-det(I + S W)^-1/2 exp(-1/2 err^T W y), (I + S W) y = err, by ``eliminate_system`` on [I + S W | err] in ``ft``, one element
  at a time.  -> (cost [N] in ``ft``, swapped [N, d - 1] bool: column k exchanged rows in element n).
  ``mutation``: a wrong swap branch of ``eliminate_system``, for test_a_wrong_row_exchange_misses_the_bar."""
  n_el, d = mean.shape
  Wf = np.asarray(W, dtype=ft)
  cost = np.zeros(n_el, dtype=ft)
  swapped = np.zeros((n_el, max(d - 1, 0)), dtype=bool)
  for n in range(n_el):
    err = np.asarray(mean[n], dtype=ft) - np.asarray(target, dtype=ft)
    y, det, rows = eliminate_system(np.eye(d, dtype=ft) + np.asarray(cov[n], dtype=ft) @ Wf, err[:, None], ft=ft, mutation=mutation)
    swapped[n] = (rows != np.arange(d))[:d - 1]
    with np.errstate(invalid="ignore"):
      cost[n] = -np.exp(ft(-0.5) * (err @ (Wf @ y[:, 0]))) / np.sqrt(det)
  return cost, swapped


def _f32_inputs(d):
  """What the f32 kernel receives: every input rounded to float32 (as float64 arrays of those values)."""
  return tuple(np.asarray(a, dtype=np.float32).astype(np.float64) for a in gen(d))


@functools.lru_cache(maxsize=None)
def _reference(d, f32):
  """The longdouble reference on the inputs of one dtype, computed once and shared (read only)."""
  want, swapped = eliminate(*(_f32_inputs(d) if f32 else gen(d)))
  return want, swapped


def _rel(got, want):
  """Per element: |got - want| / |want| (float64)."""
  want = np.asarray(want, dtype=np.longdouble)
  return np.asarray(np.abs(np.asarray(got, dtype=np.longdouble) - want) / np.abs(want), dtype=np.float64)


# ---- CPU: the inputs do what the GPU test relies on ----------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS8 + DSL)
def test_inputs_pivot_and_the_f64_replay_meets_the_reference(d):
  """For d >= 2: at least a quarter of the elements swap, at least half of the columns 0 .. d-2 swap somewhere in the batch, and
  at least one element swaps nowhere (on the f64 inputs and on the f32-rounded ones: the kernel of each dtype must pivot).  The
  same routine in float64 -- the arithmetic of the kernel, up to its fma and its order of operations -- agrees with the
  longdouble reference per element to a tenth of the f64 bar: the bar is 10x the floor of the best any f64 code can do."""
  assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is not wider than float64 here"
  for f32 in (False, True):
    inputs = _f32_inputs(d) if f32 else gen(d)
    want, _ = _reference(d, f32)
    got, swapped = eliminate(*inputs, ft=np.float64)
    floor = _rel(got, want).max()
    el, cols = int(swapped.any(1).sum()), int(swapped.any(0).sum())
    print(f"cost inputs d={d} {'f32-rounded' if f32 else 'f64'}: {el} of {N} elements swap, {cols} of {max(d - 1, 0)} columns; "
          f"|cost| {float(np.abs(want).min()):.1e} .. {float(np.abs(want).max()):.1e}; f64 replay vs longdouble {floor:.1e}")
    assert np.isfinite(np.asarray(want, dtype=np.float64)).all() and (want < 0).all()
    assert floor <= 0.1 * F64_BAR
    if d >= 2:
      assert 4 * el >= N and 2 * cols >= d - 1
      assert not swapped.any(1).all()
      # the swapping elements are the first half (scales ascending), as constructed
      assert swapped[:N // 2].any(1).sum() >= swapped[N // 2:].any(1).sum()
    else:
      assert swapped.size == 0


@pytest.mark.parametrize("d", [d for d in DS8 + DSL if d >= 2])
def test_a_wrong_row_exchange_misses_the_bar(d):
  """What the GPU test can and cannot catch, shown on CPU mutations of the reference (the kernel is not touched).
  * A swap done WRONG is far outside the bar on the swapping elements and nowhere else: the right-hand side left behind while the
    matrix rows move changes them by 1e-4 .. 0.1 relative, a determinant whose sign is not flipped makes every element with an odd
    number of exchanges NaN.  These are the two things the kernel's swap code does beside moving the matrix rows.
  * A swap branch that is never taken is NOT visible in the values: elimination without row exchange solves the same system, and
    on these inputs (no leading minor is tiny) it is as accurate -- <= 3e-16 in longdouble.  That the branch runs at all rests
    on the swap counts asserted in test_inputs_pivot_and_the_f64_replay_meets_the_reference, which replays the kernel's pivot
    rule on the kernel's inputs."""
  inputs = gen(d)
  want, swapped = _reference(d, False)
  sw, odd = swapped.any(1), swapped.sum(1) % 2 == 1
  assert odd.any()
  rhs, _ = eliminate(*inputs, mutation="rhs_stays")
  rel = _rel(rhs, want)
  print(f"cost mutation d={d}: rhs left behind moves the swapping elements by {rel[sw].min():.1e} .. {rel[sw].max():.1e}")
  assert (rel[~sw] == 0.0).all() and rel[sw].min() > F32_BAR
  nosign, _ = eliminate(*inputs, mutation="no_sign")
  assert np.isnan(nosign[odd].astype(np.float64)).all() and (_rel(nosign[~odd], want[~odd]) == 0.0).all()
  nox, never = eliminate(*inputs, mutation="no_exchange")
  print(f"cost mutation d={d}: no exchange at all moves the costs by {_rel(nox, want).max():.1e}")
  assert not never.any() and _rel(nox, want).max() < F64_BAR


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", DS8 + DSL)
def test_gpu_expected_cost_on_pivoting_inputs(d, dtype, device):
  from gpflowpilco_amd import ops
  f32 = dtype == torch.float32
  mean, cov, target, W = _f32_inputs(d) if f32 else gen(d)
  want, swapped = _reference(d, f32)
  got = ops.expected_cost(to_dev(mean, device, dtype), to_dev(cov, device, dtype), to_dev(target, device, dtype),
                          to_dev(W, device, dtype))
  assert got.shape == (N,) and got.dtype == dtype
  rel = _rel(got.double().cpu().numpy(), want)
  sw = swapped.any(1)
  worst_sw = float(rel[sw].max()) if sw.any() else 0.0
  print(f"expected cost d={d} {dtype}: worst per-element error {rel.max():.3e} (swapping elements {worst_sw:.3e}, "
        f"others {float(rel[~sw].max()):.3e})")
  assert (rel <= (F32_BAR if f32 else F64_BAR)).all(), (d, int(np.argmax(rel)), float(rel.max()))
