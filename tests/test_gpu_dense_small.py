"""The device overloads of ``mma_spd_inverse`` and ``mma_solve_pivot`` (csrc/mm_adjoint.h) on the GPU, one matrix per workgroup, against
Gaussian elimination with partial pivoting in ``np.longdouble`` (tests/test_gpu_cost_pivoting.eliminate_system).

On the device overload resolution picks code that no CPU test runs: wave 0 holds the matrix in registers (one entry per lane for
n <= 8 under ``MMADevCtx``, four per lane for 8 < n <= 16 under ``MMAWideCtx<true>``) and broadcasts by wave shuffles; everything
else, and all of ``MMAWideCtx<false>`` above 8, is the templated code.  tests/devcheck/dense_small.hip runs each (function, context,
lane count) group in one launch at the lane counts of the launch sites (inverse: 256; solve: 64, and 256 for the idle waves) on LDS
carved as the callers carve it, and returns the whole LDS block, every lane's return value and every lane's ``ok``.

Bars (u = 2^-53, kappa = ||A||inf ||A^-1||inf from the reference): inverse / solution per case max|X - Xref| <= 8 kappa u max|Xref|;
log det absolute 2 d kappa u; det relative 2 n kappa u.  They come from float64 numpy replays of the device algorithms (Gauss-Jordan
without pivoting, multiplication by 1/p and the final symmetrisation; Gauss-Jordan with partial pivoting; Cholesky, L^-1, Y^T Y; the
templated elimination), which differ from the device only in fma contraction and the order of sums within one entry: on every
committed case each replay stays within a quarter of the bar (asserted on the CPU).

That the check can fail is shown on CPU mutations of the replays (test_mutated_replays_miss_the_checks).  Figures on the committed
cases (n <= 17), the miss as a multiple of the bar over the cases a mutation touches:
  solve, exchange branch never taken     96 of the 219 exchanging cases outside the bar, up to 5e+09 (solution) -- every permuted matrix
                                         with 1e-9 under the pivot by more than 1e+03; det is NOT affected (0.5 of its bar)
  solve, right-hand side left behind     1e+11 .. 9e+14 (solution) on every exchanging case; det unchanged
  solve, sign of det not flipped         2e+11 .. 2e+15 (det) on each of the 119 cases with an odd number of exchanges; solution unchanged
  solve, the wrong tie partner's row     not finite (a duplicated row: a zero pivot) on each of the 67 tie cases
  inverse, step d - 1 skipped            1e+03 .. 7e+14 (inverse), 522 of 525 cases above 1e+04; log det 2e+04 .. 6e+14
  inverse, no symmetrisation             NOT visible in the value bars (rounding level: 0.11 of the bar at the most); it is the
                                         bit-symmetry assertion that fails, on 80 % of the Gauss-Jordan cases with d >= 2
Which of two tied rows the device takes cannot be seen in the values either (both are valid eliminations; on integer matrices both
are exact): the tie cases pin that a tie is resolved CONSISTENTLY -- the row fetched is the row written back."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_cost_pivoting import eliminate_system, gen

DEVCHECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devcheck")
U = 2.0 ** -53
SENTINEL = np.uint64(0x7FF8DEAD0000BEEF)          # a quiet NaN with a payload: whatever reads it shows, whatever overwrites it shows
GUARD = 32                                        # doubles behind the largest case of a group
MAGIC = 0x444E53454431
INV, SOLVE = 0, 1
DEV, WIDE, GEN = 0, 1, 2
CTX_NAME = {DEV: "MMADevCtx", WIDE: "MMAWideCtx<true>", GEN: "MMAWideCtx<false>"}
FN_NAME = {INV: "mma_spd_inverse", SOLVE: "mma_solve_pivot"}

SPREADS = (1.0, 1e2, 1e4, 1e6, 1e8, 1e10)         # eigenvalue spread of S + diag(l^2), the issue's list
TIGHT_SPREADS = (3.0, 6.0, 12.0, 24.0)            # more of the well-conditioned ones: bars near 1e-14
INV_SIZES = {DEV: tuple(range(1, 17)) + (17, 20), WIDE: tuple(range(1, 17)) + (17, 20), GEN: (9, 12, 16, 17, 20, 32)}
SOLVE_SIZES = {DEV: tuple(range(1, 17)) + (17,), WIDE: tuple(range(1, 17)) + (17,), GEN: (9, 17, 24, 32)}
BAD_STEPS = {1: (0,), 5: (0, 2, 4), 8: (0, 4, 7), 9: (0, 4, 8), 12: (0, 3, 10, 11), 16: (0, 7, 8, 15), 20: (0, 10, 19)}
SINGULAR_AT = {2: (0,), 5: (2,), 12: (2, 9), 20: (12,)}     # d: first row of a 2 x 2 block of ones in the identity
NAN_SIZES = (5, 9, 12, 17)
ODD_LD_SIZES = (6, 9, 13, 17)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
class Case:
  def __init__(self, fn, kind, A, R=None, ld=None, **info):
    self.fn, self.kind, self.A, self.R, self.info = fn, kind, np.ascontiguousarray(A, dtype=np.float64), R, info
    self.n = self.A.shape[0]
    self.nr = self.n if fn == SOLVE else 0
    self.ld = ld if ld is not None else (self.n + 1 if fn == INV else 2 * self.n)
    self.numeric = kind not in ("bad", "singular", "nan")       # compared with the reference in value

  def doubles(self):
    return (2 if self.fn == INV else 1) * self.n * self.ld

  def image(self, blk):
    """The LDS block of the case: the matrix (and right-hand sides) in place, the sentinel everywhere else."""
    img = np.full(blk, SENTINEL, dtype=np.uint64).view(np.float64)
    rows = img[:self.n * self.ld].reshape(self.n, self.ld)
    rows[:, :self.n] = self.A
    if self.fn == SOLVE:
      rows[:, self.n:self.n + self.nr] = self.R
    return img


def _spd(rng, d, spread, order):
  """S + diag(l^2), S = Q diag(ev) Q^T, eigenvalues of the sum spread^1/2 .. spread^-1/2; ``order``: row and column scales over 0.4
  decades, sorted ascending ("asc") or descending ("desc"), or none.  Symmetric to the bit.
  * The eigenvalues and the scales are centred on 1 so that |log det| stays of order 1 where kappa is: the rounding of a float64
    log det is 2^-53 |log det|, which an absolute bar of 2 d kappa u cannot allow for at |log det| = 23 and kappa = 1.  At d = 1,
    where kappa is 1 whatever the entry, the entry is drawn from 0.7 .. 1.4 (|log| < 0.5).
  * Spread 1 is c I, kappa = 1 and a bar of 8 u: the sqrt - reciprocal - square chain of the templated code rounds three times
    per entry, up to 3 u (0.375 of the bar on Q Q^T, 0.30 on 0.7 Q Q^T, log det 0.54 on 4 I), so no c I but the identity itself
    keeps that replay within a quarter of the bar; the spread-1 cases are therefore I (unscaled) and diag(s^2) (scaled), and the
    near-identity matrices with a rounding-level bar are those of TIGHT_SPREADS."""
  if d == 1:
    return np.array([[rng.uniform(0.7, 1.4)]])
  if spread == 1.0:
    A = np.eye(d)
  else:
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.exp(np.log(spread) * (0.5 - np.sort(rng.uniform(size=d))))
    lam[0], lam[-1] = np.sqrt(spread), 1.0 / np.sqrt(spread)
    l2 = 0.5 * lam.min()
    A = (Q * (lam - l2)) @ Q.T + l2 * np.eye(d)
  if order is not None:
    s = np.sort(10.0 ** rng.uniform(-0.2, 0.2, size=d))
    s = s if order == "asc" else s[::-1]
    A = A * s[:, None] * s[None, :]
  return 0.5 * (A + A.T)


def _no_pivot_steps(A):
  """The pivots of elimination without row exchange in longdouble (the Schur complements: Gauss-Jordan's p, Cholesky's l_kk^2)."""
  M = np.array(A, dtype=np.longdouble)
  piv = np.zeros(len(M), dtype=np.longdouble)
  for k in range(len(M)):
    piv[k] = M[k, k]
    if piv[k] == 0:
      break
    M[k + 1:, k:] = M[k + 1:, k:] - np.outer(M[k + 1:, k] / M[k, k], M[k, k:])
  return piv


@functools.lru_cache(maxsize=None)
def inverse_cases(d):
  rng = np.random.default_rng(7000 + d)
  out = []
  for spread in SPREADS + TIGHT_SPREADS:
    orders = (None, None, "asc", "desc") if spread in SPREADS else (None, "asc", "desc")
    for order in orders:
      out.append(Case(INV, "spd", _spd(rng, d, spread, order), spread=spread, order=order))
  out.append(Case(INV, "spd", np.diag(2.0 ** rng.uniform(-0.5, 0.5, size=d)), spread=None, order="diagonal"))
  for k in BAD_STEPS.get(d, ()):
    A = _spd(rng, d, 10.0, None)
    A[k, k] -= 2.0 * float(_no_pivot_steps(A)[k])         # the pivot of step k becomes its own negative, the earlier ones stay
    out.append(Case(INV, "bad", A, step=k))
  for j0 in SINGULAR_AT.get(d, ()):
    A = np.eye(d)
    A[j0:j0 + 2, j0:j0 + 2] = 1.0
    out.append(Case(INV, "singular", A, step=j0 + 1))
  return tuple(out)


def _column_dominant(rng, n, noise):
  """No exchange under partial pivoting: every diagonal entry dominates its column, before and after elimination."""
  return np.diag(2.0 ** rng.uniform(-1.5, 1.5, size=n) * rng.choice([-1.0, 1.0], size=n)) + noise * rng.uniform(-1.0, 1.0, size=(n, n))


def _tie(rng, n, k, rows):
  """Small integers: blockdiag(2 I_k, T), so column k reaches step k untouched; there the rows ``rows`` hold +-2, row k holds 1
  and the others 0 or +-1: the pivot is the FIRST of ``rows``, and an exchange."""
  A = 2.0 * np.eye(n)
  m = n - k
  T = rng.choice([-1.0, 0.0, 1.0], size=(m, m), p=[0.15, 0.7, 0.15])
  T[np.arange(1, m), np.arange(1, m)] = 4.0
  T[:, 0] = rng.choice([-1.0, 0.0, 1.0], size=m)
  T[0, 0] = 1.0
  for t, r in enumerate(rows):
    T[r - k, 0] = 2.0 if t % 2 == 0 else -2.0
  A[k:, k:] = T
  return A


@functools.lru_cache(maxsize=None)
def solve_cases(n):
  rng = np.random.default_rng(9000 + n)
  out = []
  _, cov, _, W = gen(n, N=6, seed=300 + n)                # the cost's I + W S | W: 3 with scales ascending (exchanges), 3 descending
  for e in range(6):
    out.append(Case(SOLVE, "cost", np.eye(n) + W @ cov[e], W.copy(), order="asc" if e < 3 else "desc"))
  R = lambda: rng.standard_normal((n, n))
  out.append(Case(SOLVE, "none", _column_dominant(rng, n, 0.15 / n), R()))
  if n >= 2:
    for noise in (0.15 / n, 0.15 / n, 1e-9, 1e-9):          # permuted rows: an exchange at most steps, pivot rows all over the matrix
      out.append(Case(SOLVE, "perm", _column_dominant(rng, n, noise)[rng.permutation(n)], R(), noise=noise))
    first, last = np.arange(n), np.arange(n)
    first[[0, n - 1]] = [n - 1, 0]
    last[[n - 2, n - 1]] = [n - 1, n - 2]
    out.append(Case(SOLVE, "first", _column_dominant(rng, n, 1e-9)[first], R()))
    out.append(Case(SOLVE, "last", _column_dominant(rng, n, 1e-9)[last], R()))
  ties = []
  if n >= 3:
    ties.append((0, (1, 2)))                              # adjacent rows
  if n >= 4:
    ties.append((0, (1, n - 1)))                          # distant rows
    ties.append((1, (2, n - 1)) if n == 4 else (1, (2, 3, n - 1)))   # three rows
  if n >= 10:
    ties += [(2, (5, 9)),                                 # one lane group (p & 3 = 1), two registers
             (1, (6, 9)),                                 # two lane groups, the smaller row in the higher group
             (3, (4, 7, 8, 9))]                           # four rows over three groups
  for k, rows in ties:
    out.append(Case(SOLVE, "tie", _tie(rng, n, k, rows), rng.integers(-3, 4, size=(n, n)).astype(np.float64), step=k, rows=rows))
  if n in NAN_SIZES:
    A = _column_dominant(rng, n, 0.15 / n)
    A[:, n // 2] = np.nan
    out.append(Case(SOLVE, "nan", A, R()))
  if n in ODD_LD_SIZES:
    out.append(Case(SOLVE, "perm", _column_dominant(rng, n, 0.15 / n)[rng.permutation(n)], R(), ld=2 * n + 3, noise=0.15 / n))
  return tuple(out)


def groups():
  """(function, context, lanes, cases): one launch each."""
  out = []
  for ctx in (DEV, WIDE, GEN):
    out.append((INV, ctx, 256, tuple(c for d in INV_SIZES[ctx] for c in inverse_cases(d))))
  for lanes in (64, 256):
    for ctx in (DEV, WIDE, GEN):
      out.append((SOLVE, ctx, lanes, tuple(c for n in SOLVE_SIZES[ctx] for c in solve_cases(n))))
  return out


# ---- the reference --------------------------------------------------------------------------------------------------------------------
class Ref:
  pass


_REF = {}


def reference(case):
  """Longdouble elimination with partial pivoting on [A | R | I]: the solution (or the inverse), det, kappa_inf, the exchanged rows.
  Computed once per case and shared (read only)."""
  r = _REF.get(id(case))
  if r is None:
    n = case.n
    rhs = np.eye(n) if case.fn == INV else np.concatenate([case.R, np.eye(n)], axis=1)
    X, det, rows = eliminate_system(case.A, rhs)
    r = Ref()
    r.inv = X[:, -n:]
    r.X = X[:, :n]
    r.det, r.rows = det, rows
    r.kappa = float(np.abs(np.asarray(case.A, dtype=np.longdouble)).sum(1).max() * np.abs(r.inv).sum(1).max())
    r.scale = float(np.abs(r.X).max())
    _REF[id(case)] = r
  return r


def ratios(case, X, ret):
  """(value error, returned scalar's error), each as a multiple of its bar."""
  r = reference(case)
  n = case.n
  ex = float(np.abs(np.asarray(X, dtype=np.longdouble) - r.X).max()) / (8.0 * r.kappa * U * r.scale)
  with np.errstate(invalid="ignore"):
    if case.fn == INV:
      es = float(abs(np.longdouble(ret) - np.log(r.det))) / (2.0 * n * r.kappa * U)
    else:
      es = float(abs((np.longdouble(ret) - r.det) / r.det)) / (2.0 * n * r.kappa * U)
  return (ex if np.isfinite(ex) else np.inf), (es if np.isfinite(es) else np.inf)


# ---- float64 replays of the device algorithms --------------------------------------------------------------------------------------
def gj_spd(A, mutation=None):
  """mma_gj_spd8 / mma_gj_spd16: Gauss-Jordan without pivoting, multiplication by 1/p, the final symmetrisation.
  -> (inverse, log det, ok).  ``mutation``: "no_sym", "skip_last"."""
  d = len(A)
  a = np.array(A, dtype=np.float64)
  ok, logdet = True, 0.0
  with np.errstate(all="ignore"):
    for k in range(d - 1 if mutation == "skip_last" else d):
      p = a[k, k]
      ok = ok and bool(p > 0.0)
      ip = 1.0 / p
      rk, m = a[k].copy(), -a[:, k] * ip
      a = a + np.outer(m, rk)
      a[k], a[:, k], a[k, k] = rk * ip, m, ip
      logdet += np.log(p)
    if mutation != "no_sym":
      a = 0.5 * (a + a.T)
  return a, logdet, ok


def chol_spd(A):
  """The templated mma_spd_inverse: Cholesky of the lower triangle, Y = L^-1, A = Y^T Y.  -> (inverse, log det, ok)."""
  d = len(A)
  L = np.tril(np.array(A, dtype=np.float64))
  ok = True
  with np.errstate(all="ignore"):
    for k in range(d):
      ok = ok and bool(L[k, k] > 0.0)
      L[k, k] = np.sqrt(L[k, k])
      L[k + 1:, k] /= L[k, k]
      L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
    logdet = 2.0 * np.log(np.diag(L)).sum()
    Y = np.zeros((d, d))
    for i in range(d):
      Y[i, i] = 1.0 / L[i, i]
      Y[i, :i] = -(L[i, :i] @ Y[:i, :i]) / L[i, i]
    return Y.T @ Y, logdet, ok


def gj_solve(A, R, mutation=None):
  """The register elimination of mma_solve_pivot: Gauss-Jordan with partial pivoting (first largest), multiplication by 1/piv.
  -> (X, det, exchanged rows).  ``mutation``: "no_exchange", "rhs_stays", "no_sign", "wrong_tie" (row k receives the row of the
  LAST of the tied rows, the first tied row receives row k: the fetch and the write-back disagree on the partner)."""
  n = len(A)
  a, b = np.array(A, dtype=np.float64), np.array(R, dtype=np.float64)
  det, rows = 1.0, np.arange(n)
  with np.errstate(all="ignore"):
    for k in range(n):
      col = np.abs(a[k:, k])
      p = k + int(np.argmax(col))
      if p != k and mutation != "no_exchange":
        src = k + int(np.flatnonzero(col == col[p - k])[-1]) if mutation == "wrong_tie" else p
        ak, bk = a[k].copy(), b[k].copy()
        a[k], a[p] = a[src].copy(), ak
        if mutation != "rhs_stays":
          b[k], b[p] = b[src].copy(), bk
        if mutation != "no_sign":
          det = -det
        rows[k] = p
      piv = a[k, k]
      ip = 1.0 / piv
      det *= piv
      rk, bk, m = a[k].copy(), b[k].copy(), -a[:, k] * ip
      a, b = a + np.outer(m, rk), b + np.outer(m, bk)
      a[k], b[k] = rk * ip, bk * ip
  return b, det, rows


def fast(fn, ctx, n):
  """Whether (function, context) takes a one-wave register path at size n: MMAWideCtx<Fast> forwards to MMADevCtx's at n <= 8."""
  return n <= 8 or (ctx == WIDE and n <= 16)


@functools.lru_cache(maxsize=None)
def _replay(case, is_fast):
  if case.fn == INV:
    return gj_spd(case.A) if is_fast else chol_spd(case.A)
  if is_fast:
    return gj_solve(case.A, case.R)
  with np.errstate(all="ignore"):
    return eliminate_system(case.A, case.R, ft=np.float64)


def replay(case, ctx):
  return _replay(case, fast(case.fn, ctx, case.n))


def _all_cases():
  seen = {}
  for _, _, _, cases in groups():
    for c in cases:
      seen[id(c)] = c
  return list(seen.values())


# ---- CPU: the cases do what the GPU test relies on -------------------------------------------------------------------------------------
def test_np_longdouble_is_wider_than_float64():
  assert np.finfo(np.longdouble).eps < 2.0 ** -60


def test_inverse_cases_are_what_they_claim():
  """Symmetric to the bit; the SPD ones positive definite with a condition number that grows with the spread; each non-positive-pivot
  case has ONE negative eigenvalue (the singular ones: a zero one) and its first non-positive pivot at the step it was built for --
  0, a middle one, the last, and on both sides of 8 at d = 12 and 16."""
  for d in sorted(set(INV_SIZES[DEV]) | set(INV_SIZES[GEN])):
    cases = inverse_cases(d)
    assert all((c.A == c.A.T).all() for c in cases)
    kap = {}
    for c in cases:
      piv = _no_pivot_steps(c.A)
      ev = np.linalg.eigvalsh(c.A)
      if c.kind == "spd":
        assert (piv > 0).all() and ev.min() > 0
        kap.setdefault(c.info["spread"], []).append(reference(c).kappa)
      else:
        k = c.info["step"]
        assert (piv[:k] > 0).all() and (piv[k] == 0 if c.kind == "singular" else piv[k] < 0), (d, c.kind, k)
        assert (ev < -1e-12).sum() == (0 if c.kind == "singular" else 1) and (np.abs(ev) < 1e-12).sum() == (c.kind == "singular")
    if d > 1:
      assert max(kap[1e10]) > 1e9 and max(kap[1.0]) < 1e2
    print(f"inverse d={d}: {len(cases)} cases, kappa_inf {min(min(v) for v in kap.values()):.1e} .. {max(max(v) for v in kap.values()):.1e}; "
          f"non-positive pivot at steps {[c.info['step'] for c in cases if not c.numeric]}")
  steps12 = [c.info["step"] for c in inverse_cases(12) if not c.numeric]
  assert min(steps12) == 0 and any(0 < s < 8 for s in steps12) and any(s >= 8 for s in steps12) and 11 in steps12
  assert any(np.count_nonzero(c.A) == d for d in (1, 5) for c in inverse_cases(d) if c.info.get("order") == "diagonal")


def test_solve_cases_exchange_where_the_gpu_test_relies_on_it():
  """From the longdouble elimination: per size, which cases exchange rows at which step and where the pivot row sits (lane group
  p & 3 and register p >> 2 of the 16 x 16 layout).  A seed that stops producing them fails here."""
  for n in sorted(set(SOLVE_SIZES[DEV]) | set(SOLVE_SIZES[GEN])):
    cases = [c for c in solve_cases(n) if c.kind != "nan"]
    rows = {id(c): reference(c).rows for c in cases}
    ex = {id(c): np.flatnonzero(rows[id(c)] != np.arange(n)) for c in cases}
    by_kind = lambda kind: [c for c in cases if c.kind == kind]
    cost = by_kind("cost")
    assert len(cost) == 6 and all(np.isfinite(reference(c).kappa) for c in cases)
    steps = np.zeros(n, dtype=int)
    grp, reg = np.zeros(4, dtype=int), np.zeros(8, dtype=int)
    for c in cases:
      steps[ex[id(c)]] += 1
      for k in ex[id(c)]:
        grp[rows[id(c)][k] & 3] += 1
        reg[rows[id(c)][k] >> 2] += 1
    print(f"solve n={n}: {sum(len(ex[id(c)]) > 0 for c in cases)} of {len(cases)} cases exchange; exchanges by step {steps.tolist()}, "
          f"by lane group of the pivot row {grp.tolist()}, by register {reg[:(n + 3) // 4].tolist()}")
    assert all(len(ex[id(c)]) == 0 for c in by_kind("none"))
    if n >= 2:
      asc = sum(len(ex[id(c)]) for c in cost[:3])
      assert asc >= sum(len(ex[id(c)]) for c in cost[3:]) and (n < 3 or asc > 0)
      assert all(ex[id(c)].tolist() == [0] and rows[id(c)][0] == n - 1 for c in by_kind("first"))
      assert all(ex[id(c)].tolist() == [n - 2] for c in by_kind("last"))
      assert steps[0] > 0 and steps[n - 2] > 0 and steps[n - 1] == 0
    if n >= 4:
      assert (steps[:n - 1] > 0).all()                                   # every step that can exchange does, in some case
    if n >= 9:
      assert (grp > 0).all() and (reg[:(n + 3) // 4] > 0).all()          # a pivot row in each lane group and each register
    for c in by_kind("tie"):
      k, tied = c.info["step"], c.info["rows"]
      assert not c.A[k:, :k].any() and not c.A[:k, k:].any()             # column k reaches step k as it is written here
      col = np.abs(c.A[k:, k])
      assert (np.flatnonzero(col == col.max()) + k).tolist() == list(tied) and rows[id(c)][k] == tied[0] != k
      assert (c.A == np.round(c.A)).all() and np.abs(c.A).max() <= 4
    if n >= 10:
      tied = [c.info["rows"] for c in by_kind("tie")]
      assert any(len({r & 3 for r in t}) == 1 and len(t) > 1 for t in tied)                       # within one lane group
      assert any(len({r & 3 for r in t}) > 1 and (t[0] & 3) > min(r & 3 for r in t[1:]) for t in tied)   # across, the winner in a higher group
      assert any(len(t) >= 3 for t in tied)
    elif n >= 4:
      tied = [c.info["rows"] for c in by_kind("tie")]
      assert any(t[1] - t[0] == 1 for t in tied) and any(t[-1] - t[0] == n - 2 for t in tied)     # adjacent and distant rows
    # the register elimination's own pivot choice (float64) is the reference's on the constructed cases
    for c in cases:
      if c.kind in ("none", "perm", "first", "last", "tie"):
        assert (gj_solve(c.A, c.R)[2] == rows[id(c)]).all()
  assert [c.ld for n in ODD_LD_SIZES for c in solve_cases(n) if c.ld != 2 * n] == [2 * n + 3 for n in ODD_LD_SIZES]
  assert all(sum(c.kind == "nan" for c in solve_cases(n)) == 1 for n in NAN_SIZES)


def _group_report(fn, ctx, cases, results):
  """Per size: the worst ratio to the bar of (value, scalar) over the numeric cases, and how many of them are tight (kappa < 1e2).
  ``results(case)`` -> (X, scalar)."""
  worst, table = [0.0, 0.0], {}
  for c in cases:
    if c.numeric:
      ex, es = ratios(c, *results(c))
      t = table.setdefault(c.n, [0.0, 0.0, 0, 0])
      t[0], t[1], t[2], t[3] = max(t[0], ex), max(t[1], es), t[2] + 1, t[3] + (reference(c).kappa < 1e2)
      worst = [max(worst[0], ex), max(worst[1], es)]
  return worst, table


def test_replays_stay_within_a_quarter_of_the_bar():
  """On every case of the committed list, for every context: the float64 replay of the algorithm that context runs at that size is
  within a quarter of the bar, its ``ok`` is what the case was built for, and at least a third of each (context, size) group has
  kappa_inf < 1e2 -- bars near 1e-14, where a rounding-level mistake shows."""
  for fn, ctx, lanes, cases in groups():
    if lanes != 256:
      continue
    worst, table = _group_report(fn, ctx, cases, lambda c: replay(c, ctx)[:2])
    print(f"replay {FN_NAME[fn]} {CTX_NAME[ctx]}: {len(cases)} cases; worst ratio to the bar: "
          f"{'inverse' if fn == INV else 'solution'} {worst[0]:.3f}, {'log det' if fn == INV else 'det'} {worst[1]:.3f}")
    for n, (ex, es, count, tight) in sorted(table.items()):
      print(f"    n={n}: {count} cases, {tight} with kappa < 1e2, worst {ex:.3f} / {es:.3f}")
      assert ex <= 0.25 and es <= 0.25, (fn, ctx, n, ex, es)
      assert 3 * tight >= count, (fn, ctx, n, tight, count)
    if fn == INV:
      for c in cases:
        assert replay(c, ctx)[2] == (c.kind == "spd"), (ctx, c.n, c.kind, c.info)


def test_mutated_replays_miss_the_checks():
  """What the GPU test can and cannot catch, on CPU mutations of the replays (no kernel is touched); the figures are in the module's
  docstring.  A wrong exchange, a skipped step or a wrong tie partner is far outside the bar on the cases it touches and leaves the
  others bit for bit alone; a missing symmetrisation is at rounding level -- inside the bar -- and is caught by bit symmetry."""
  solve = [c for n in SOLVE_SIZES[DEV] for c in solve_cases(n) if c.numeric]
  exchanging = [c for c in solve if (reference(c).rows != np.arange(c.n)).any()]
  odd = [c for c in exchanging if (reference(c).rows != np.arange(c.n)).sum() % 2 == 1 and (gj_solve(c.A, c.R)[2] == reference(c).rows).all()]
  tie = [c for c in solve if c.kind == "tie"]
  assert len(exchanging) > 50 and len(odd) > 20 and len(tie) > 20

  def miss(cases, mutation):
    r = np.array([ratios(c, *gj_solve(c.A, c.R, mutation)[:2]) for c in cases])
    return r[:, 0], r[:, 1]

  ex, es = miss(exchanging, "no_exchange")
  fin = np.isfinite(ex)
  print(f"solve mutation no_exchange: {int((ex > 1).sum())} of {len(ex)} exchanging cases outside the bar, {int((~fin).sum())} of them not "
        f"finite (a zero pivot); worst finite miss {ex[fin].max():.1e} (solution), {es[np.isfinite(es)].max():.1e} (det)")
  assert ex[fin].max() > 1e4 and (ex > 1e4).sum() > 50
  hard = [c for c in exchanging if c.kind in ("first", "last") or (c.kind == "perm" and c.info["noise"] == 1e-9)]
  ex, es = miss(hard, "no_exchange")
  assert (ex > 1e3).all(), ex.min()                                       # every case with 1e-9 under the pivot
  ex, es = miss(exchanging, "rhs_stays")
  print(f"solve mutation rhs_stays: miss {ex.min():.1e} .. {ex.max():.1e} (solution), det {es.max():.3f}")
  assert (ex > 1e4).all() and (es <= 0.25).all()
  ex, es = miss(odd, "no_sign")
  print(f"solve mutation no_sign: det miss {es.min():.1e} .. {es.max():.1e} on the {len(odd)} cases with an odd number of exchanges")
  assert (es > 1e4).all() and (ex <= 0.25).all()
  ex, es = miss(tie, "wrong_tie")
  print(f"solve mutation wrong_tie: miss {ex.min():.1e} .. {ex.max():.1e} on the {len(tie)} tie cases")
  assert (ex > 1e4).all()
  for m in ("no_exchange", "rhs_stays", "no_sign", "wrong_tie"):           # nothing else moves: the mutations are what they say
    for c in solve:
      if c not in exchanging:
        assert all((x == y).all() for x, y in zip(gj_solve(c.A, c.R, m)[:2], gj_solve(c.A, c.R)[:2]))

  inv = [c for d in range(2, 17) for c in inverse_cases(d) if c.numeric and (c.A != np.eye(d)).any()]      # (I: its last step changes nothing)
  r = np.array([ratios(c, *gj_spd(c.A, "skip_last")[:2]) for c in inv])
  print(f"inverse mutation skip_last: miss {r[:, 0].min():.1e} .. {r[:, 0].max():.1e} (inverse; {int((r[:, 0] > 1e4).sum())} of {len(inv)} cases "
        f"above 1e4), {r[:, 1].min():.1e} .. {r[:, 1].max():.1e} (log det)")
  assert (r[:, 0] > 10.0).all() and (r[:, 0] > 1e4).mean() > 0.9
  nosym = [gj_spd(c.A, "no_sym") for c in inv]
  r = np.array([ratios(c, *g[:2]) for c, g in zip(inv, nosym)])
  asym = np.mean([(g[0] != g[0].T).any() for g in nosym])
  print(f"inverse mutation no_sym: worst ratio to the bar {r[:, 0].max():.3f} (inside it); {100 * asym:.0f} % of the cases not symmetric to the bit")
  assert r[:, 0].max() < 1.0 and asym > 0.5
  assert all((gj_spd(c.A)[0] == gj_spd(c.A)[0].T).all() for c in inv)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _driver():
  """tests/devcheck/dense_small, built by ``__graft_entry__.build()``; rebuilt here when it is missing or older than its sources."""
  exe = os.path.join(DEVCHECK, "dense_small")
  csrc = os.path.join(DEVCHECK, os.pardir, os.pardir, "gpflowpilco_amd", "csrc")
  deps = [os.path.join(DEVCHECK, "dense_small.hip"), os.path.join(DEVCHECK, "build.sh")]
  deps += [os.path.join(csrc, h) for h in ("mm_adjoint.h", "mm_compose.h", "mm_mono.h", "mm_common.h")]
  if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
    subprocess.run(["bash", os.path.join(DEVCHECK, "build.sh")], check=True)
  return exe


def _blk(cases):
  return max(c.doubles() for c in cases) + GUARD


def write_cases(path, grps):
  with open(path, "wb") as f:
    f.write(np.array([MAGIC, len(grps)], dtype="<i8").tobytes())
    for fn, ctx, lanes, cases in grps:
      blk = _blk(cases)
      f.write(np.array([fn, ctx, lanes, len(cases), blk], dtype="<i8").tobytes())
      f.write(np.array([[c.n, max(c.nr, 1), c.ld] for c in cases], dtype="<i8").tobytes())
      f.write(np.stack([c.image(blk) for c in cases]).astype("<f8").tobytes())


def read_results(path, grps):
  """-> per group (block [cases, blk] f64, ret [cases, lanes] f64, ok [cases, lanes] i32)."""
  raw = np.fromfile(path, dtype=np.uint8)
  out, at = [], 0
  for _, _, lanes, cases in grps:
    blk, nc = _blk(cases), len(cases)
    take = lambda count, dt: np.frombuffer(raw, dtype=dt, count=count, offset=at)
    block = take(nc * blk, "<f8").reshape(nc, blk)
    at += 8 * nc * blk
    ret = take(nc * lanes, "<f8").reshape(nc, lanes)
    at += 8 * nc * lanes
    ok = take(nc * lanes, "<i4").reshape(nc, lanes)
    at += 4 * nc * lanes
    out.append((block, ret, ok))
  assert at == raw.size, (at, raw.size)
  return out


def _bits(x):
  return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _case_output(case, block):
  rows = block[:case.n * case.ld].reshape(case.n, case.ld)
  return rows[:, :case.n] if case.fn == INV else rows[:, case.n:case.n + case.nr]


def check_group(fn, ctx, lanes, cases, block, ret, ok):
  """Every comparison of one group; -> (failures [str], worst ratios [value, scalar])."""
  bad = []
  name = f"{FN_NAME[fn]} {CTX_NAME[ctx]} {lanes} lanes"
  results = {}
  for i, c in enumerate(cases):
    tag = f"{name} case {i} (n={c.n} {c.kind} {c.info})"
    n, ld = c.n, c.ld
    # every lane, the idle waves included, returns the same bits
    if (_bits(ret[i]) != _bits(ret[i])[0]).any() or (ok[i] != ok[i][0]).any():
      bad.append(f"{tag}: lanes disagree")
    # the sentinel: padding columns, unused scratch, the guard band
    keep = np.ones(block.shape[1], dtype=bool)
    used = keep[:c.doubles()].reshape(-1, ld)
    if fn == INV:
      used[:n, :n] = False                                                # A
      if fast(fn, ctx, n):
        keep[n * ld:n * ld + 2] = False                                   # Y[0..1]: log det and ok
      else:
        used[n:, :n] = False                                              # Y: scratch
    else:
      used[:, :n + c.nr] = False                                          # left block: scratch; right block: X
    if (_bits(block[i])[keep] != SENTINEL).any():
      bad.append(f"{tag}: wrote outside its block at doubles {np.flatnonzero(_bits(block[i])[keep] != SENTINEL)[:8].tolist()} of the kept ones")
    X = _case_output(c, block[i])
    results[id(c)] = (X, ret[i, 0])
    if fn == INV:
      if (_bits(X) != _bits(X.T)).any() and c.numeric:
        bad.append(f"{tag}: inverse not symmetric to the bit")
      if bool(ok[i].all()) != (c.kind == "spd") or bool(ok[i].any()) != (c.kind == "spd"):
        bad.append(f"{tag}: ok = {ok[i][0]}")
    if c.kind == "nan" and not (np.isnan(X).all() and np.isnan(ret[i]).all()):
      bad.append(f"{tag}: a column of NaNs gave det {ret[i, 0]} and {int(np.isfinite(X).sum())} finite entries")
  worst, table = _group_report(fn, ctx, cases, lambda c: results[id(c)])
  for i, c in enumerate(cases):
    if c.numeric:
      ex, es = ratios(c, *results[id(c)])
      if not (ex <= 1.0 and es <= 1.0):
        bad.append(f"{name} case {i} (n={c.n} {c.kind} {c.info}): {ex:.3f} / {es:.3f} of the bar, kappa {reference(c).kappa:.1e}")
  print(f"device {name}: {len(cases)} cases; worst ratio to the bar: {'inverse' if fn == INV else 'solution'} {worst[0]:.3f}, "
        f"{'log det' if fn == INV else 'det'} {worst[1]:.3f}")
  for n, (ex, es, count, tight) in sorted(table.items()):
    print(f"    n={n}: {count} cases, worst {ex:.3f} / {es:.3f}")
  return bad, worst


def _same_bits(name, ga, gb, grps, res, sizes):
  """Two groups agree bit for bit (output, return value, ok) on the cases they share at ``sizes``."""
  bad = []
  ia = {id(c): i for i, c in enumerate(grps[ga][3])}
  for j, c in enumerate(grps[gb][3]):
    if c.n in sizes and id(c) in ia:
      i = ia[id(c)]
      same = ((_bits(_case_output(c, res[ga][0][i])) == _bits(_case_output(c, res[gb][0][j])))
              | (np.isnan(_case_output(c, res[ga][0][i])) & np.isnan(_case_output(c, res[gb][0][j])))).all()
      same = same and _bits(res[ga][1][i, :1]) == _bits(res[gb][1][j, :1]) and res[ga][2][i, 0] == res[gb][2][j, 0]
      if not same:
        bad.append(f"{name}: case n={c.n} {c.kind} {c.info} differs")
  return bad


@pytest.mark.gpu
def test_gpu_dense_small_solvers_against_longdouble(tmp_path, device):
  grps = groups()
  exe = _driver()
  write_cases(tmp_path / "in.bin", grps)
  outs = []
  for run in (0, 1):
    out = tmp_path / f"out{run}.bin"
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    outs.append(out.read_bytes())
  assert outs[0] == outs[1], "two runs of the driver differ"
  res = read_results(tmp_path / "out0.bin", grps)
  bad = []
  for (fn, ctx, lanes, cases), (block, ret, ok) in zip(grps, res):
    b, _ = check_group(fn, ctx, lanes, cases, block, ret, ok)
    bad += b
  at = {(fn, ctx, lanes): g for g, (fn, ctx, lanes, _) in enumerate(grps)}
  le8, gt16 = tuple(range(1, 9)), (17, 20, 24, 32)
  bad += _same_bits("inverse: MMAWideCtx<true> forwards to MMADevCtx at d <= 8", at[INV, DEV, 256], at[INV, WIDE, 256], grps, res, le8)
  bad += _same_bits("inverse: MMAWideCtx<true> is the generic code at d > 16", at[INV, GEN, 256], at[INV, WIDE, 256], grps, res, gt16)
  bad += _same_bits("inverse: MMADevCtx is the generic code at d > 8", at[INV, GEN, 256], at[INV, DEV, 256], grps, res, (9, 12, 16) + gt16)
  for lanes in (64, 256):
    bad += _same_bits("solve: MMAWideCtx<true> forwards to MMADevCtx at n <= 8", at[SOLVE, DEV, lanes], at[SOLVE, WIDE, lanes], grps, res, le8)
    bad += _same_bits("solve: MMAWideCtx<true> is the generic code at n > 16", at[SOLVE, GEN, lanes], at[SOLVE, WIDE, lanes], grps, res, gt16)
    bad += _same_bits("solve: MMADevCtx is the generic code at n > 8", at[SOLVE, GEN, lanes], at[SOLVE, DEV, lanes], grps, res, (9,) + gt16)
  for ctx in (DEV, WIDE, GEN):                                             # the idle waves change nothing
    bad += _same_bits(f"solve {CTX_NAME[ctx]}: 64 and 256 lanes", at[SOLVE, ctx, 64], at[SOLVE, ctx, 256], grps, res, tuple(range(1, 33)))
  assert not bad, (len(bad), bad[:20])
