#!/usr/bin/env python
"""Collapsed (SGPR) training of the SVGP drift against the ELBO route: the streamed Gram statistics alone, one loss-plus-gradient
evaluation, and a whole fit.

Shapes: ``cartpole`` N 600, M 100, d 6, L 4; ``large`` N 4000, M 512, d 8, L 8 (``bench_svgp_fit.py``'s two); ``huge`` N 262 144,
M 512, d 8, L 8, where one [L, M, N] float64 tensor is 8.6 GB.  Per shape, in one process and in alternating windows
(``bench_multiaction.alternating``: the variants take turns window by window, median of ``--repeats`` windows after warm-up):

1. ``stats_native``  ``ops.gram_stats_se`` + ``ops.gram_stats_se_backward`` (K never stored) against ``stats_composed``, the same
   results from existing parts with bounded memory: per chunk of N, ``ops.gram_se`` -> ``bmm`` for Phi and Psi, then
   ``bmm`` for the adjoint of K -> ``ops.gram_se_backward``.  ``stats_fwd_native`` / ``stats_fwd_composed``: the forward alone, and
   its rate on N L M (M + 1) flops against the 78.6 TFLOP/s float64 matrix peak -- an END-TO-END figure of the call, formation of K
   and the sum launch included.
2. ``collapsed_native`` / ``collapsed_torch`` / ``elbo_native``: loss + gradient of ``collapsed_training_loss`` on its two routes
   and of ``training_loss`` on the same tree; ``peak_MiB_*``: the allocator's peak over one such call.  A variant that does not
   fit is recorded as the error it raised.
3. ``fit_default`` / ``fit_collapsed`` (``--fit-iters`` > 0; not on ``huge``): ``fit_svgp`` from the same
   ``SVGP.initialize(seed=...)`` on a smooth function plus noise: wall seconds, iterations, and ``model.elbo`` of the fitted model.

``--sweep`` adds row 1 over M 64 .. 512 at L 8, d 8, N 4000 and 65 536: the origin of ``models.STATS_STREAMED_MAX_M``.
``--huge-elbo`` also tries the ELBO on the huge shape.

Prints one JSON line and writes it to ``--out`` (default profiles/svgp_collapsed_bench.json)."""
import argparse
import json
import os
import sys
import time

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _here)
sys.path.insert(0, os.path.join(_here, "tools"))

import torch  # noqa: E402

from bench_multiaction import alternating  # noqa: E402
from bench_svgp_fit import build  # noqa: E402
from gpflowpilco_amd import models as gp, ops  # noqa: E402
from gpflowpilco_amd.training import fit_svgp  # noqa: E402

F64 = torch.float64
SHAPES = {"cartpole": dict(N=600, M=100, d=6, L=4), "large": dict(N=4000, M=512, d=8, L=8), "huge": dict(N=262144, M=512, d=8, L=8)}
PEAK_F64_MATRIX = 78.6e12


def composed(X, R, Z, ls, var, GPhi, GPsi, backward):
  """Phi, Psi (and gZ, gls, gvar) from ``ops.gram_se`` / ``bmm`` / ``ops.gram_se_backward`` in chunks of N."""
  L, M, _ = Z.shape
  chunk = max(1, gp.PREDICT_CHUNK_BYTES // (8 * L * M))
  Gs = GPhi + GPhi.transpose(1, 2)

  def call():
    Phi, Psi = torch.zeros_like(GPhi), torch.zeros_like(GPsi)
    for s in range(0, X.shape[0], chunk):
      K = ops.gram_se(X[s:s + chunk], Z, ls, var)
      Phi.baddbmm_(K, K.transpose(1, 2))
      Psi.add_(K @ R[s:s + chunk])
    if not backward:
      return Phi, Psi
    gZ, gls, gvar = torch.zeros_like(Z), torch.zeros_like(ls), torch.zeros_like(var)
    for s in range(0, X.shape[0], chunk):
      K = ops.gram_se(X[s:s + chunk], Z, ls, var)
      GK = torch.baddbmm(GPsi @ R[s:s + chunk].T, Gs, K)
      for acc, g in zip((gZ, gls, gvar), ops.gram_se_backward(GK, X[s:s + chunk], Z, ls, var)):
        acc.add_(g)
    return Phi, Psi, gZ, gls, gvar
  return call


def sweep(device, repeats, inner):
  """Row 1 alone over M at L 8, d 8 and two N: where the streamed kernel stops being the faster route."""
  rows = []
  for N in (4000, 65536):
    for M in (64, 128, 192, 256, 320, 384, 512):
      g = torch.Generator().manual_seed(M + N)
      r = lambda *s: torch.randn(*s, dtype=F64, generator=g).to(device)
      L, d = 8, 8
      X, R, Z, ls, var = r(N, d), r(N, L + 1), r(L, M, d), 1.5 + r(L, d).abs(), 0.6 + r(L).abs()
      GPhi, GPsi = r(L, M, M), r(L, M, L + 1)
      fns = {"stats_native": lambda: (ops.gram_stats_se(X, R, Z, ls, var), ops.gram_stats_se_backward(GPhi, GPsi, X, R, Z, ls, var)),
             "stats_composed": composed(X, R, Z, ls, var, GPhi, GPsi, True)}
      out = alternating(fns, 1, inner, repeats, 3)
      rows.append(dict(N=N, M=M, L=L, d=d, stats_native=out["stats_native"], stats_composed=out["stats_composed"],
                       native_over_composed=out["stats_native"]["median"] / out["stats_composed"]["median"]))
      print(json.dumps(rows[-1]), flush=True)
  return rows


def measured(fn):
  """(peak MiB over one call after a first one, None) or (None, the error's first line)."""
  try:
    fn()                                                          # cached workspaces and library handles exist from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20, None
  except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
    torch.cuda.empty_cache()
    return None, f"{type(e).__name__}: {str(e).splitlines()[0][:200]}"


def fit_rows(N, M, d, L, device, iters, seed=0):
  g = torch.Generator().manual_seed(500 + seed)
  X = torch.randn(N, d, dtype=F64, generator=g)
  W = torch.randn(d, L, dtype=F64, generator=g) / d ** 0.5
  Y = torch.sin(1.5 * X @ W) + 0.1 * torch.randn(N, L, dtype=F64, generator=g)
  data = (X.to(device), Y.to(device))
  out = {}
  for name, collapsed in (("fit_default", False), ("fit_collapsed", True)):
    model = gp.SVGP.initialize((X, Y), M, seed=seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    history = fit_svgp(model, data, max_iter=iters, collapsed=collapsed)
    torch.cuda.synchronize()
    out[name] = dict(seconds=time.perf_counter() - t0, iterations=len(history) - 1, final_loss=history[-1],
                     final_elbo=float(model.elbo(data)))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default="cartpole,large,huge")
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--inner", type=int, default=10, help="calls per window (1 on the huge shape)")
  ap.add_argument("--fit-iters", type=int, default=30, help="max_iter of the two fits (0: no fit rows)")
  ap.add_argument("--sweep", action="store_true", help="also row 1 over M (the origin of models.STATS_STREAMED_MAX_M)")
  ap.add_argument("--huge-elbo", action="store_true", help="also try the ELBO on the huge shape (its [L,M,N] working set)")
  ap.add_argument("--label", default="")
  ap.add_argument("--out", default=os.path.join(_here, "profiles", "svgp_collapsed_bench.json"))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_svgp_collapsed.py needs the GPU (no CPU timing is meaningful)")
  device = "cuda"
  res = {"tool": "bench_svgp_collapsed", "label": args.label, "unit": "ms per call; median of alternating windows", "shapes": {}}
  for name in args.shapes.split(","):
    shape = SHAPES[name]
    N, M, d, L = (shape[k] for k in "NMdL")
    huge = name == "huge"
    model, data, params = build(device=device, **shape)
    with torch.no_grad():
      Z, ls, var = gp._stack_kernel_params(model.latent_kernels, [iv.Z for iv in model.inducing_variable.inducing_variables], device)
    X = data[0]
    R = torch.cat([data[1], torch.ones(N, 1, dtype=F64, device=device)], 1)
    g = torch.Generator().manual_seed(9)
    GPhi, GPsi = torch.randn(L, M, M, dtype=F64, generator=g).to(device), torch.randn(L, M, L + 1, dtype=F64, generator=g).to(device)

    def loss_grad(loss_fn, native):
      def call():
        for t in params:
          t.grad = None
        loss = loss_fn(data, native=native)
        loss.backward()
        return loss
      return call

    fns = {"stats_fwd_native": lambda: ops.gram_stats_se(X, R, Z, ls, var),
           "stats_fwd_composed": composed(X, R, Z, ls, var, GPhi, GPsi, False),
           "stats_native": lambda: (ops.gram_stats_se(X, R, Z, ls, var), ops.gram_stats_se_backward(GPhi, GPsi, X, R, Z, ls, var)),
           "stats_composed": composed(X, R, Z, ls, var, GPhi, GPsi, True),
           "collapsed_native": loss_grad(model.collapsed_training_loss, None)}
    optional = {"collapsed_torch": loss_grad(model.collapsed_training_loss, False), "elbo_native": loss_grad(model.training_loss, None)}
    out = {}
    for k in ("collapsed_native", "collapsed_torch", "elbo_native"):
      if huge and k == "elbo_native" and not args.huge_elbo:
        out["peak_MiB_elbo_native"], out["error_elbo_native"] = None, "not measured (--huge-elbo)"
        continue
      fn = fns.get(k) or optional[k]
      out[f"peak_MiB_{k}"], err = measured(fn)
      if err is None:
        fns[k] = fn
      else:
        out[f"error_{k}"] = err
    out.update(alternating(fns, 1, 1 if huge else args.inner, 3 if huge else args.repeats, 1 if huge else 3))
    out["loss_collapsed_native"] = float(fns["collapsed_native"]().detach())
    t_f = out["stats_fwd_native"]["median"] * 1e-3
    out["stats_fwd_native_fraction_of_f64_matrix_peak_end_to_end"] = N * L * M * (M + 1) / t_f / PEAK_F64_MATRIX
    out["native_over_composed_stats"] = out["stats_native"]["median"] / out["stats_composed"]["median"]
    out["native_over_composed_stats_fwd"] = out["stats_fwd_native"]["median"] / out["stats_fwd_composed"]["median"]
    if "elbo_native" in fns:
      out["collapsed_over_elbo_loss_and_grad"] = out["collapsed_native"]["median"] / out["elbo_native"]["median"]
    del model, data, params, fns, optional
    torch.cuda.empty_cache()
    if args.fit_iters > 0 and not huge:
      out.update(fit_rows(N, M, d, L, device, args.fit_iters))
    else:
      out["fit_default"] = out["fit_collapsed"] = "not measured"
    res["shapes"][name] = dict(shape=shape, **out)
    print(json.dumps({name: res["shapes"][name]}), flush=True)
  if args.sweep:
    res["sweep"] = sweep(device, args.repeats, args.inner)
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")


if __name__ == "__main__":
  main()
