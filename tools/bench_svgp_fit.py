#!/usr/bin/env python
"""Time of one loss-plus-gradient evaluation of the SVGP training loss on its two Gram routes, and of the Gram entries alone.

Shapes: ``cartpole`` N 600, M 100, d 6, L 4 (an episode buffer) and ``large`` N 4000, M 512, d 8, L 8.  Per shape, in one process and
in alternating windows (``bench_multiaction.alternating``: the variants take turns window by window, median of ``--repeats``
windows after warm-up), ms per call of
  ``loss_and_grad_native`` / ``_torch``   ``training_loss_closure(data, native=None | False)()`` and its ``backward()`` into every
                                          parameter -- the Cholesky factor, the solves and the products are torch's on both routes
  ``gram_native`` / ``gram_torch``        Kuf [L,M,N] alone: ``mm_gram_se`` against the torch route's broadcast chain
  ``gram_grad_native`` / ``_torch``       Kuf and its adjoint for a fixed G: ``mm_gram_se`` + ``mm_gram_se_backward`` (K recomputed)
                                          against torch autograd of the chain
  ``self_native`` / ``self_grad_native``  the self mode, Kuu [L,M,M], forward and forward + adjoint
and, from shapes, what the native entries move and compute per call (8 bytes and 3 d + 30 flops per entry forward; 8 bytes and
7 d + 33 flops per entry in the adjoint), as achieved GB/s and GFLOP/s.  ``peak_MiB_*``: the allocator's peak over one
loss-plus-gradient call of each route.  Prints one JSON line and writes it to ``--out`` (default profiles/svgp_fit_bench.json)."""
import argparse
import json
import os
import sys

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _here)
sys.path.insert(0, os.path.join(_here, "tools"))

import torch  # noqa: E402

from bench_multiaction import alternating  # noqa: E402
from gpflowpilco_amd import models as gp, ops  # noqa: E402

F64 = torch.float64
SHAPES = {"cartpole": dict(N=600, M=100, d=6, L=4), "large": dict(N=4000, M=512, d=8, L=8)}


def build(N, M, d, L, device, seed=0):
  """A whitened model with every parameter a leaf on the device, inducing points drawn from the data, and its data."""
  g = torch.Generator().manual_seed(400 + seed)
  X = torch.randn(N, d, dtype=F64, generator=g)
  Y = torch.randn(N, L, dtype=F64, generator=g)
  params = []

  def leaf(t):
    params.append(t.to(device).requires_grad_(True))
    return params[-1]
  kernels = [gp.SquaredExponential(leaf(0.6 + torch.rand((), dtype=F64, generator=g)),
                                   leaf(1.5 + torch.rand(d, dtype=F64, generator=g))) for _ in range(L)]
  ivs = [gp.InducingPoints(leaf(X[torch.randperm(N, generator=g)[:M]].clone())) for _ in range(L)]
  model = gp.SVGP(gp.SeparateIndependent(kernels), gp.SeparateIndependentInducingVariables(ivs),
                  leaf(0.1 * torch.randn(M, L, dtype=F64, generator=g)), leaf(torch.eye(M, dtype=F64).repeat(L, 1, 1)), whiten=True,
                  mean_function=gp.Constant(leaf(torch.zeros(L, dtype=F64))), likelihood=gp.GaussianLikelihood(leaf(torch.tensor(0.1, dtype=F64))),
                  num_latent_gps=L)
  return model, (X.to(device), Y.to(device)), params


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default="cartpole,large")
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--inner", type=int, default=20, help="loss + gradient calls per window (a window then lasts 60 - 250 ms)")
  ap.add_argument("--inner-gram", type=int, default=400, help="calls per window of the stand-alone Gram rows (6 - 600 ms)")
  ap.add_argument("--label", default="")
  ap.add_argument("--out", default=os.path.join(_here, "profiles", "svgp_fit_bench.json"))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_svgp_fit.py needs the GPU (no CPU timing is meaningful)")
  device = "cuda"
  res = {"tool": "bench_svgp_fit", "label": args.label, "unit": "ms per call; median of alternating windows", "shapes": {}}
  for name in args.shapes.split(","):
    shape = SHAPES[name]
    N, M, d, L = (shape[k] for k in "NMdL")
    model, data, params = build(device=device, **shape)

    def loss_grad(native):
      closure = model.training_loss_closure(data, native=native)

      def call():
        for t in params:
          t.grad = None
        loss = closure()
        loss.backward()
        return loss
      return call

    with torch.no_grad():
      Z, ls, var = gp._stack_kernel_params(model.latent_kernels, [iv.Z for iv in model.inducing_variable.inducing_variables], device)
    X = data[0]
    G = torch.randn(L, M, N, dtype=F64, device=device)
    Gs = torch.randn(L, M, M, dtype=F64, device=device)

    def gram_torch(grad):
      Zr, lr, vr = (t.clone().requires_grad_(grad) for t in (Z, ls, var))

      def call():
        K = vr[:, None, None] * gp.stationary_profile(gp._scaled_sqdist(Zr / lr[:, None, :], X[None] / lr[:, None, :]), gp.KERNEL_SE)
        return torch.autograd.grad((G * K).sum(), (Zr, lr, vr)) if grad else K
      return call

    fns = {"loss_and_grad_native": loss_grad(None), "loss_and_grad_torch": loss_grad(False),
           "gram_native": lambda: ops.gram_se(X, Z, ls, var), "gram_torch": gram_torch(False),
           "gram_grad_native": lambda: (ops.gram_se(X, Z, ls, var), ops.gram_se_backward(G, X, Z, ls, var)),
           "gram_grad_torch": gram_torch(True),
           "self_native": lambda: ops.gram_se_self(Z, ls, var),
           "self_grad_native": lambda: (ops.gram_se_self(Z, ls, var), ops.gram_se_backward(Gs, None, Z, ls, var))}
    inner = {k: args.inner if k.startswith("loss") else args.inner_gram for k in fns}
    out = alternating(fns, 1, inner, args.repeats, 3)
    values = {k: float(fns[f"loss_and_grad_{k}"]().detach()) for k in ("native", "torch")}
    out["loss_native"], out["loss_torch"] = values["native"], values["torch"]
    for route in ("native", "torch"):
      torch.cuda.synchronize()
      torch.cuda.reset_peak_memory_stats()
      base = torch.cuda.memory_allocated()
      fns[f"loss_and_grad_{route}"]()
      torch.cuda.synchronize()
      out[f"peak_MiB_{route}"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    entries = L * M * N
    t_f, t_fb = out["gram_native"]["median"] * 1e-3, out["gram_grad_native"]["median"] * 1e-3
    out["gram_native_GBps"] = 8.0 * entries / t_f / 1e9
    out["gram_native_GFLOPs"] = (3 * d + 30) * entries / t_f / 1e9
    out["gram_grad_native_GFLOPs"] = ((3 * d + 30) + (7 * d + 33)) * entries / t_fb / 1e9
    out["native_over_torch_loss_and_grad"] = out["loss_and_grad_native"]["median"] / out["loss_and_grad_torch"]["median"]
    out["native_over_torch_gram_grad"] = out["gram_grad_native"]["median"] / out["gram_grad_torch"]["median"]
    res["shapes"][name] = dict(shape=shape, **out)
    del model, data, params, fns
    torch.cuda.empty_cache()
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")


if __name__ == "__main__":
  main()
