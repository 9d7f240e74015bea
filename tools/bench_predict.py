#!/usr/bin/env python
"""Time of ``SVGP.predict_f`` on its two routes, and of ``sampled_moments`` on top of them.

Shapes (N, M, d, L): ``mid`` (262144, 512, 8, 8), ``wide`` (65536, 2000, 8, 8) and ``drift`` (1048576, 100, 6, 4); ``sampled_moments``
at the last one (S = 524288 draws of B = 2 states: the same 1048576 points).  Per shape, in one process and in alternating windows
(``bench_multiaction.alternating``: the routes take turns window by window, device events around each window, median of
``--repeats`` windows after warm-up), ms per call under ``torch.no_grad()`` of
  ``native``   ``predict_f(X, native=True)``: ``mm_predict_se`` on the cached ``precompute`` (nothing is factored per call)
  ``torch``    ``predict_f(X, native=False)``: the Cholesky factor, the triangular solves and the products, chunked over N
and from them ``native_over_torch``; the rate of the native route on the ALGORITHMIC work N L M (M + 1) flops (the quadratic form
with the symmetry of C used; the entries of K, the mean and the mixing are not counted) and that rate as a fraction of the
78.6 TFLOP/s f64 peak DESIGN.md section 8 normalises by -- an end-to-end figure of the call, not a kernel's share of peak; and the
largest difference between the two routes' outputs at the timed size, relative to the largest variance.  Prints one JSON line and
writes it to ``--out`` (default profiles/predict_bench.json)."""
import argparse
import json
import os
import sys

_here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _here)
sys.path.insert(0, os.path.join(_here, "tools"))

import torch  # noqa: E402

from bench_multiaction import alternating  # noqa: E402
from gpflowpilco_amd.moment_matching import GaussianMoments, sampled_moments  # noqa: E402
from gpflowpilco_amd.synthetic import make_inputs, make_svgp  # noqa: E402

F64 = torch.float64
F64_PEAK = 78.6e12
SHAPES = {"mid": dict(N=262144, M=512, d=8, L=8, inner=8), "wide": dict(N=65536, M=2000, d=8, L=8, inner=2),
          "drift": dict(N=1048576, M=100, d=6, L=4, inner=20)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default="mid,wide,drift")
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--label", default="")
  ap.add_argument("--out", default=os.path.join(_here, "profiles", "predict_bench.json"))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_predict.py needs the GPU (no CPU timing is meaningful)")
  device = "cuda"
  res = {"tool": "bench_predict", "label": args.label, "unit": "ms per call; median of alternating windows", "f64_peak": F64_PEAK,
         "shapes": {}}
  torch.set_grad_enabled(False)
  for name in args.shapes.split(","):
    shape = dict(SHAPES[name])
    inner = shape.pop("inner")
    N, M, d, L = (shape[k] for k in "NMdL")
    model = make_svgp(L, M, d, seed=70 + M, device=device, mean_c=True).to_model(device)
    X = (1.4 * torch.rand(N, d, dtype=F64, generator=torch.Generator().manual_seed(N + M)) - 0.2).to(device)
    fns = {"native": lambda: model.predict_f(X, native=True), "torch": lambda: model.predict_f(X, native=False)}
    out = alternating(fns, 1, inner, args.repeats, 2)
    (mn, vn), (mt, vt) = fns["native"](), fns["torch"]()
    scale = float(vt.abs().max())
    out["routes_max_diff_over_max_var"] = {"mean": float((mn - mt).abs().max()) / scale, "var": float((vn - vt).abs().max()) / scale}
    flops = float(N) * L * M * (M + 1)
    out["algorithmic_flops"] = flops
    out["native_over_torch"] = out["native"]["median"] / out["torch"]["median"]
    out["native_TFLOPs"] = flops / (out["native"]["median"] * 1e-3) / 1e12
    out["native_frac_f64_peak"] = out["native_TFLOPs"] * 1e12 / F64_PEAK
    if name == "drift":
      mu, Sigma = make_inputs(2, d, seed=3, scale=0.1, lo=0.3, hi=0.7)
      x = GaussianMoments(moments=(torch.tensor(mu, dtype=F64, device=device), torch.tensor(Sigma, dtype=F64, device=device)), centered=True)
      S = N // 2
      gen = torch.Generator(device=device)

      class Route:                                  # the model with predict_f pinned to one route
        def __init__(self, native):
          self.native = native

        def predict_f(self, Xs, **kw):
          return model.predict_f(Xs, native=self.native, **kw)
      sm = {k: (lambda r=Route(k == "native"): sampled_moments(x, r, num_samples=S, generator=gen.manual_seed(11))) for k in ("native", "torch")}
      sm_out = alternating(sm, 1, 3, args.repeats, 1)
      a, b = sm["native"](), sm["torch"]()
      sm_out["routes_max_diff"] = float((a.y.covariance() - b.y.covariance()).abs().max())
      sm_out["native_over_torch"] = sm_out["native"]["median"] / sm_out["torch"]["median"]
      sm_out["num_samples"], sm_out["batch"] = S, 2
      out["sampled_moments"] = sm_out
    res["shapes"][name] = dict(shape=shape, **out)
    del model, X, fns
    torch.cuda.empty_cache()
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")


if __name__ == "__main__":
  main()
