"""Per-call cost of drawing new sample paths: ``pathwise.generate_paths`` (torch, from nothing each call) against
``pathwise.PathSampler.draw`` (cached factor, preallocated buffers, csrc/mm_pathwise_sample.hip), and what it does to the training
step of ``loops.pathwise_policy_loss_closure`` with ``paths=None`` (PathwisePILCO: new paths on every optimiser step).

Per size and stream dtype, in ONE process, alternating windows (each window = ``inner`` calls, closed by a device synchronise;
medians with ranges over ``--repeats`` windows, two warm-up calls of everything first):

  generate_paths / draw                      one call each
  closure_off / closure_on                   loss + gradient of the cartpole-shaped closure (nx 4, one angle, one action, policy of
                                             30 centres, H steps), eager, ``native_sampler`` off / on
  closure_on_replayed                        the same from a ``GraphedPolicyLoss`` replay (each replay draws new paths)
  pack / copy                                ``mm_pathwise_pack_stream`` alone against a plain device-to-device ``copy_`` that moves
                                             the same number of bytes (read + written), as bytes per second

Sizes: S 1024 / M 256 (the reference's cartpole sizes) and S 8192 / M 2000 (the C5 shard), K 1024, L 4, d 6.

  python tools/bench_path_sampler.py [--sizes small,big] [--dtypes f32,f64] [--steps 10] [--repeats 7] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpflowpilco_amd import _lib, bijectors as tfb, dynamics, models as gp  # noqa: E402
from gpflowpilco_amd.components import GaussianObjective, TrigonometricEncoder  # noqa: E402
from gpflowpilco_amd.loops import GraphedPolicyLoss, pathwise_policy_loss_closure  # noqa: E402
from gpflowpilco_amd.pathwise import PathwiseSVGP, generate_paths  # noqa: E402
from gpflowpilco_amd.synthetic import make_policy, make_svgp  # noqa: E402

F64 = torch.float64
SIZES = {"small": dict(S=1024, M=256, inner=10), "big": dict(S=8192, M=2000, inner=2)}
K, L, D, NX = 1024, 4, 6, 4


def timed(fn, inner):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(inner):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / inner * 1e3


def alternating(fns, inners, repeats):
  """ms per call: every function warmed twice, then ``repeats`` rounds that visit the functions in turn."""
  for fn in fns.values():
    fn(); fn()
  times = {k: [] for k in fns}
  for _ in range(repeats):
    for k, fn in fns.items():
      times[k].append(timed(fn, inners[k]))
  return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "windows": len(v), "inner": inners[k]}
          for k, v in times.items()}


def system_of(M, S, dtype, device, seed=50):
  base = make_svgp(NX, M, D, seed=seed, device=device, ls_bounds=(0.8, 3.0)).to_model(device)
  drift = PathwiseSVGP(kernel=base.kernel, inducing_variable=base.inducing_variable, q_mu=base.q_mu, q_sqrt=base.q_sqrt, whiten=True,
                       num_latent_gps=NX)
  pol = make_policy(30, NX + 1, seed=seed + 1).to_model(device)
  params = [pol.q_mu, pol.inducing_variable.inducing_variables[0].Z, pol.kernel.kernels[0].lengthscales, pol.kernel.kernels[0].variance]
  for t in params:
    t.requires_grad_(True)
  head = tfb.Chain([tfb.Scale(2.0), tfb.Shift(-0.5), tfb.NormalCDF()])
  system = dynamics.DynamicalSystem(drift=drift, policy=gp.InverseLinkWrapper(gp.KernelRegressor(pol), invlink=head),
                                    encoder=TrigonometricEncoder(active_dims=(1,)), solver=dynamics.Euler())
  target = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0], dtype=dtype, device=device)
  objective = GaussianObjective(target=target, precis=torch.eye(NX + 1, dtype=dtype, device=device))
  x0 = 0.2 + 0.6 * torch.rand(S, NX, dtype=dtype, device=device, generator=torch.Generator(device=device).manual_seed(seed + 2))
  return system, objective, drift, params, x0


def pack_against_copy(sampler, dtype, device, repeats, inner):
  """The pack kernel alone on the sampler's own buffers, and a ``copy_`` that moves as many bytes."""
  B = sampler.buffers
  S, Lq, Kq = B["w"].shape
  M = B["rhs"].shape[1]
  code = _lib.MM_F64 if dtype == F64 else _lib.MM_F32
  lib, stream = _lib.lib(), torch.cuda.current_stream(device).cuda_stream
  moved = (B["w"].numel() + B["rhs"].numel()) * 8 + B["wb"].numel() * B["wb"].element_size()      # read + written
  src = torch.empty(moved // 2, dtype=torch.uint8, device=device).random_(0, 255)
  dst = torch.empty_like(src)

  def pack():
    rc = lib.mm_pathwise_pack_stream(S, Lq, Kq, M, code, B["w"].data_ptr(), B["rhs"].data_ptr(), B["wb"].data_ptr(), stream)
    assert rc == 0, rc
  res = alternating({"pack": pack, "copy": lambda: dst.copy_(src)}, {"pack": inner, "copy": inner}, repeats)
  for k in ("pack", "copy"):
    res[k]["bytes_moved"] = moved if k == "pack" else 2 * src.numel()
    res[k]["GB_per_s"] = res[k]["bytes_moved"] / (res[k]["median"] * 1e-3) / 1e9
  res["pack_over_copy_rate"] = res["pack"]["GB_per_s"] / res["copy"]["GB_per_s"]
  return res


def one(size, dtype, H, repeats, device):
  S, M, inner = SIZES[size]["S"], SIZES[size]["M"], SIZES[size]["inner"]
  out = {"shape": {"S": S, "M": M, "K": K, "L": L, "d": D, "H": H, "dtype": str(dtype)}}
  with warnings.catch_warnings():
    warnings.simplefilter("error", RuntimeWarning)            # a fall-back to the torch composition would be timed as native: refuse
    # the capture first, on fresh parameters (an eager backward pins their gradient accumulation to the default stream)
    system, objective, drift, params, x0 = system_of(M, S, dtype, device)
    on = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.1, num_bases=K, native=True, native_sampler=True)
    off = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.1, num_bases=K, native=True)
    try:
      graphed = GraphedPolicyLoss(on, params)
    except Exception as e:                                     # noqa: BLE001 -- reported, the eager rows are still measured
      graphed = None
      out["capture_error"] = f"{type(e).__name__}: {e}"[:400]
      system, objective, drift, params, x0 = system_of(M, S, dtype, device)
      on = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.1, num_bases=K, native=True, native_sampler=True)
      off = pathwise_policy_loss_closure(system, objective, lambda: x0, H, dt=0.1, num_bases=K, native=True)

    def loss_grad(closure):
      def run():
        for t in params:
          t.grad = None
        loss = closure().mean()
        loss.backward()
        return loss
      return run
    sampler = drift.path_sampler(S, K, dtype=dtype, device=device)
    fns = {"generate_paths": lambda: generate_paths(drift, S, K, dtype=dtype, device=device), "draw": sampler.draw,
           "closure_off": loss_grad(off), "closure_on": loss_grad(on)}
    if graphed is not None:
      fns["closure_on_replayed"] = graphed.loss_and_grad
    inners = {k: inner for k in fns}
    out.update(alternating(fns, inners, repeats))
    if graphed is not None:
      graphed.check()
  med = lambda k: out[k]["median"]
  out["generate_paths_over_draw"] = med("generate_paths") / med("draw")
  out["closure_off_over_on"] = med("closure_off") / med("closure_on")
  if graphed is not None:
    out["closure_off_over_on_replayed"] = med("closure_off") / med("closure_on_replayed")
  out["pack_kernel"] = pack_against_copy(sampler, dtype, device, repeats, max(inner, 5))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sizes", default="small,big")
  ap.add_argument("--dtypes", default="f32,f64")
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_path_sampler needs a GPU: timings on anything else say nothing")
  device = "cuda"
  res = {"tool": "bench_path_sampler", "unit": "ms per call (median, min, max over alternating windows)", "device": torch.cuda.get_device_name(0)}
  for size in args.sizes.split(","):
    for name in args.dtypes.split(","):
      dtype = {"f32": torch.float32, "f64": F64}[name]
      res[f"{size}_{name}"] = one(size, dtype, args.steps, args.repeats, device)
      torch.cuda.empty_cache()
      if args.out:                                             # after every row: a later row that fails loses nothing
        with open(args.out, "w") as f:
          json.dump(res, f, indent=1)
  print(json.dumps(res))


if __name__ == "__main__":
  main()
