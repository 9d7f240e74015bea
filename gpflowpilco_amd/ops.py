"""torch-tensor front end of the C ABI (device pointers + current HIP stream).

PyTorch is plumbing here: it owns the device buffers and the stream; every
floating-point operation of the moment match happens in the HIP kernels of
``csrc/``.  Nothing in this module runs on the CPU -- tensors must live on a
ROCm device.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import (MM_F32, MM_F64, MM_FORCE_GENERIC, MM_FULL_OUTPUT_COV, MM_WORKSPACE_CURRENT, MM_SUMS_CURRENT,
                   MM_MODEL_UNCERTAINTY, check, lib)

_DTYPES = {torch.float32: MM_F32, torch.float64: MM_F64}


def _dtype_code(dtype: torch.dtype) -> int:
  try:
    return _DTYPES[dtype]
  except KeyError:
    raise TypeError(f"moment matching supports float32/float64 states, got {dtype}") from None


def _ptr(t: Optional[torch.Tensor]):
  return None if t is None else t.data_ptr()


def _require_device(*tensors: torch.Tensor):
  for t in tensors:
    if t is not None and not t.is_cuda:
      raise RuntimeError("gpflowpilco_amd kernels run on the GPU only (no CPU fallback): "
                         f"got a tensor on {t.device}")


def _stream(device) -> int:
  return torch.cuda.current_stream(device).cuda_stream


def make_flags(full_output_cov: bool = True, model_uncertainty: bool = True,
               force_generic: bool = False) -> int:
  return ((MM_FULL_OUTPUT_COV if full_output_cov else 0)
          | (MM_MODEL_UNCERTAINTY if model_uncertainty else 0)
          | (MM_FORCE_GENERIC if force_generic else 0))


@dataclass
class PackedModel:
  """Device-resident packed model (output of ``mm_pack_model``)."""
  L: int
  M: int
  d: int
  dtype: torch.dtype
  with_C: bool
  buf: torch.Tensor                      # uint8 [packed_bytes]
  _workspaces: Dict[Tuple[int, int], torch.Tensor] = field(default_factory=dict, repr=False)
  _ws_gen: Dict[Tuple[int, int], int] = field(default_factory=dict, repr=False)
  _status: Optional[torch.Tensor] = field(default=None, repr=False)
  _keep: Optional[tuple] = field(default=None, repr=False)
  _perm: Optional[torch.Tensor] = field(default=None, repr=False)

  @property
  def device(self):
    return self.buf.device

  @property
  def nbytes(self) -> int:
    return self.buf.numel()

  def workspace(self, B: int, flags: int, peek: bool = False) -> torch.Tensor:
    """The per-(B, flags) scratch buffer of the kernels.  Every request counts as a use (``workspace_generation``):
    whoever asks may overwrite it; ``peek`` looks without counting."""
    key = (B, flags & (MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY))
    if not peek:
      self._ws_gen[key] = self._ws_gen.get(key, 0) + 1
    ws = self._workspaces.get(key)
    if ws is None:
      n = lib().mm_workspace_bytes(B, self.L, self.M, self.d, _dtype_code(self.dtype), flags)
      if n == 0:
        raise ValueError("mm_workspace_bytes rejected the shape")
      ws = torch.empty(n, dtype=torch.uint8, device=self.device)
      self._workspaces[key] = ws
    return ws

  def workspace_generation(self, B: int, flags: int) -> int:
    """Counter of the requests for this workspace: unchanged since a forward <=> that forward's q stage is still on it."""
    return self._ws_gen.get((B, flags & (MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)), 0)

  def perm(self) -> torch.Tensor:
    """[L, M] int64: the caller's index of the inducing point at packed position m (``mm_pack_perm``: packs of M > 256 points
    are sorted per latent by |(z - mean z) / lengthscale|).  ``q_forward``'s q is in the caller's order; the per-point sums of
    ``mm_backward_sums`` are in packed order."""
    if self._perm is None:
      p32 = torch.empty(self.L, self.M, dtype=torch.int32, device=self.device)
      check(lib().mm_pack_perm(self.buf.data_ptr(), self.nbytes, self.L, self.M, self.d, _dtype_code(self.dtype),
                               p32.data_ptr(), _stream(self.device)), "mm_pack_perm")
      self._perm = p32.long()
    return self._perm

  def status(self) -> torch.Tensor:
    if self._status is None:
      self._status = torch.zeros(4, dtype=torch.int32, device=self.device)
    return self._status

  def routed(self) -> Tuple[int, int]:
    """(forward, backward) counts of (batch element, off-diagonal pair) items a float32 pack re-reduced in float64 since the
    status word was last zeroed (csrc/mm_route.hip: items whose estimated f32 rounding error exceeded MM_ROUTE_TOL of the
    covariance block's scale).  Synchronises."""
    st = self.status().tolist()
    return st[2], st[3]

  def check_status(self, B: int):
    """Synchronising check of the non-PD flag (the reference raises at this point)."""
    st = self.status().tolist()
    if st[0] != 0 and st[1] == -1:
      self._status.zero_()
      raise RuntimeError(
          f"moment_match_backward was told the workspace still holds the forward's q stage (MM_WORKSPACE_CURRENT), but batch "
          f"element {B - st[0]} of it belongs to another state: something wrote the workspace in between without going "
          "through PackedModel.workspace() (a graph replay, another stream, an external ABI caller)")
    if st[0] != 0 and st[1] == -2:
      self._status.zero_()
      raise RuntimeError(
          f"moment_match_backward was given kept sums (MM_SUMS_CURRENT) that were swept for another state: batch element "
          f"{B - st[0]} of `sums` does not belong to this (mu, Sigma)")
    if st[0] != 0:
      self._status.zero_()
      raise FloatingPointError(
          f"Cholesky of (Sigma + V) failed for batch element {B - st[0]} (item {st[1]}): "
          "the input covariance is not positive definite")


def pack_model(Z: torch.Tensor, lengthscales: torch.Tensor, variance: torch.Tensor,
               beta: torch.Tensor, C: Optional[torch.Tensor] = None,
               mean_c: Optional[torch.Tensor] = None,
               dtype: torch.dtype = torch.float32, sync: bool = True) -> PackedModel:
  """Z [L,M,d], lengthscales [L,d], variance [L], beta [L,M], C [L,M,M]|None, mean_c [L]|None
  (all float64 on the GPU) -> PackedModel whose reduce operands are stored as ``dtype``.
  ``sync=False`` (graph capture): no stream synchronisation; the f64 inputs are kept alive on the returned object."""
  _require_device(Z, lengthscales, variance, beta, C, mean_c)
  L, M, d = Z.shape
  f64 = lambda t: None if t is None else t.to(torch.float64).contiguous()
  Z, lengthscales, variance, beta, C, mean_c = map(f64, (Z, lengthscales, variance, beta, C, mean_c))
  assert lengthscales.shape == (L, d) and variance.shape == (L,) and beta.shape == (L, M)
  assert C is None or C.shape == (L, M, M)
  assert mean_c is None or mean_c.shape == (L,)
  code = _dtype_code(dtype)
  n = lib().mm_packed_model_bytes(L, M, d, code, int(C is not None))
  if n == 0:
    raise ValueError(f"unsupported model shape L={L} M={M} d={d} (d <= {_lib.MM_DMAX})")
  buf = torch.empty(n, dtype=torch.uint8, device=Z.device)
  rc = lib().mm_pack_model(buf.data_ptr(), n, L, M, d, code, _ptr(Z), _ptr(lengthscales),
                           _ptr(variance), _ptr(beta), _ptr(C), _ptr(mean_c), _stream(Z.device))
  check(rc, "mm_pack_model")
  # the f64 inputs must outlive the asynchronous pack kernels
  pm = PackedModel(L=L, M=M, d=d, dtype=dtype, with_C=C is not None, buf=buf)
  if sync:
    torch.cuda.current_stream(Z.device).synchronize()
  else:
    pm._keep = (Z, lengthscales, variance, beta, C, mean_c)
  return pm


def _prep_state(pm: PackedModel, mu: torch.Tensor, Sigma: torch.Tensor):
  _require_device(mu, Sigma)
  if mu.dtype != pm.dtype or Sigma.dtype != pm.dtype:
    raise TypeError(f"state dtype {mu.dtype}/{Sigma.dtype} does not match the packed model ({pm.dtype})")
  B, d = mu.shape
  if d != pm.d or Sigma.shape != (B, d, d):
    raise ValueError(f"expected mu [B,{pm.d}] and Sigma [B,{pm.d},{pm.d}], got {tuple(mu.shape)}, {tuple(Sigma.shape)}")
  return B, mu.contiguous(), Sigma.contiguous()


def moment_match(pm: PackedModel, mu: torch.Tensor, Sigma: torch.Tensor,
                 full_output_cov: bool = True, model_uncertainty: bool = True,
                 jitter: float = 0.0, force_generic: bool = False, extra_flags: int = 0):
  """(mu [B,d], Sigma [B,d,d]) -> f1 [B,L], Sff [B,L,L] | [B,L], Sigma^-1 Cov(x,f) [B,d,L].
  ``extra_flags``: test / measurement bits of the C ABI (``MM_FORCE_ROUTE``, ``MM_NO_ROUTE``, ``MM_FORCE_WORST_TIER``; the
  internal A/B bits of csrc/mm_common.h, e.g. ``_lib.MM_ISTAGE_OLD_SKIP_BOUND`` / ``MM_ISTAGE_NO_BOUND_SKIP``)."""
  B, mu, Sigma = _prep_state(pm, mu, Sigma)
  flags = make_flags(full_output_cov, model_uncertainty, force_generic) | int(extra_flags)
  f1 = torch.empty(B, pm.L, dtype=pm.dtype, device=pm.device)
  Sff = torch.empty((B, pm.L, pm.L) if full_output_cov else (B, pm.L), dtype=pm.dtype, device=pm.device)
  cross = torch.empty(B, pm.d, pm.L, dtype=pm.dtype, device=pm.device)
  if B == 0:                       # an empty batch gives empty outputs (as the reference's tensor ops do); no launch
    if model_uncertainty and not pm.with_C:
      check(-5, "mm_moment_match")                    # MM_E_NO_C, as the C ABI reports it
    return f1, Sff, cross
  ws = pm.workspace(B, flags)
  rc = lib().mm_moment_match(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B,
                             mu.data_ptr(), Sigma.data_ptr(), flags, float(jitter),
                             f1.data_ptr(), Sff.data_ptr(), cross.data_ptr(),
                             ws.data_ptr(), ws.numel(), pm.status().data_ptr(), _stream(pm.device))
  check(rc, "mm_moment_match")
  return f1, Sff, cross


def q_forward(pm: PackedModel, mu: torch.Tensor, Sigma: torch.Tensor, flags: int, want_q: bool = False):
  """Stage 1: <K_xZ> terms.  Returns f1, cross_pre, q ([B,L,M] or None)."""
  B, mu, Sigma = _prep_state(pm, mu, Sigma)
  ws = pm.workspace(B, flags)
  f1 = torch.empty(B, pm.L, dtype=pm.dtype, device=pm.device)
  cross = torch.empty(B, pm.d, pm.L, dtype=pm.dtype, device=pm.device)
  q = torch.empty(B, pm.L, pm.M, dtype=pm.dtype, device=pm.device) if want_q else None
  rc = lib().mm_q_forward(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B,
                          mu.data_ptr(), Sigma.data_ptr(), flags, f1.data_ptr(), cross.data_ptr(), _ptr(q),
                          ws.data_ptr(), ws.numel(), pm.status().data_ptr(), _stream(pm.device))
  check(rc, "mm_q_forward")
  return f1, cross, q


def Q_reduce_forward(pm: PackedModel, B: int, flags: int, jitter: float = 0.0):
  """Stage 2: fused <K_Zx K_xZ'> reduce -> Sff.  Must follow ``q_forward`` with the same B/flags."""
  ws = pm.workspace(B, flags)
  full = bool(flags & MM_FULL_OUTPUT_COV)
  Sff = torch.empty((B, pm.L, pm.L) if full else (B, pm.L), dtype=pm.dtype, device=pm.device)
  rc = lib().mm_Q_reduce_forward(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B,
                                 flags, float(jitter), Sff.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _stream(pm.device))
  check(rc, "mm_Q_reduce_forward")
  return Sff


def offdiag_stats(pm: PackedModel, B: int, flags: int):
  """(collapsed, total, wholly inside) (b, off-diagonal pair) items of the last ``q_forward`` / ``moment_match`` with
  this B and flags (f32 models with d <= 8; zeros otherwise): items whose degree-3..6 remainder polynomial comes from
  weight moments (Cauchy-Schwarz bound on |b| <= 1/2), all items, and collapsed items whose bound puts every |b| <= 1/4 (the
  tile kernel does nothing for them).  Synchronises."""
  ws = pm.workspace(B, flags, peek=True)
  out = torch.zeros(6, dtype=torch.int32, device=pm.device)
  rc = lib().mm_offdiag_stats(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B, flags,
                              ws.data_ptr(), ws.numel(), out.data_ptr(), _stream(pm.device))
  check(rc, "mm_offdiag_stats")
  c, n, inside, _, _, _ = out.tolist()
  return c, n, inside


def offdiag_row_groups(pm: PackedModel, B: int, flags: int):
  """(partly collapsed items, collapsed 64-row groups, all row groups) of the last ``q_forward`` / ``moment_match``: the collapse is
  decided per group of 64 rows of an item (csrc/mm_mono.h); an item counted by ``offdiag_stats`` as collapsed has all its groups
  collapsed, a partly collapsed one some.  Synchronises."""
  ws = pm.workspace(B, flags, peek=True)
  out = torch.zeros(6, dtype=torch.int32, device=pm.device)
  rc = lib().mm_offdiag_stats(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B, flags,
                              ws.data_ptr(), ws.numel(), out.data_ptr(), _stream(pm.device))
  check(rc, "mm_offdiag_stats")
  o = out.tolist()
  Mp = (pm.M + _lib.MM_M_ALIGN - 1) // _lib.MM_M_ALIGN * _lib.MM_M_ALIGN
  return o[4], o[5], o[1] * (Mp // 64)


def offdiag_routed(pm: PackedModel, B: int, flags: int) -> int:
  """Items of the last ``moment_match`` / ``Q_reduce_forward`` with this B and flags that were re-reduced in float64
  (``mm_offdiag_stats`` out[3]; float32 models, else 0).  Synchronises."""
  if pm.dtype != torch.float32 or pm.L < 2 or not (flags & MM_FULL_OUTPUT_COV):
    return 0
  ws = pm.workspace(B, flags, peek=True)
  out = torch.zeros(6, dtype=torch.int32, device=pm.device)
  rc = lib().mm_offdiag_stats(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B, flags,
                              ws.data_ptr(), ws.numel(), out.data_ptr(), _stream(pm.device))
  check(rc, "mm_offdiag_stats")
  return int(out[3])


def offdiag_worklist_len(pm: PackedModel, B: int, flags: int) -> int:
  """Items the last ``moment_match`` / ``Q_reduce_forward`` with this B and flags put on the persistent off-diagonal sweep's work
  list: those with a tile to visit (``mm_offdiag_worklist_len``; float32 packs with d <= 8 and M <= 2048, else 0).  Synchronises."""
  if pm.dtype != torch.float32 or pm.L < 2 or not (flags & MM_FULL_OUTPUT_COV):
    return 0
  ws = pm.workspace(B, flags, peek=True)
  out = torch.zeros(1, dtype=torch.int32, device=pm.device)
  rc = lib().mm_offdiag_worklist_len(pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B, flags, ws.data_ptr(), ws.numel(),
                                     out.data_ptr(), _stream(pm.device))
  check(rc, "mm_offdiag_worklist_len")
  return int(out[0])


def offdiag_skip_bounds(pm: PackedModel, B: int, flags: int):
  """(zt2s [L, Mp/32], gmax2s [B, P - L, Mp/64]) float32: the column and row factors of the lengthscale-scaled Cauchy-Schwarz
  bound the float32 off-diagonal sweep skips tiles by, as the pack and the last ``q_forward`` / ``moment_match`` with this B and
  flags left them (``mm_offdiag_skip_bounds``; float32 packs with d <= 8)."""
  Mp = (pm.M + _lib.MM_M_ALIGN - 1) // _lib.MM_M_ALIGN * _lib.MM_M_ALIGN
  Po = pm.L * (pm.L - 1) // 2 if (flags & MM_FULL_OUTPUT_COV) else 0
  zt2s = torch.zeros(pm.L, Mp // 32, dtype=torch.float32, device=pm.device)
  gmax2s = torch.zeros(B, Po, Mp // 64, dtype=torch.float32, device=pm.device)
  ws = pm.workspace(B, flags, peek=True)
  rc = lib().mm_offdiag_skip_bounds(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B, flags,
                                    ws.data_ptr(), ws.numel(), zt2s.data_ptr(), gmax2s.data_ptr(), _stream(pm.device))
  check(rc, "mm_offdiag_skip_bounds")
  return zt2s, gmax2s


def route_estimates(pm: PackedModel, B: int, flags: int) -> torch.Tensor:
  """[B, P - L, 2] float64: per (batch element, off-diagonal pair) the last sweep's estimate of its own f32 rounding error and the
  scale it is compared with (``mm_route_estimates``; float32 packs)."""
  Po = pm.L * (pm.L - 1) // 2 if (flags & MM_FULL_OUTPUT_COV) else 0
  out = torch.zeros(B, Po, 2, dtype=torch.float64, device=pm.device)
  if Po:
    ws = pm.workspace(B, flags, peek=True)
    rc = lib().mm_route_estimates(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B, flags,
                                  ws.data_ptr(), ws.numel(), out.data_ptr(), _stream(pm.device))
    check(rc, "mm_route_estimates")
  return out


def euler_update(mu, Sigma, f1, Sff, cross_pre, dt: float = 1.0):
  """MomentMatchingEuler.step on the GPU (d == L)."""
  _require_device(mu, Sigma, f1, Sff, cross_pre)
  B, d = mu.shape
  if f1.shape != (B, d) or Sff.shape != (B, d, d) or cross_pre.shape != (B, d, d):
    raise ValueError("euler_update needs d == L and a full output covariance")
  args = [t.contiguous() for t in (mu, Sigma, f1, Sff, cross_pre)]
  mu_o, S_o = torch.empty_like(args[0]), torch.empty_like(args[1])
  rc = lib().mm_euler_update(B, d, _dtype_code(mu.dtype), float(dt), *[t.data_ptr() for t in args],
                             mu_o.data_ptr(), S_o.data_ptr(), _stream(mu.device))
  check(rc, "mm_euler_update")
  return mu_o, S_o


def rollout_closed(pm: PackedModel, mu: torch.Tensor, Sigma: torch.Tensor, num_steps: int,
                   dt: float = 1.0, model_uncertainty: bool = True, jitter: float = 0.0,
                   keep_trajectory: bool = False, force_generic: bool = False):
  """Drift-only moment-matched rollout, H steps enqueued back-to-back (state dim == d == L).

  Returns (mu_H, Sigma_H) or (mu_H, Sigma_H, traj_mu [H,B,d], traj_Sigma [H,B,d,d]).
  The inputs are not modified.
  """
  B, mu, Sigma = _prep_state(pm, mu, Sigma)
  mu, Sigma = mu.clone(), Sigma.clone()
  flags = make_flags(True, model_uncertainty, force_generic)
  ws = pm.workspace(B, flags)
  tmu = tS = None
  if keep_trajectory:
    tmu = torch.empty(num_steps, B, pm.d, dtype=pm.dtype, device=pm.device)
    tS = torch.empty(num_steps, B, pm.d, pm.d, dtype=pm.dtype, device=pm.device)
  rc = lib().mm_rollout_closed(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B,
                               int(num_steps), float(dt), flags, float(jitter),
                               mu.data_ptr(), Sigma.data_ptr(), _ptr(tmu), _ptr(tS),
                               ws.data_ptr(), ws.numel(), pm.status().data_ptr(), _stream(pm.device))
  check(rc, "mm_rollout_closed")
  return (mu, Sigma, tmu, tS) if keep_trajectory else (mu, Sigma)


class GraphedRollout:
  """``rollout_closed`` captured once into a HIP graph and replayed (hipGraph through
  ``torch.cuda.CUDAGraph``): small configurations (C1: B = 1, M ~ 100) are launch-latency bound --
  7 kernels per step, each a few microseconds -- and the graph removes the per-launch host cost.

  The shapes (B, H), flags and the packed model are frozen at construction; ``__call__`` copies
  (mu, Sigma) into static buffers, replays, and returns the static output buffers (valid until the
  next call; clone to keep).  The device-side non-PD flag is still written: ``pm.check_status(B)``.
  """

  def __init__(self, pm: PackedModel, B: int, num_steps: int, dt: float = 1.0, model_uncertainty: bool = True,
               jitter: float = 0.0, keep_trajectory: bool = False):
    if pm.L != pm.d:
      raise ValueError("closed rollout needs state dim == d == L")
    self.pm, self.B, self.H = pm, int(B), int(num_steps)
    kw = dict(dtype=pm.dtype, device=pm.device)
    self.mu_in, self.S_in = torch.zeros(B, pm.d, **kw), torch.eye(pm.d, **kw).expand(B, pm.d, pm.d).contiguous()
    self.mu, self.S = torch.empty(B, pm.d, **kw), torch.empty(B, pm.d, pm.d, **kw)
    self.tmu = torch.empty(num_steps, B, pm.d, **kw) if keep_trajectory else None
    self.tS = torch.empty(num_steps, B, pm.d, pm.d, **kw) if keep_trajectory else None
    flags = make_flags(True, model_uncertainty, False)
    self._flags = flags
    ws = pm.workspace(B, flags)
    status = pm.status()

    def enqueue():
      self.mu.copy_(self.mu_in); self.S.copy_(self.S_in)
      rc = lib().mm_rollout_closed(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), self.B,
                                   self.H, float(dt), flags, float(jitter),
                                   self.mu.data_ptr(), self.S.data_ptr(), _ptr(self.tmu), _ptr(self.tS),
                                   ws.data_ptr(), ws.numel(), status.data_ptr(), _stream(pm.device))
      check(rc, "mm_rollout_closed")

    side = torch.cuda.Stream(device=pm.device)          # warm-up off the capture (module load, lazy init)
    side.wait_stream(torch.cuda.current_stream(pm.device))
    with torch.cuda.stream(side):
      enqueue()
    torch.cuda.current_stream(pm.device).wait_stream(side)
    torch.cuda.synchronize(pm.device)
    status.zero_()
    self.graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(self.graph):
      enqueue()

  def __call__(self, mu: torch.Tensor, Sigma: torch.Tensor):
    if tuple(mu.shape) != (self.B, self.pm.d) or tuple(Sigma.shape) != (self.B, self.pm.d, self.pm.d):
      raise ValueError(f"graph was captured for B={self.B}, d={self.pm.d}")
    _require_device(mu, Sigma)
    self.mu_in.copy_(mu); self.S_in.copy_(Sigma)
    self.pm.workspace(self.B, self._flags)                 # the replay overwrites it: counts as a use (workspace_generation)
    self.graph.replay()
    return (self.mu, self.S, self.tmu, self.tS) if self.tmu is not None else (self.mu, self.S)


class _ComposedFamily(NamedTuple):
  """One family of native composed-rollout entries (include/gpflowpilco_mm.h): its four roles, its three size queries, and what
  sets its argument lists apart from the other families'."""
  name: str
  forward: str
  taped: str
  backward: str
  seeded: str               # the reverse sweep that takes seeds on the taped states after g_cost
  compose_ws: str           # size queries: all take (B[, H], nx, na, the family's extra dims, ...)
  tape_bytes: str
  backward_ws: str
  head_arrays: bool         # head constants: nu and two arrays of nu doubles (else two doubles by value)
  mix: bool                 # mix_W, mix_c trail the forward and the taped entry, mix_W the sweep -- which is seeded only
  latent_axis: bool         # g_policy is [B, nu, npar] and backward_ws also takes the policy's M (else [B, npar])
  plain: str                # the family without mixing: errors name its entries, and the tape's slots are its compose workspaces


_COMPOSED = {
    "one": _ComposedFamily("one", "mm_rollout_composed", "mm_rollout_composed_taped", "mm_rollout_composed_backward",
                           "mm_rollout_composed_backward_seeded", "mm_compose_workspace_bytes", "mm_compose_tape_bytes",
                           "mm_compose_backward_workspace_bytes", head_arrays=False, mix=False, latent_axis=False, plain="one"),
    "nd": _ComposedFamily("nd", "mm_rollout_composed_nd", "mm_rollout_composed_taped_nd", "mm_rollout_composed_backward_nd",
                          "mm_rollout_composed_backward_nd_seeded", "mm_compose_nd_workspace_bytes", "mm_compose_tape_bytes_nd",
                          "mm_compose_backward_workspace_bytes_nd", head_arrays=True, mix=False, latent_axis=True, plain="nd"),
    "nd_mixed": _ComposedFamily("nd_mixed", "mm_rollout_composed_nd_mixed", "mm_rollout_composed_taped_nd_mixed",
                                "mm_rollout_composed_backward_nd_mixed", "mm_rollout_composed_backward_nd_mixed",
                                "mm_compose_nd_mixed_workspace_bytes", "mm_compose_tape_bytes_nd_mixed",
                                "mm_compose_backward_workspace_bytes_nd_mixed", head_arrays=True, mix=True, latent_axis=True,
                                plain="nd"),
    # 8 < ne <= 16 in the gradient: the forward, the tape and their size queries are the _nd family's (general in ne), the reverse
    # sweep and its size query are the wide entries (csrc/mm_compose_bwd_nd.hip)
    "wide": _ComposedFamily("wide", "mm_rollout_composed_nd", "mm_rollout_composed_taped_nd", "mm_compose_wide_backward",
                            "mm_compose_wide_backward_seeded", "mm_compose_nd_workspace_bytes", "mm_compose_tape_bytes_nd",
                            "mm_compose_backward_workspace_bytes_wide", head_arrays=True, mix=False, latent_axis=True, plain="wide"),
    "wide_mixed": _ComposedFamily("wide_mixed", "mm_rollout_composed_nd_mixed", "mm_rollout_composed_taped_nd_mixed",
                                  "mm_compose_wide_backward_mixed", "mm_compose_wide_backward_mixed_seeded",
                                  "mm_compose_nd_mixed_workspace_bytes", "mm_compose_tape_bytes_nd_mixed",
                                  "mm_compose_backward_workspace_bytes_wide_mixed", head_arrays=True, mix=True, latent_axis=True,
                                  plain="wide"),
}


class ComposedRollout:
  """The whole moment-matched policy rollout of the cartpole-shaped system on the device (``mm_rollout_composed``):
  TrigonometricEncoder -> policy (SVGP mean, Chain[Scale, Shift, NormalCDF]) -> drift SVGP with the
  ``forward_sde`` cross-covariance bookkeeping -> Euler moment update -> per-step expected cost.

  ``drift`` / ``policy``: PackedModel (drift with C; policy with one latent per action, ``nu = policy.L``).  ``nu == 1`` is
  ``mm_rollout_composed``; ``nu > 1`` (up to 4 actions) ``mm_rollout_composed_nd`` (csrc/mm_compose_nd.hip: the head's cross
  moments are bivariate normal CDFs); ``taped`` / ``backward`` are one-action, ``taped_nd`` / ``backward_nd`` the tape and reverse
  sweep for 1 to 4 actions (csrc/mm_compose_bwd_nd.hip).  ``head_scale`` / ``head_shift``: a float or one value per action.
  ``__call__(mx, Sxx, H)`` returns ``(mx_H, Sxx_H, cost [B, H])`` (and the trajectory if asked); the inputs are not modified.
  ``taped_wide`` / ``backward_wide``: the same tape and the wide reverse sweep (``mm_compose_wide_backward*``) for up to 16
  encoded dims, where ``taped_nd`` / ``backward_nd`` stop at 8 (``supports_backward_wide``).

  ``mix_W`` [nx, Lg] (and optionally ``mix_c`` [nx]): the drift is coregionalised -- ``drift`` packs its Lg <= nx latents (with C, no
  mean) and its outputs are f = W g + c, mixed on the device after every drift match (csrc/mm_mix.h).  Such a rollout (``mixed``)
  takes the ``_nd_mixed`` entries for any nu, one action included: ``__call__``, ``taped_nd`` / ``backward_nd`` and the size queries;
  ``taped`` / ``backward`` (the one-action entries) do not take it.

  The three entry families are described once (``_COMPOSED``); every public method picks one and hands it to the one
  implementation of its role (``_forward``, ``_taped``, ``_sweep``, the size queries: ``_bytes``).
  """

  def __init__(self, drift: PackedModel, policy: PackedModel, nx: int, active_dims, head_scale, head_shift,
               target: torch.Tensor, precis: torch.Tensor, mix_W: Optional[torch.Tensor] = None,
               mix_c: Optional[torch.Tensor] = None):
    self.drift, self.policy = drift, policy
    self.mixed = mix_W is not None
    if mix_c is not None and mix_W is None:
      raise ValueError("mix_c without mix_W")
    self.nx, self.active = int(nx), tuple(int(i) for i in active_dims)
    self.na = len(self.active)
    self.ne = self.nx + self.na
    self.nu = int(policy.L)
    self.nd = self.ne + self.nu
    if drift.dtype != policy.dtype:
      raise TypeError("drift and policy must be packed with the same dtype")
    self._mixing = ()                                    # what trails a mixed entry's arguments: (mix_W, mix_c | NULL)
    if self.mixed:
      if mix_W.ndim != 2 or mix_W.shape[0] != self.nx or mix_W.shape[1] != drift.L:
        raise ValueError(f"mix_W must be [nx = {self.nx}, Lg = {drift.L}] (the drift pack's latents), got {tuple(mix_W.shape)}")
      if drift.L > self.nx:
        raise ValueError(f"a coregionalised drift with more latents than outputs (Lg = {drift.L} > nx = {self.nx}) is not taken")
      if mix_c is not None and mix_c.numel() != self.nx:
        raise ValueError(f"mix_c must have nx = {self.nx} entries")
      self.mix_W = mix_W.detach().to(dtype=torch.float64, device=drift.device).contiguous()
      self.mix_c = None if mix_c is None else mix_c.detach().to(dtype=torch.float64, device=drift.device).reshape(-1).contiguous()
      self._mixing = (self.mix_W.data_ptr(), _ptr(self.mix_c))
    if (not self.mixed and drift.L != self.nx) or drift.d != self.nd or policy.d != self.ne:
      raise ValueError(f"shapes do not compose: drift L={drift.L} d={drift.d} (want {self.nx}, {self.nd}), "
                       f"policy L={policy.L} d={policy.d} (want {self.nu}, {self.ne})")
    if not drift.with_C:
      raise ValueError("the drift is evaluated with model uncertainty: pack it with C")
    if self.nu == 1:
      self.scale, self.shift = float(head_scale), float(head_shift)
      scales, shifts = (self.scale,), (self.shift,)
    else:
      self.scale, self.shift = scales, shifts = self._per_action(head_scale, "head_scale"), self._per_action(head_shift, "head_shift")
    self.target = target.to(dtype=drift.dtype, device=drift.device).contiguous()
    self.precis = precis.to(dtype=drift.dtype, device=drift.device).contiguous()
    self._act = (_lib.C.c_int32 * self.na)(*self.active)
    # what of an entry's argument list never changes, built once (``drift``, ``target``, ``precis``, ``mix_W`` / ``mix_c`` and the head
    # constants are fixed after construction: their device pointers are read here, and a later reassignment would go unseen --
    # build a new rollout instead, as ``loops.current_roll`` does): the drift pack, and (nx, na, active dims, head, target, precision)
    # with the head constants in the two forms the entries take them -- ``head_arrays``: nu and two arrays, else (one action) two floats
    self._drift_args = (drift.buf.data_ptr(), drift.nbytes, drift.L, drift.M, drift.d)
    cost_args = (self.target.data_ptr(), self.precis.data_ptr())
    heads = {True: (self.nu, (_lib.C.c_double * self.nu)(*scales), (_lib.C.c_double * self.nu)(*shifts))}
    if self.nu == 1:
      heads[False] = (self.scale, self.shift)
    self._consts = {arrays: (self.nx, self.na, self._act, *head, *cost_args) for arrays, head in heads.items()}
    # the dims a family's size queries take after (nx, na), by family name; the family this rollout runs in, and the one its
    # _nd methods take
    self._dims = {"one": (), "nd": (self.nu,), "nd_mixed": (self.nu, int(drift.L)), "wide": (self.nu,),
                  "wide_mixed": (self.nu, int(drift.L))}
    self._nd_family = _COMPOSED["nd_mixed" if self.mixed else "nd"]
    self._wide_family = _COMPOSED["wide_mixed" if self.mixed else "wide"]
    # the differentiable ops (autodiff.ComposedRolloutFunction / ComposedTrajectoryFunction) tape and sweep through the wide family
    self.use_wide = False
    self._family = self._nd_family if self.uses_nd else _COMPOSED["one"]
    self._wsc = {}

  def _per_action(self, v, name):
    """A float (the same for every action) or a length-nu sequence / tensor -> tuple of nu floats."""
    if isinstance(v, torch.Tensor):
      v = v.detach().cpu().tolist()
    vals = tuple(float(t) for t in v) if hasattr(v, "__len__") else (float(v),) * self.nu
    if len(vals) != self.nu:
      raise ValueError(f"{name}: expected a float or {self.nu} values (one per action), got {len(vals)}")
    return vals

  @property
  def uses_nd(self) -> bool:
    """The rollout runs in the ``_nd`` family (several actions, or a coregionalised drift with any number of actions)."""
    return self.nu > 1 or self.mixed

  # ---- the size queries and the argument lists of the three families ---------------------------------------------------------
  def _bytes(self, fam: _ComposedFamily, query: str, lead: tuple, tail: tuple) -> int:
    """``query`` (compose_ws / tape_bytes / backward_ws) of ``fam``: (lead.., nx, na, the family's extra dims, tail..) -> bytes;
    0: the shape is refused."""
    return getattr(lib(), getattr(fam, query))(*lead, self.nx, self.na, *self._dims[fam.name], *tail)

  def _tape_bytes(self, fam, B, H, code):
    return self._bytes(fam, "tape_bytes", (B, H), (self.drift.M, code))

  def _backward_ws_bytes(self, fam, B, policy_M):
    return self._bytes(fam, "backward_ws", (B,), (self.drift.M, policy_M) if fam.latent_axis else (self.drift.M,))

  def _prefix(self, fam, pol, B, H, dt):
    """What every entry's argument list begins with: the drift and policy packs, the dims, the head and the cost constants."""
    return (*self._drift_args, pol.buf.data_ptr(), pol.nbytes, pol.M, pol.d, _dtype_code(self.drift.dtype), B, H, float(dt),
            *self._consts[fam.head_arrays])

  def _forward_call(self, fam, pol, B, H, dt, mx, Sxx, cost, tmu, tS, wd, wp, wc, status, stream):
    """(entry name, arguments) of the forward rollout on prepared buffers; so ``_taped_call`` / ``_sweep_call`` for their roles."""
    return fam.forward, (*self._prefix(fam, pol, B, H, dt), mx.data_ptr(), Sxx.data_ptr(), cost.data_ptr(), _ptr(tmu), _ptr(tS),
                         wd.data_ptr(), wd.numel(), wp.data_ptr(), wp.numel(), wc.data_ptr(), wc.numel(),
                         status.data_ptr(), stream, *(self._mixing if fam.mix else ()))

  def _taped_call(self, fam, pol, B, H, dt, mx, Sxx, cost, wd, wp, tape, status, stream):
    return fam.taped, (*self._prefix(fam, pol, B, H, dt), mx.data_ptr(), Sxx.data_ptr(), cost.data_ptr(),
                       wd.data_ptr(), wd.numel(), wp.data_ptr(), wp.numel(), tape.data_ptr(), tape.numel(),
                       status.data_ptr(), stream, *(self._mixing if fam.mix else ()))

  def _sweep_call(self, fam, pol, B, H, dt, tape, g_cost, seeds, g_pol, g_m, g_S, wd, wb, status, stream):
    """``seeds``: None (the unseeded entry) or (g_xm | None, g_xS | None).  The ``_nd_mixed`` sweep always takes the seeded
    signature (it has no unseeded entry)."""
    if fam.mix and seeds is None and fam.backward == fam.seeded:
      seeds = (None, None)
    return (fam.backward if seeds is None else fam.seeded,
            (*self._prefix(fam, pol, B, H, dt), tape.data_ptr(), tape.numel(), g_cost.data_ptr(),
             *(() if seeds is None else (_ptr(seeds[0]), _ptr(seeds[1]))), g_pol.data_ptr(), _ptr(g_m), _ptr(g_S),
             wd.data_ptr(), wd.numel(), wb.data_ptr(), wb.numel(), status.data_ptr(), stream, *(self._mixing[:1] if fam.mix else ())))

  # ---- one implementation per role ------------------------------------------------------------------------------------------
  def _compose_ws(self, fam, B, fresh=False):
    """The compose workspace of ``fam``: the one this rollout keeps per B for its own family, or a ``fresh`` one."""
    ws = None if fresh else self._wsc.get(B)
    if ws is None:
      n = self._bytes(fam, "compose_ws", (B,), (_dtype_code(self.drift.dtype),))
      if n == 0:
        raise ValueError(f"{_COMPOSED[fam.plain].compose_ws if fresh else 'mm_compose_workspace_bytes'} rejected the shape")
      ws = torch.empty(n, dtype=torch.uint8, device=self.drift.device)
      if not fresh:
        self._wsc[B] = ws
    return ws

  def _policy_pack(self, policy: Optional[PackedModel]) -> PackedModel:
    """``policy`` (another pack of the same shape: the current parameters of a trainable policy) or ``self.policy``; a pack
    of another (L, M, d, dtype) would be read through the wrong layout -- the C side only sees a byte count."""
    pol = self.policy if policy is None else policy
    if (pol.L, pol.M, pol.d, pol.dtype) != (self.policy.L, self.policy.M, self.policy.d, self.policy.dtype):
      raise ValueError("the policy pack does not have the shape this rollout was built for")
    return pol

  def _check_state(self, mx: torch.Tensor, Sxx: torch.Tensor) -> int:
    _require_device(mx, Sxx)
    dt_ = self.drift.dtype
    if mx.dtype != dt_ or Sxx.dtype != dt_:
      raise TypeError(f"state dtype {mx.dtype} / {Sxx.dtype} does not match the packed models ({dt_})")
    B = mx.shape[0]
    if mx.shape != (B, self.nx) or Sxx.shape != (B, self.nx, self.nx):
      raise ValueError(f"expected mx [B,{self.nx}], Sxx [B,{self.nx},{self.nx}]")
    return B

  def _forward(self, fam, pol, mx, Sxx, num_steps, dt, keep_trajectory, fresh_ws=False):
    """The forward rollout through ``fam``.  ``fresh_ws`` (``call_nd_entry``: ``fam`` need not be the family this rollout runs in):
    on a compose workspace of its own -- the kept one may be the other family's -- and reported under the plain family's name."""
    B = self._check_state(mx, Sxx)
    dt_ = self.drift.dtype
    mx, Sxx = mx.contiguous().clone(), Sxx.contiguous().clone()
    H = int(num_steps)
    cost = torch.empty(H, B, dtype=dt_, device=mx.device)
    tmu = torch.empty(H, B, self.nx, dtype=dt_, device=mx.device) if keep_trajectory else None
    tS = torch.empty(H, B, self.nx, self.nx, dtype=dt_, device=mx.device) if keep_trajectory else None
    wd = self.drift.workspace(B, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)
    wp = pol.workspace(B, MM_FULL_OUTPUT_COV)
    wc = self._compose_ws(fam, B, fresh=fresh_ws)
    entry, args = self._forward_call(fam, pol, B, H, dt, mx, Sxx, cost, tmu, tS, wd, wp, wc, self.drift.status(),
                                     _stream(mx.device))
    check(getattr(lib(), entry)(*args), _COMPOSED[fam.plain].forward if fresh_ws else entry)
    out = (mx, Sxx, cost.T.contiguous())
    return out + (tmu, tS) if keep_trajectory else out

  def _taped(self, fam, mx, Sxx, num_steps, dt, policy):
    """The taped forward through ``fam``: -> (mx_H, Sxx_H, cost [H, B], tape)."""
    pol = self._policy_pack(policy)
    dt_ = self.drift.dtype
    B, H = self._check_state(mx, Sxx), int(num_steps)
    if fam.latent_axis:
      why = self.backward_wide_refusal() if fam is self._wide_family else self.backward_nd_refusal()
      if why is not None:
        raise ValueError(why)
    mx, Sxx = mx.contiguous().clone(), Sxx.contiguous().clone()
    cost = torch.empty(H, B, dtype=dt_, device=mx.device)
    tape = torch.empty(self._tape_bytes(fam, B, H, _dtype_code(dt_)), dtype=torch.uint8, device=mx.device)
    wd = self.drift.workspace(B, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)
    wp = pol.workspace(B, MM_FULL_OUTPUT_COV)
    entry, args = self._taped_call(fam, pol, B, H, dt, mx, Sxx, cost, wd, wp, tape, self.drift.status(), _stream(mx.device))
    check(getattr(lib(), entry)(*args), _COMPOSED[fam.plain].taped)
    return mx, Sxx, cost, tape

  def _sweep(self, fam, tape, g_cost, B, num_steps, dt, policy, want_state_grad, g_traj):
    """The reverse sweep through ``fam``, seeded with ``g_traj`` or not: -> (g_policy, g_mx0 | None, g_Sxx0 | None)."""
    pol = self._policy_pack(policy)
    dev = tape.device
    H = int(num_steps)
    f64 = torch.float64
    g_cost = g_cost.to(f64).contiguous()
    if g_cost.shape != (H, B):
      raise ValueError(f"g_cost must be [H={H}, B={B}]")
    seeds = None if g_traj is None else self._seeds(g_traj, H, B)
    npar = pol.M * pol.d + pol.M + pol.d + 2
    g_pol = torch.empty((B, self.nu, npar) if fam.latent_axis else (B, npar), dtype=f64, device=dev)
    g_m = torch.empty(B, self.nx, dtype=f64, device=dev) if want_state_grad else None
    g_S = torch.empty(B, self.nx, self.nx, dtype=f64, device=dev) if want_state_grad else None
    wd = self.drift.workspace(B, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)
    plain = _COMPOSED[fam.plain]
    key = ("bwd_wide" if fam is self._wide_family else "bwd_nd" if fam.latent_axis else "bwd", B)
    wb = self._wsc.get(key)
    if wb is None:
      n = self._backward_ws_bytes(fam, B, pol.M)
      if n == 0:
        raise ValueError(f"{plain.backward_ws} rejected the shape")
      wb = torch.empty(n, dtype=torch.uint8, device=dev)
      self._wsc[key] = wb
    entry, args = self._sweep_call(fam, pol, B, H, dt, tape, g_cost, seeds, g_pol, g_m, g_S, wd, wb, self.drift.status(),
                                   _stream(dev))
    check(getattr(lib(), entry)(*args), plain.backward)
    return g_pol, g_m, g_S

  def _seeds(self, g_traj, H, B):
    """``g_traj`` of ``backward`` / ``backward_nd`` as contiguous f64 tensors of the tape's shapes (``(None, None)`` passes the
    seeded entry null seeds)."""
    g_xm, g_xS = g_traj
    if (g_xm is None) != (g_xS is None):
      raise ValueError("g_traj: both seeds or neither")
    if g_xm is None:
      return None, None
    g_xm, g_xS = g_xm.to(torch.float64).contiguous(), g_xS.to(torch.float64).contiguous()
    if g_xm.shape != (H, B, self.nx) or g_xS.shape != (H, B, self.nx, self.nx):
      raise ValueError(f"g_traj must be (g_xm [H={H}, B={B}, {self.nx}], g_xS [H, B, {self.nx}, {self.nx}])")
    return g_xm, g_xS

  # ---- forward -------------------------------------------------------------------------------------------------------------
  def __call__(self, mx: torch.Tensor, Sxx: torch.Tensor, num_steps: int, dt: float = 1.0, keep_trajectory: bool = False,
               policy: Optional[PackedModel] = None):
    """``policy``: another pack of the same shape to evaluate instead of ``self.policy`` (the current parameters of a
    trainable policy, packed by the caller)."""
    return self._forward(self._family, self._policy_pack(policy), mx, Sxx, num_steps, dt, keep_trajectory)

  def call_nd_entry(self, mx: torch.Tensor, Sxx: torch.Tensor, num_steps: int, dt: float = 1.0):
    """The same rollout through ``mm_rollout_composed_nd`` whatever nu is (a one-action rollout normally takes
    ``mm_rollout_composed``): -> (mx_H, Sxx_H, cost [B, H]).  The two entries must agree for nu == 1."""
    return self._forward(self._nd_family, self.policy, mx, Sxx, num_steps, dt, False, fresh_ws=True)

  # ---- differentiable form: tape + reverse sweep (csrc/mm_compose_bwd.hip) -------------------------------------------
  BACKWARD_MAX_POLICY_M = 256

  def supports_backward(self) -> bool:
    """The native reverse sweep exists for one-action f64 rollouts whose policy has M <= 256 centres on ne <= 8 encoded
    dims (one workgroup per batch element sweeps the policy's M x M block from LDS: 120 KB at M = 256, ne = 8)."""
    return (self.nu == 1 and not self.mixed and self.drift.dtype == torch.float64
            and self.policy.M <= self.BACKWARD_MAX_POLICY_M and self.ne <= 8)

  def _one_action_family(self):
    if self.nu != 1:
      raise NotImplementedError("the tape and the native reverse sweep are one-action (supports_backward() is False)")
    if self.mixed:
      raise NotImplementedError("a coregionalised drift takes taped_nd / backward_nd (the one-action entries do not mix)")
    return _COMPOSED["one"]

  def taped(self, mx: torch.Tensor, Sxx: torch.Tensor, num_steps: int, dt: float = 1.0, policy: Optional[PackedModel] = None):
    """``mm_rollout_composed_taped``: -> (mx_H, Sxx_H, cost [H, B], tape).  ``policy``: another pack of the same shape
    (the current parameters of a trainable policy)."""
    return self._taped(self._one_action_family(), mx, Sxx, num_steps, dt, policy)

  def backward(self, tape: torch.Tensor, g_cost: torch.Tensor, B: int, num_steps: int, dt: float = 1.0,
               policy: Optional[PackedModel] = None, want_state_grad: bool = True, g_traj=None):
    """``mm_rollout_composed_backward``: g_cost [H, B] -> (g_policy [B, M d + M + d + 2], g_mx0 [B,nx] | None,
    g_Sxx0 [B,nx,nx] | None): the gradient w.r.t. the packed policy (Z, beta, lengthscales^2, variance, mean) per batch
    element and w.r.t. the initial state.  ``policy`` must be the pack the tape was recorded with (``taped(policy=...)``).
    ``g_traj = (g_xm [H,B,nx], g_xS [H,B,nx,nx])``: seeds d loss / d (m_{h+1}, S_{h+1}) on the taped states, added to the sweep's
    carry beside the built-in cost's adjoint (``mm_rollout_composed_backward_seeded``)."""
    return self._sweep(self._one_action_family(), tape, g_cost, B, num_steps, dt, policy, want_state_grad, g_traj)

  def tape_states(self, tape: torch.Tensor, B: int, num_steps: int):
    """The states x_1 .. x_H a taped rollout left on its tape: -> (xm [H, B, nx], xS [H, B, nx, nx]), float64 copies."""
    H = int(num_steps)
    fam = self._wide_family if self.use_wide else self._family
    n = self._tape_bytes(fam, B, H, MM_F64)
    slot = self._bytes(_COMPOSED[fam.plain], "compose_ws", (B,), (MM_F64,))
    if n == 0 or tape.numel() < n or tape.dtype != torch.uint8:
      raise ValueError("not a tape of this rollout")
    # MMTapeLayout (csrc/mm_compose.h): H + 1 slots, then x_0 .. x_H means and covariances, each block aligned to 256 bytes
    nx, align = self.nx, lambda v: (v + 255) // 256 * 256
    off_m = (H + 1) * slot
    off_S = align(off_m + (H + 1) * B * nx * 8)
    xm = tape[off_m:off_m + (H + 1) * B * nx * 8].view(torch.float64).view(H + 1, B, nx)
    xS = tape[off_S:off_S + (H + 1) * B * nx * nx * 8].view(torch.float64).view(H + 1, B, nx, nx)
    return xm[1:].clone(), xS[1:].clone()

  # ---- the same for 1 to 4 actions (csrc/mm_compose_nd.hip, csrc/mm_compose_bwd_nd.hip) -----------------------------------
  def backward_nd_refusal(self) -> Optional[str]:
    """Why ``taped_nd`` / ``backward_nd`` do not take this rollout (None: they do)."""
    if self.drift.dtype != torch.float64:
      return "the multi-action tape and reverse sweep are float64 only"
    if self._backward_ws_bytes(self._nd_family, 1, self.policy.M) == 0:
      return (f"the policy (M = {self.policy.M} centres on ne = {self.ne} dims, {self.nu} actions) is past the LDS bound of the "
              "multi-action reverse sweep (M <= 256, ne <= 8 and 160 KB of LDS per workgroup: M <= 166 at ne = 8)")
    return None

  def supports_backward_nd(self) -> bool:
    """The multi-action tape and reverse sweep (``taped_nd`` / ``backward_nd``) take this rollout: f64, policy M <= 256 centres
    on ne <= 8 encoded dims, up to 4 actions, inside the sweep's LDS bound (``backward_nd_refusal`` names the reason if not)."""
    return self.backward_nd_refusal() is None

  def tape_bytes_nd(self, B: int, num_steps: int) -> int:
    """Size of the tape ``taped_nd`` records (``mm_compose_tape_bytes_nd`` / ``_nd_mixed``; 0: shape refused)."""
    return self._tape_bytes(self._nd_family, B, int(num_steps), _dtype_code(self.drift.dtype))

  def taped_nd(self, mx: torch.Tensor, Sxx: torch.Tensor, num_steps: int, dt: float = 1.0, policy: Optional[PackedModel] = None):
    """``mm_rollout_composed_taped_nd``: -> (mx_H, Sxx_H, cost [H, B], tape), for any nu in 1..4."""
    return self._taped(self._nd_family, mx, Sxx, num_steps, dt, policy)

  def backward_nd(self, tape: torch.Tensor, g_cost: torch.Tensor, B: int, num_steps: int, dt: float = 1.0,
                  policy: Optional[PackedModel] = None, want_state_grad: bool = True, g_traj=None):
    """``mm_rollout_composed_backward_nd``: g_cost [H, B] -> (g_policy [B, nu, M d + M + d + 2], g_mx0 [B,nx] | None,
    g_Sxx0 [B,nx,nx] | None): per batch element and latent the gradient w.r.t. the packed policy (Z, beta, lengthscales^2,
    variance, mean), and the gradient w.r.t. the initial state.  ``policy`` must be the pack the tape was recorded with.
    ``g_traj``: seeds on the taped states as in ``backward`` (``mm_rollout_composed_backward_nd_seeded``)."""
    return self._sweep(self._nd_family, tape, g_cost, B, num_steps, dt, policy, want_state_grad, g_traj)

  # ---- the same for 8 < ne <= 16 encoded dims: the tape of the _nd family, the wide reverse sweep --------------------------------
  WIDE_MAX_NE = 16

  def max_policy_M_wide(self) -> int:
    """The largest number of policy centres the wide reverse sweep takes at this rollout's (ne, nu): its LDS bound (0: none)."""
    for M in range(self.BACKWARD_MAX_POLICY_M, 0, -1):
      if self._backward_ws_bytes(self._wide_family, 1, M):
        return M
    return 0

  def backward_wide_refusal(self) -> Optional[str]:
    """Why ``taped_wide`` / ``backward_wide`` do not take this rollout (None: they do)."""
    if self.drift.dtype != torch.float64:
      return "the wide tape and reverse sweep are float64 only"
    if self.ne > self.WIDE_MAX_NE:
      return f"encoded dim ne = {self.ne} > {self.WIDE_MAX_NE} (the wide reverse sweep takes ne <= {self.WIDE_MAX_NE})"
    if self._backward_ws_bytes(self._wide_family, 1, self.policy.M) == 0:
      return (f"the policy (M = {self.policy.M} centres on ne = {self.ne} dims, {self.nu} actions) is past the LDS bound of the "
              f"wide reverse sweep (M <= 256 and 160 KB of LDS per workgroup: M <= {self.max_policy_M_wide()} at these dims)")
    return None

  def supports_backward_wide(self) -> bool:
    """The wide reverse sweep (``taped_wide`` / ``backward_wide``) takes this rollout: f64, ne <= 16 (ne <= 8 included), up to 4
    actions, policy M <= 256 inside the sweep's LDS bound (``backward_wide_refusal`` names the reason if not)."""
    return self.backward_wide_refusal() is None

  def taped_wide(self, mx: torch.Tensor, Sxx: torch.Tensor, num_steps: int, dt: float = 1.0, policy: Optional[PackedModel] = None):
    """``taped_nd`` for the shapes ``backward_wide`` takes (the tape is the ``_nd`` family's): -> (mx_H, Sxx_H, cost [H, B], tape)."""
    return self._taped(self._wide_family, mx, Sxx, num_steps, dt, policy)

  def backward_wide(self, tape: torch.Tensor, g_cost: torch.Tensor, B: int, num_steps: int, dt: float = 1.0,
                    policy: Optional[PackedModel] = None, want_state_grad: bool = True, g_traj=None):
    """``mm_compose_wide_backward`` (``_seeded`` with ``g_traj``; ``_mixed`` for a coregionalised drift): ``backward_nd`` for
    ne <= 16 encoded dims, with the same results' shapes."""
    return self._sweep(self._wide_family, tape, g_cost, B, num_steps, dt, policy, want_state_grad, g_traj)


class GraphedComposedRollout:
  """``ComposedRollout`` captured once into a HIP graph (``torch.cuda.CUDAGraph``) and replayed: at cartpole sizes
  (B = 1) a composed step is ~16 launches of a few microseconds each, and the eager path is paced by the host
  enqueueing them.  Shapes (B, H) are frozen at construction; ``__call__`` copies (mx, Sxx) into static buffers,
  replays, and returns static outputs ``(mx_H, Sxx_H, cost [B, H])`` (valid until the next call)."""

  def __init__(self, roll: ComposedRollout, B: int, num_steps: int, dt: float = 1.0):
    self.roll, self.B, self.H = roll, int(B), int(num_steps)
    kw = dict(dtype=roll.drift.dtype, device=roll.drift.device)
    self.mx_in = torch.zeros(B, roll.nx, **kw)
    self.S_in = torch.eye(roll.nx, **kw).expand(B, roll.nx, roll.nx).contiguous() * 1e-2
    dev = roll.drift.device
    side = torch.cuda.Stream(device=dev)                  # warm-up off the capture (module load, workspaces)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      roll(self.mx_in, self.S_in, self.H, dt=dt)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    roll.drift.status().zero_()
    self.graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(self.graph):
      self.out = roll(self.mx_in, self.S_in, self.H, dt=dt)

  def __call__(self, mx: torch.Tensor, Sxx: torch.Tensor):
    if tuple(mx.shape) != (self.B, self.roll.nx):
      raise ValueError(f"graph was captured for B={self.B}, nx={self.roll.nx}")
    self.mx_in.copy_(mx); self.S_in.copy_(Sxx)
    self.roll.drift.workspace(self.B, MM_FULL_OUTPUT_COV | MM_MODEL_UNCERTAINTY)      # (see GraphedRollout.__call__)
    self.graph.replay()
    return self.out


def expected_cost(mean: torch.Tensor, cov: torch.Tensor, target: torch.Tensor, precis: torch.Tensor):
  """GaussianObjective expected cost on the GPU: mean [...,d], cov [...,d,d] -> [...]."""
  _require_device(mean, cov, target, precis)
  d = mean.shape[-1]
  lead = mean.shape[:-1]
  m2 = mean.reshape(-1, d).contiguous()
  c2 = cov.reshape(-1, d, d).contiguous().to(mean.dtype)
  out = torch.empty(m2.shape[0], dtype=mean.dtype, device=mean.device)
  rc = lib().mm_expected_cost(m2.shape[0], d, _dtype_code(mean.dtype), m2.data_ptr(), c2.data_ptr(),
                              target.to(mean).contiguous().data_ptr(), precis.to(mean).contiguous().data_ptr(),
                              out.data_ptr(), _stream(mean.device))
  check(rc, "mm_expected_cost")
  return out.reshape(lead)


def backward_supported(pm: PackedModel) -> bool:
  """Whether ``moment_match_backward`` runs on this pack itself (else: on a float64 pack of the same model)."""
  return pm.dtype == torch.float64 or bool(lib().mm_bwd_f32_supported(pm.d))


def backward_workspace_bytes(pm: PackedModel, B: int, flags: int) -> int:
  return lib().mm_moment_match_backward_bytes_dtype(B, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), flags)


def moment_match_with_sums(pm: PackedModel, mu: torch.Tensor, Sigma: torch.Tensor, full_output_cov: bool = True,
                           model_uncertainty: bool = True, jitter: float = 0.0):
  """``mm_moment_match_with_sums``: the outputs of ``moment_match`` computed from the q stage and the BACKWARD's M x M sweeps
  (whose sums do not depend on the incoming gradient and contain the forward's), which stay on the returned buffer: the
  matching ``moment_match_backward(..., sums=buffer)`` is then the chain rule alone -- value and gradient for one pair of
  sweeps instead of two (C3 shape: 38 instead of 49 ms).  Returns (f1, Sff, cross_pre, sums, generation)."""
  if not backward_supported(pm):
    raise NotImplementedError("float32 packs with d > 8 differentiate through a float64 pack of the model")
  B, mu, Sigma = _prep_state(pm, mu, Sigma)
  flags = make_flags(full_output_cov, model_uncertainty)
  f1 = torch.empty(B, pm.L, dtype=pm.dtype, device=pm.device)
  Sff = torch.zeros((B, pm.L, pm.L) if full_output_cov else (B, pm.L), dtype=pm.dtype, device=pm.device)
  cross = torch.empty(B, pm.d, pm.L, dtype=pm.dtype, device=pm.device)
  if B == 0:
    return f1, Sff, cross, None, 0
  ws = pm.workspace(B, flags)
  wb = torch.empty(backward_workspace_bytes(pm, B, flags), dtype=torch.uint8, device=pm.device)   # owned by the caller's tape
  rc = lib().mm_moment_match_with_sums(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B, mu.data_ptr(),
                                       Sigma.data_ptr(), flags, float(jitter), f1.data_ptr(), Sff.data_ptr(), cross.data_ptr(),
                                       ws.data_ptr(), ws.numel(), wb.data_ptr(), wb.numel(), pm.status().data_ptr(),
                                       _stream(pm.device))
  check(rc, "mm_moment_match_with_sums")
  return f1, Sff, cross, wb, pm.workspace_generation(B, flags)


def moment_match_backward(pm: PackedModel, mu: torch.Tensor, Sigma: torch.Tensor, g_f1: torch.Tensor, g_Sff: torch.Tensor,
                          g_cross: torch.Tensor, full_output_cov: bool = True, model_uncertainty: bool = True,
                          forward_generation: Optional[int] = None, stages: int = 0, sums: Optional[torch.Tensor] = None):
  """``mm_moment_match_backward``: the vector-Jacobian product of one moment match of a frozen pack,
  (g_f1 [B,L], g_Sff [B,L,L] | [B,L], g_cross [B,d,L]) -> (g_mu [B,d], g_Sigma [B,d,d] symmetric), gradients in float64.
  float64 packs: f64 sweeps for every pair; float32 packs with d <= 8 (``backward_supported``): f64 for the diagonal
  pairs, moment + bf16-MFMA aggregates for the off-diagonal pairs (csrc/mm_bwd_f32.hip).
  ``stages`` (``MM_STAGE_*``, measurement only): run just those parts of the backward on what earlier calls left behind.
  ``sums``: the buffer ``moment_match_with_sums`` returned for exactly this (mu, Sigma, flags): chain rule alone."""
  if not backward_supported(pm):
    raise NotImplementedError("float32 packs with d > 8 differentiate through a float64 pack of the model")
  B, mu, Sigma = _prep_state(pm, mu, Sigma)
  flags = make_flags(full_output_cov, model_uncertainty)
  f64 = torch.float64
  g_f1, g_Sff, g_cross = (t.to(f64).contiguous() for t in (g_f1, g_Sff, g_cross))
  # forward_generation: pm.workspace_generation(B, flags) right after the forward of THIS match (same mu, Sigma, flags): if
  # nobody has asked for the workspace since, its q stage is still there and is not run again (MM_WORKSPACE_CURRENT)
  if B == 0:                        # an empty batch has an empty gradient (as the forward returns empty outputs); no launch
    return (torch.empty(0, pm.d, dtype=f64, device=pm.device), torch.empty(0, pm.d, pm.d, dtype=f64, device=pm.device))
  current = (forward_generation is not None and forward_generation > 0
             and forward_generation == pm.workspace_generation(B, flags))
  ws = pm.workspace(B, flags, peek=current)
  key = ("bwd", B, flags)
  wb = sums if sums is not None else pm._workspaces.get(key)
  if wb is None:
    wb = torch.empty(backward_workspace_bytes(pm, B, flags), dtype=torch.uint8, device=pm.device)
    pm._workspaces[key] = wb
  if sums is not None:
    if sums.numel() < backward_workspace_bytes(pm, B, flags) or sums.device != pm.device:
      raise ValueError("`sums` is not the buffer moment_match_with_sums returned for this pack, batch and flags")
    stages |= MM_SUMS_CURRENT
  g_mu = torch.empty(B, pm.d, dtype=f64, device=pm.device)
  g_S = torch.empty(B, pm.d, pm.d, dtype=f64, device=pm.device)
  rc = lib().mm_moment_match_backward(pm.buf.data_ptr(), pm.nbytes, pm.L, pm.M, pm.d, _dtype_code(pm.dtype), B, mu.data_ptr(), Sigma.data_ptr(),
                                      flags | (MM_WORKSPACE_CURRENT if current else 0) | stages, g_f1.data_ptr(), g_Sff.data_ptr(),
                                      g_cross.data_ptr(), g_mu.data_ptr(),
                                      g_S.data_ptr(), 0, ws.data_ptr(), ws.numel(), wb.data_ptr(), wb.numel(),
                                      pm.status().data_ptr(), _stream(pm.device))
  check(rc, "mm_moment_match_backward")
  return g_mu, g_S


def _gram_operands(X: Optional[torch.Tensor], Z: torch.Tensor, ls: torch.Tensor, var: torch.Tensor):
  """Checked, contiguous float64 operands of the Gram entries and (L, M, N, d); ``X`` None is the self mode (N = M)."""
  _require_device(X, Z, ls, var)
  if Z.ndim != 3 or ls.shape != (Z.shape[0], Z.shape[2]) or var.shape != (Z.shape[0],):
    raise ValueError(f"gram_se: Z [L,M,d], ls [L,d], var [L] expected, got {tuple(Z.shape)}, {tuple(ls.shape)}, {tuple(var.shape)}")
  L, M, d = Z.shape
  if X is not None:
    if X.requires_grad:
      raise ValueError("gram_se: the data X are constants (the adjoint has no gradient with respect to X)")
    if X.ndim != 2 or X.shape[1] != d:
      raise ValueError(f"gram_se: X [N,{d}] expected, got {tuple(X.shape)}")
  f64 = torch.float64
  ops_ = [None if t is None else t.detach().to(f64).contiguous() for t in (X, Z, ls, var)]
  return ops_, (L, M, M if X is None else X.shape[0], d)


def gram_se(X: Optional[torch.Tensor], Z: torch.Tensor, ls: torch.Tensor, var: torch.Tensor) -> torch.Tensor:
  """``mm_gram_se``: K [L,M,N] = var_l exp(-1/2 |(x_n - z_lm) / ls_l|^2) in float64, the squared distance from differences
  (csrc/mm_gram.hip).  X [N,d] (None: ``gram_se_self``), Z [L,M,d], ls [L,d], var [L].  Not differentiable by itself:
  ``autodiff.GramSEFunction``."""
  (X, Z, ls, var), (L, M, N, d) = _gram_operands(X, Z, ls, var)
  K = torch.empty(L, M, N, dtype=torch.float64, device=Z.device)
  check(lib().mm_gram_se(L, M, N, d, _ptr(X), Z.data_ptr(), ls.data_ptr(), var.data_ptr(), K.data_ptr(), _stream(Z.device)),
        "mm_gram_se")
  return K


def gram_se_self(Z: torch.Tensor, ls: torch.Tensor, var: torch.Tensor) -> torch.Tensor:
  """K [L,M,M] = k_l(Z_l, Z_l): symmetric to the bit, diagonal exactly var_l (no jitter)."""
  return gram_se(None, Z, ls, var)


def gram_se_backward(G: torch.Tensor, X: Optional[torch.Tensor], Z: torch.Tensor, ls: torch.Tensor, var: torch.Tensor):
  """``mm_gram_se_backward``: G [L,M,N] -> (gZ [L,M,d], gls [L,d], gvar [L]); K is recomputed from the operands.  X None: the self
  mode, G a general [L,M,M] matrix, the derivative through both argument slots.  Deterministic: two calls are bit-equal."""
  (X, Z, ls, var), (L, M, N, d) = _gram_operands(X, Z, ls, var)
  _require_device(G)
  if G.shape != (L, M, N):
    raise ValueError(f"gram_se_backward: G [{L},{M},{N}] expected, got {tuple(G.shape)}")
  G = G.detach().to(torch.float64).contiguous()
  nbytes = lib().mm_gram_workspace_bytes(L, M, N, d)
  ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=Z.device)
  gZ, gls, gvar = torch.empty_like(Z), torch.empty_like(ls), torch.empty_like(var)
  check(lib().mm_gram_se_backward(L, M, N, d, G.data_ptr(), _ptr(X), Z.data_ptr(), ls.data_ptr(), var.data_ptr(), gZ.data_ptr(),
                                  gls.data_ptr(), gvar.data_ptr(), ws.data_ptr(), ws.numel(), _stream(Z.device)),
        "mm_gram_se_backward")
  return gZ, gls, gvar


_PREDICT_WS: Dict[Tuple[int, int, int, str], torch.Tensor] = {}      # (L, M, d, device) -> the K strips of mm_predict_se


def predict_se(X: torch.Tensor, Z: torch.Tensor, ls: torch.Tensor, var: torch.Tensor, beta: torch.Tensor,
               C: Optional[torch.Tensor] = None, mean_c: Optional[torch.Tensor] = None):
  """``mm_predict_se`` (csrc/mm_predict.hip): mean [N,L] = K^T beta (+ mean_c) and var [N,L] = var_l + k^T C k of SE-ARD latents at the
  points X [N,d], in float64, K formed tile by tile (no [M,N] buffer) and the symmetric C [L,M,M] read on and below its block
  diagonal only.  Z [L,M,d], ls [L,d], var [L], beta [L,M]; ``C`` None: the mean alone, the second result is None.  Runs on the
  current stream and can be captured once the workspace of this (L, M, d) exists (it is cached: call once before capturing).
  Deterministic: two calls are bit-equal.  Not differentiable."""
  _require_device(X, Z, ls, var, beta, C, mean_c)
  if Z.ndim != 3 or ls.shape != (Z.shape[0], Z.shape[2]) or var.shape != (Z.shape[0],) or beta.shape != Z.shape[:2]:
    raise ValueError(f"predict_se: Z [L,M,d], ls [L,d], var [L], beta [L,M] expected, got {tuple(Z.shape)}, {tuple(ls.shape)}, "
                     f"{tuple(var.shape)}, {tuple(beta.shape)}")
  L, M, d = Z.shape
  if X.ndim != 2 or X.shape[1] != d:
    raise ValueError(f"predict_se: X [N,{d}] expected, got {tuple(X.shape)}")
  if C is not None and C.shape != (L, M, M):
    raise ValueError(f"predict_se: C [{L},{M},{M}] expected, got {tuple(C.shape)}")
  if mean_c is not None and mean_c.shape != (L,):
    raise ValueError(f"predict_se: mean_c [{L}] expected, got {tuple(mean_c.shape)}")
  for name, t in (("X", X), ("Z", Z), ("ls", ls), ("var", var), ("beta", beta), ("C", C), ("mean_c", mean_c)):
    if t is not None and t.dtype != torch.float64:
      raise ValueError(f"predict_se: {name} is {t.dtype}; MM_E_DTYPE: the predictive kernel is float64 only")
  N = X.shape[0]
  X, Z, ls, var, beta, C, mean_c = (None if t is None else t.detach().contiguous() for t in (X, Z, ls, var, beta, C, mean_c))
  nbytes = lib().mm_predict_workspace_bytes(L, M, max(N, 1), d)
  if nbytes == 0:
    check(-2, "mm_predict_workspace_bytes")      # the size query's 0 is MM_E_DIM
  key = (L, M, d, str(Z.device))
  ws = _PREDICT_WS.get(key)
  if ws is None or ws.numel() < nbytes:
    ws = _PREDICT_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=Z.device)
  mean = torch.empty(N, L, dtype=torch.float64, device=Z.device)
  fvar = None if C is None else torch.empty(N, L, dtype=torch.float64, device=Z.device)
  if N == 0:
    return mean, fvar
  check(lib().mm_predict_se(L, M, N, d, X.data_ptr(), Z.data_ptr(), ls.data_ptr(), var.data_ptr(), beta.data_ptr(), _ptr(C),
                            _ptr(mean_c), mean.data_ptr(), _ptr(fvar), ws.data_ptr(), ws.numel(), _stream(Z.device)),
        "mm_predict_se")
  return mean, fvar


_GRAM_STATS_WS: Dict[Tuple[int, int, int, int, str], torch.Tensor] = {}      # (L, M, d, Q, device) -> the workspace of mm_gram_stats_se*


def _gram_stats_operands(who: str, X, R, Z, ls, var):
  """Checked, contiguous float64 operands of the streamed Gram statistics, (L, M, N, d, Q) and the cached workspace."""
  _require_device(X, R, Z, ls, var)
  if Z.ndim != 3 or ls.shape != (Z.shape[0], Z.shape[2]) or var.shape != (Z.shape[0],):
    raise ValueError(f"{who}: Z [L,M,d], ls [L,d], var [L] expected, got {tuple(Z.shape)}, {tuple(ls.shape)}, {tuple(var.shape)}")
  L, M, d = Z.shape
  if X.requires_grad or (R is not None and R.requires_grad):
    raise ValueError(f"{who}: the data X and R are constants (the adjoint has no gradient with respect to them)")
  if X.ndim != 2 or X.shape[1] != d:
    raise ValueError(f"{who}: X [N,{d}] expected, got {tuple(X.shape)}")
  N = X.shape[0]
  if R is not None and (R.ndim != 2 or R.shape[0] != N):
    raise ValueError(f"{who}: R [{N},Q] expected, got {tuple(R.shape)}")
  Q = 0 if R is None else R.shape[1]
  if Q == 0:
    R = None
  nbytes = lib().mm_gram_stats_workspace_bytes(L, M, N, d, Q)
  if nbytes == 0:
    check(-2, "mm_gram_stats_workspace_bytes")      # the size query's 0 is MM_E_DIM
  key = (L, M, d, Q, str(Z.device))
  ws = _GRAM_STATS_WS.get(key)
  if ws is None or ws.numel() < nbytes:
    ws = _GRAM_STATS_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=Z.device)
  ops_ = [None if t is None else t.detach().to(torch.float64).contiguous() for t in (X, R, Z, ls, var)]
  return ops_, (L, M, N, d, Q), ws


def gram_stats_se(X: torch.Tensor, R: Optional[torch.Tensor], Z: torch.Tensor, ls: torch.Tensor, var: torch.Tensor):
  """``mm_gram_stats_se`` (csrc/mm_gram_stats.hip): Phi [L,M,M] = K K^T and Psi [L,M,Q] = K R of the SE-ARD Gram matrix K [L,M,N]
  between X [N,d] and Z [L,M,d] (``gram_se``'s entries), in float64, K formed tile by tile and never stored: no buffer grows with
  N.  ``R`` None (or with no column): Phi alone, the second result is None.  Phi is symmetric to the bit.  Deterministic: two calls
  are bit-equal.  Not differentiable by itself: ``autodiff.GramStatsSEFunction``."""
  (X, R, Z, ls, var), (L, M, N, d, Q), ws = _gram_stats_operands("gram_stats_se", X, R, Z, ls, var)
  Phi = torch.empty(L, M, M, dtype=torch.float64, device=Z.device)
  Psi = None if R is None else torch.empty(L, M, Q, dtype=torch.float64, device=Z.device)
  check(lib().mm_gram_stats_se(L, M, N, d, Q, X.data_ptr(), _ptr(R), Z.data_ptr(), ls.data_ptr(), var.data_ptr(), Phi.data_ptr(),
                               _ptr(Psi), ws.data_ptr(), ws.numel(), _stream(Z.device)), "mm_gram_stats_se")
  return Phi, Psi


def gram_stats_se_backward(GPhi: torch.Tensor, GPsi: Optional[torch.Tensor], X: torch.Tensor, R: Optional[torch.Tensor],
                           Z: torch.Tensor, ls: torch.Tensor, var: torch.Tensor):
  """``mm_gram_stats_se_backward``: GPhi [L,M,M] (any matrix: GPhi + GPhi^T is used) and GPsi [L,M,Q] -> (gZ [L,M,d], gls [L,d],
  gvar [L]) of ``gram_stats_se``; the adjoint of K, (GPhi + GPhi^T) K + GPsi R^T, is formed tile by tile and never stored.
  Deterministic: two calls are bit-equal."""
  (X, R, Z, ls, var), (L, M, N, d, Q), ws = _gram_stats_operands("gram_stats_se_backward", X, R, Z, ls, var)
  _require_device(GPhi, GPsi)
  if GPhi.shape != (L, M, M):
    raise ValueError(f"gram_stats_se_backward: GPhi [{L},{M},{M}] expected, got {tuple(GPhi.shape)}")
  if (GPsi is None) != (R is None) or (GPsi is not None and GPsi.shape != (L, M, Q)):
    raise ValueError(f"gram_stats_se_backward: GPsi [{L},{M},{Q}] with R, or neither, expected")
  GPhi = GPhi.detach().to(torch.float64).contiguous()
  GPsi = None if GPsi is None else GPsi.detach().to(torch.float64).contiguous()
  gZ, gls, gvar = torch.empty_like(Z), torch.empty_like(ls), torch.empty_like(var)
  check(lib().mm_gram_stats_se_backward(L, M, N, d, Q, GPhi.data_ptr(), _ptr(GPsi), X.data_ptr(), _ptr(R), Z.data_ptr(),
                                        ls.data_ptr(), var.data_ptr(), gZ.data_ptr(), gls.data_ptr(), gvar.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream(Z.device)), "mm_gram_stats_se_backward")
  return gZ, gls, gvar
