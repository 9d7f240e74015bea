"""The f64 pack's moment match and its backward (row f-1) against a reference that shares no M x M code with the kernels:
tests.helpers.materialised_reference -- autodiff.moment_match_torch and its float64 autograd on the CPU, on the very
precompute() operands the pack was built from (no Kuu, no factorisation, no tiers, no packing order, no padding).

Every case checks value AND gradient.  The draws (tests.helpers.REFERENCE_DRAWS) are the smallest that select each launch
path of mm_backward_sums_impl and of the forward's f64 sweep, and between them put wave tiles in every range tier of the
factored diagonal sweeps, past the last one, and where e^b underflows; the further routes (MM_FORCE_GENERIC, MM_FORCE_WORST_TIER, value
and gradient from one pair of sweeps, the backward on the forward's q stage) run on a subset against the same reference.

Bar, for each of f1, Sff, cross, g_mu, g_Sigma:  max|got - want| <= max(1e-9, 100 x floor) x max|want|,  floor = the
reference's own conditioning floor on that draw (<= 1e-10 on every draw: tests/test_f64_reference_host.py), so no bar exceeds
1e-8.  1e-9 is three decades over the reference's typical floor -- room for another summation order over up to 600^2 terms
under the same cancellation.  The measured errors are in DESIGN.md section 8 f-1.

Three rows run the f32 pack (the only place k_bwd_diag<..., LOWP = true> meets an outside reference below M = 2000) at the
project's f32 bars, reference at the f32-rounded state."""
import pytest
import torch

from gpflowpilco_amd import _lib, ops
from tests.helpers import REFERENCE_DRAWS, contract_err, f32_state, materialised_reference, reference_draw, scale_err, to_dev

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAMES = ("f1", "Sff", "cross", "g_mu", "g_Sigma")
_CASES = {}


def _case(name, device, dtype=F64):
  """The draw on the device, its pack, and the reference with its floors: built once per (draw, pack type) and left unchanged."""
  key = (name, dtype)
  if key not in _CASES:
    syn, mu, S, g, full, unc = reference_draw(name, device)
    if dtype == torch.float32:
      mu, S = f32_state(mu, S)
    model = syn.to_model(device)
    pm = model.packed(dtype, unc, device)
    pre = model._cache._pre                                    # the float64 operands mm_pack_model received
    want, floors = materialised_reference(pre, mu, S, full, unc, *g, floor_trials=2 if dtype == F64 else 0)
    _CASES[key] = dict(pm=pm, mu=to_dev(mu, device, dtype), S=to_dev(S, device, dtype), g=[t.to(device) for t in g],
                       full=full, unc=unc, B=mu.shape[0], want=want, floors=floors)
  return _CASES[key]


def _assert_at_the_bar(name, route, got, c):
  errs = [scale_err(a_, b_.numpy()) for a_, b_ in zip(got, c["want"])]
  bars = [min(max(1e-9, 100.0 * f), 1e-8) for f in c["floors"]]
  print(f"f64ref {name} {route} " + " ".join(f"{n}={e:.2e}/{b:.0e}" for n, e, b in zip(NAMES, errs, bars))
        + f" value={max(errs[:3]):.2e} gradient={max(errs[3:]):.2e}")
  assert all(e <= b for e, b in zip(errs, bars)), (name, route, dict(zip(NAMES, errs)), bars)


def _run(c, route):
  pm, mu, S, g, full, unc, B = (c[k] for k in ("pm", "mu", "S", "g", "full", "unc", "B"))
  if route == "with_sums":      # value and gradient from one pair of sweeps
    f1, Sff, cross, sums, gen = ops.moment_match_with_sums(pm, mu, S, full, unc)
    gmu, gS = ops.moment_match_backward(pm, mu, S, *g, full, unc, forward_generation=gen, sums=sums)
  elif route == "q_stage_kept":  # the backward on the forward's q stage
    f1, Sff, cross = ops.moment_match(pm, mu, S, full, unc)
    gen = pm.workspace_generation(B, ops.make_flags(full, unc))
    gmu, gS = ops.moment_match_backward(pm, mu, S, *g, full, unc, forward_generation=gen)
  else:
    bit = {"default": 0, "generic": _lib.MM_FORCE_GENERIC, "worst_tier": _lib.MM_FORCE_WORST_TIER}[route]
    f1, Sff, cross = ops.moment_match(pm, mu, S, full, unc, extra_flags=bit)
    gmu, gS = ops.moment_match_backward(pm, mu, S, *g, full, unc, stages=bit)
  pm.check_status(B)
  return f1, Sff, cross, gmu, gS


@pytest.mark.parametrize("name", list(REFERENCE_DRAWS))
def test_f64_pack_value_and_gradient_equal_the_materialised_reference(name, device):
  c = _case(name, device)
  _assert_at_the_bar(name, "default", _run(c, "default"), c)


@pytest.mark.parametrize("name", ["diag_ks2", "diag_nounc", "ks3", "tiers", "ks8", "tiers_mid", "tiers_deep"])
def test_portable_kernels_equal_the_materialised_reference(name, device):
  """MM_FORCE_GENERIC: the VALU reduce of the forward and k_bwd_sums in the backward."""
  c = _case(name, device)
  _assert_at_the_bar(name, "generic", _run(c, "generic"), c)


@pytest.mark.parametrize("name", ["diag_ks2", "diag_nounc", "ks3", "tiers", "tiers_mid", "tiers_deep"])
@pytest.mark.parametrize("route", ["worst_tier", "with_sums", "q_stage_kept"])
def test_further_routes_equal_the_materialised_reference(route, name, device):
  """MM_FORCE_WORST_TIER: every forward tile through the any-argument e^x, the unfactored kernel for every pair of the backward;
  with_sums: mm_moment_match_with_sums, then the chain rule alone on its sums; q_stage_kept: MM_WORKSPACE_CURRENT."""
  c = _case(name, device)
  _assert_at_the_bar(name, route, _run(c, route), c)


@pytest.mark.parametrize("name", ["diag_ks2", "diag_nounc", "L1"])
def test_f32_pack_value_and_gradient_against_the_materialised_reference(name, device):
  """The f32 pack on the f32-rounded state, at the project's f32 bars: Sff by the accuracy contract (3e-4 of the off-diagonal
  block's scale, 2e-5 of the largest variance), f1 and cross 2e-6 (tests/test_gpu_parity.py), the gradient 1e-4 of its scale
  (tests/test_gpu_backward_f32.py)."""
  c = _case(name, device, torch.float32)
  f1, Sff, cross, gmu, gS = _run(c, "default")
  w_f1, w_Sff, w_cross, w_gmu, w_gS = (t.numpy() for t in c["want"])
  off, dia = contract_err(Sff, w_Sff)
  e_f1, e_cross, e_gmu, e_gS = scale_err(f1, w_f1), scale_err(cross, w_cross), scale_err(gmu, w_gmu), scale_err(gS, w_gS)
  print(f"f64ref {name} f32pack Sff_off={off:.2e}/3e-04 Sff_diag={dia:.2e}/2e-05 f1={e_f1:.2e}/2e-06 cross={e_cross:.2e}/2e-06 "
        f"g_mu={e_gmu:.2e}/1e-04 g_Sigma={e_gS:.2e}/1e-04")
  assert off < 3e-4 and dia < 2e-5, (off, dia)
  assert e_f1 < 2e-6 and e_cross < 2e-6, (e_f1, e_cross)
  assert e_gmu < 1e-4 and e_gS < 1e-4, (e_gmu, e_gS)
