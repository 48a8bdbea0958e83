"""The kernels in front of and behind the bf16 convolutions on full-mantissa operands, every output held to the bound its
float64 reference implies: the ClusterNet5g stem (csrc/stem.hip, csrc/stem_bwd2.hip), the VGG first convolution
(csrc/firstconv2.hip and its first-generation fallback in csrc/vgg.hip) and the segmentation head with its unfused chain
(csrc/seg_head.hip).  pytest -m gpu.

tests/first_layer_f64_cases.py holds the draws, the references and the bounds, tests/parity.py the derivations
(fma_acc_bound, pooled_bracket, bf16_bracket); tests/test_first_layer_f64_cpu.py proves without a GPU that correct fp32
pipelines stay inside and that a truncating store, BatchNorm on a rounded conv output, sums or an arg-max taken from
rounded values, a doubly rounded dW operand, a partial rounded before its fold and a shortened accumulator do not --
defects that the lattice operands of tests/test_gpu_first_layer_exact.py and the older tolerances let through.  The
shapes are those of the exact tests (tests/lattice.py): every kernel family, the ragged segments, the first-generation
fallbacks, both weight-gradient kernels of the head.  No tolerance here is tuned.
"""
import json
import os

import pytest
import torch

from tests import first_layer_f64_cases as fc
from tests import lattice as L
from tests.lattice import record
from tests.parity import WORST, assert_bits, assert_in_bracket, assert_within, pool_s2p1
from tests.test_gpu_kernels import HOOKS, hook

pytestmark = pytest.mark.gpu


def dev():
  assert torch.cuda.is_available(), "no GPU visible"
  return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _worst_figures():
  """After the module: one FIGURES line per family (bound-only families: worst |err| / bound; bracket families: worst
  |got - ref| / (b + spacing), smallest decisive share, elements) -- the table of LAB.md S15.  IIC_PARITY_REPORT names
  a JSON file for the same."""
  yield
  rec = {k: (v if isinstance(v, dict) else {"ratio": v}) for k, v in WORST.items() if k.startswith("fl64")}
  for fam in sorted(rec):
    record(kind="first_layer_f64 worst", family=fam, **rec[fam])
  if os.environ.get("IIC_PARITY_REPORT"):
    with open(os.environ["IIC_PARITY_REPORT"], "w") as f:
      json.dump(rec, f, indent=1, sort_keys=True)


def _ring_zero(pt, P, what):
  o = pt.float()
  for name, edge in (("top", o[:, :P]), ("bottom", o[:, -P:]), ("left", o[:, :, :P]), ("right", o[:, :, -P:])):
    assert float(edge.abs().max()) == 0.0, "%s: %s ring of the PT tensor was written" % (what, name)


# ----------------------------------------------------------------------------------------------------------------------
# stem
# ----------------------------------------------------------------------------------------------------------------------
BCOEFS = ("G1", "G2", "G3", "general")


def _bcoef(s, which):
  return s["bcoef"] if which == "general" else fc.unit_bcoef(which)


def _check_dw(s, got, which, form, what):
  """Against the float64 dW, the patch's rounding charged; and, where x carries a full mantissa, against the float64 sums
  over bf16_rne(x) -- an input's rounding is known exactly -- without that charge."""
  bound = {"two-pass": fc.stem_dw_two_pass, "one-pass": fc.stem_dw_one_pass}[form]
  fam = "fl64 stem dW %s %s %s" % (form, which, s["draw"])
  ref, tol = bound(s, _bcoef(s, which))
  assert_within(got, ref, tol, "%s: %s dW, bcoef %s" % (what, form, which), fam)
  if s["draw"] == "full":
    ref, tol = bound(s, _bcoef(s, which), exact_patch=True)
    assert_within(got, ref, tol, "%s: %s dW, bcoef %s, against the sums over bf16_rne(x)" % (what, form, which), fam + " xh")


def _check_forward(s, what, coef=None):
  """stem_stats cells and stem_apply_pool on `coef` (default: the case's own)."""
  from iic_amd import ops
  cin, H, W, N = s["case"]
  d = dev()
  x, w = s["x"].to(d), s["w"].to(d)
  st = ops.new_stats(fc.CO, d)
  ops.stem_stats(x, w, st)
  got = ops.stats_decode(st, fc.CO).cpu()
  y = s["y"]
  assert_within(got[0], y.sum((0, 2, 3)), s["stat_tol"][0], what + ": stem_stats sum y", "fl64 stem S1")
  assert_within(got[1], (y * y).sum((0, 2, 3)), s["stat_tol"][1], what + ": stem_stats sum y^2", "fl64 stem S2")
  out = torch.zeros((N, H // 2 + 3, W // 2 + 3, fc.CO), dtype=torch.bfloat16, device=d)
  ops.stem_apply_pool(x, w, s["coef"].to(d) if coef is None else coef, out)
  torch.cuda.synchronize()
  return st, out


def _run_stem(case, draw, bwd2=True):
  from iic_amd import ops
  cin, H, W, N = case
  s = fc.stem(case, draw)
  what = "stem %r %s" % (case, draw)
  assert s["undecided_share"] <= fc.UNDECIDED_CAP and s["decisive"] >= fc.DECISIVE_FLOOR
  d = dev()
  x, w, coef = s["x"].to(d), s["w"].to(d), s["coef"].to(d)
  _, out = _check_forward(s, what)
  assert_in_bracket(ops.pt_to_nchw(out, 1).cpu(), s["pool_lo"], s["pool_hi"], what + ": stem_apply_pool", "fl64 stem pool",
                    ref=s["pool"], b=pool_s2p1(s["bz"]))
  _ring_zero(out, 1, what + ": stem_apply_pool")
  # backward sums
  dpp = ops.pt_from_nchw(s["dpool"].to(d), 1)
  sums = ops.new_stats(fc.CO, d)
  ops.stem_bwd_reduce(x, w, coef, dpp, sums)
  sg = ops.stats_decode(sums, fc.CO).cpu()
  assert_within(sg[0], s["sum_g"], s["tol_sum_g"], what + ": stem_bwd_reduce sum g", "fl64 stem sum g")
  assert_within(sg[1], s["sum_gy"], s["tol_sum_gy"], what + ": stem_bwd_reduce sum g*y", "fl64 stem sum g*y")
  ran = []
  # one-pass form first: its partials live in the buffer the two-pass form reuses
  if ops.stem_bwd_fused_ok(cin) and L.stem_width_served("bwd_fused", cin, W, bwd2):
    sums2 = ops.new_stats(fc.CO, d)
    h = ops.stem_bwd_fused(x, w, coef, dpp, sums2)
    sg2 = ops.stats_decode(sums2, fc.CO).cpu()
    assert_within(sg2[0], s["sum_g"], s["tol_sum_g"], what + ": stem_bwd_fused sum g", "fl64 stem sum g")
    assert_within(sg2[1], s["sum_gy"], s["tol_sum_gy"], what + ": stem_bwd_fused sum g*y", "fl64 stem sum g*y")
    # bit-equal on general operands too: both entry points run one routing code on one grid -- stem_bwd2_kernel with and
    # without its GEMMs, or stem_bwd_kernel<CIN, 2> and <CIN, 0> -- hence one order of the fp32 partial sums
    assert_bits(sg2, sg, what + ": the sums of stem_bwd_fused and stem_bwd_reduce")
    for which in BCOEFS:
      _check_dw(s, ops.stem_wgrad_combine(h, _bcoef(s, which).to(d), w), which, "one-pass", what)
    ran.append("bwd_fused")
  if L.stem_width_served("bwd_wgrad", cin, W):
    for which in BCOEFS:
      _check_dw(s, ops.stem_bwd_wgrad(x, w, coef, _bcoef(s, which).to(d), dpp), which, "two-pass", what)
    ran.append("bwd_wgrad")
  torch.cuda.synchronize()
  record(kernel="stem f64", case=list(case), draw=draw, ran=ran, undecided=s["undecided_share"], decisive=s["decisive"])


@pytest.mark.parametrize("draw", fc.STEM_DRAWS)
@pytest.mark.parametrize("case", L.STEM_CASES)
def test_stem_within_float64_bounds(case, draw):
  _run_stem(case, draw)


@HOOKS
@pytest.mark.parametrize("draw", fc.STEM_DRAWS)
def test_stem_fused_backward_fallback_within_float64_bounds(draw):
  """iic_debug_enable_stem_bwd2(0): iic_stem_bwd_fused runs stem_bwd_kernel<CIN, 2> at the flagship shape."""
  hook("iic_debug_enable_stem_bwd2", 0)
  try:
    _run_stem((2, 96, 96, 2), draw, bwd2=False)
  finally:
    hook("iic_debug_enable_stem_bwd2", 1)


@pytest.mark.parametrize("draw", fc.STEM_DRAWS)
@pytest.mark.parametrize("case", [(1, 24, 24, 3), (2, 96, 96, 2), (3, 4, 254, 2)])
def test_stem_fused_sums_equal_stem_bwd_reduce_bit_for_bit(case, draw):
  """The sums of iic_stem_bwd_fused against those of iic_stem_bwd_reduce, bit for bit, on general operands, where the
  register-resident kernel serves both (csrc/stem_bwd2.hip; (3, 4, 254, 2) is its widest image).  On the lattice any two
  summation orders agree; here they do only because iic_stem_bwd_reduce runs the same routing code on the same grid
  (stem_bwd2_kernel<CIN, false>: the sums without the dW GEMMs).  With stem_bwd_kernel<CIN, 0> behind that entry point --
  per-thread sums over windows, threads folded in index order, against per-lane sums folded by a shuffle and through
  LDS -- sum g*y differed in all 64 channels, by up to 4.9e-4 of its float64 bound at (1, 24, 24, 3)."""
  from iic_amd import ops
  s = fc.stem(case, draw)
  d = dev()
  x, w, coef = s["x"].to(d), s["w"].to(d), s["coef"].to(d)
  dpp = ops.pt_from_nchw(s["dpool"].to(d), 1)
  sums, sums2 = ops.new_stats(fc.CO, d), ops.new_stats(fc.CO, d)
  ops.stem_bwd_reduce(x, w, coef, dpp, sums)
  ops.stem_bwd_fused(x, w, coef, dpp, sums2)
  a, b = ops.stats_decode(sums, fc.CO).cpu(), ops.stats_decode(sums2, fc.CO).cpu()
  assert_within(a[1], s["sum_gy"], s["tol_sum_gy"], "stem_bwd_reduce sum g*y", "fl64 stem sum g*y")
  assert float(a[1].abs().max()) > 0
  assert_bits(b, a, "the sums of stem_bwd_fused and stem_bwd_reduce")


def test_stem_on_the_finalisers_own_coefficients():
  """ops.stem_stats -> ops.bn_finalize -> ops.stem_apply_pool: scale and shift as the kernels produce them; the reference
  is recomputed from the returned coef."""
  from iic_amd import ops
  case = (3, 64, 64, 2)
  cin, H, W, N = case
  s0 = fc.stem(case, "full")
  d = dev()
  st = ops.new_stats(fc.CO, d)
  ops.stem_stats(s0["x"].to(d), s0["w"].to(d), st)
  rng = torch.Generator().manual_seed(5)
  gamma = 1.0 + 0.2 * torch.randn(fc.CO, generator=rng)
  gamma[::7] = -gamma[::7]
  beta = 0.1 * torch.randn(fc.CO, generator=rng)
  coef = ops.bn_finalize(st, gamma.to(d), beta.to(d), None, None, None, fc.CO, N * H * W, True)
  torch.cuda.synchronize()
  s = fc.stem_reference(s0["x"], s0["w"], coef.cpu(), s0["dpool"], case)
  assert s["decisive"] >= fc.DECISIVE_FLOOR
  what = "stem %r on bn_finalize's coefficients" % (case,)
  _, out = _check_forward(s, what, coef=coef)
  assert_in_bracket(ops.pt_to_nchw(out, 1).cpu(), s["pool_lo"], s["pool_hi"], what, "fl64 stem pool finalised",
                    ref=s["pool"], b=pool_s2p1(s["bz"]))
  _ring_zero(out, 1, what)


# ----------------------------------------------------------------------------------------------------------------------
# first conv
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", fc.DRAWS)
@pytest.mark.parametrize("case", L.FIRSTCONV_CASES)
def test_firstconv_within_float64_bounds(case, draw):
  """Output bracket with the ring zero, S1 / S2 and dW; W % 4 != 0 takes the first-generation kernels."""
  from iic_amd import ops
  cin, K, H, W, N = case
  pad, P = (K - 1) // 2, 2
  s = fc.firstconv(case, draw)
  what = "firstconv %r %s" % (case, draw)
  d = dev()
  x = s["x"].to(d)
  out = torch.zeros((N, H + 2 * P, W + 2 * P, fc.CO), dtype=torch.bfloat16, device=d)
  st = ops.new_stats(fc.CO, d)
  ops.firstconv_fwd(x, s["w"].to(d), out, st, K, pad, P)
  torch.cuda.synchronize()
  assert_in_bracket(ops.pt_to_nchw(out, P).cpu(), s["lo"], s["hi"], what + ": output", "fl64 firstconv out " + draw,
                    ref=s["y"], b=s["b"])
  _ring_zero(out, P, what)
  got = ops.stats_decode(st, fc.CO).cpu()
  assert_within(got[0], s["y"].sum((0, 2, 3)), s["stat_tol"][0], what + ": sum y", "fl64 firstconv S1 " + draw)
  assert_within(got[1], (s["y"] ** 2).sum((0, 2, 3)), s["stat_tol"][1], what + ": sum y^2", "fl64 firstconv S2 " + draw)
  dW = ops.firstconv_wgrad(x, ops.pt_from_nchw(s["dy"].to(d), P), tuple(s["w"].shape), K, pad, P)
  torch.cuda.synchronize()
  assert_within(dW, s["dW"], s["tol_dW"], what + ": dW", "fl64 firstconv dW " + draw)
  record(kernel="firstconv f64", case=list(case), draw=draw, decisive=s["decisive"])


# ----------------------------------------------------------------------------------------------------------------------
# segmentation head
# ----------------------------------------------------------------------------------------------------------------------
def _seg_setup(case, draw):
  from iic_amd import ops
  C, k, N, Hf = case
  P = 3
  s = fc.seg_head(case, draw)
  d = dev()
  xp = ops.pt_from_nchw(s["f"].to(d), P)
  Hp = Hf + 2 * P
  geo = (N, Hf + 2, Hf + 2, Hp, Hp, P - 1)       # N, Hw, Ww, Hp, Wp, off as archs/seg.py::_head_probs derives them
  return s, xp, geo, P


def _check_dx(s, dx_pt, P, what, fam):
  from iic_amd import ops
  assert_in_bracket(ops.pt_to_nchw(dx_pt, P).cpu(), s["dx_lo"], s["dx_hi"], what, fam, ref=s["dx"], b=s["b_dx"])
  _ring_zero(dx_pt, P, what)


@pytest.mark.parametrize("draw", fc.DRAWS)
@pytest.mark.parametrize("case", L.SEG_HEAD_CASES)
def test_seg_head_within_float64_bounds(case, draw):
  """iic_seg_head_fwd / _bwd_dx / _wgrad called directly: logits over C terms, the dx bracket with the ring of the PT
  gradient exactly zero, dW with the chunk fold."""
  from iic_amd._lib import check, lib, ptr, stream_ptr
  C, k, N, Hf = case
  s, xp, geo, P = _seg_setup(case, draw)
  d, st, Lb = dev(), stream_ptr(), lib()
  M = s["M"]
  what = "seg head %r %s" % (case, draw)
  assert Lb.iic_seg_head_supported(C, k)
  w2 = s["w"].reshape(k, C).contiguous().to(d)
  dlog = s["dlog_rows"].float().to(d)
  logits = torch.zeros((M, k), device=d)
  check(Lb.iic_seg_head_fwd(ptr(xp), ptr(w2), ptr(logits), *geo, C, k, st), "iic_seg_head_fwd")
  assert_within(logits, s["logits"], s["tol_logits"], what + ": logits", "fl64 seg logits " + draw)
  dx = torch.zeros(tuple(xp.shape), dtype=torch.bfloat16, device=d)
  check(Lb.iic_seg_head_bwd_dx(ptr(dlog), ptr(w2), ptr(dx), *geo, C, k, st), "iic_seg_head_bwd_dx")
  torch.cuda.synchronize()
  _check_dx(s, dx, P, what + ": dx", "fl64 seg dx " + draw)
  nch = Lb.iic_seg_head_wgrad_chunks(M)
  assert nch == fc.seg_chunks(M)
  part = torch.zeros((nch, k * C), device=d)
  check(Lb.iic_seg_head_wgrad(ptr(dlog), ptr(xp), ptr(part), *geo, C, k, st), "iic_seg_head_wgrad")
  dW = torch.empty((k, C), device=d)
  check(Lb.iic_colsum_f32(ptr(part), ptr(dW), nch, k * C, 0, st), "iic_colsum_f32")
  torch.cuda.synchronize()
  assert_within(dW, s["dW"], fc.seg_dw_tol(s, nch), what + ": dW", "fl64 seg dW " + draw)
  record(kernel="seg head f64", case=list(case), draw=draw, chunks=nch, decisive=s["decisive"])


@pytest.mark.parametrize("draw", fc.DRAWS)
@pytest.mark.parametrize("case", L.SEG_CHAIN_CASES)
def test_seg_head_unfused_chain_within_float64_bounds(case, draw):
  """iic_seg_window_gather -> ops.gemm_f32 -> iic_gemm_f32_splitk / iic_seg_window_scatter: the same bounds, the
  scatter's RNE store in the bracket."""
  from iic_amd import ops
  from iic_amd._lib import check, lib, ptr, stream_ptr
  C, k, N, Hf = case
  s, xp, geo, P = _seg_setup(case, draw)
  d, st, Lb = dev(), stream_ptr(), lib()
  M = s["M"]
  what = "seg chain %r %s" % (case, draw)
  w2 = s["w"].reshape(k, C).contiguous().to(d)
  dlog = s["dlog_rows"].float().to(d)
  Fm = torch.zeros((M, C), device=d)
  check(Lb.iic_seg_window_gather(ptr(xp), ptr(Fm), *geo, C, st), "iic_seg_window_gather")
  logits = torch.zeros((M, k), device=d)
  ops.gemm_f32(Fm, C, 1, w2, 1, C, logits, k, M, k, C)
  assert_within(logits, s["logits"], s["tol_logits"], what + ": logits", "fl64 seg chain logits " + draw)
  dW = torch.zeros((k, C), device=d)
  splitk = max(1, min(512, M // 2048))
  check(Lb.iic_gemm_f32_splitk(ptr(dlog), 1, k, ptr(Fm), C, 1, ptr(dW), C, k, C, M, splitk, st), "iic_gemm_f32_splitk")
  torch.cuda.synchronize()
  assert_within(dW, s["dW"], fc.seg_dw_tol(s, splitk + 1), what + ": dW", "fl64 seg chain dW " + draw)
  dF = torch.zeros((M, C), device=d)
  ops.gemm_f32(dlog, k, 1, w2, C, 1, dF, C, M, C, k)
  dx = torch.zeros(tuple(xp.shape), dtype=torch.bfloat16, device=d)
  check(Lb.iic_seg_window_scatter(ptr(dF), ptr(dx), *geo, C, st), "iic_seg_window_scatter")
  torch.cuda.synchronize()
  _check_dx(s, dx, P, what + ": dx", "fl64 seg chain dx " + draw)
  record(kernel="seg chain f64", case=list(case), draw=draw, splitk=splitk, decisive=s["decisive"])
