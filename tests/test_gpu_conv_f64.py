"""The conv kernels on full-mantissa bf16 operands, every output element inside the bracket its float64 convolution
implies (tests/parity.py: conv_acc_bound, bf16_bracket, bf16_bracket_epilogue; tests/conv_f64_cases.py: the draws and the
statistic bounds; tests/test_conv_f64_cpu.py proves on the CPU that correct fp32 accumulation stays inside and that a
truncating store, a bf16-sized intermediate, a damaged mantissa bit, statistics from the rounded tile and a shortened
accumulator do not -- defects that the lattice operands of tests/test_gpu_conv_exact.py and the 1e-2 * max criterion of
tests/test_gpu_kernels.py both let through).

Everything runs through the product dispatch (ops.conv_igemm, ops.conv_wgrad, ops.PreppedWeights, ops.weight_prep); the
references are F.conv2d / torch.nn.grad.* in float64 on the bf16-rounded operands.  Operand `f32` (ops.fp32_mode()) stores
fp32: the accumulation bound alone applies there.  The only skips are geometries the library reports unsupported.

Kernel families the default dispatch reaches only at size are taken at the smallest shape that reaches them, and the
kernel that ran is asserted through iic_debug_conv_plan / iic_debug_wgrad_plan where the instrumented library is loaded
(tests/test_conv_f64_cpu.py asserts the default plans of the un-hooked shapes on the host):
  * the persistent 64 -> 64 kernel, 2 x 49 x 49 on a forced grid of 2 (9-10 tiles per workgroup);
  * 256-row tiles of the first-generation kernel (iic_debug_force_bm);
  * the stride-1 persistent kernel conv_igemm_pw.hip: by default it takes a launch of >= 2.5 tiles per workgroup slot,
    i.e. >= 1280 tiles of 256 rows -- a workload-size shape; iic_debug_enable_pw 2 puts 128 -> 128 on 20 x 25 x 25 (49
    tiles) on it, iic_debug_pw_gx_cap 1 makes each of its 8 workgroups walk 6 tiles with the statistics carried;
  * block tiles: 64 -> 128 on 1 x 33 x 82 with PT border 3, the smallest image for which conv_make_plan chooses them in
    both directions (forward 128-cout tiles, backward-data 64-cout tiles), reduced from the 40 x 640 of
    tests/test_gpu_conv_exact.py.

Non-finite operands: the class (finite / +inf / -inf / NaN) of every output equals the float64 reference's, the finite
ones stay in their brackets, and every channel's statistic cells decode to NaN (the poison counter).  Denormal operands
are left out: whether the matrix pipe flushes them is a property of the MFMA instruction's mode, not of these kernels.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_f64_cases as cc
from tests.conftest import hook
from tests.lattice import record
from tests.nonfinite_cases import cls as nonfinite_cls
from tests.parity import (BF16_MAX, U32, WORST, assert_in_bracket, assert_within, bf16_bracket, conv_acc_bound)
from tests.test_gpu_kernels import CONV_CASES

pytestmark = pytest.mark.gpu
HOOKS = pytest.mark.hooks

CASES = [cc.of(c) for c in CONV_CASES]
P64_FORCED = cc.Case(64, 64, 3, 1, 1, 2, 49)
PW_FORCED = cc.Case(128, 128, 3, 1, 1, 20, 25)
BLOCK_TILED = cc.Case(64, 128, 3, 1, 1, 1, 33, W=82, P=3)
CONV_NONE, CONV_P64, CONV_PW, CONV_BD = 0, 1, 2, 3          # csrc/conv_plan.h
W_REG, W_DMA, W_PL, W_PL2, W_B2D = 1, 2, 3, 4, 5


def dev():
  assert torch.cuda.is_available(), "no GPU visible"
  return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _worst_figures():
  """After the module: one FIGURES line per family (worst |got - ref| / (b + spacing), smallest decisive share; for
  bound-only families the worst |err| / bound) -- the table of LAB.md."""
  yield
  for fam in sorted(k for k in WORST if k.startswith("conv64")):
    w = WORST[fam]
    record(kind="conv_f64 worst", family=fam, **(w if isinstance(w, dict) else {"ratio": w}))


def _plan(g):
  from iic_amd import _lib
  out = (ctypes.c_int * 12)()
  ctypes.CDLL(_lib.LIB_PATH).iic_debug_conv_plan(ctypes.byref(g), out)
  return dict(zip(("kernel", "ms", "wn", "gather", "pad", "bw", "bh", "mtiles", "grid", "lds_a", "lds", "red_ok"), out))


def _wplan(g, use_tr):
  from iic_amd import _lib
  out = (ctypes.c_int * 28)()
  ctypes.CDLL(_lib.LIB_PATH).iic_debug_wgrad_plan(ctypes.byref(g), int(use_tr), out)
  return dict(kernel=out[0], bmk=out[5], nsplit=out[17])


def _has_hooks():
  from iic_amd import _lib
  return _lib.HAS_HOOKS


class _mode(object):
  """fp32_mode() for the exact-fp32 path, nothing for the bf16 product path."""

  def __init__(self, operand):
    self.f32 = operand == "f32"

  def __enter__(self):
    if self.f32:
      from iic_amd import ops
      self.ctx = ops.fp32_mode()
      self.ctx.__enter__()
    return self

  def __exit__(self, *exc):
    if self.f32:
      self.ctx.__exit__(*exc)
    return False


def _operand(case, w_dev, operand, bwd, geoms):
  """rows = the row-major bf16 operand of ops.weight_prep (first-generation kernel); frag = ops.PreppedWeights (the
  weights-direct kernels wherever ops.frag_supported); f32 = the parameter itself (exact-fp32 path)."""
  from iic_amd import ops
  if operand == "rows":
    return ops.weight_prep(w_dev)[1 if bwd else 0]
  if operand == "frag" and not all(ops.frag_supported(g) for g in geoms):
    assert not (case.cin == 64 and case.cout == 64 and case.K == 3 and case.s == 1), "64->64 3x3 must run on the persistent kernel"
    pytest.skip("geometry not served by the weights-direct kernels (library: iic_conv_igemm_frag_supported = 0)")
  return ops.PreppedWeights(w_dev)[1 if bwd else 0]


def _pt_dtype(operand):
  return torch.float32 if operand == "f32" else torch.bfloat16


def _borders_zero(pt, P, what):
  o = pt.float()
  for name, edge in (("top", o[:, :P]), ("bottom", o[:, -P:]), ("left", o[:, :, :P]), ("right", o[:, :, -P:])):
    assert float(edge.abs().max()) == 0.0, "%s: %s border of the PT tensor was written" % (what, name)


def _fam(kind, operand, draw):
  return "conv64 %s %s %s" % (kind, operand, draw)


# --------------------------------------------------------------------------------------
# forward + BatchNorm statistics
# --------------------------------------------------------------------------------------
def _forward(case, draw, operand, check_plan=None, tag=None):
  from iic_amd import geom, ops
  t = cc.inputs(case, draw)
  ref, b, lo, hi = cc.forward_bracket(case, draw)
  Ho, Wo = case.out_hw
  P = case.P
  with _mode(operand):
    g = geom.fwd_geom(case.spec, case.N, case.H, case.W, P, P)
    if check_plan:
      check_plan(g)
    wop = _operand(case, t["w"].to(dev()), operand, False, [g])
    xp = ops.pt_from_nchw(t["x"].to(dev()), P)
    out = torch.zeros((case.N, Ho + 2 * P, Wo + 2 * P, case.cout), dtype=_pt_dtype(operand), device=dev())
    stats = ops.new_stats(case.cout, dev())
    ops.conv_igemm(g, xp, wop, out, stats=stats)
    torch.cuda.synchronize()
  got = ops.pt_to_nchw(out, P).cpu()
  what = "forward %r %s %s" % (case, operand, draw)
  fam = _fam("forward", tag or operand, draw)
  if operand == "f32":
    assert_within(got, ref, b, what, fam)
  else:
    assert_in_bracket(got, lo, hi, what, fam, ref=ref, b=b)
  _borders_zero(out, P, what)
  st = ops.stats_decode(stats, case.cout).cpu()
  tol1, tol2 = cc.stat_bounds(ref, b, case.count)
  assert_within(st[0], ref.sum((0, 2, 3)), tol1, what + ": statistics, sum", _fam("S1", tag or operand, draw))
  assert_within(st[1], (ref * ref).sum((0, 2, 3)), tol2, what + ": statistics, sum of squares", _fam("S2", tag or operand, draw))


@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("operand", ["rows", "frag", "f32"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_forward_and_statistics_in_float64_brackets(case, operand, draw):
  _forward(case, draw, operand)


# --------------------------------------------------------------------------------------
# backward-data and its epilogues
# --------------------------------------------------------------------------------------
def _backward_data(case, draw, operand, check_plan=None, tag=None, epilogues=True):
  from iic_amd import geom, ops
  t = cc.inputs(case, draw)
  ref, b, lo, hi = cc.backward_data_bracket(case, draw)
  P = case.P
  fam = _fam("backward-data", tag or operand, draw)
  with _mode(operand):
    geoms = geom.bwd_data_geoms(case.spec, case.N, case.H, case.W, P, P)
    if check_plan:
      for g in geoms:
        check_plan(g)
    wop = _operand(case, t["w"].to(dev()), operand, True, geoms)
    dyp = ops.pt_from_nchw(t["dy"].to(dev()), P)
    pts = {k: ops.pt_from_nchw(t[k].to(dev()), P) for k in ("prev", "rg", "act")}

    def run(start, **kw):
      dx = start.clone() if start is not None else torch.zeros((case.N, case.H + 2 * P, case.W + 2 * P, case.cin),
                                                               dtype=_pt_dtype(operand), device=dev())
      for g in geoms:
        ops.conv_igemm(g, dyp, wop, dx, **kw)
      torch.cuda.synchronize()
      return dx

    what = "backward-data %r %s %s" % (case, operand, draw)
    dx = run(None)
    got = ops.pt_to_nchw(dx, P).cpu()
    if operand == "f32":
      assert_within(got, ref, b, what, fam)
    else:
      assert_in_bracket(got, lo, hi, what, fam, ref=ref, b=b)      # (pixels no geometry covers: ref = lo = hi = 0)
    _borders_zero(dx, P, what)
    if not (epilogues and geom.bwd_data_covers_all(case.spec)):
      return      # (1x1 stride 2: an epilogue only runs on the pixels its launch stores)
    for name, kw, reads in cc.EPILOGUES:
      kw = dict(kw)
      premask = kw.get("premask", False)
      if "rg" in reads:
        kw["res_grad"] = pts["rg"]
      if "act" in reads:
        kw["res_act"] = pts["act"]
      dx = run(pts["prev"] if "prev" in reads else None, **kw)
      got = ops.pt_to_nchw(dx, P).cpu()
      ewhat = "%s, epilogue '%s'" % (what, name)
      efam = fam + " epilogue"
      if operand == "f32":
        # fp32 store: value = acc [+ prev] [+ rg] in at most two fp32 additions; masked elements exactly zero
        prev = t["prev"].double() if "prev" in reads else torch.zeros_like(ref)
        keep = (t["act"] > 0) if "act" in reads else torch.ones_like(ref, dtype=torch.bool)
        rg = t["rg"].double() if "rg" in reads else torch.zeros_like(ref)
        if not premask:
          rg = torch.where(keep, rg, torch.zeros_like(rg))
        want = ref + prev + rg
        tol = b + 3 * U32 * (ref.abs() + b + prev.abs() + rg.abs())
        if premask:
          want, tol = torch.where(keep, want, torch.zeros_like(want)), torch.where(keep, tol, torch.zeros_like(tol))
        assert_within(got, want, tol, ewhat, efam)
      else:
        lo2, hi2 = cc.epilogue_bracket(lo, hi, t, reads, premask)
        assert_in_bracket(got, lo2, hi2, ewhat, efam)
      _borders_zero(dx, P, ewhat)


@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("operand", ["rows", "frag", "f32"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_backward_data_and_epilogues_in_float64_brackets(case, operand, draw):
  _backward_data(case, draw, operand)


# --------------------------------------------------------------------------------------
# weight gradient
# --------------------------------------------------------------------------------------
def _backward_weight(case, draw, use_tr=True, splits=(None,), operand="bf16", check_geom=None, check_plan=None, tag=None):
  from iic_amd import geom, ops
  t = cc.inputs(case, draw)
  T = case.K * case.K
  fam = _fam("weight-gradient", tag or operand, draw)
  with _mode(operand):
    g = geom.fwd_geom(case.spec, case.N, case.H, case.W, case.P, case.P)
    if check_geom:
      check_geom(g)
    if check_plan:
      check_plan(g)
    default = 1 if operand == "f32" else int(ops.lib().iic_conv_wgrad_nsplit(ctypes.byref(g)))
    xp, dyp = ops.pt_from_nchw(t["x"].to(dev()), case.P), ops.pt_from_nchw(t["dy"].to(dev()), case.P)
    for ns in splits:
      used = default if ns is None else ns
      ref, tol = cc.weight_gradient_bound(case, draw, used)
      got = ops.conv_wgrad(g, xp, dyp, T, use_tr=use_tr, nsplit=ns)
      torch.cuda.synchronize()
      assert_within(got.view(case.cout, case.cin, case.K, case.K), ref, tol,
                    "weight gradient %r %s nsplit=%r use_tr=%r" % (case, draw, ns, use_tr), fam)
    # accumulate=True onto a non-zero dW
    prev = cc.bf16(torch.from_numpy(np.random.default_rng(21).uniform(-1, 1, (case.cout, case.cin, case.K, case.K)).astype(np.float32)))
    ref, tol = cc.weight_gradient_bound(case, draw, default, prev=prev)
    acc = prev.to(dev()).view(case.cout, case.cin, T).contiguous()
    ops.conv_wgrad(g, xp, dyp, T, use_tr=use_tr, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert_within(acc.view(case.cout, case.cin, case.K, case.K), ref, tol,
                  "weight gradient %r %s accumulated onto a previous dW" % (case, draw), fam)


@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("use_tr", [False, True])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_weight_gradient_within_float64_bound_for_every_split(case, use_tr, draw):
  _backward_weight(case, draw, use_tr, splits=(1, 2, 3, None))


@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_f32_weight_gradient_within_float64_bound(case, draw):
  _backward_weight(case, draw, operand="f32")


# --------------------------------------------------------------------------------------
# layer geometries of tests/conv_layer_cases.py that CONV_CASES lack (cc.LAYER_CASES): the 25-tap 5 x 5 layers, a 3 x 3
# plane, 64 -> 64 on 33 x 33, stride 2 on 17 x 17.  Bounds and brackets unchanged; families of their own ("layers-...")
# so that their worst ratios are listed beside the others'.  The references of a (case, draw) are shared by its runs.
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("case", cc.LAYER_CASES, ids=repr)
def test_layer_geometries_forward_and_statistics_in_float64_brackets(case, draw):
  from iic_amd import geom, ops
  assert ops.frag_supported(geom.fwd_geom(case.spec, case.N, case.H, case.W, case.P, case.P))
  for operand in ("rows", "frag"):
    _forward(case, draw, operand, tag="layers-" + operand)


@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("case", cc.LAYER_CASES, ids=repr)
def test_layer_geometries_backward_data_and_epilogues_in_float64_brackets(case, draw):
  from iic_amd import geom, ops
  assert all(ops.frag_supported(g) for g in geom.bwd_data_geoms(case.spec, case.N, case.H, case.W, case.P, case.P))
  for operand in ("rows", "frag"):
    _backward_data(case, draw, operand, tag="layers-" + operand)


@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("case", cc.LAYER_CASES, ids=repr)
def test_layer_geometries_weight_gradient_within_float64_bound(case, draw):
  for use_tr in (False, True):
    _backward_weight(case, draw, use_tr, splits=(1, 2, 3, None), tag="layers")


DILATED = cc.Case(128, 128, 3, 1, 2, 4, 20, d=2, P=2)
# padded row numbering (g.MP > plane), two images so that the padding rows sit inside the row range: H = 62 is the
# smallest for which geom pads a 64 -> 128 layer with PT border 3
PADDED = cc.Case(64, 128, 3, 1, 1, 2, 62, P=3)


@pytest.mark.parametrize("draw", cc.DRAWS)
def test_weight_gradient_dilation_2(draw):
  _backward_weight(DILATED, draw, splits=(1, None), tag="dilated")


@pytest.mark.parametrize("draw", cc.DRAWS)
def test_weight_gradient_padded_row_numbering(draw):
  from iic_amd import geom

  def padded(g):
    assert g.MP > g.MY * g.MX and g.MP % 256 == 0, "this case is meant to exercise the padded row numbering"
    smaller = geom.fwd_geom(cc.Case(64, 128, 3, 1, 1, 2, 61, P=3).spec, 2, 61, 61, 3, 3)
    assert not (smaller.MP > smaller.MY * smaller.MX), "a smaller image pads too: use it"
  _backward_weight(PADDED, draw, splits=(2, None), check_geom=padded, tag="padded")


def _wgrad_dma(mode):
  hook("iic_debug_enable_wgrad_dma", int(mode))


# the register-staged kernel (0) and the 64-pixel ring (3), each on two shapes: a 64-cout and a 128-cout tile width,
# several K-tiles per workgroup (nsplit 2)
@pytest.mark.parametrize("dma,kernel,bmk", [pytest.param(0, W_REG, 128, marks=HOOKS), pytest.param(3, None, 64, marks=HOOKS)])
@pytest.mark.parametrize("case", [cc.of((64, 64, 3, 1, 1, 2, 49)), cc.of((512, 512, 3, 1, 1, 6, 7))], ids=repr)
def test_weight_gradient_register_staged_kernel_and_64_pixel_ring(case, dma, kernel, bmk):
  def plan(g):
    if _has_hooks():
      p = _wplan(g, True)
      assert p["bmk"] == bmk and (kernel is None or p["kernel"] == kernel) and p["kernel"] != 0, p
      if dma == 3:
        assert p["kernel"] in (W_DMA, W_PL, W_PL2), p
  _wgrad_dma(dma)
  try:
    for draw in cc.DRAWS:
      _backward_weight(case, draw, splits=(2, None), check_plan=plan, tag="dma%d" % dma)
  finally:
    _wgrad_dma(1)


# --------------------------------------------------------------------------------------
# kernel families that the default dispatch reaches only at size
# --------------------------------------------------------------------------------------
def _expect(kernel, **fields):
  def check(g):
    if _has_hooks():
      g._frag_ok = g._red_ok = None
      p = _plan(g)
      assert p["kernel"] == kernel, p
      for k, v in fields.items():
        assert (v(p[k]) if callable(v) else p[k] == v), (k, p)
  return check


@HOOKS
@pytest.mark.parametrize("draw", cc.DRAWS)
def test_persistent_64_to_64_kernel_on_a_forced_small_grid(draw):
  hook("iic_debug_p64_grid", 2)
  try:
    check = _expect(CONV_P64, grid=2, mtiles=19)
    _forward(P64_FORCED, draw, "frag", check_plan=check, tag="p64-grid2")
    _backward_data(P64_FORCED, draw, "frag", check_plan=check, tag="p64-grid2")
  finally:
    hook("iic_debug_p64_grid", 0)


@HOOKS
@pytest.mark.parametrize("case", [cc.of((64, 64, 3, 1, 1, 5, 13)), cc.of((512, 512, 3, 1, 1, 6, 7))], ids=repr)
def test_256_row_tiles_of_the_first_generation_kernel(case):
  hook("iic_debug_force_bm", 256)
  try:
    for draw in cc.DRAWS:
      _forward(case, draw, "rows", tag="rows-bm256")
      _backward_data(case, draw, "rows", tag="rows-bm256")
  finally:
    hook("iic_debug_force_bm", 0)


@HOOKS
@pytest.mark.parametrize("draw", cc.DRAWS)
def test_stride_1_persistent_kernel_with_carried_statistics(draw):
  hook("iic_debug_enable_pw", 2)
  hook("iic_debug_pw_gx_cap", 1)
  try:
    check = _expect(CONV_PW, mtiles=49, grid=8)
    _forward(PW_FORCED, draw, "frag", check_plan=check, tag="pw")
    _backward_data(PW_FORCED, draw, "frag", check_plan=check, tag="pw")
  finally:
    hook("iic_debug_pw_gx_cap", 0)
    hook("iic_debug_enable_pw", 1)


@pytest.mark.parametrize("draw", cc.DRAWS)
def test_block_tiled_kernel_both_tile_widths(draw):
  from iic_amd import geom, ops
  case = BLOCK_TILED
  gf = geom.fwd_geom(case.spec, case.N, case.H, case.W, case.P, case.P)
  (gb,) = geom.bwd_data_geoms(case.spec, case.N, case.H, case.W, case.P, case.P)
  assert ops.frag_supported(gf) and ops.frag_supported(gb)
  _forward(case, draw, "frag", check_plan=_expect(CONV_BD, wn=2, bw=lambda v: v > 0), tag="block-tiled")
  _backward_data(case, draw, "frag", check_plan=_expect(CONV_BD, wn=1, bw=lambda v: v > 0), tag="block-tiled")


# --------------------------------------------------------------------------------------
# non-finite operands and overflow of the bf16 range
# --------------------------------------------------------------------------------------
SMALL64 = cc.Case(64, 64, 3, 1, 1, 1, 7)
SMALL128 = cc.Case(128, 128, 3, 1, 1, 4, 7)
NONFINITE = [(SMALL64, "rows"), (SMALL64, "frag"), (SMALL128, "frag")]      # first generation, persistent 64 -> 64, weights-direct


_classes = nonfinite_cls      # 0 finite, 1 +inf, 2 -inf, 3 NaN


@pytest.mark.parametrize("zero_weight", [False, True], ids=["dense-weights", "zero-weight-under-inf"])
@pytest.mark.parametrize("case,operand", NONFINITE, ids=["%r-%s" % co for co in NONFINITE])
def test_non_finite_pixels_propagate_as_in_float64(case, operand, zero_weight):
  """One +inf, one -inf and one NaN pixel whose 3 x 3 windows do not meet; then the same with a zero weight under the
  +inf (inf * 0 = NaN in that one output channel at that one pixel)."""
  from iic_amd import geom, ops
  t = cc.inputs(case, "mixed")
  x, w = t["x"].clone(), t["w"].clone()
  x[0, 3, 2, 2], x[0, 17, 5, 5], x[0, 40, 0, 6] = float("inf"), float("-inf"), float("nan")
  if zero_weight:
    w[9, 3, 1, 1] = 0.0
  fin = torch.isfinite(x)
  ref = cc.conv64(case, x, w)
  cls = _classes(ref)
  assert {int(c) for c in cls.unique()} == {0, 1, 2, 3} and int((cls[0] != 0).sum()) == case.cout * (9 + 9 + 4)
  assert (int(cls[0, 9, 2, 2]) == 3) == zero_weight
  xf = torch.where(fin, x, torch.zeros_like(x))
  A = cc.conv64(case, xf.abs(), w.abs())
  b = conv_acc_bound(case.terms_fwd, A)
  P = case.P
  g = geom.fwd_geom(case.spec, case.N, case.H, case.W, P, P)
  if operand == "frag":
    assert ops.frag_supported(g)
  wop = _operand(case, w.to(dev()), operand, False, [g])
  out = torch.zeros((case.N, case.H + 2 * P, case.W + 2 * P, case.cout), dtype=torch.bfloat16, device=dev())
  stats = ops.new_stats(case.cout, dev())
  ops.conv_igemm(g, ops.pt_from_nchw(x.to(dev()), P), wop, out, stats=stats)
  torch.cuda.synchronize()
  got = ops.pt_to_nchw(out, P).cpu()
  bad = _classes(got) != cls
  assert not bool(bad.any()), "%d elements of another class than the float64 reference; first at %s" % (
    int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]))
  finite = cls == 0
  safe = torch.where(finite, ref, torch.zeros_like(ref))
  lo, hi = bf16_bracket(safe, torch.where(finite, b, torch.zeros_like(b)))
  assert_in_bracket(torch.where(finite, got.double(), safe), lo, hi, "finite elements beside non-finite pixels", "conv64 non-finite")
  _borders_zero(out, P, "non-finite")
  st = ops.stats_decode(stats, case.cout).cpu()
  assert bool(torch.isnan(st).all()), "a channel that saw a non-finite value must decode to NaN (poison counter)"


@pytest.mark.parametrize("case,operand", NONFINITE, ids=["%r-%s" % co for co in NONFINITE])
def test_accumulator_beyond_the_bf16_range_stores_inf(case, operand):
  """Two products sum to 255.75 / 128 * 2^127: finite in fp32 (below 2^128), beyond the largest bf16 value 255 / 128 *
  2^127 by more than half a spacing -- RNE stores inf, a clamp would store the largest finite value.  The neighbouring
  channel sums to 255.25 / 128 * 2^127 and must store the largest finite bf16 value."""
  from iic_amd import geom, ops
  x = torch.zeros(case.N, case.cin, case.H, case.W)
  w = torch.zeros(case.cout, case.cin, 3, 3)
  x[0, 1, 3, 3] = x[0, 2, 3, 3] = 2.0 ** 64
  w[:, 1, 1, 1] = 2.0 ** 63 * (255.0 / 128.0)
  w[0::2, 2, 1, 1] = 2.0 ** 56 * 0.75
  w[1::2, 2, 1, 1] = 2.0 ** 56 * 0.25
  w[5, 1, 1, 1] *= -1.0
  w[5, 2, 1, 1] *= -1.0
  assert torch.equal(cc.bf16(x), x) and torch.equal(cc.bf16(w), w)
  ref = cc.conv64(case, x, w)
  lo, hi = bf16_bracket(ref, conv_acc_bound(case.terms_fwd, cc.conv64(case, x.abs(), w.abs())))
  assert float(lo[0, 0, 3, 3]) == float("inf") and float(hi[0, 1, 3, 3]) == BF16_MAX and float(hi[0, 5, 3, 3]) == -BF16_MAX
  P = case.P
  g = geom.fwd_geom(case.spec, case.N, case.H, case.W, P, P)
  wop = _operand(case, w.to(dev()), operand, False, [g])
  out = torch.zeros((case.N, case.H + 2 * P, case.W + 2 * P, case.cout), dtype=torch.bfloat16, device=dev())
  ops.conv_igemm(g, ops.pt_from_nchw(x.to(dev()), P), wop, out)
  torch.cuda.synchronize()
  got = ops.pt_to_nchw(out, P).cpu()
  assert_in_bracket(got, lo, hi, "accumulator beyond the bf16 range", "conv64 overflow")
  assert bool(torch.isposinf(got[0, 0::2, 3, 3]).all()) and bool((got[0, 1::2, 3, 3].abs() == BF16_MAX).all())
