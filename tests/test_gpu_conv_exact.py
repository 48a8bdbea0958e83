"""Convolutions on an integer lattice, bit for bit (tests/lattice.py explains why that is possible).

Operands from {-1, 0, +1}: every product and every partial sum is an exactly representable integer, so the bf16 MFMA
kernels (iic_conv_igemm, iic_conv_igemm_frag and the kernels they dispatch to: persistent 64 -> 64, block-tiled,
pointwise), the weight-gradient kernels for any split-K factor, the fused BatchNorm-backward reduction and the exact-fp32
path must reproduce float64 F.conv2d / its autograd EXACTLY.  The 1e-2 * max criterion of tests/test_gpu_kernels.py
cannot see a term dropped at a border pixel, a K-chunk skipped in a tail tile, a split-K partial counted twice or a
statistic taken from the wrong tensor; this file can (tests/test_conv_exact_cpu.py proves the comparison on the CPU).

Preconditions are asserted on the reference, never skipped: max |ref| <= 255 wherever the result is stored in bf16,
per-channel sum of squares < 2^24 for the statistic accumulators.  Densities below 1/2 are input choices that make them
hold; each is written beside its shape.  The only skips are geometries the library reports unsupported
(ops.frag_supported, ops.red_supported).  Everything runs through the product library's own dispatch.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.lattice import F32_EXACT_BOUND, assert_bf16_exact_range, assert_exact, lattice, record
from tests.test_gpu_kernels import CONV_CASES

pytestmark = pytest.mark.gpu

HALF, QUARTER, EIGHTH = 0.5, 0.25, 0.125


def dev():
  assert torch.cuda.is_available(), "no GPU visible"
  return torch.device("cuda:0")


class Shape(object):
  """One convolution problem: nn.Conv2d(cin, cout, K, stride s, padding p, dilation d) on N images of H x W, PT border
  P.  dens = density of (activation / output gradient, weight): tests/lattice.py."""

  def __init__(self, cin, cout, K, s, p, N, H, W=None, d=1, P=1, dens=(HALF, HALF), seed=0):
    self.cin, self.cout, self.K, self.s, self.p, self.N, self.H, self.W = cin, cout, K, s, p, N, H, (W or H)
    self.d, self.P, self.dens, self.seed = d, P, dens, seed

  @property
  def spec(self):
    from iic_amd import geom
    return geom.ConvSpec(self.cin, self.cout, self.K, self.s, self.p, self.d)

  @property
  def out_hw(self):
    return self.spec.out_size(self.H), self.spec.out_size(self.W)

  def __repr__(self):
    return "%dto%d_k%ds%dp%dd%d_n%d_%dx%d_P%d_dens%g-%g" % (self.cin, self.cout, self.K, self.s, self.p, self.d, self.N,
                                                            self.H, self.W, self.P, self.dens[0], self.dens[1])

  def figures(self, **kw):
    record(shape=repr(self), **kw)

  # ---- inputs and float64 references ----------------------------------------------------------
  def rng(self, salt):
    return np.random.default_rng([self.seed, salt, self.cin, self.cout, self.H])

  def x(self):
    return lattice(self.rng(1), (self.N, self.cin, self.H, self.W), self.dens[0])

  def w(self):
    return lattice(self.rng(2), (self.cout, self.cin, self.K, self.K), self.dens[1])

  def dy(self):
    return lattice(self.rng(3), (self.N, self.cout) + self.out_hw, self.dens[0])

  def like_x(self, salt, density=HALF):
    return lattice(self.rng(salt), (self.N, self.cin, self.H, self.W), density)

  def ref_forward(self, x, w):
    return F.conv2d(x.double(), w.double(), stride=self.s, padding=self.p, dilation=self.d)

  def ref_backward_data(self, dy, w):
    return torch.nn.grad.conv2d_input((self.N, self.cin, self.H, self.W), w.double(), dy.double(), stride=self.s,
                                      padding=self.p, dilation=self.d)

  def ref_backward_weight(self, x, dy):
    return torch.nn.grad.conv2d_weight(x.double(), (self.cout, self.cin, self.K, self.K), dy.double(), stride=self.s,
                                       padding=self.p, dilation=self.d)


def _case(c, **kw):
  cin, cout, K, s, p, N, H = c
  return Shape(cin, cout, K, s, p, N, H, **kw)


BASE = [_case(c) for c in CONV_CASES]
# 64 -> 64 3x3 at enough images that the persistent kernel's workgroups walk several tiles (one workgroup per CU)
PERSISTENT = Shape(64, 64, 3, 1, 1, 40, 49)
# SegmentationNet10a layers as archs/seg.py builds them (PT border 3, dilated convs with padding 1) and a wide image
# that only block tiles can serve (tests/test_gpu_kernels.py: block-tiled / wide-image parametrisations)
SEG_DILATED = Shape(256, 512, 3, 1, 1, 1, 100, d=2, P=3)
SEG_PLAIN = Shape(64, 128, 3, 1, 1, 1, 200, P=3)
WIDE = Shape(64, 128, 3, 1, 1, 1, 40, W=640, P=3)
LARGE = [PERSISTENT, SEG_DILATED, SEG_PLAIN, WIDE]


def _ids(shapes):
  return [repr(s) for s in shapes]


def _borders_zero(pt, P, what):
  o = pt.float()
  for name, edge in (("top", o[:, :P]), ("bottom", o[:, -P:]), ("left", o[:, :, :P]), ("right", o[:, :, -P:])):
    assert float(edge.abs().max()) == 0.0, "%s: %s border of the PT tensor was written" % (what, name)


def _operand(sh, w_dev, operand, bwd, geoms):
  """rows = the row-major bf16 operand of ops.weight_prep (first-generation kernel); frag = ops.PreppedWeights (the
  weights-direct kernels wherever ops.frag_supported, else skipped); product = the same handle without the skip (a
  stride-2 layer whose one-tap parity class only the first-generation kernel serves: tests/test_gpu_conv_layers_exact.py
  asserts which geometries are refused); f32 = the parameter itself (exact-fp32 path)."""
  from iic_amd import ops
  if operand == "rows":
    return ops.weight_prep(w_dev)[1 if bwd else 0]
  if operand == "product":      # the handle the architectures pass: ops.conv_igemm takes each geometry to the kernel that serves it
    return ops.PreppedWeights(w_dev)[1 if bwd else 0]
  if operand == "frag" and not all(ops.frag_supported(g) for g in geoms):
    assert not (sh.cin == 64 and sh.cout == 64 and sh.K == 3 and sh.s == 1), "64->64 3x3 must run on the persistent kernel"
    pytest.skip("geometry not served by the weights-direct kernels (library: iic_conv_igemm_frag_supported = 0)")
  return ops.PreppedWeights(w_dev)[1 if bwd else 0]


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


def _pt_dtype(operand):
  return torch.float32 if operand == "f32" else torch.bfloat16


# --------------------------------------------------------------------------------------
# forward + BatchNorm statistics
# --------------------------------------------------------------------------------------
def _forward(sh, operand):
  from iic_amd import geom, ops
  x, w = sh.x(), sh.w()
  y = sh.ref_forward(x, w)
  top = assert_bf16_exact_range(y, "forward %r" % sh)
  s1, s2 = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
  assert float(s2.max()) < F32_EXACT_BOUND, "per-channel sum of squares %g >= 2^24: lower the density" % float(s2.max())
  sh.figures(kind="forward", operand=operand, max_ref=top, max_sum_sq=float(s2.max()))
  Ho, Wo = sh.out_hw
  P = sh.P
  with _mode(operand):
    g = geom.fwd_geom(sh.spec, sh.N, sh.H, sh.W, P, P)
    wop = _operand(sh, w.to(dev()), operand, False, [g])
    xp = ops.pt_from_nchw(x.to(dev()), P)
    out = torch.zeros((sh.N, Ho + 2 * P, Wo + 2 * P, sh.cout), dtype=_pt_dtype(operand), device=dev())
    stats = ops.new_stats(sh.cout, dev())
    ops.conv_igemm(g, xp, wop, out, stats=stats)
    torch.cuda.synchronize()
  assert_exact(ops.pt_to_nchw(out, P), y, "forward output")
  _borders_zero(out, P, "forward")
  st = ops.stats_decode(stats, sh.cout).cpu()
  assert_exact(st[0], s1, "statistics: per-channel sum")
  assert_exact(st[1], s2, "statistics: per-channel sum of squares")


@pytest.mark.parametrize("operand", ["rows", "frag"])
@pytest.mark.parametrize("sh", BASE, ids=_ids(BASE))
def test_forward_and_statistics_exact(sh, operand):
  _forward(sh, operand)


@pytest.mark.parametrize("sh", LARGE, ids=_ids(LARGE))
def test_forward_and_statistics_exact_persistent_block_tiled_and_wide(sh):
  from iic_amd import geom, ops
  assert ops.frag_supported(geom.fwd_geom(sh.spec, sh.N, sh.H, sh.W, sh.P, sh.P)), "these shapes are the weights-direct kernels' own"
  _forward(sh, "frag")


# --------------------------------------------------------------------------------------
# backward-data and its epilogues
# --------------------------------------------------------------------------------------
def _covered(sh, geoms):
  """[H, W] bool: input pixels some backward-data geometry writes."""
  m = torch.zeros(sh.H, sh.W, dtype=torch.bool)
  for g in geoms:
    m[g.py - sh.P::g.ty, g.px - sh.P::g.tx] = True
  return m


def _backward_data_setup(sh, operand):
  from iic_amd import geom, ops
  dy, w = sh.dy(), sh.w()
  r = sh.ref_backward_data(dy, w)
  geoms = geom.bwd_data_geoms(sh.spec, sh.N, sh.H, sh.W, sh.P, sh.P)
  wop = _operand(sh, w.to(dev()), operand, True, geoms)
  dyp = ops.pt_from_nchw(dy.to(dev()), sh.P)
  return r, geoms, wop, dyp


def _new_dx(sh, operand, fill=None):
  from iic_amd import ops
  if fill is not None:
    return ops.pt_from_nchw(fill.to(dev()), sh.P)
  return torch.zeros((sh.N, sh.H + 2 * sh.P, sh.W + 2 * sh.P, sh.cin), dtype=_pt_dtype(operand), device=dev())


def _backward_data(sh, operand):
  from iic_amd import geom, ops
  with _mode(operand):
    r, geoms, wop, dyp = _backward_data_setup(sh, operand)
    top = assert_bf16_exact_range(r, "backward-data %r" % sh)
    sh.figures(kind="backward-data", operand=operand, max_ref=top, geometries=len(geoms))
    dx = _new_dx(sh, operand)
    for g in geoms:
      ops.conv_igemm(g, dyp, wop, dx)
    torch.cuda.synchronize()
  got = ops.pt_to_nchw(dx, sh.P)
  assert_exact(got, r, "backward-data output")
  _borders_zero(dx, sh.P, "backward-data")
  cov = _covered(sh, geoms)
  assert bool(cov.all()) == geom.bwd_data_covers_all(sh.spec)
  if not bool(cov.all()):       # stride-2 1x1: pixels of the odd parity classes receive no tap -- nothing may be written there
    assert float(r[:, :, ~cov].abs().max()) == 0.0
    assert float(got.cpu()[:, :, ~cov].abs().max()) == 0.0, "a pixel no geometry covers was written"


@pytest.mark.parametrize("operand", ["rows", "frag"])
@pytest.mark.parametrize("sh", BASE, ids=_ids(BASE))
def test_backward_data_exact(sh, operand):
  _backward_data(sh, operand)


BWD_LARGE = [PERSISTENT, SEG_DILATED, WIDE]


@pytest.mark.parametrize("sh", BWD_LARGE, ids=_ids(BWD_LARGE))
def test_backward_data_exact_persistent_block_tiled_and_wide(sh):
  _backward_data(sh, "frag")


def _epilogue_density(c):
  """Density of the output gradient for the epilogue runs: 2 * ref and ref + 1 must stay within 255, so the long
  reductions (K = cout * taps >= 2304) take 1/8 and the others 1/4 (weights stay at 1/2)."""
  cin, cout, K, s, p, N, H = c
  return EIGHTH if cout * K * K >= 2304 else QUARTER


def _covers_all(c):
  from iic_amd import geom
  cin, cout, K, s, p, N, H = c
  return geom.bwd_data_covers_all(geom.ConvSpec(cin, cout, K, s, p))


# (the 1x1 stride-2 case leaves pixels uncovered: an epilogue only runs on the pixels its launch stores)
EPILOGUE = [_case(c, dens=(_epilogue_density(c), HALF)) for c in CONV_CASES if _covers_all(c)]


def _backward_data_epilogues(sh, operand):
  """IIC_ACC_ADD, the fused ReLU-masked residual gradient and the four IIC_ACC_PREMASK forms (include/iic_hip.h), with
  res_grad, res_act and the previous contents on the lattice too: every expected value is an exact integer."""
  from iic_amd import ops
  with _mode(operand):
    r, geoms, wop, dyp = _backward_data_setup(sh, operand)
    top = float(r.abs().max())
    assert 2 * top <= 255 and top + 2 <= 255, "epilogue sums leave the bf16-exact range (max |ref| = %g): lower the density" % top
    sh.figures(kind="backward-data epilogues", operand=operand, max_ref=top, max_expected=max(2 * top, top + 2))
    rg, ra, prev = sh.like_x(11), sh.like_x(12), sh.like_x(13)
    rgp, rap = ops.pt_from_nchw(rg.to(dev()), sh.P), ops.pt_from_nchw(ra.to(dev()), sh.P)
    rg, ra, prev = rg.double(), ra.double(), prev.double()
    m = (ra > 0).double()
    forms = [
      ("accumulate onto itself", "plain", dict(accumulate=True), 2 * r),
      ("accumulate onto previous contents", prev, dict(accumulate=True), prev + r),
      ("res_grad + res_act", None, dict(res_grad=rgp, res_act=rap), r + rg * m),
      ("premask alone", None, dict(premask=True), r),
      ("premask + res_grad", None, dict(premask=True, res_grad=rgp), r + rg),
      ("premask + res_act", None, dict(premask=True, res_act=rap), r * m),
      ("premask + res_grad + res_act", None, dict(premask=True, res_grad=rgp, res_act=rap), (r + rg) * m),
      ("premask + accumulate + res_grad + res_act", prev, dict(premask=True, accumulate=True, res_grad=rgp, res_act=rap),
       (prev + r + rg) * m),
    ]
    for name, start, kw, want in forms:
      assert float(want.abs().max()) <= 255
      if isinstance(start, str):
        dx = _new_dx(sh, operand)
        for g in geoms:
          ops.conv_igemm(g, dyp, wop, dx)
      else:
        dx = _new_dx(sh, operand, start.float() if start is not None else None)
      for g in geoms:
        ops.conv_igemm(g, dyp, wop, dx, **kw)
      torch.cuda.synchronize()
      assert_exact(ops.pt_to_nchw(dx, sh.P), want, "backward-data epilogue '%s'" % name)
      _borders_zero(dx, sh.P, "backward-data epilogue '%s'" % name)


@pytest.mark.parametrize("operand", ["rows", "frag"])
@pytest.mark.parametrize("sh", EPILOGUE, ids=_ids(EPILOGUE))
def test_backward_data_epilogues_exact(sh, operand):
  _backward_data_epilogues(sh, operand)


# --------------------------------------------------------------------------------------
# weight gradient: K = the whole batch, any split-K factor
# --------------------------------------------------------------------------------------
def _large_split(g):
  """A split-K factor above the library's default: 2 * default + 1 (odd, so the K-tiles divide unevenly, and past the
  number of K-tiles for the small batches, where the trailing splits are empty and must contribute zero)."""
  from iic_amd import ops
  return 2 * int(ops.lib().iic_conv_wgrad_nsplit(ctypes.byref(g))) + 1


def _backward_weight(sh, use_tr=True, splits=(None,), operand="bf16", check_geom=None):
  from iic_amd import geom, ops
  x, dy = sh.x(), sh.dy()
  dw = sh.ref_backward_weight(x, dy)
  top = float(dw.abs().max())
  assert top < F32_EXACT_BOUND       # (|dW| <= N*Ho*Wo: stored in fp32, the 255 limit does not apply)
  T = sh.K * sh.K
  with _mode(operand):
    g = geom.fwd_geom(sh.spec, sh.N, sh.H, sh.W, sh.P, sh.P)
    if check_geom:
      check_geom(g)
    xp, dyp = ops.pt_from_nchw(x.to(dev()), sh.P), ops.pt_from_nchw(dy.to(dev()), sh.P)
    used = []
    for ns in splits:
      ns = _large_split(g) if ns == "large" else ns
      used.append(ns)
      got = ops.conv_wgrad(g, xp, dyp, T, use_tr=use_tr, nsplit=ns)
      torch.cuda.synchronize()
      assert_exact(got.view(sh.cout, sh.cin, sh.K, sh.K), dw, "weight gradient, nsplit=%r use_tr=%r" % (ns, use_tr))
    # accumulate=True onto a lattice-valued gradient
    prev = lattice(sh.rng(21), (sh.cout, sh.cin, sh.K, sh.K))
    acc = prev.to(dev()).view(sh.cout, sh.cin, T).contiguous()
    ops.conv_wgrad(g, xp, dyp, T, use_tr=use_tr, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert_exact(acc.view(sh.cout, sh.cin, sh.K, sh.K), prev.double() + dw, "weight gradient accumulated onto previous contents")
  sh.figures(kind="backward-weight", operand=operand, use_tr=use_tr, max_ref=top, k_range=sh.N * sh.out_hw[0] * sh.out_hw[1],
             splits=[("default" if s is None else s) for s in used],
             default_split=None if operand == "f32" else int(ops.lib().iic_conv_wgrad_nsplit(ctypes.byref(g))))


@pytest.mark.parametrize("use_tr", [False, True])
@pytest.mark.parametrize("sh", BASE, ids=_ids(BASE))
def test_backward_weight_exact_for_any_split(sh, use_tr):
  _backward_weight(sh, use_tr, splits=(None, 1, "large"))


# planar-kernel shapes (dilation 2, short image rows) of tests/test_gpu_kernels.py, PT border = dilation
PLANAR = [Shape(128, 128, 3, 1, 2, 4, 20, d=2, P=2), Shape(64, 128, 3, 1, 1, 9, 12), Shape(64, 64, 3, 1, 2, 3, 30, d=2, P=2)]
# padded row numbering (g.MP > plane): the second image is what makes the padding rows sit INSIDE the row range
PADDED = [Shape(64, 128, 3, 1, 1, 2, 200, P=3), Shape(128, 128, 3, 1, 1, 2, 100, d=2, P=3)]
# SegmentationNet10a layers (PT border 3, dilated convs with padding 1) at the smallest batch that keeps the geometry's
# row numbering and LDS patch (iic_conv_geom MP / NP) of the batch sizes tests/test_gpu_kernels.py lists
SEGNET = [Shape(128, 256, 3, 1, 1, 2, 100, P=3), Shape(64, 128, 3, 1, 1, 1, 128, P=3), Shape(256, 512, 3, 1, 1, 2, 64, d=2, P=3),
          Shape(512, 512, 3, 1, 1, 2, 62, d=2, P=3), Shape(64, 128, 3, 1, 1, 1, 200, P=3),
          Shape(256, 512, 3, 1, 1, 1, 100, d=2, P=3), Shape(512, 512, 3, 1, 1, 1, 98, d=2, P=3)]


@pytest.mark.parametrize("sh", PLANAR + SEGNET, ids=_ids(PLANAR + SEGNET))
def test_backward_weight_exact_planar_and_segmentation_shapes(sh):
  _backward_weight(sh, True, splits=(None, 1, "large"))


@pytest.mark.parametrize("sh", PADDED, ids=_ids(PADDED))
def test_backward_weight_exact_padded_row_numbering(sh):
  def padded(g):
    assert g.MP > g.MY * g.MX and g.MP % 256 == 0, "this case is meant to exercise the padded row numbering"
  _backward_weight(sh, True, splits=(None, 1, "large"), check_geom=padded)


# --------------------------------------------------------------------------------------
# fused BatchNorm-backward reduction in the backward-data epilogue
# --------------------------------------------------------------------------------------
RED = [(Shape(128, 128, 3, 1, 1, 40, 13), False, True), (Shape(256, 128, 3, 1, 1, 33, 9), True, False),
       (Shape(512, 512, 3, 1, 1, 16, 7, dens=(QUARTER, HALF)), False, False),
       (Shape(512, 512, 3, 1, 1, 16, 7, dens=(QUARTER, HALF), seed=1), True, True)]


def _fused_reduction(sh, has2, masked, require=True):
  """iic_conv_igemm_frag_red: red_stats += (sum g, sum g*y) [and (sum g, sum g*y2)] over the stored gradient g, masked
  with (scale*y + shift > 0) when the BatchNorm's coefficients are given.  g is an integer, y and y2 are on the lattice,
  scale and shift are powers of two (so the mask expression is exact): the four sums are exact integers.  Of a layer
  with several parity classes, every class ops.red_supported serves carries the reduction and the sums are expected over
  the pixels of those classes; the other classes are launched without one.  require=False: skip where no class is served."""
  from iic_amd import geom, ops
  dy, w = sh.dy(), sh.w()
  r = sh.ref_backward_data(dy, w)
  rg, ra, y, y2 = sh.like_x(11).double(), sh.like_x(12).double(), sh.like_x(14).double(), sh.like_x(15).double()
  gexp = (r + rg) * (ra > 0).double()
  top = assert_bf16_exact_range(gexp, "fused reduction %r" % sh)
  rng = sh.rng(16)
  scale = torch.from_numpy(rng.choice([1.0, -1.0, 2.0, 0.5, -0.25], sh.cin)).double()
  shift = torch.from_numpy(rng.choice([0.5, -0.5, 0.25, 0.0, -2.0, 1.0], sh.cin)).double()
  geoms = geom.bwd_data_geoms(sh.spec, sh.N, sh.H, sh.W, sh.P, sh.P)
  pw = ops.PreppedWeights(w.to(dev()))
  served = [ops.red_supported(g, pw[1]) for g in geoms]
  if not any(served):
    assert not require, "no parity class of %r carries a fused reduction" % sh
    pytest.skip("library: iic_conv_igemm_red_supported = 0 for this geometry")
  inred = torch.zeros(sh.H, sh.W, dtype=torch.bool)      # pixels whose launch carries the reduction
  for g, ok in zip(geoms, served):
    if ok:
      inred |= _covered(sh, [g])
  gm = gexp * ((y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)) > 0).double() if masked else gexp
  gm = gm * inred.double()
  want = [torch.stack([gm.sum((0, 2, 3)), (gm * y).sum((0, 2, 3))]), torch.stack([gm.sum((0, 2, 3)), (gm * y2).sum((0, 2, 3))])]
  assert float(gm.abs().sum((0, 2, 3)).max()) < F32_EXACT_BOUND      # any float partial of these sums is exact
  sh.figures(kind="fused reduction", has2=has2, masked=masked, max_ref=top, max_abs_sum=float(gm.abs().sum((0, 2, 3)).max()),
             classes=len(geoms), classes_reduced=sum(served))
  P = sh.P
  coef = torch.stack([scale.float(), shift.float(), torch.zeros(sh.cin), torch.ones(sh.cin), torch.zeros(sh.cin)]).to(dev())
  pt = lambda t: ops.pt_from_nchw(t.float().to(dev()), P)
  dx = torch.zeros((sh.N, sh.H + 2 * P, sh.W + 2 * P, sh.cin), dtype=torch.bfloat16, device=dev())
  s1, s2 = ops.new_stats(sh.cin, dev()), ops.new_stats(sh.cin, dev())
  dyp, rgp, rap, yp, y2p = pt(dy), pt(rg), pt(ra), pt(y), pt(y2)
  for g, ok in zip(geoms, served):
    red = (yp, coef if masked else None, s1, y2p if has2 else None, s2 if has2 else None) if ok else None
    ops.conv_igemm(g, dyp, pw[1], dx, res_grad=rgp, res_act=rap, premask=True, red=red)
  torch.cuda.synchronize()
  cov = _covered(sh, geoms)
  assert_exact(ops.pt_to_nchw(dx, P), gexp * cov.double(), "gradient stored by the fused launch")
  assert_exact(ops.stats_decode(s1, sh.cin).cpu(), want[0], "fused sums (sum g, sum g*y)")
  if has2:
    assert_exact(ops.stats_decode(s2, sh.cin).cpu(), want[1], "fused sums (sum g, sum g*y2)")


@pytest.mark.parametrize("sh,has2,masked", RED, ids=["%r-y2%d-mask%d" % (s, h, m) for s, h, m in RED])
def test_fused_bn_backward_reduction_exact(sh, has2, masked):
  from iic_amd import geom
  (gb,) = geom.bwd_data_geoms(sh.spec, sh.N, sh.H, sh.W, sh.P, sh.P)      # stride 1: one launch, as the trunk fuses it
  _fused_reduction(sh, has2, masked, require=False)


# --------------------------------------------------------------------------------------
# exact-fp32 path (csrc/f32_path.hip) through ops.fp32_mode(): the parity instrument itself
# --------------------------------------------------------------------------------------
# One thread per output with serial loops: small shapes.  Geometries the bf16 cases lack: 5x5 pad 2, dilation 2, channel
# counts that are no multiple of 8 (3, 5), stride 2 with and without full coverage, a wide PT border.
F32 = [Shape(3, 5, 5, 1, 2, 2, 9, P=2), Shape(5, 3, 3, 1, 2, 2, 8, W=11, d=2, P=2), Shape(16, 24, 3, 2, 1, 3, 9),
       Shape(8, 16, 1, 2, 0, 2, 7), Shape(64, 64, 3, 1, 1, 2, 13), Shape(6, 10, 3, 1, 1, 1, 6, W=5, P=3)]


@pytest.mark.parametrize("sh", F32, ids=_ids(F32))
def test_f32_conv_forward_and_statistics_exact(sh):
  _forward(sh, "f32")


@pytest.mark.parametrize("sh", F32, ids=_ids(F32))
def test_f32_conv_transposed_exact(sh):
  _backward_data(sh, "f32")


F32_EPILOGUE = [s for s in F32 if not (s.K == 1 and s.s == 2)]


@pytest.mark.parametrize("sh", F32_EPILOGUE, ids=_ids(F32_EPILOGUE))
def test_f32_conv_epilogue_flags_exact(sh):
  _backward_data_epilogues(sh, "f32")


@pytest.mark.parametrize("sh", F32, ids=_ids(F32))
def test_f32_wgrad_exact(sh):
  _backward_weight(sh, operand="f32")
