"""The exact-arithmetic convolution harness of tests/test_gpu_conv_exact.py, proven without a GPU.

iic_amd.geom.emulate_igemm / emulate_wgrad model the kernels' indexing (GEMM row -> input pixel, output pixel, tap list).
The same lattice generator and the same comparison as the GPU tests are run against them, then the comparison must
reject seeded defects of the kinds a kernel can have -- while the criterion of tests/test_gpu_kernels.py,
max |got - ref| <= 1e-2 * max |ref|, accepts them.

What "accepts" can mean.  On these inputs a defect that involves a whole 64-channel slice (a tap dropped with all its
input channels, a GEMM row copied to its neighbour in every output channel) moves some element by several units, about
7 % and more of the largest value: the old criterion sees that too, and the tests below say so with the figures.  What
it cannot see is the same defect confined to one term: one input channel of one tap at one border pixel, one output
channel of the copied row, one unit in one element of the weight gradient.  Those are the seeded defects held against
both criteria; the whole-slice forms are held against the exact comparison as well (it must reject them, whatever the
old criterion says).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iic_amd import geom
from tests.lattice import (BF16_EXACT_MAX, F32_EXACT_BOUND, assert_bf16_exact_range, assert_exact, exact_mismatch,
                           lattice, tolerance_accepts)

# cin, cout, K, stride, pad, dil, N, H
BIG_K = (512, 128, 3, 1, 1, 1, 2, 7)        # K = 4608 per output: max |y| > 100, so one unit is < 1 % of it
LONG_BATCH = (64, 64, 3, 1, 1, 1, 4, 28)    # weight-gradient K = N*Ho*Wo = 3136: max |dW| > 100
STRIDE2 = (64, 128, 3, 2, 1, 1, 2, 9)       # four backward-data geometries
CASES = [BIG_K, LONG_BATCH, STRIDE2]


def _inputs(case, seed=0, density=0.5):
  cin, cout, K, s, p, d, N, H = case
  rng = np.random.default_rng(seed)
  spec = geom.ConvSpec(cin, cout, K, s, p, d)
  Ho = spec.out_size(H)
  x = lattice(rng, (N, cin, H, H), density)
  w = lattice(rng, (cout, cin, K, K), density)
  dy = lattice(rng, (N, cout, Ho, Ho), density)
  return spec, x, w, dy


def _references(case, x, w, dy):
  cin, cout, K, s, p, d, N, H = case
  xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
  y = F.conv2d(xd, wd, stride=s, padding=p, dilation=d)
  y.backward(dy.double())
  return y.detach(), xd.grad, wd.grad


def _rows(w):
  """OIHW -> [T][Co][Ci] float64 numpy (the forward operand of emulate_igemm)."""
  co, ci, kh, kw = w.shape
  return w.double().permute(2, 3, 0, 1).reshape(kh * kw, co, ci).numpy()


def _emulate_forward(case, spec, x, w):
  cin, cout, K, s, p, d, N, H = case
  g = geom.fwd_geom(spec, N, H, H, max(p, 1), 1)
  xp = geom.to_pt(x.double().numpy(), max(p, 1))
  return g, xp, geom.emulate_igemm(g, xp, _rows(w))


@pytest.mark.parametrize("case", CASES)
def test_emulated_kernels_equal_the_float64_reference_exactly(case):
  """Forward, backward-data (every geometry of bwd_data_geoms) and backward-weight of the emulation against float64
  F.conv2d and its autograd, with the preconditions asserted on the reference as the GPU tests assert them."""
  cin, cout, K, s, p, d, N, H = case
  spec, x, w, dy = _inputs(case)
  y, dx, dw = _references(case, x, w, dy)
  assert_bf16_exact_range(y, "forward")
  assert_bf16_exact_range(dx, "backward-data")
  assert float((y * y).sum((0, 2, 3)).max()) < F32_EXACT_BOUND
  assert float(dw.abs().max()) < F32_EXACT_BOUND
  g, xp, out = _emulate_forward(case, spec, x, w)
  assert_exact(geom.from_pt(out, 1), y, "forward")
  dyp = geom.to_pt(dy.double().numpy(), 1)
  dxp = np.zeros((N, H + 2, H + 2, cin))
  wb = np.transpose(_rows(w), (0, 2, 1))
  for gb in geom.bwd_data_geoms(spec, N, H, H, 1, 1):
    geom.emulate_igemm(gb, dyp, wb, dxp)
  assert_exact(geom.from_pt(dxp, 1), dx, "backward-data")
  gw = geom.fwd_geom(spec, N, H, H, 1, 1)
  got = geom.emulate_wgrad(gw, geom.to_pt(x.double().numpy(), 1), dyp, K * K)
  assert_exact(np.transpose(got, (1, 2, 0)).reshape(cout, cin, K, K), dw, "backward-weight")


def _border_pixel_and_term(g, xp, wr, out):
  """The first border output pixel (image 0, top row) and (tap, ci, co) whose single product is non-zero."""
  xf = xp.reshape(-1, g.Cin)
  for m in range(g.MX):                       # GEMM rows of the top output row of image 0
    pin, pout = int(geom._pin(g, m)), int(geom._pout(g, m))
    for t in range(g.ntaps):
      src = xf[pin + g.tap_off[t]]
      for ci in np.flatnonzero(src):
        co = np.flatnonzero(wr[g.tap_w[t]][:, ci])
        if len(co):
          return m, pout, t, int(ci), int(co[0]), pin
  raise AssertionError("no non-zero term in the top row: the inputs are degenerate")


def test_exact_comparison_rejects_a_dropped_tap_that_the_tolerance_accepts():
  """Defect 1: a tap omitted at one border pixel.  One input channel of it (one term, +-1): the 1e-2 * max criterion
  accepts, the exact comparison rejects.  All 512 input channels of it: rejected by the exact comparison too (here the
  old criterion also notices: the slice sums to several units)."""
  spec, x, w, dy = _inputs(BIG_K)
  y, _, _ = _references(BIG_K, x, w, dy)
  top = assert_bf16_exact_range(y, "forward")
  assert top >= 100, "the case is chosen so that one unit is below 1 %% of max |ref| (got %g)" % top
  g, xp, out = _emulate_forward(BIG_K, spec, x, w)
  wr = _rows(w)
  assert exact_mismatch(geom.from_pt(out, 1), y) is None
  m, pout, t, ci, co, pin = _border_pixel_and_term(g, xp, wr, out)
  xf = xp.reshape(-1, g.Cin)
  one = out.copy()
  one.reshape(-1, g.Cout)[pout, co] -= xf[pin + g.tap_off[t], ci] * wr[g.tap_w[t], co, ci]
  got = geom.from_pt(one, 1)
  assert tolerance_accepts(got, y), "the old criterion was expected to accept a one-term defect"
  msg = exact_mismatch(got, y)
  assert msg is not None and msg.startswith("1 of "), msg
  whole = out.copy()
  whole.reshape(-1, g.Cout)[pout] -= xf[pin + g.tap_off[t]] @ wr[g.tap_w[t]].T
  assert exact_mismatch(geom.from_pt(whole, 1), y) is not None


def test_exact_comparison_rejects_a_duplicated_tile_row_that_the_tolerance_accepts():
  """Defect 2: a GEMM row of a tile stored into its neighbour as well.  In one output channel where the two rows differ
  by one unit: accepted by 1e-2 * max, rejected exactly.  In every output channel: rejected exactly as well."""
  spec, x, w, dy = _inputs(BIG_K)
  y, _, _ = _references(BIG_K, x, w, dy)
  assert assert_bf16_exact_range(y, "forward") >= 100
  g, xp, out = _emulate_forward(BIG_K, spec, x, w)
  of = out.reshape(-1, g.Cout)
  found = None
  for m in range(geom.gemm_rows(g) - 1):     # neighbours in one image row
    if (m + 1) % g.MX == 0:
      continue
    a, b = int(geom._pout(g, m)), int(geom._pout(g, m + 1))
    co = np.flatnonzero(np.abs(of[a] - of[b]) == 1)
    if len(co):
      found = (a, b, int(co[0]))
      break
  assert found, "no neighbouring rows that differ by one unit in some channel: the inputs are degenerate"
  a, b, co = found
  one = out.copy()
  one.reshape(-1, g.Cout)[b, co] = of[a, co]
  got = geom.from_pt(one, 1)
  assert tolerance_accepts(got, y), "the old criterion was expected to accept a one-unit copy"
  msg = exact_mismatch(got, y)
  assert msg is not None and msg.startswith("1 of "), msg
  whole = out.copy()
  whole.reshape(-1, g.Cout)[b] = of[a]
  assert exact_mismatch(geom.from_pt(whole, 1), y) is not None


def test_exact_comparison_rejects_a_weight_gradient_off_by_one_that_the_tolerance_accepts():
  """Defect 3: one element of the weight gradient off by one (one row of the batch counted twice or not at all).  Its K
  range is the whole batch, so max |dW| is large and one unit is inside 1e-2 * max; the exact comparison rejects and
  names the element."""
  cin, cout, K, s, p, d, N, H = LONG_BATCH
  spec, x, w, dy = _inputs(LONG_BATCH)
  _, _, dw = _references(LONG_BATCH, x, w, dy)
  top = float(dw.abs().max())
  assert 100 <= top < F32_EXACT_BOUND, top
  g = geom.fwd_geom(spec, N, H, H, 1, 1)
  got = geom.emulate_wgrad(g, geom.to_pt(x.double().numpy(), 1), geom.to_pt(dy.double().numpy(), 1), K * K)
  got = np.transpose(got, (1, 2, 0)).reshape(cout, cin, K, K).copy()
  assert exact_mismatch(got, dw) is None
  got[cout // 2, cin // 3, 1, 2] += 1.0
  assert tolerance_accepts(got, dw), "the old criterion was expected to accept one unit in one element"
  msg = exact_mismatch(got, dw)
  assert msg is not None and msg.startswith("1 of ") and "(%d, %d, 1, 2)" % (cout // 2, cin // 3) in msg, msg


def test_exact_comparison_names_nan_and_shape_errors():
  ref = torch.zeros(2, 3, dtype=torch.float64)
  got = torch.zeros(2, 3)
  assert exact_mismatch(got, ref) is None
  assert exact_mismatch(-got, ref) is None             # a zero of either sign is zero
  got[1, 2] = float("nan")
  assert "(1, 2)" in exact_mismatch(got, ref)
  assert "shape" in exact_mismatch(torch.zeros(3, 2), ref)
  assert BF16_EXACT_MAX == 255 and float(torch.tensor(255.0).to(torch.bfloat16)) == 255.0
  assert float(torch.tensor(257.0).to(torch.bfloat16)) != 257.0
