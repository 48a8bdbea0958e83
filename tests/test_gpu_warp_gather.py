"""iic_affine_warp_bwd_gather (csrc/warp.hip), the backward of the general affine warp without float atomics, and its way
into IID_segmentation_loss: bit for bit against the host emulation of tests/warp_gather_cases.py (proved on the CPU by
tests/test_warp_gather_cpu.py), against the atomic kernel and the exact adjoint on lattice inputs, launch against launch,
against float64 grid_sample, with non-finite gradients, for the matrices iic_affine_warp_gather_supported refuses, and
through the public losses.  pytest -m gpu.

Every dx starts as NaN: an element the kernel does not write fails the comparison."""
import functools

import numpy as np
import pytest
import torch

from tests import iid_stage_cases as sc
from tests import warp_gather_cases as wc
from tests.lattice import assert_exact
from tests.parity import assert_bits, assert_within, call, dev, ok

pytestmark = pytest.mark.gpu
NAN = float("nan")
IIC_ERR_UNSUPPORTED = -3


def _ids(shape):
  return "x".join(map(str, shape))


def gather(dout, M, shape, sx, sy):
  N, K, H, W = shape
  dx = torch.full(shape, NAN, device=dev())
  ok("iic_affine_warp_bwd_gather", dout, M.to(dev()), M, dx, N, K, H, W, sx, sy)
  return dx


def atomic(dout, M, shape, sx, sy):
  N, K, H, W = shape
  dx = torch.full(shape, NAN, device=dev())
  ok("iic_affine_warp_bwd", dout, M.to(dev()), dx, N, K, H, W, sx, sy)
  return dx


@functools.lru_cache(maxsize=None)
def emulated(shape, ci):
  c = wc.cases(shape)[ci]
  return wc.emulate(wc.random_dout(shape), c.M, c.sx, c.sy)["dx"]


def served(shape):
  return [(i, c) for i, c in enumerate(wc.cases(shape)) if c.served]


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_a_every_element_written_and_equal_to_the_emulation_bitwise(shape):
  dout = wc.random_dout(shape).to(dev())
  for i, c in served(shape):
    dx = gather(dout, c.M, shape, c.sx, c.sy)
    assert not bool(torch.isnan(dx).any()), (shape, c.name)
    assert_bits(dx, emulated(shape, i), "gather vs emulation %s %s" % (shape, c.name))


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_b_lattice_inputs_gather_atomic_and_exact_adjoint_agree(shape):
  inp = sc.warp_inputs(shape)
  dout = inp["dout"].to(dev())
  for i, c in served(shape):
    if not c.exact:
      continue
    dx = gather(dout, c.M, shape, c.sx, c.sy)
    assert_exact(dx.cpu(), sc.warp_bwd_ref(inp["dout"], c.M, c.sx, c.sy), "gather %s %s" % (shape, c.name))
    assert_bits(dx, atomic(dout, c.M, shape, c.sx, c.sy), "gather vs atomic %s %s" % (shape, c.name))


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_c_two_launches_are_bit_identical(shape):
  dout = wc.random_dout(shape).to(dev())
  for i, c in served(shape):
    a, b = gather(dout, c.M, shape, c.sx, c.sy), gather(dout, c.M, shape, c.sx, c.sy)
    assert torch.equal(a, b), (shape, c.name)


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_d_within_the_grid_sample_bound_of_float64(shape):
  """F.affine_grid + F.grid_sample backward in float64, the bound of test_gpu_seg_loss.py::
  test_affine_warp_matches_grid_sample: |dx - ref| < 2e-5 max(1, max |ref|).  Cases without a shift (grid_sample has
  none); pixel matrices go back to theta through iid_stage_cases.pixel_to_theta."""
  N, K, H, W = shape
  g = wc.random_dout(shape)
  dout = g.to(dev())
  n = 0
  for i, c in served(shape):
    if c.sx or c.sy:
      continue
    theta, ac = (c.theta, c.ac) if c.theta is not None else (sc.pixel_to_theta(c.M, H, W), False)
    xr = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    grid = torch.nn.functional.affine_grid(theta.double(), list(shape), align_corners=ac)
    torch.nn.functional.grid_sample(xr, grid, padding_mode="zeros", align_corners=ac).backward(g.double())
    dx = gather(dout, c.M, shape, 0, 0)
    err = float((dx.cpu().double() - xr.grad).abs().max())
    assert err < 2e-5 * max(1.0, float(xr.grad.abs().max())), (shape, c.name, err)
    n += 1
  assert n >= 8


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_e_nan_and_inf_land_where_the_emulation_puts_them(shape):
  N, K, H, W = shape
  g = wc.random_dout(shape).clone()
  g[0, 0, H // 2, W // 2] = NAN
  g[N - 1, K - 1, H - 1, 0] = float("inf")
  dout = g.to(dev())
  hits = 0
  for i, c in served(shape):
    want = wc.emulate(g, c.M, c.sx, c.sy)["dx"]
    dx = gather(dout, c.M, shape, c.sx, c.sy).cpu()
    assert torch.equal(torch.isnan(dx), torch.isnan(want)), (shape, c.name)
    assert torch.equal(torch.isposinf(dx), torch.isposinf(want)) and torch.equal(torch.isneginf(dx), torch.isneginf(want))
    fin = torch.isfinite(want)
    assert_bits(torch.where(fin, dx, torch.zeros_like(dx)), torch.where(fin, want, torch.zeros_like(want)),
                "finite part %s %s" % (shape, c.name))
    hits += int((~fin).sum())
  assert hits > 0


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_f_refused_matrices_query_launch_and_fallback(shape):
  from iic_amd import _lib, seg_losses
  N, K, H, W = shape
  g = wc.random_dout(shape)
  dout = g.to(dev())
  for c in wc.refused_cases(shape):
    assert _lib.lib().iic_affine_warp_gather_supported(c.M.data_ptr(), N) == 0, c.name
    dx = torch.full(shape, NAN, device=dev())
    rc = call("iic_affine_warp_bwd_gather", dout, c.M.to(dev()), c.M, dx, N, K, H, W, 0, 0)
    assert rc == IIC_ERR_UNSUPPORTED, (c.name, rc)
    assert bool(torch.isnan(dx).all()), "a refused launch wrote dx"
    # the public path falls back to the atomic kernel: its gradient inside the grid_sample bound
    x = torch.zeros(shape, device=dev(), requires_grad=True)
    seg_losses._AffineWarpFn.apply(x, c.M.to(dev()), 0, 0, c.M).backward(dout)
    theta = sc.pixel_to_theta(c.M, H, W)
    xr = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    grid = torch.nn.functional.affine_grid(theta, list(shape), align_corners=False)
    torch.nn.functional.grid_sample(xr, grid, padding_mode="zeros", align_corners=False).backward(g.double())
    err = float((x.grad.cpu().double() - xr.grad).abs().max())
    assert err < 2e-5 * max(1.0, float(xr.grad.abs().max())), (shape, c.name, err)


def test_f_autograd_function_takes_the_gather_kernel_when_served_and_the_switch_selects_the_atomic_one():
  """_AffineWarpFn with the host matrices: the gather kernel's bits; with WARP_BWD_GATHER off, or without host matrices,
  the atomic kernel's result (equal to the gather's to rounding)."""
  from iic_amd import seg_losses
  shape = wc.SHAPES[0]
  i, c = served(shape)[0]
  dout = wc.random_dout(shape).to(dev())

  def grad(host):
    x = torch.zeros(shape, device=dev(), requires_grad=True)
    seg_losses._AffineWarpFn.apply(x, c.M.to(dev()), c.sx, c.sy, host).backward(dout)
    return x.grad

  assert_bits(grad(c.M), emulated(shape, i), "autograd, gather")
  ref = atomic(dout, c.M, shape, c.sx, c.sy)
  seg_losses.WARP_BWD_GATHER[0] = False
  try:
    off = grad(c.M)
  finally:
    seg_losses.WARP_BWD_GATHER[0] = True
  # two float32 sums of the same terms in two orders: each inside the accumulation bound of the exact adjoint
  g = wc.random_dout(shape)
  tol = 2.0 * wc.accumulation_bound(g, c.M, c.sx, c.sy, wc.emulate(g, c.M, c.sx, c.sy)["counts"])
  for other in (off, grad(None)):
    assert_within(other, ref.cpu(), tol, "atomic backward through the switch vs a direct launch")
    assert_within(other, sc.warp_bwd_ref(g, c.M, c.sx, c.sy), tol, "atomic backward through the switch")


@pytest.mark.parametrize("collapsed", [False, True], ids=["uncollapsed", "collapsed"])
@pytest.mark.parametrize("sparse", [0, 2], ids=["affine", "affine_sparse_shift"])
def test_g_public_losses_reproducible_and_within_the_oracle_tolerance(collapsed, sparse):
  """IID_segmentation_loss / _uncollapsed at (bn, k, h, w, T) = (2, 5, 13, 20, 1) with general affines, without and with a
  non-zero sparse shift: two calls give bit-identical x2.grad (and x1.grad, loss); the loss and both gradients against
  oracle.iid_oracle in float64 with the tolerances of test_gpu_seg_loss.py::test_seg_loss_golden_fixture2 -- the loss
  max(1e-5 relative + 2e-7, twice the float32 oracle's own distance), the gradients 5e-5 in relative L2 norm."""
  from iic_amd import seg_losses
  from oracle import iid_oracle
  from oracle.gen_golden import make_seg_inputs
  from oracle.gen_golden_seg2 import random_affines
  bn, k, h, w, T = 2, 5, 13, 20, 1
  x1, x2, _, mask = make_seg_inputs(bn, k, h, w, 0.0, 0.8, 31)
  aff = random_affines(bn, 131)
  fh = seg_losses.IID_segmentation_loss if collapsed else seg_losses.IID_segmentation_loss_uncollapsed
  fr = iid_oracle.IID_segmentation_loss if collapsed else iid_oracle.IID_segmentation_loss_uncollapsed

  def run():
    a = torch.from_numpy(x1).to(dev()).requires_grad_(True)
    b = torch.from_numpy(x2).to(dev()).requires_grad_(True)
    np.random.seed(7)            # the sparse shift is drawn from numpy's global RNG, as the reference does
    l, ln = fh(a, b, all_affine2_to_1=torch.from_numpy(aff).to(dev()), all_mask_img1=torch.from_numpy(mask).to(dev()),
               lamb=1.5, half_T_side_dense=T, half_T_side_sparse_min=sparse, half_T_side_sparse_max=sparse)
    l.backward()
    return l.detach(), ln.detach(), a.grad, b.grad

  r1, r2 = run(), run()
  for p, q in zip(r1, r2):
    assert torch.equal(p, q)
  def oracle(dt):
    a = torch.from_numpy(x1).to(dt).requires_grad_(True)
    b = torch.from_numpy(x2).to(dt).requires_grad_(True)
    np.random.seed(7)
    res = fr(a, b, all_affine2_to_1=torch.from_numpy(aff).to(dt), all_mask_img1=torch.from_numpy(mask).to(dt),
             lamb=1.5, half_T_side_dense=T, half_T_side_sparse_min=sparse, half_T_side_sparse_max=sparse)
    return a, b, res

  a64, b64, (r, rn) = oracle(torch.float64)
  r.backward()
  _, _, (r32, rn32) = oracle(torch.float32)       # (the fixture's second term: twice the float32 oracle's own error)
  l, ln, ga, gb = r1
  assert abs(l.item() - float(r)) <= max(1e-5 * abs(float(r)) + 2e-7, 2 * abs(float(r32) - float(r))), (l.item(), float(r))
  assert abs(ln.item() - float(rn)) <= max(1e-5 * abs(float(rn)) + 2e-7, 2 * abs(float(rn32) - float(rn))), \
    (ln.item(), float(rn))
  for mine, ref, key in ((ga, a64.grad, "dx1"), (gb, b64.grad, "dx2")):
    err = float((mine.cpu().double() - ref).norm() / ref.norm())
    assert err <= 5e-5, (key, err)
