"""IID segmentation losses on the HIP path (through the C ABI) vs the reference golden
vectors and the float64 oracle.  pytest -m gpu.  Tolerance = the loss clause of the
north star: |ours - ref| <= 1e-5*|ref64| + 2e-7; gradients ||d||/||g|| <= 1e-5, or no worse
than the fp32 reference's own error w.r.t. float64."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def dev():
  return torch.device("cuda:0")


def _check(fn_hip, fn_ref64, x1, x2, aff, mask, lamb, T, ref32=None):
  a = torch.from_numpy(x1).to(dev()).requires_grad_(True)
  b = torch.from_numpy(x2).to(dev()).requires_grad_(True)
  l, ln = fn_hip(a, b, all_affine2_to_1=torch.from_numpy(aff).to(dev()),
                 all_mask_img1=torch.from_numpy(mask).to(dev()), lamb=lamb, half_T_side_dense=T,
                 half_T_side_sparse_min=0, half_T_side_sparse_max=0)
  (l + 0.5 * ln).backward()
  a64 = torch.from_numpy(x1).double().requires_grad_(True)
  b64 = torch.from_numpy(x2).double().requires_grad_(True)
  r, rn = fn_ref64(a64, b64, all_affine2_to_1=torch.from_numpy(aff).double(),
                   all_mask_img1=torch.from_numpy(mask).double(), lamb=lamb, half_T_side_dense=T)
  (r + 0.5 * rn).backward()
  assert abs(l.item() - float(r)) <= 1e-5 * abs(float(r)) + 2e-7, (l.item(), float(r))
  assert abs(ln.item() - float(rn)) <= 1e-5 * abs(float(rn)) + 2e-7, (ln.item(), float(rn))
  for mine, ref in ((a.grad.cpu().double(), a64.grad), (b.grad.cpu().double(), b64.grad)):
    err = float((mine - ref).norm() / ref.norm())
    assert err <= 2e-5, err


@pytest.mark.parametrize("ci", [0, 1, 2])
@pytest.mark.parametrize("collapsed", [False, True])
def test_seg_loss_golden(ci, collapsed):
  from iic_amd import seg_losses
  from oracle import iid_oracle
  from oracle.gen_golden import SEG_CASES, make_seg_inputs
  g = np.load(os.path.join(G, "iid_seg_loss.npz"), allow_pickle=True)
  bn, k, h, w, T, lamb, ff, mp, seed = SEG_CASES[ci]
  x1, x2, aff, mask = make_seg_inputs(bn, k, h, w, ff, mp, seed)
  name = "col" if collapsed else "unc"
  fn = seg_losses.IID_segmentation_loss if collapsed else seg_losses.IID_segmentation_loss_uncollapsed
  a = torch.from_numpy(x1).to(dev()).requires_grad_(True)
  b = torch.from_numpy(x2).to(dev()).requires_grad_(True)
  l, ln = fn(a, b, all_affine2_to_1=torch.from_numpy(aff).to(dev()),
             all_mask_img1=torch.from_numpy(mask).to(dev()), lamb=lamb, half_T_side_dense=T,
             half_T_side_sparse_min=0, half_T_side_sparse_max=0)
  l.backward()
  ref = g["c%d_%s_loss_f64" % (ci, name)]
  assert abs(l.item() - ref[0]) <= 1e-5 * abs(ref[0]) + 2e-7, (l.item(), ref[0])
  assert abs(ln.item() - ref[1]) <= 1e-5 * abs(ref[1]) + 2e-7
  for t, key in ((a, "dx1"), (b, "dx2")):
    g64 = g["c%d_%s_%s_f64" % (ci, name, key)]
    g32 = g["c%d_%s_%s_f32" % (ci, name, key)].astype(np.float64)
    nrm = np.linalg.norm(g64)
    err = np.linalg.norm(t.grad.cpu().numpy().astype(np.float64) - g64) / nrm
    assert err <= max(1e-5, np.linalg.norm(g32 - g64) / nrm), (key, err)


@pytest.mark.parametrize("bn,k,h,w,T", [(3, 15, 40, 64, 10), (2, 24, 24, 40, 5), (2, 45, 16, 32, 3), (2, 3, 30, 50, 1),
                                        # edge shapes: no shift at all, one sample, k = 2, odd sizes (w % 4 != 0 takes the
                                        # generic kernels), a shift range almost as large as the image
                                        (1, 2, 9, 13, 0), (2, 3, 17, 23, 2), (1, 33, 8, 12, 1), (2, 5, 8, 9, 6),
                                        # round 6: 33 <= k <= 48 on the streaming kernels (three class tiles) -- the
                                        # overclustering heads of the reference's 15- / 6-class runs (k_A = 45 / 36,
                                        # commands.txt:80,89) at their row widths and shift ranges, reduced heights
                                        (1, 45, 24, 128, 10), (1, 36, 12, 200, 5), (2, 48, 6, 72, 2)])
@pytest.mark.parametrize("collapsed", [False, True])
def test_seg_loss_larger_vs_oracle(bn, k, h, w, T, collapsed):
  from iic_amd import seg_losses
  from oracle import iid_oracle
  from oracle.gen_golden import make_seg_inputs
  x1, x2, aff, mask = make_seg_inputs(bn, k, h, w, 0.5, 0.8, 7)
  aff[-1, 1, 1] = -1.0   # also a y-flip on the last sample
  fh = seg_losses.IID_segmentation_loss if collapsed else seg_losses.IID_segmentation_loss_uncollapsed
  fr = iid_oracle.IID_segmentation_loss if collapsed else iid_oracle.IID_segmentation_loss_uncollapsed
  _check(fh, fr, x1, x2, aff, mask, 1.5, T)


def test_lds_limit_follows_the_launches_of_the_generic_joint_kernel():
  """iic_launch_lds (csrc/common.h) on a kernel whose dynamic LDS goes past 64 KB: seg_joint_kernel<3, 3> (k = 33, widths
  that are no multiple of 4) stages 192 rows of about 2 w floats -- 36 864 bytes at w = 30, 51 456 at w = 130, 79 104 at
  w = 202 -- launched in that order and at w = 30 again, in one process, every loss and gradient against the float64
  oracle with test_seg_loss_larger_vs_oracle's bounds.  No other test of this process launches that instantiation above
  48 KB, and a limit left at an earlier launch's size fails the third launch wherever the runtime draws its line."""
  from iic_amd import seg_losses
  from oracle import iid_oracle
  from oracle.gen_golden import make_seg_inputs
  for w in (30, 130, 202, 30):
    x1, x2, aff, mask = make_seg_inputs(1, 33, 4, w, 0.5, 0.8, 7)
    _check(seg_losses.IID_segmentation_loss, iid_oracle.IID_segmentation_loss, x1, x2, aff, mask, 1.5, 1)


def test_seg_loss_shift_range_beyond_the_image_is_nan_like_the_reference():
  """half_T_side_dense >= the image side: shifts without any overlap have an all-zero joint, the uncollapsed loss
  normalises every shift by its own sum (IID_losses.py:130-157) => 0 / 0: the reference returns NaN, so do we (no published
  run comes near: T = 10 on 128 / 200-pixel images).  The collapsed loss sums the shifts first and stays finite."""
  from iic_amd import seg_losses
  from oracle import iid_oracle
  from oracle.gen_golden import make_seg_inputs
  x1, x2, aff, mask = make_seg_inputs(2, 5, 6, 7, 0.5, 0.8, 7)
  kw = dict(lamb=1.5, half_T_side_dense=6)
  r, _ = iid_oracle.IID_segmentation_loss_uncollapsed(
    torch.from_numpy(x1).double().requires_grad_(True), torch.from_numpy(x2).double().requires_grad_(True),
    all_affine2_to_1=torch.from_numpy(aff).double(), all_mask_img1=torch.from_numpy(mask).double(), **kw)
  a = torch.from_numpy(x1).float().to(dev()).requires_grad_(True)
  b = torch.from_numpy(x2).float().to(dev()).requires_grad_(True)
  l, _ = seg_losses.IID_segmentation_loss_uncollapsed(
    a, b, all_affine2_to_1=torch.from_numpy(aff).float().to(dev()), all_mask_img1=torch.from_numpy(mask).float().to(dev()),
    half_T_side_sparse_min=0, half_T_side_sparse_max=0, **kw)
  assert math.isnan(float(r.detach())) and math.isnan(float(l.detach()))
  _check(seg_losses.IID_segmentation_loss, iid_oracle.IID_segmentation_loss, x1, x2, aff, mask, 1.5, 6)


@pytest.mark.parametrize("case_i", range(7))
@pytest.mark.parametrize("collapsed", [False, True])
def test_seg_loss_golden_fixture2(case_i, collapsed):
  """Reference-generated goldens at BASELINE.json shapes (k = 24 / 15 / 3, T = 10, masks), for
  general affine matrices (perform_affine_tf) and with the sparse random translation."""
  from iic_amd import seg_losses
  from oracle.gen_golden_seg2 import SEG2_CASES, case_inputs
  g = np.load(os.path.join(G, "iid_seg_loss2.npz"))
  case = SEG2_CASES[case_i]
  name, bn, k, h, w, T, lamb, ff, mp, seed, affine, smin, smax, np_seed = case
  x1, x2, aff, mask = case_inputs(case)
  vname = "col" if collapsed else "unc"
  fn = seg_losses.IID_segmentation_loss if collapsed else seg_losses.IID_segmentation_loss_uncollapsed
  a = torch.from_numpy(x1).to(dev()).requires_grad_(True)
  b = torch.from_numpy(x2).to(dev()).requires_grad_(True)
  np.random.seed(np_seed)      # the sparse shift is drawn from numpy's global RNG, as the reference does
  l, ln = fn(a, b, all_affine2_to_1=torch.from_numpy(aff).to(dev()),
             all_mask_img1=torch.from_numpy(mask).to(dev()), lamb=lamb, half_T_side_dense=T,
             half_T_side_sparse_min=smin, half_T_side_sparse_max=smax)
  l.backward()
  ref = g["%s_%s_loss_f64" % (name, vname)]
  ref32 = g["%s_%s_loss_f32" % (name, vname)]
  tol = max(1e-5 * abs(ref[0]) + 2e-7, 2 * abs(ref32[0] - ref[0]))
  assert abs(l.item() - ref[0]) <= tol, (name, l.item(), ref[0], ref32[0])
  assert abs(ln.item() - ref[1]) <= max(1e-5 * abs(ref[1]) + 2e-7, 2 * abs(ref32[1] - ref[1]))
  for t, key in ((a, "dx1"), (b, "dx2")):
    g64 = g["%s_%s_%s" % (name, vname, key)].astype(np.float64)
    nrm = np.linalg.norm(g64)
    err = np.linalg.norm(t.grad.cpu().numpy().astype(np.float64) - g64) / nrm
    # the stored gradients are the float64 run rounded to float32 (6e-8); MI ~ 0 cases are
    # cancellation-limited exactly like the clustering loss (DESIGN.md parity tiers)
    assert err <= 5e-5, (name, key, err)


def test_affine_warp_matches_grid_sample():
  """csrc/warp.hip vs F.affine_grid + F.grid_sample (perform_affine_tf, transforms.py:131-143)."""
  from iic_amd import seg_losses
  from oracle.gen_golden_seg2 import random_affines
  torch.manual_seed(0)
  for (n, k, h, w) in ((3, 5, 17, 23), (2, 24, 40, 40)):
    x = torch.rand(n, k, h, w)
    aff = torch.from_numpy(random_affines(n, 3))
    for ac in (False, True):
      seg_losses.ALIGN_CORNERS[0] = ac
      try:
        xd = x.to(dev()).requires_grad_(True)
        mats = seg_losses._pixel_matrices(aff, h, w).to(dev())
        out = seg_losses._AffineWarpFn.apply(xd, mats, 0, 0)
        gout = torch.rand(n, k, h, w)
        out.backward(gout.to(dev()))
      finally:
        seg_losses.ALIGN_CORNERS[0] = False
      xr = x.clone().double().requires_grad_(True)
      grid = torch.nn.functional.affine_grid(aff.double(), list(x.shape), align_corners=ac)
      ref = torch.nn.functional.grid_sample(xr, grid, padding_mode="zeros", align_corners=ac)
      ref.backward(gout.double())
      assert (out.detach().cpu().double() - ref.detach()).abs().max() < 2e-5
      assert (xd.grad.cpu().double() - xr.grad).abs().max() < 2e-5 * max(1.0, float(xr.grad.abs().max()))


@pytest.mark.parametrize("bn,k,h,w,T", [(2, 24, 14, 200, 10), (3, 15, 20, 128, 10), (2, 3, 9, 200, 1),
                                        (2, 9, 11, 64, 3), (1, 32, 7, 40, 2), (2, 16, 6, 8, 1),
                                        (2, 5, 6, 8, 0), (3, 24, 1, 12, 2), (1, 1, 5, 256, 10), (2, 17, 3, 132, 4),
                                        (1, 36, 5, 200, 5), (2, 45, 4, 128, 10), (2, 48, 3, 40, 1), (1, 33, 4, 132, 3)])
@pytest.mark.parametrize("collapsed", [False, True])
@pytest.mark.hooks
def test_stream_kernels_match_generic_kernels_bitwise(bn, k, h, w, T, collapsed):
  """The float4 / prefetching kernels (default when w % 4 == 0, k <= 32) against the element-wise
  generic ones, same inputs incl. per-image x/y flips and a blob mask, at the BASELINE row widths
  (200, 128): same tiles and MFMA order, so partial joints and both gradients must be bit-equal."""
  import ctypes
  from iic_amd import _lib
  from iic_amd._lib import check, lib, ptr, stream_ptr
  L, dbg = lib(), ctypes.CDLL(_lib.LIB_PATH)
  g = torch.Generator().manual_seed(7 + k + w)
  x1 = torch.softmax(torch.randn(bn, k, h, w, generator=g) * 2, 1).to(dev())
  x2 = torch.softmax(torch.randn(bn, k, h, w, generator=g) * 2, 1).to(dev())
  mask = (torch.rand(bn, h, w, generator=g) < 0.6).float().to(dev())
  flips = torch.tensor([[i & 1, (i >> 1) & 1] for i in range(1, bn + 1)], dtype=torch.int32).to(dev())
  nq = 2 * T + 1
  H = 1 if collapsed else nq * nq
  dR1 = torch.randn(H, k, k, generator=g).to(dev())
  dR2 = torch.randn(H, k, k, generator=g).to(dev())
  g1 = torch.randn(H, generator=g).to(dev())
  g2 = torch.randn(H, generator=g).to(dev())
  ns = L.iic_seg_joint_nsplit(bn, h, k, T)
  res = {}
  try:
    dbg.iic_debug_seg_bf16(0)       # (the bf16-split joint of round 6 agrees to rounding, not bitwise: its own test below)
    for mode in (0, 1):
      dbg.iic_debug_seg_stream(mode)
      part = torch.full((ns, nq * nq, k, k), float("nan"), device=dev())
      check(L.iic_seg_joint_raw(ptr(x1), ptr(x2), ptr(mask), ptr(flips), ptr(part), bn, k, h, w, T, ns,
                                stream_ptr()), "joint")
      ws = torch.empty(L.iic_seg_grad_workspace_bytes(k, T) // 4, device=dev())
      outs = []
      for which, src in ((0, x2), (1, x1)):
        o = torch.full_like(x1, float("nan"))
        check(L.iic_seg_grad(ptr(src), ptr(mask), ptr(flips), ptr(dR1), ptr(dR2), ptr(g1), ptr(g2), ptr(o),
                             bn, k, h, w, T, which, 1 if collapsed else 0, ptr(ws), stream_ptr()), "grad")
        outs.append(o)
      torch.cuda.synchronize()
      res[mode] = (part, outs[0], outs[1])
  finally:
    dbg.iic_debug_seg_stream(1)
    dbg.iic_debug_seg_bf16(1)
  for i, (a, b) in enumerate(zip(res[0], res[1])):
    assert torch.isfinite(a).all()
    if i == 0 or k % 4 == 0:
      assert torch.equal(a, b), float((a - b).abs().max())
    else:
      # gradient kernel, k % 4 != 0: the streaming kernel pads the classes of every column shift to
      # a multiple of 4, so its MFMA steps group the same products differently (rounding only)
      assert float((a - b).norm() / a.norm()) <= 2e-6


@pytest.mark.parametrize("bn,k,h,w,T", [(3, 15, 20, 128, 10), (2, 24, 14, 200, 10), (2, 3, 9, 200, 5), (2, 9, 11, 64, 3),
                                        (1, 32, 7, 40, 2), (2, 16, 6, 8, 1), (1, 1, 5, 256, 10), (2, 17, 3, 132, 4),
                                        # three class tiles: the bf16 joint has none, mode 2 stays on the fp32 one
                                        (2, 45, 4, 128, 10), (1, 33, 4, 132, 3)])
@pytest.mark.parametrize("collapsed", [False, True])
@pytest.mark.hooks
def test_bf16_split_kernels_match_the_exact_fp32_mfma_kernels(bn, k, h, w, T, collapsed):
  """Round 6: the joint on the bf16 matrix pipe (every fp32 operand element as three bf16 terms, six
  v_mfma_f32_16x16x32_bf16 per product; the product path uses it at k <= 16, T >= 5) against the exact-fp32 MFMA kernel
  on the same inputs -- per-image flips, a blob mask, ragged class counts and widths: the dropped terms are below 2^-24
  of a product, so the two agree to fp32 summation noise.  The switch serves the joint only: the gradient has no bf16
  kernel (retired, LAB.md S17), so under mode 2 the gradient cases check the fp32 kernels a second time."""
  import ctypes
  from iic_amd import _lib
  from iic_amd._lib import check, lib, ptr, stream_ptr
  L, dbg = lib(), ctypes.CDLL(_lib.LIB_PATH)
  g = torch.Generator().manual_seed(17 + k + w)
  x1 = torch.softmax(torch.randn(bn, k, h, w, generator=g) * 2, 1).to(dev())
  x2 = torch.softmax(torch.randn(bn, k, h, w, generator=g) * 2, 1).to(dev())
  mask = (torch.rand(bn, h, w, generator=g) < 0.6).float().to(dev())
  flips = torch.tensor([[i & 1, (i >> 1) & 1] for i in range(1, bn + 1)], dtype=torch.int32).to(dev())
  nq = 2 * T + 1
  H = 1 if collapsed else nq * nq
  dR1 = torch.randn(H, k, k, generator=g).to(dev())
  dR2 = torch.randn(H, k, k, generator=g).to(dev())
  g1 = torch.randn(H, generator=g).to(dev())
  g2 = torch.randn(H, generator=g).to(dev())
  ns = L.iic_seg_joint_nsplit(bn, h, k, T)
  res = {}
  try:
    for mode in (0, 2):
      dbg.iic_debug_seg_bf16(mode)
      part = torch.full((ns, nq * nq, k, k), float("nan"), device=dev())
      check(L.iic_seg_joint_raw(ptr(x1), ptr(x2), ptr(mask), ptr(flips), ptr(part), bn, k, h, w, T, ns,
                                stream_ptr()), "joint")
      ws = torch.empty(L.iic_seg_grad_workspace_bytes(k, T) // 4, device=dev())
      outs = []
      for which, src in ((0, x2), (1, x1)):
        o = torch.full_like(x1, float("nan"))
        check(L.iic_seg_grad(ptr(src), ptr(mask), ptr(flips), ptr(dR1), ptr(dR2), ptr(g1), ptr(g2), ptr(o),
                             bn, k, h, w, T, which, 1 if collapsed else 0, ptr(ws), stream_ptr()), "grad")
        outs.append(o)
      torch.cuda.synchronize()
      res[mode] = (part.double().sum(0), outs[0], outs[1])
  finally:
    dbg.iic_debug_seg_bf16(1)
  a, b = res[0], res[2]
  assert all(torch.isfinite(t).all() for t in b)
  assert float((a[0] - b[0]).abs().max()) <= 2e-6 * float(a[0].abs().max()), float((a[0] - b[0]).abs().max() / a[0].abs().max())
  for i in (1, 2):
    assert float((a[i] - b[i]).norm() / a[i].norm()) <= 5e-6, float((a[i] - b[i]).norm() / a[i].norm())


@pytest.mark.parametrize("name,bn,k,h,w,T,dens", [("potsdam3", 75, 24, 200, 200, 10, 1.0),
                                                  ("coco3", 120, 15, 128, 128, 10, 0.6)])
def test_full_size_joint_and_gradient_vs_independent_float64(name, bn, k, h, w, T, dens):
  """BASELINE.json shapes at FULL size (the oracle only finishes reduced sizes in seconds):
  (1) checksum of checksums -- softmax rows sum to 1, so sum_ij R_t[i][j] must equal the mask's
      autocorrelation at t (integers, computed independently);
  (2) sampled shifts of the joint against a float64 torch contraction of the shifted slices;
  (3) the gradient kernel on sampled output pixels against the closed form
      dX1_i(n,v) = mask(v) * sum_t sum_j G_t[i][j] x2m_j(n, v - t) in float64, plus linearity in G."""
  from iic_amd._lib import check, lib, ptr, stream_ptr
  L = lib()
  g = torch.Generator().manual_seed(11)
  x1 = torch.softmax(torch.randn(bn, k, h, w, generator=g) * 2, 1).to(dev())
  x2 = torch.softmax(torch.randn(bn, k, h, w, generator=g) * 2, 1).to(dev())
  mask = (torch.rand(bn, h, w, generator=g) < dens).float().to(dev())
  fl = torch.tensor([[i & 1, (i >> 1) & 1] for i in range(bn)], dtype=torch.int32)
  flips = fl.to(dev())
  nq = 2 * T + 1
  ns = L.iic_seg_joint_nsplit(bn, h, k, T)
  part = torch.empty((ns, nq * nq, k, k), device=dev())
  check(L.iic_seg_joint_raw(ptr(x1), ptr(x2), ptr(mask), ptr(flips), ptr(part), bn, k, h, w, T, ns, stream_ptr()), "joint")
  R = part.double().sum(0).view(nq, nq, k, k)                     # [p][q][i][j]
  # masked / inverse-warped maps in float64, independent of the kernels
  x2i = x2.double().clone()
  for n in range(bn):
    dims = [d for d, f in ((2, int(fl[n, 0])), (1, int(fl[n, 1]))) if f]
    if dims:
      x2i[n] = torch.flip(x2i[n], dims)
  m64 = mask.double()
  x1m, x2m = x1.double() * m64[:, None], x2i * m64[:, None]

  def shifted(a, ty, tx):     # a(n, ., y + ty, x + tx), zero outside
    out = torch.zeros_like(a)
    ys, ye = max(0, -ty), min(h, h - ty)
    xs, xe = max(0, -tx), min(w, w - tx)
    out[..., ys:ye, xs:xe] = a[..., ys + ty:ye + ty, xs + tx:xe + tx]
    return out

  # (1) every shift: sum_ij R_t = sum_u mask(u + t) mask(u)
  tot = R.sum((2, 3))
  for p in range(nq):
    for q in (0, T, nq - 1, (3 * p) % nq):
      want = float((shifted(m64, p - T, q - T) * m64).sum())
      assert abs(float(tot[p, q]) - want) <= 2e-5 * max(want, 1.0), (p, q, float(tot[p, q]), want)
  # (2) sampled shifts, all k x k entries
  for p, q in ((0, 0), (T, T), (nq - 1, 3), (4, nq - 1), (T + 1, T - 2)):
    want = torch.einsum("nihw,njhw->ij", shifted(x1m, p - T, q - T), x2m)
    err = float((R[p, q] - want).abs().max() / want.abs().max())
    assert err <= 2e-5, (p, q, err)
  # (3) gradient w.r.t. x1 on sampled pixels; G random per shift
  H = nq * nq
  dR1 = torch.randn(H, k, k, generator=g).to(dev())
  dR2 = torch.randn(H, k, k, generator=g).to(dev())
  g1 = torch.randn(H, generator=g).to(dev())
  g2 = torch.randn(H, generator=g).to(dev())
  ws = torch.empty(L.iic_seg_grad_workspace_bytes(k, T) // 4, device=dev())

  def grad(which, src, a, b):
    o = torch.empty_like(x1)
    check(L.iic_seg_grad(ptr(src), ptr(mask), ptr(flips), ptr(a), ptr(b), ptr(g1), ptr(g2), ptr(o), bn, k, h, w, T,
                         which, 0, ptr(ws), stream_ptr()), "grad")
    return o

  dx1 = grad(0, x2, dR1, dR2)
  G = (g1.double()[:, None, None] * dR1.double() + g2.double()[:, None, None] * dR2.double()).view(nq, nq, k, k)
  x2p = torch.nn.functional.pad(x2m, (T, T, T, T))                # zero padded, index + T
  rs = torch.Generator().manual_seed(5)
  for _ in range(40):
    n = int(torch.randint(bn, (1,), generator=rs)); y = int(torch.randint(h, (1,), generator=rs))
    x = int(torch.randint(w, (1,), generator=rs))
    if _ % 4 == 0:
      y, x = (0, w - 1) if _ % 8 == 0 else (h - 1, 0)              # corners: the halo paths
    win = x2p[n, :, y:y + nq, x:x + nq].flip(1, 2)                 # win[j][p][q] = x2m_j(v - t), t = (p - T, q - T)
    want = torch.einsum("pqij,jpq->i", G, win) * m64[n, y, x]
    got = dx1[n, :, y, x].double()
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max() + 1e-3), (n, y, x)
  # linearity in G: grad(dR1 + dR1', .) = grad(dR1, .) + grad(dR1', .)  (dR2 weight set to zero)
  zero = torch.zeros_like(dR2)
  a = grad(1, x1, dR1, zero)
  b = grad(1, x1, dR2, zero)
  c = grad(1, x1, dR1 + dR2, zero)
  assert float((a + b - c).norm() / c.norm()) <= 1e-5
