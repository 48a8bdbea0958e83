"""The segmentation loss and the up-sampling beyond 48 classes and 256-pixel rows (csrc/seg_loss_tiled.hip, the windowed
kernels of csrc/seg_head.hip): the tiled joint and its four gradients EXACTLY on the dyadic-lattice cases of
tests/seg_tiled_cases.py (proved without a GPU by tests/test_seg_tiled_cpu.py), bit-reproducible, with the bits of today's
kernels on the shapes both serve; the joint on full-mantissa operands inside the accumulation bound of its family; the
public losses against the float64 oracle; the windowed up-sampling bit for bit against the resident kernels and, on the
shapes those refuse, against float64; the k > 32 head's weight gradient from fixed-order partials (iic_seg_window_wgrad),
exact and reproducible; and one training step of the two-head network at input_sz = 264, k_A = 64.  pytest -m gpu.

Every output buffer starts as NaN: an element never written fails."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import iid_stage_cases as sc
from tests import seg_tiled_cases as tc
from tests.conftest import hook
from tests.lattice import assert_exact, record
from tests.parity import WORST, assert_bits, assert_within, dev, fma_acc_bound_each, ok

pytestmark = pytest.mark.gpu
HOOKS = pytest.mark.hooks
NAN = float("nan")
PATH_NONE, PATH_RESIDENT, PATH_TILED = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
  yield
  record(file="test_gpu_seg_tiled", worst={f: WORST[f] for f in ("seg_joint_tiled", "bilinear_win_fwd") if f in WORST})


def L():
  from iic_amd import _lib
  return _lib.lib()


def nan_like(shape):
  return torch.full(tuple(shape), NAN, device=dev())


def shifted_copy(t, off):
  """The tensor's values at an address `off` floats past a 256-byte boundary: off = 1 leaves no 16-byte alignment."""
  buf = torch.empty(t.numel() + 64, dtype=t.dtype, device=dev())
  assert buf.data_ptr() % 256 == 0
  v = buf[off:off + t.numel()].view(t.shape)
  v.copy_(t)
  return v


def tiled_partials(inp, ns, off=0):
  bn, k, h, w, T = inp["case"]
  nq = 2 * T + 1
  part = shifted_copy(nan_like((ns, nq * nq, k, k)), off)
  ok("iic_seg_tiled_joint_raw", shifted_copy(inp["x1"], off), shifted_copy(inp["x2"], off), shifted_copy(inp["mask"], off),
     inp["flips"].to(dev()), part, bn, k, h, w, T, ns)
  return part.cpu()


def fold(part, case):
  nq = 2 * case[4] + 1
  return part.double().sum(0).view(nq, nq, case[1], case[1])


def tiled_grad(inp, which, collapsed, off=0):
  bn, k, h, w, T = inp["case"]
  n = "c" if collapsed else "u"
  src = shifted_copy(inp["x2" if which == 0 else "x1"], off)
  ws = nan_like((L().iic_seg_tiled_grad_workspace_bytes(k, T, 1 if collapsed else 0) // 4,))
  out = shifted_copy(nan_like(src.shape), off)
  d = dev()
  ok("iic_seg_tiled_grad", src, shifted_copy(inp["mask"], off), inp["flips"].to(d), inp["dR1" + n].to(d),
     inp["dR2" + n].to(d), inp["gl" + n].to(d), inp["gnl" + n].to(d), out, bn, k, h, w, T, which, 1 if collapsed else 0, ws)
  return out.cpu()


def split_counts(case):
  """The rule of tests/test_gpu_iid_stages.py: 1, the recommended count, bn h, and one that does not divide bn h."""
  bn, k, h, w, T = case
  rows = bn * h
  odd = next(n for n in (3, 4, 5, 7) if rows % n)
  return sorted(set([1, L().iic_seg_tiled_joint_nsplit(bn, h, w, k, T), rows, odd]))


# ---- 1. joint and four gradients, exact and reproducible ------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.CASES)
def test_tiled_joint_exact(case):
  bn, k, h, w, T = case
  assert L().iic_seg_loss_path(k, w, T) == PATH_TILED
  inp, ref = tc.inputs(case), tc.reference(case)
  for ns in split_counts(case):
    first = tiled_partials(inp, ns)
    assert_exact(fold(first, case), ref["R"], "joint %s nsplit %d" % (case, ns))
    assert_bits(tiled_partials(inp, ns), first, "joint %s nsplit %d, second run" % (case, ns))
  # the same bits from tensors without 16-byte alignment: one form, whatever the alignment
  ns = L().iic_seg_tiled_joint_nsplit(bn, h, w, k, T)
  assert_bits(tiled_partials(inp, ns, off=1), tiled_partials(inp, ns), "joint %s unaligned" % (case,))


@pytest.mark.parametrize("case", tc.CASES)
def test_tiled_grad_exact(case):
  bn, k, h, w, T = case
  inp, ref = tc.inputs(case), tc.reference(case)
  if bn * h > 1 and w > 1:      # the flips move the second gradient: a kernel that stores it unflipped differs from the reference
    assert not torch.equal(ref["du1"], sc.flip_samples(ref["du1"], inp["flips"]))
  for collapsed in (False, True):
    for which in (0, 1):
      name = "d%s%d" % ("c" if collapsed else "u", which)
      what = "gradient %s which %d collapsed %d" % (case, which, collapsed)
      first = tiled_grad(inp, which, collapsed)
      assert_exact(first, ref[name], what)
      assert_bits(tiled_grad(inp, which, collapsed), first, what + ", second run")
      assert_bits(tiled_grad(inp, which, collapsed, off=1), first, what + ", unaligned")


# ---- 2. the bits of today's kernels on the shapes both serve --------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.SHARED)
def test_tiled_entries_give_the_bits_of_the_resident_kernels(case):
  """On the lattice any order is exact, so this holds by construction and catches indexing only."""
  bn, k, h, w, T = case
  assert L().iic_seg_loss_path(k, w, T) == PATH_RESIDENT
  inp = sc.seg_inputs(case)
  d = dev()
  nq = 2 * T + 1
  ns = L().iic_seg_joint_nsplit(bn, h, k, T)
  part = nan_like((ns, nq * nq, k, k))
  ok("iic_seg_joint_raw", inp["x1"].to(d), inp["x2"].to(d), inp["mask"].to(d), inp["flips"].to(d), part, bn, k, h, w, T, ns)
  want = fold(part.cpu(), case)
  for nt in split_counts(case):
    got = fold(tiled_partials(inp, nt), case)
    assert torch.equal(got, want), "joint %s: float64 sums of the partials differ (tiled nsplit %d)" % (case, nt)
  for collapsed in (False, True):
    n = "c" if collapsed else "u"
    for which in (0, 1):
      src = inp["x2" if which == 0 else "x1"].to(d)
      ws = torch.empty(L().iic_seg_grad_workspace_bytes(k, T) // 4, device=d)
      out = nan_like(src.shape)
      ok("iic_seg_grad", src, inp["mask"].to(d), inp["flips"].to(d), inp["dR1" + n].to(d), inp["dR2" + n].to(d),
         inp["gl" + n].to(d), inp["gnl" + n].to(d), out, bn, k, h, w, T, which, 1 if collapsed else 0, ws)
      assert_bits(tiled_grad(inp, which, collapsed), out, "gradient %s which %d collapsed %d" % (case, which, collapsed))


# ---- 3. full-mantissa joint -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.F64_CASES)
def test_tiled_joint_full_mantissa_within_its_family_bound(case):
  bn, k, h, w, T = case
  f = sc.seg_f64_inputs(case)
  x1m, x2m = sc.seg_maps(f["x1"], f["x2"], f["mask"], f["flips"])
  ref = sc.seg_joint_ref(x1m, x2m, T)      # operands >= 0: the reference is its own magnitude sum A
  bound = fma_acc_bound_each(sc.seg_terms(case)[:, :, None, None], ref)
  first = tiled_partials(f, L().iic_seg_tiled_joint_nsplit(bn, h, w, k, T))
  assert_within(fold(first, case), ref, bound, "joint %s" % (case,), "seg_joint_tiled")
  assert_bits(tiled_partials(f, L().iic_seg_tiled_joint_nsplit(bn, h, w, k, T), off=1), first, "joint %s unaligned" % (case,))


# ---- 4. the public functions ----------------------------------------------------------------------------------------------------
def _oracle(fn, x1, x2, aff, mask, lamb, T, dtype):
  a = torch.from_numpy(x1).to(dtype).requires_grad_(True)
  b = torch.from_numpy(x2).to(dtype).requires_grad_(True)
  r, rn = fn(a, b, all_affine2_to_1=torch.from_numpy(aff).to(dtype), all_mask_img1=torch.from_numpy(mask).to(dtype),
             lamb=lamb, half_T_side_dense=T)
  (r + 0.5 * rn).backward()
  return float(r), float(rn), a.grad.double(), b.grad.double()


@pytest.mark.parametrize("bn,k,h,w,T", [(2, 49, 6, 260, 2), (1, 64, 8, 264, 10), (2, 97, 5, 12, 1),
                                        # 12 rows: every one of the 21 x 21 shifts overlaps, the uncollapsed loss is finite
                                        (1, 64, 12, 264, 10)])
@pytest.mark.parametrize("collapsed", [False, True])
def test_public_losses_vs_oracle(bn, k, h, w, T, collapsed):
  """Tolerances of tests/test_gpu_seg_loss.py::_check: loss 1e-5 |ref| + 2e-7; gradient, relative norm, max(2e-5, e32), e32
  the error of the same oracle evaluated in float32 on the CPU (measured against the reference, never against the kernels)."""
  from iic_amd import seg_losses
  from oracle import iid_oracle
  from oracle.gen_golden import make_seg_inputs
  x1, x2, aff, mask = make_seg_inputs(bn, k, h, w, 0.5, 0.8, 7)
  aff[-1, 1, 1] = -1.0   # also a y-flip on the last sample
  fh = seg_losses.IID_segmentation_loss if collapsed else seg_losses.IID_segmentation_loss_uncollapsed
  fr = iid_oracle.IID_segmentation_loss if collapsed else iid_oracle.IID_segmentation_loss_uncollapsed
  a = torch.from_numpy(x1).to(dev()).requires_grad_(True)
  b = torch.from_numpy(x2).to(dev()).requires_grad_(True)
  l, ln = fh(a, b, all_affine2_to_1=torch.from_numpy(aff).to(dev()), all_mask_img1=torch.from_numpy(mask).to(dev()),
             lamb=1.5, half_T_side_dense=T, half_T_side_sparse_min=0, half_T_side_sparse_max=0)
  (l + 0.5 * ln).backward()
  r, rn, ga, gb = _oracle(fr, x1, x2, aff, mask, 1.5, T, torch.float64)
  _, _, ga32, gb32 = _oracle(fr, x1, x2, aff, mask, 1.5, T, torch.float32)
  print("loss %.9g ref %.9g | no-lamb %.9g ref %.9g" % (l.item(), r, ln.item(), rn))
  if not collapsed and h <= T:
    # shifts of 8 rows or more leave no overlap in an 8-row image: their joint is all zero and the uncollapsed loss, which
    # normalises every shift by its own sum (IID_losses.py:130-157), is 0 / 0 in the reference -- NaN there, NaN here
    # (tests/test_gpu_seg_loss.py::test_seg_loss_shift_range_beyond_the_image_is_nan_like_the_reference)
    assert np.isnan(r) and np.isnan(rn) and np.isnan(l.item()) and np.isnan(ln.item()), (l.item(), r)
    return
  assert abs(l.item() - r) <= 1e-5 * abs(r) + 2e-7, (l.item(), r)
  assert abs(ln.item() - rn) <= 1e-5 * abs(rn) + 2e-7, (ln.item(), rn)
  for mine, ref, ref32 in ((a.grad.cpu().double(), ga, ga32), (b.grad.cpu().double(), gb, gb32)):
    err = float((mine - ref).norm() / ref.norm())
    e32 = float((ref32 - ref).norm() / ref.norm())
    print("gradient: relative norm error %.3e, float32 oracle %.3e" % (err, e32))
    assert err <= max(2e-5, e32), (err, e32)


def test_public_loss_names_the_limit_it_refuses():
  from iic_amd import seg_losses
  from iic_amd._lib import IICLibraryError
  from oracle.gen_golden import make_seg_inputs
  assert L().iic_seg_loss_path(49, 16, 11) == PATH_NONE and L().iic_seg_loss_path(5, 16, 11) == PATH_NONE
  tmax = L().iic_seg_tiled_limit(1)
  assert (L().iic_seg_tiled_limit(0), tmax) == (255, 10) and L().iic_seg_tiled_limit(2) >= 1024
  for k in (5, 49):
    x1, x2, aff, mask = make_seg_inputs(2, k, 24, 16, 0.5, 0.8, 7)
    a = torch.from_numpy(x1).to(dev()).requires_grad_(True)
    b = torch.from_numpy(x2).to(dev()).requires_grad_(True)
    with pytest.raises(IICLibraryError) as e:
      seg_losses.IID_segmentation_loss(a, b, all_affine2_to_1=torch.from_numpy(aff).to(dev()),
                                       all_mask_img1=torch.from_numpy(mask).to(dev()), lamb=1.0, half_T_side_dense=11)
    assert "half_T_side_dense <= %d" % tmax in str(e.value) and "IIC_ERR_UNSUPPORTED" in str(e.value), str(e.value)
  # the entries of the resident kernels refuse what they refused
  part = nan_like((1, 9, 49, 49))
  z = torch.zeros((1, 49, 2, 8), device=dev())
  from tests.parity import call
  assert call("iic_seg_joint_raw", z, z, z[:, 0], torch.zeros((1, 2), dtype=torch.int32, device=dev()), part, 1, 49, 2, 8, 1,
              1) == -3


# ---- 5. bilinear up-sampling ----------------------------------------------------------------------------------------------------
def _bl_inputs(N, Hl, Wl, k, S, seed=0):
  g = torch.Generator().manual_seed(1000 * seed + Hl + Wl + k + S)
  p = F.softmax(torch.randn((N, k, Hl, Wl), generator=g) * 3, dim=1)          # NCHW fp32, CPU
  dy = torch.randn((N, k, S, S), generator=g)
  return p, dy


def _bl_run(p, dy, S):
  N, k, Hl, Wl = p.shape
  xin = p.permute(0, 2, 3, 1).contiguous().to(dev())                            # [N][Hl][Wl][k]
  out = nan_like((N, k, S, S))
  ok("iic_bilinear_fwd", xin, out, N, Hl, Wl, k, S)
  din = nan_like((N, Hl, Wl, k))
  ok("iic_bilinear_bwd", dy.to(dev()), din, N, Hl, Wl, k, S)
  return xin, out.cpu(), din.cpu()


@HOOKS
@pytest.mark.parametrize("N,Hl,Wl,k,S", [(2, 10, 10, 3, 24), (2, 62, 62, 15, 128), (1, 4, 336, 24, 8)])
def test_windowed_bilinear_is_bit_equal_to_the_resident_form(N, Hl, Wl, k, S):
  p, dy = _bl_inputs(N, Hl, Wl, k, S)
  bwd = 2 * S <= 7 * Hl and 2 * S <= 7 * Wl      # (the backward serves up-sampling factors up to 3.5, in either form)
  if not bwd:
    dy = None
  def run():
    xin = p.permute(0, 2, 3, 1).contiguous().to(dev())
    out = nan_like((N, k, S, S))
    ok("iic_bilinear_fwd", xin, out, N, Hl, Wl, k, S)
    din = None
    if bwd:
      din = nan_like((N, Hl, Wl, k))
      ok("iic_bilinear_bwd", dy.to(dev()), din, N, Hl, Wl, k, S)
    return out.cpu(), din.cpu() if bwd else None
  want_out, want_din = run()
  try:
    hook("iic_debug_bilinear_window", 1)
    got_out, got_din = run()
  finally:
    hook("iic_debug_bilinear_window", 0)
  assert_bits(got_out, want_out, "forward %s" % ((N, Hl, Wl, k, S),))
  if bwd:
    assert_bits(got_din, want_din, "backward %s" % ((N, Hl, Wl, k, S),))


@pytest.mark.parametrize("N,Hl,Wl,k,S,fwd_windowed,bwd_windowed", [
  (1, 130, 130, 64, 264, True, False),      # 2 Wl k floats = 66 560 bytes: the forward was refused
  (1, 76, 160, 45, 264, False, False),      # 57 600 bytes: the resident kernels serve it; held to the same derived bound
  (1, 66, 66, 255, 132, True, True)])       # Wl k floats = 67 320 bytes: forward and backward were refused
def test_bilinear_at_shapes_beyond_the_resident_rows(N, Hl, Wl, k, S, fwd_windowed, bwd_windowed):
  """Forward against float64 F.interpolate(align_corners=False) within 2^-23 (Hl + Wl) D + 3 2^-24 V, D the largest
  difference of adjacent source pixels, V the largest |v|: the source coordinate carries at most two fp32 roundings (each
  moves the sample by at most 2^-24 of a coordinate below Hl or Wl, i.e. the value by that times D, along either axis), the
  blend three.  Backward against the float64 adjoint at 1e-4 max |ref|.  The label map is the arg-max of the forward."""
  assert (2 * Wl * k * 4 > 64 * 1024, Wl * k * 4 > 64 * 1024) == (fwd_windowed, bwd_windowed)
  p, dy = _bl_inputs(N, Hl, Wl, k, S)
  xin, out, din = _bl_run(p, dy, S)
  p64 = p.double().requires_grad_(True)
  ref = F.interpolate(p64, size=S, mode="bilinear", align_corners=False)
  ref.backward(dy.double())
  pd = p.double()
  D = max(float((pd[:, :, 1:] - pd[:, :, :-1]).abs().max()), float((pd[:, :, :, 1:] - pd[:, :, :, :-1]).abs().max()))
  V = float(pd.abs().max())
  bound = 2.0 ** -23 * (Hl + Wl) * D + 3 * 2.0 ** -24 * V
  assert_within(out, ref.detach(), bound, "forward %s" % ((N, Hl, Wl, k, S),), "bilinear_win_fwd")
  want = p64.grad.permute(0, 2, 3, 1)
  err = float((din.double() - want).abs().max())
  print("backward: max |err| %.3e, max |ref| %.3e" % (err, float(want.abs().max())))
  assert err <= 1e-4 * float(want.abs().max()), err
  lab = torch.full((N, S, S), 255, dtype=torch.uint8, device=dev())
  ok("iic_seg_label_map", xin, lab, N, Hl, Wl, k, S)
  assert np.array_equal(lab.cpu().numpy(), out.numpy().argmax(axis=1))


# ---- the head's weight gradient above 32 classes: fixed-order partials -----------------------------------------------------------
@pytest.mark.parametrize("M,C,k", [(2500, 256, 49), (1030, 512, 81), (5, 512, 3), (2049, 256, 255), (1024, 512, 64)])
def test_window_weight_gradient_exact_and_reproducible(M, C, k):
  """iic_seg_window_wgrad + iic_colsum_f32 on {-1, 0, +1} operands: every partial sum an integer below 2^24, so the float64
  reference must be met exactly; two runs give the same bits (the atomic split-K GEMM it replaces in the k > 32 head did
  not promise that)."""
  from tests.lattice import lattice
  rng = np.random.default_rng(M + C + k)
  dlog, Fm = lattice(rng, (M, k)), lattice(rng, (M, C))
  want = dlog.double().t() @ Fm.double()
  assert float(want.abs().max()) > 0 and M < 2 ** 24
  nch = L().iic_seg_head_wgrad_chunks(M)
  d = dev()

  def run():
    part, dW = nan_like((nch, k * C)), nan_like((k, C))
    ok("iic_seg_window_wgrad", dlog.to(d), Fm.to(d), part, M, C, k)
    ok("iic_colsum_f32", part, dW, nch, k * C, 0)
    return dW.cpu()
  first = run()
  assert_exact(first, want, "dW %s" % ((M, C, k),))
  assert_bits(run(), first, "dW %s, second run" % ((M, C, k),))
  from tests.parity import call
  assert call("iic_seg_window_wgrad", dlog.to(d), Fm.to(d), nan_like((nch, k * 384)), M, 384, k) == -3


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False])
def test_two_head_network_trains_at_264_pixels_and_64_classes(train):
  from iic_amd import archs, seg_losses
  torch.manual_seed(3)
  S, n = 264, 2
  cfg = types.SimpleNamespace(in_channels=4, input_sz=S, batchnorm_track=True, num_sub_heads=1, output_k_A=64, output_k_B=3)
  net = archs.SegmentationNet10aTwoHead(cfg).to(dev())
  net.train(train)
  state = copy.deepcopy(net.state_dict())
  rng = np.random.default_rng(5)
  img1 = torch.from_numpy(rng.random((n, 4, S, S)).astype(np.float32)).to(dev())
  img2 = torch.flip(img1, dims=[3]) + 0.05 * torch.from_numpy(rng.standard_normal((n, 4, S, S)).astype(np.float32)).to(dev())
  aff = torch.zeros((n, 2, 3))
  aff[:, 0, 0], aff[:, 1, 1] = -1.0, 1.0
  mask = torch.from_numpy((rng.random((n, S, S)) < 0.9).astype(np.float32)).to(dev())

  def step():
    net.load_state_dict(state)
    net.zero_grad(set_to_none=True)
    x1, x2 = net(img1, head="A"), net(img2, head="A")
    assert tuple(x1[0].shape) == (n, 64, S, S)
    loss, loss_nl = seg_losses.IID_segmentation_loss(x1[0], x2[0], all_affine2_to_1=aff.to(dev()), all_mask_img1=mask,
                                                     lamb=1.0, half_T_side_dense=10, half_T_side_sparse_min=0,
                                                     half_T_side_sparse_max=0)
    loss.backward()
    torch.cuda.synchronize()
    unused = [name for name, p in net.named_parameters() if p.grad is None]
    assert unused and all(name.startswith("head_B.") for name in unused), unused      # head A's step: head B takes no part
    return loss.detach().cpu(), {name: p.grad.detach().cpu().clone() for name, p in net.named_parameters()
                                 if p.grad is not None}

  loss1, g1 = step()
  loss2, g2 = step()
  assert bool(torch.isfinite(loss1)), loss1
  for name, g in g1.items():
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
    assert_bits(g2[name], g, "second run, %s" % name)
  assert_bits(loss2, loss1, "second run, loss")
  with torch.no_grad():
    labels = net.predict_labels(img1, head="A")[0]
    out = net(img1, head="A")[0]
  assert np.array_equal(labels.cpu().numpy(), out.cpu().numpy().argmax(axis=1))
