"""float64 parity for exported kernels that no kernel-level test reached: pools, column sums, the segmentation head's
window copies, deferred running statistics, the one-launch weight preparation, equality counts, the device-counter Adam
and the streaming kernels of the exact-fp32 path (csrc/f32_path.hip), which other tests use as their yardstick.

References are plain torch-CPU / numpy in float64.  Tolerances are derived, not tuned: U32 = 2^-24 per fp32 operation
and U16 = 2^-8 per bf16 store -- one unit in the last place each, so neither round-to-nearest nor truncation is presumed
for an intermediate; an n-term fp32 sum gets n * U32 * sum |terms|.  Kernels that move or select data without arithmetic
are held to bit equality.  Output buffers are pre-filled with a sentinel wherever the header promises that only interior
pixels are written (include/iic_hip.h: "Kernels only ever write interior pixels").
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.parity import (SENTINEL, U16, U32, _mask_act, _masked_g, _pow2_coef, assert_bits, assert_border,  # noqa: F401
                          assert_within, bits, call, dev, interior, ok, pt_of, rnd)

IIC_ERR_ARG = -1


POOL_SHAPES = [(5, 7, 7, 1, 512), (3, 3, 5, 2, 64), (1, 1, 1, 1, 64), (2, 13, 9, 1, 130)]


# --------------------------------------------------------------------------------------
# iic_avgpool_fwd / iic_avgpool_bwd (bf16 PT -> fp32 features) and their fp32 twins
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("N,H,W,P,C", POOL_SHAPES)
def test_avgpool_forward_backward_vs_float64(N, H, W, P, C, fp32):
  """iic_avgpool_fwd / iic_avgpool_bwd and iic_f32_avgpool_fwd / iic_f32_avgpool_bwd.  Forward: the H*W-term fp32 sum
  scaled to the mean, H*W * U32 * mean|x|, plus U32 * |ref| for the multiplication by the rounded 1/(H*W).  Backward:
  dfeats * fl(1/(H*W)) is one fp32 product of a rounded factor (U32 * |ref|; 2 * U32 when the fp32 twin stores it
  unrounded and both roundings count in full) and the bf16 store adds U16 * |ref|; with mask_act exactly zero where
  act <= 0 (-0 and negative values included).  The border of the PT gradient is not written (header: interiors only)."""
  rng = np.random.default_rng(N * 1000 + C)
  dt = torch.float32 if fp32 else torch.bfloat16
  pre = "iic_f32_avgpool" if fp32 else "iic_avgpool"
  x = rnd(rng, N, H, W, C).to(dt)
  feats = torch.full((N, C), SENTINEL, device=dev())
  ok(pre + "_fwd", pt_of(x, P, dt), feats, N, H, W, P, C)
  xd = x.double()
  ref = xd.mean((1, 2))
  assert_within(feats, ref, H * W * U32 * xd.abs().mean((1, 2)) + U32 * ref.abs(), "avgpool forward")
  dfeats = rnd(rng, N, C)
  ref_b = (dfeats.double() / (H * W)).view(N, 1, 1, C).expand(N, H, W, C)
  tol_b = (2 * U32 if fp32 else U16 + U32) * ref_b.abs()
  for masked in (False, True):
    act = _mask_act(rng, N, H, W, C).to(dt)
    din = torch.full((N, H + 2 * P, W + 2 * P, C), SENTINEL, dtype=dt, device=dev())
    ok(pre + "_bwd", dfeats.to(dev()), din, N, H, W, P, C, pt_of(act, P, dt) if masked else None)
    got = interior(din, P)
    assert_border(din, P, SENTINEL, "avgpool backward")
    if masked:
      keep = act.float() > 0
      assert 0.2 < float(keep.float().mean()) < 0.8
      assert bool((got.float()[~keep] == 0).all()), "gradient not zero where the activation is <= 0"
      assert_within(got[keep], ref_b[keep], tol_b[keep], "avgpool backward (masked)")
    else:
      assert_within(got, ref_b, tol_b, "avgpool backward")


def test_avgpool_odd_channel_count_is_an_argument_error():
  t = torch.zeros(3 * 3 * 66, dtype=torch.bfloat16, device=dev())
  f = torch.zeros(66, device=dev())
  assert call("iic_avgpool_fwd", t, f, 1, 1, 1, 1, 65) == IIC_ERR_ARG
  assert call("iic_avgpool_bwd", f, t, 1, 1, 1, 1, 65, None) == IIC_ERR_ARG


# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 3), (700, 50), (1320, 70), (4097, 33), (3, 257)])
def test_colsum_f32_vs_float64(rows, cols, accumulate):
  """iic_colsum_f32: an n-term fp32 sum per column (n = rows, + 1 for the previous contents when accumulating) in
  whatever order: n * U32 * sum |terms|."""
  rng = np.random.default_rng(rows + cols)
  A, prev = rnd(rng, rows, cols), rnd(rng, cols)
  out = prev.clone().to(dev())
  ok("iic_colsum_f32", A.to(dev()), out, rows, cols, accumulate)
  ref, mag, n = A.double().sum(0), A.double().abs().sum(0), rows
  if accumulate:
    ref, mag, n = ref + prev.double(), mag + prev.double().abs(), rows + 1
  assert_within(out, ref, n * U32 * mag, "column sums")


# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("C", [8, 64, 512])
@pytest.mark.parametrize("N,Hw,Ww,off", [(2, 6, 9, 0), (2, 7, 5, 2), (1, 3, 4, 1)])
def test_window_gather_scatter_move_bits(N, Hw, Ww, off, C, fp32):
  """iic_seg_window_gather / iic_seg_window_scatter and iic_f32_window_gather / iic_f32_window_scatter: the gather is
  bit-equal to slicing the window out of the PT tensor; the scatter writes the window's interior (its first ring is the
  1x1 conv's padding) and nothing else, bit-equal to torch's fp32 -> bf16 conversion."""
  rng = np.random.default_rng(C + Hw)
  dt = torch.float32 if fp32 else torch.bfloat16
  pre = "iic_f32_window" if fp32 else "iic_seg_window"
  Hp, Wp = Hw + 2 * off + 1, Ww + 2 * off + 2
  pt = rnd(rng, N, Hp, Wp, C).to(dt)
  out = torch.full((N * Hw * Ww, C), SENTINEL, device=dev())
  ok(pre + "_gather", pt.to(dev()), out, N, Hw, Ww, Hp, Wp, off, C)
  assert_bits(out, pt[:, off:off + Hw, off:off + Ww].float().reshape(N * Hw * Ww, C), "window gather")
  src = rnd(rng, N, Hw, Ww, C)
  dst = torch.full((N, Hp, Wp, C), SENTINEL, dtype=dt, device=dev())
  ok(pre + "_scatter", src.to(dev()), dst, N, Hw, Ww, Hp, Wp, off, C)
  want = torch.full((N, Hp, Wp, C), SENTINEL, dtype=dt)
  want[:, off + 1:off + Hw - 1, off + 1:off + Ww - 1] = src[:, 1:-1, 1:-1].to(dt)
  assert_bits(dst, want, "window scatter (interior converted, everything else untouched)")


# --------------------------------------------------------------------------------------
# max pools against F.max_pool2d on tie-dense data
# --------------------------------------------------------------------------------------
def _tie_dense(rng, N, C, H, W):
  """Three levels, the top one most likely: most windows hold their maximum more than once."""
  lv = rng.choice(np.array([-0.5, 0.25, 1.0], dtype=np.float32), size=(N, C, H, W), p=[0.1, 0.15, 0.75])
  return torch.from_numpy(lv)


def _tie_share(x, padding=0):
  """Share of the pooling windows whose maximum occurs more than once, among the windows that hold more than one
  element (with padding 1 a corner window holds one pixel); None when there is no such window."""
  cols = F.unfold(x.reshape(-1, 1, x.shape[2], x.shape[3]), 2, stride=2, padding=padding)
  valid = (F.unfold(torch.ones(1, 1, x.shape[2], x.shape[3]), 2, stride=2, padding=padding) > 0).expand_as(cols)
  cols = torch.where(valid, cols, torch.full_like(cols, -float("inf")))
  multi = valid.sum(1) > 1
  if not bool(multi.any()):
    return None
  top = cols.max(1, keepdim=True).values
  return float(((cols == top).sum(1) > 1)[multi].float().mean())


def _pool_reference(x, dout, **pool):
  xr = x.double().requires_grad_(True)
  y = F.max_pool2d(xr, 2, 2, **pool)
  y.backward(dout.double())
  return y.detach(), xr.grad


@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("H,W,Pi,Po,C", [(7, 9, 1, 2, 8), (2, 2, 3, 1, 8), (3, 2, 1, 3, 16), (200, 10, 1, 2, 8), (24, 24, 3, 1, 64)])
def test_maxpool2_vs_torch_on_tie_dense_data(H, W, Pi, Po, C, fp32):
  """iic_maxpool2_fwd / iic_maxpool2_bwd and iic_f32_maxpool2_fwd / iic_f32_maxpool2_bwd against F.max_pool2d(2, 2) and
  its autograd: odd sizes, Pi != Po, data on three levels so that more than half of the windows tie (asserted on the
  inputs).  Output and routed gradient bit-equal; odd trailing rows / columns receive zero; borders are not written."""
  N = 2
  rng = np.random.default_rng(H * 100 + W)
  dt = torch.float32 if fp32 else torch.bfloat16
  pre = "iic_f32_maxpool2" if fp32 else "iic_maxpool2"
  x = _tie_dense(rng, N, C, H, W)
  assert _tie_share(x) > 0.5
  Ho, Wo = H // 2, W // 2
  dout = rnd(rng, N, C, Ho, Wo).to(dt).float()
  y, dx = _pool_reference(x, dout)
  xp = pt_of(x.permute(0, 2, 3, 1), Pi, dt)
  out = torch.full((N, Ho + 2 * Po, Wo + 2 * Po, C), SENTINEL, dtype=dt, device=dev())
  ok(pre + "_fwd", xp, out, N, H, W, Pi, Po, C)
  assert_bits(interior(out, Po), y.permute(0, 2, 3, 1).to(dt), "max-pool output")
  assert_border(out, Po, SENTINEL, "max-pool forward")
  din = torch.full((N, H + 2 * Pi, W + 2 * Pi, C), SENTINEL, dtype=dt, device=dev())
  ok(pre + "_bwd", xp, pt_of(dout.permute(0, 2, 3, 1), Po, dt), din, N, H, W, Pi, Po, C)
  got = interior(din, Pi)
  assert bool((got.double() == dx.permute(0, 2, 3, 1)).all()), "routed gradient differs from torch's"
  assert_bits(got.abs(), dx.permute(0, 2, 3, 1).to(dt).abs(), "routed gradient")
  assert bool((got[:, 2 * Ho:].float() == 0).all()) and bool((got[:, :, 2 * Wo:].float() == 0).all())
  assert_border(din, Pi, SENTINEL, "max-pool backward")


@pytest.mark.parametrize("H,W", [(24, 24), (25, 25), (6, 9), (1, 1), (2, 3)])
def test_f32_maxpool_s2p1_vs_torch_on_tie_dense_data(H, W):
  """iic_f32_maxpool_s2p1_fwd / iic_f32_maxpool_s2p1_bwd against F.max_pool2d(x, 2, 2, padding=1) and its autograd, even,
  odd and mixed sizes, tie-dense data (more than half of the windows that hold several pixels tie: asserted on the
  inputs): bit equality, borders not written."""
  N, C = 2, 5
  rng = np.random.default_rng(H * 100 + W)
  x = _tie_dense(rng, N, C, H, W)
  share = _tie_share(x, padding=1)
  assert share is None or share > 0.5, share      # (1 x 1: the only window holds one pixel)
  Ho, Wo = H // 2 + 1, W // 2 + 1
  dout = rnd(rng, N, C, Ho, Wo)
  y, dx = _pool_reference(x, dout, padding=1)
  assert tuple(y.shape[2:]) == (Ho, Wo)
  xp = pt_of(x.permute(0, 2, 3, 1), 1, torch.float32)
  out = torch.full((N, Ho + 2, Wo + 2, C), SENTINEL, device=dev())
  ok("iic_f32_maxpool_s2p1_fwd", xp, out, N, H, W, C)
  assert_bits(interior(out, 1), y.permute(0, 2, 3, 1).float(), "padded max-pool output")
  assert_border(out, 1, SENTINEL, "padded max-pool forward")
  din = torch.full((N, H + 2, W + 2, C), SENTINEL, device=dev())
  ok("iic_f32_maxpool_s2p1_bwd", xp, pt_of(dout.permute(0, 2, 3, 1), 1, torch.float32), din, N, H, W, C)
  assert_bits(interior(din, 1).abs(), dx.permute(0, 2, 3, 1).float().abs(), "padded max-pool routed gradient")
  assert bool((interior(din, 1).double() == dx.permute(0, 2, 3, 1)).all())
  assert_border(din, 1, SENTINEL, "padded max-pool backward")


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("C", [1, 2, 5])
def test_f32_nchw_to_pt_is_the_permute(C, P):
  """iic_f32_nchw_to_pt: bit-equal to the permute; the border of a zeroed buffer stays zero (and is not written at all)."""
  N, H, W = 3, 5, 7
  x = rnd(np.random.default_rng(C), N, C, H, W)
  for fill in (0.0, SENTINEL):
    out = torch.full((N, H + 2 * P, W + 2 * P, C), fill, device=dev())
    ok("iic_f32_nchw_to_pt", x.to(dev()), out, N, C, H, W, P)
    assert_bits(interior(out, P), x.permute(0, 2, 3, 1).contiguous(), "nchw -> PT")
    assert_border(out, P, fill, "nchw -> PT")


# --------------------------------------------------------------------------------------
# BatchNorm streaming kernels of the exact-fp32 path
# --------------------------------------------------------------------------------------
BN_SHAPES = [(6, 13, 13, 1, 128), (3, 3, 5, 2, 512), (1, 1, 1, 1, 64), (2, 20, 36, 2, 64)]


def _bn_inputs(N, H, W, P, C):
  rng = np.random.default_rng(N * 7 + C)
  y = torch.round(rnd(rng, N, H, W, C) * 8) / 8
  y2, res, dout, act = rnd(rng, N, H, W, C), rnd(rng, N, H, W, C), rnd(rng, N, H, W, C), _mask_act(rng, N, H, W, C)
  return rng, y, y2, res, dout, act


@pytest.mark.parametrize("N,H,W,P,C", BN_SHAPES)
def test_f32_bn_apply_vs_float64(N, H, W, P, C):
  """iic_f32_bn_apply: out = [relu](y*scale + shift [+ res] [+ y2*scale2 + shift2]) -- at most six fp32 operations (five
  when fused), each off by at most U32 times a partial result that is bounded by the sum A of the terms' magnitudes:
  6 * U32 * A.  ReLU is exact and 1-Lipschitz."""
  rng, y, y2, res, _, _ = _bn_inputs(N, H, W, P, C)
  coef, coef2 = rnd(rng, 5, C), rnd(rng, 5, C)
  f32 = torch.float32
  for relu, use_res, use_y2 in ((1, False, False), (0, False, False), (1, True, False), (1, False, True), (0, True, True)):
    out = torch.full((N, H + 2 * P, W + 2 * P, C), SENTINEL, device=dev())
    ok("iic_f32_bn_apply", pt_of(y, P, f32), coef.to(dev()), pt_of(res, P, f32) if use_res else None,
       pt_of(y2, P, f32) if use_y2 else None, coef2.to(dev()) if use_y2 else None, out, N, H, W, P, C, relu)
    c, c2 = coef.double(), coef2.double()
    v = y.double() * c[0] + c[1]
    A = (y.double() * c[0]).abs() + c[1].abs()
    if use_res:
      v, A = v + res.double(), A + res.double().abs()
    if use_y2:
      v, A = v + y2.double() * c2[0] + c2[1], A + (y2.double() * c2[0]).abs() + c2[1].abs()
    assert_within(interior(out, P), v.clamp_min(0) if relu else v, 6 * U32 * A, "bn_apply relu=%d res=%d y2=%d" % (relu, use_res, use_y2))
    assert_border(out, P, SENTINEL, "bn_apply")


@pytest.mark.parametrize("N,H,W,P,C", BN_SHAPES)
def test_f32_bn_bwd_reduce_is_the_exact_sum_of_fp32_products(N, H, W, P, C):
  """iic_f32_bn_bwd_reduce: sums += (sum g, sum g*y) [sums2: (sum g, sum g*y2)], g = dout masked by act > 0 or by
  scale*y + shift > 0.  The accumulators are exact (csrc/common.h), so the decoded value is THE sum of the fp32 values
  g and fl32(g*y): the reference forms the products in fp32 on the CPU and sums them in float64; the bound is that
  float64 summation's own error, n * 2^-53 * sum |terms|."""
  from iic_amd import ops
  rng, y, y2, _, dout, act = _bn_inputs(N, H, W, P, C)
  mcoef = _pow2_coef(rng, C)
  f32 = torch.float32
  n = N * H * W
  for mode, use_y2 in (("none", False), ("act", False), ("mask_coef", False), ("none", True), ("mask_coef", True)):
    s1, s2 = ops.new_stats(C, dev()), ops.new_stats(C, dev())
    ok("iic_f32_bn_bwd_reduce", pt_of(dout, P, f32), pt_of(act, P, f32) if mode == "act" else None, pt_of(y, P, f32),
       pt_of(y2, P, f32) if use_y2 else None, s1, s2 if use_y2 else None,
       torch.cat([mcoef, torch.zeros(3, C)]).to(dev()) if mode == "mask_coef" else None, N, H, W, P, C)
    g = _masked_g(dout, act, y, mcoef, mode)
    for st, yy in ((s1, y),) + (((s2, y2),) if use_y2 else ()):
      prod = g * yy                                             # fp32 products, as the kernel forms them
      ref = torch.stack([g.double().sum((0, 1, 2)), prod.double().sum((0, 1, 2))])
      mag = torch.stack([g.double().abs().sum((0, 1, 2)), prod.double().abs().sum((0, 1, 2))])
      assert_within(ops.stats_decode(st, C), ref, n * 2.0 ** -53 * mag, "bn_bwd_reduce mask=%s y2=%d" % (mode, use_y2))


def test_f32_bn_bwd_reduce_poisons_only_the_channel_that_saw_inf():
  """One inf in dout of one channel: that channel's sums decode to NaN (the poison counter of csrc/common.h), the
  others stay finite."""
  from iic_amd import ops
  N, H, W, P, C = 2, 5, 5, 1, 64
  rng, y, _, _, dout, _ = _bn_inputs(N, H, W, P, C)
  dout[1, 2, 3, 17] = float("inf")
  st = ops.new_stats(C, dev())
  ok("iic_f32_bn_bwd_reduce", pt_of(dout, P, torch.float32), None, pt_of(y, P, torch.float32), None, st, None, None, N, H, W, P, C)
  got = ops.stats_decode(st, C).cpu()
  assert bool(torch.isnan(got[:, 17]).all())
  others = torch.cat([got[:, :17], got[:, 18:]], 1)
  assert bool(torch.isfinite(others).all())


@pytest.mark.parametrize("N,H,W,P,C", BN_SHAPES)
def test_f32_bn_bwd_apply_vs_float64(N, H, W, P, C):
  """iic_f32_bn_bwd_apply: dy = c1*g + c2*y + c3 (and dy2 from y2 with its own coefficients): four fp32 operations, each
  within U32 of a partial result bounded by A = |c1 g| + |c2 y| + |c3|: 4 * U32 * A."""
  rng, y, y2, _, dout, act = _bn_inputs(N, H, W, P, C)
  mcoef, b1, b2 = _pow2_coef(rng, C), rnd(rng, 3, C), rnd(rng, 3, C)
  f32 = torch.float32
  for mode, use_y2 in (("none", False), ("act", False), ("mask_coef", False), ("act", True)):
    dy = torch.full((N, H + 2 * P, W + 2 * P, C), SENTINEL, device=dev())
    dy2 = torch.full_like(dy, SENTINEL)
    ok("iic_f32_bn_bwd_apply", pt_of(dout, P, f32), pt_of(act, P, f32) if mode == "act" else None, pt_of(y, P, f32),
       b1.to(dev()), dy, pt_of(y2, P, f32) if use_y2 else None, b2.to(dev()) if use_y2 else None, dy2 if use_y2 else None,
       torch.cat([mcoef, torch.zeros(3, C)]).to(dev()) if mode == "mask_coef" else None, N, H, W, P, C)
    g = _masked_g(dout, act, y, mcoef, mode).double()
    for out, yy, b in ((dy, y, b1),) + (((dy2, y2, b2),) if use_y2 else ()):
      b = b.double()
      ref = b[0] * g + b[1] * yy.double() + b[2]
      A = (b[0] * g).abs() + (b[1] * yy.double()).abs() + b[2].abs()
      assert_within(interior(out, P), ref, 4 * U32 * A, "bn_bwd_apply mask=%s y2=%d" % (mode, use_y2))
      assert_border(out, P, SENTINEL, "bn_bwd_apply")


# --------------------------------------------------------------------------------------
# iic_bn_running_update: the running statistics iic_bn_finalize writes itself, applied later
# --------------------------------------------------------------------------------------
def _finalize(C, sums, count, rm, rv, nbt):
  """iic_bn_finalize on an accumulator encoded from `sums`; returns coef."""
  from iic_amd import ops
  st = ops.new_stats(C, dev())
  ops.stats_encode(st, C, sums)
  gamma, beta = torch.ones(C, device=dev()), torch.zeros(C, device=dev())
  coef = torch.empty((5, C), device=dev())
  ok("iic_bn_finalize", st, gamma, beta, rm, rv, nbt, coef, C, count, 0, ctypes.c_float(1e-5), ctypes.c_float(0.1), 1)
  return coef


def _running_update(items, momentum=0.1):
  from iic_amd import _lib
  n = len(items)
  VP, IP = ctypes.c_void_p * n, ctypes.c_int * n
  _lib.check(_lib.lib().iic_bn_running_update(
    n, VP(*[c.data_ptr() for c, _, _, _ in items]), VP(*[rm.data_ptr() for _, rm, _, _ in items]),
    VP(*[rv.data_ptr() for _, _, rv, _ in items]), VP(*[nb.data_ptr() for _, _, _, nb in items]),
    IP(*[c.shape[1] for c, _, _, _ in items]), momentum, _lib.stream_ptr()), "iic_bn_running_update")
  torch.cuda.synchronize()


@pytest.mark.parametrize("layout", ["one", "seventy", "twice"])
def test_bn_running_update_equals_what_bn_finalize_writes(layout):
  """iic_bn_running_update against iic_bn_finalize given the running statistics directly, for the same coefficients:
  bit-equal (bn.hip: "same arithmetic, bit for bit").  one BatchNorm; a list longer than the kernel's chunk of 64 with
  channel counts on both sides of one 256-thread block; and a list that names the same BatchNorm twice (the two
  forwards of a step): num_batches_tracked advances by two and the momentum rule is applied twice in list order.
  Also against a float64 restatement of the rule, r' = (1 - m) r + m s: four fp32 operations per application."""
  rng = np.random.default_rng(5)
  count = 48
  chans = {"one": [128], "seventy": [(16, 64, 272)[i % 3] for i in range(70)], "twice": [64, 272, 64]}[layout]
  same = {2: 0} if layout == "twice" else {}         # entry 2 is BatchNorm 0 again
  direct, deferred, sums = [], [], []
  for i, C in enumerate(chans):
    v = rnd(rng, count, C) * 1.5 + 0.3
    sums.append(torch.stack([v.sum(0), (v * v).sum(0)]))
    if i in same:
      direct.append(direct[same[i]])
      deferred.append(deferred[same[i]])
    else:
      rm0, rv0 = rnd(rng, C), rnd(rng, C).abs() + 0.5
      mk = lambda: (rm0.clone().to(dev()), rv0.clone().to(dev()), torch.full((), 3, dtype=torch.long, device=dev()))
      direct.append(mk())
      deferred.append(mk())
  start = [(rm.cpu().double(), rv.cpu().double()) for rm, rv, _ in direct]
  items, coefs = [], []
  for i, C in enumerate(chans):
    ca = _finalize(C, sums[i], count, *direct[i])                       # updates the running statistics itself
    cb = _finalize(C, sums[i], count, None, None, None)                 # leaves them to the deferred update
    assert_bits(ca, cb, "coefficients with and without running statistics")
    items.append((cb,) + deferred[i])
    coefs.append(cb.cpu().double())
  _running_update(items)
  m = float(np.float32(0.1))
  for i, C in enumerate(chans):
    if i in same:
      continue
    rm_a, rv_a, nb_a = direct[i]
    rm_b, rv_b, nb_b = deferred[i]
    assert_bits(rm_b, rm_a, "running_mean of entry %d" % i)
    assert_bits(rv_b, rv_a, "running_var of entry %d" % i)
    uses = [j for j in range(len(chans)) if j == i or same.get(j) == i]
    assert int(nb_b) == int(nb_a) == 3 + len(uses)
    r, v = start[i]
    tol_r, tol_v = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for j in uses:                                                      # list order
      tol_r = tol_r + 4 * U32 * (r.abs() + coefs[j][2].abs())
      tol_v = tol_v + 4 * U32 * (v.abs() + coefs[j][4].abs())
      r, v = (1 - m) * r + m * coefs[j][2], (1 - m) * v + m * coefs[j][4]
    assert_within(rm_b, r, tol_r, "running_mean vs the float64 rule")
    assert_within(rv_b, v, tol_v, "running_var vs the float64 rule")


# --------------------------------------------------------------------------------------
def test_weight_prep_multi_rewrites_every_layout_like_the_single_launches():
  """iic_weight_prep_multi through ops.refresh_prepped: after the parameters change, ONE launch re-writes every
  materialised layout of several PreppedWeights of different shapes, bit-equal to iic_weight_prep /
  iic_weight_prep_frag (ops.weight_prep, ops.weight_prep_frag) of each."""
  from iic_amd import ops
  rng = np.random.default_rng(3)
  shapes = [(64, 64, 3), (128, 64, 1), (256, 128, 3), (128, 128, 3), (64, 128, 5)]
  ws = [rnd(rng, co, ci, k, k).to(dev()) for co, ci, k in shapes]
  pws = [ops.PreppedWeights(w) for w in ws]
  for i, pw in enumerate(pws):      # different subsets of the four layouts
    if i != 1:
      pw.frag(False)
    if i % 2 == 0:
      pw.frag(True)
    if i != 3:
      pw.rows(False)
  old = [[t.clone() for t in (pw._frag[0], pw._frag[1]) + tuple(pw._rows or (None, None)) if t is not None] for pw in pws]
  for w in ws:
    w.copy_(rnd(rng, *w.shape).to(dev()))
  assert ops.refresh_prepped(pws, dev()) is True
  torch.cuda.synchronize()
  for pw, w, before in zip(pws, ws, old):
    now = [t for t in (pw._frag[0], pw._frag[1]) + tuple(pw._rows or (None, None)) if t is not None]
    assert len(now) == len(before) > 0
    assert all(not torch.equal(a, b) for a, b in zip(now, before)), "a layout was not re-written"
    for bwd in (False, True):
      if pw._frag[int(bwd)] is not None:
        assert_bits(pw._frag[int(bwd)], ops.weight_prep_frag(w, bwd), "fragment-order operand bwd=%d of %s" % (bwd, tuple(w.shape)))
    if pw._rows is not None:
      wf, wb = ops.weight_prep(w)
      assert_bits(pw._rows[0], wf, "row-major forward operand")
      assert_bits(pw._rows[1], wb, "row-major backward-data operand")


# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 10 ** 6 + 3])
def test_count_equal_vs_torch(n):
  """iic_count_equal == (a == b).sum(), the count buffer zeroed by the call itself (n = 0 included)."""
  g = torch.Generator().manual_seed(n)
  a = torch.randint(0, 5, (max(n, 1),), generator=g)
  b = torch.randint(0, 5, (max(n, 1),), generator=g)
  cnt = torch.full((), 12345, dtype=torch.long, device=dev())
  ok("iic_count_equal", a.to(dev()), b.to(dev()), ctypes.c_long(n), cnt)
  assert int(cnt) == int((a[:n] == b[:n]).sum())


# --------------------------------------------------------------------------------------
def test_adam_step_dev_vs_float64_and_the_host_counter_variant():
  """iic_adam_step_dev (step count kept on the device; no caller inside the package): each step against a float64
  restatement of Adam from the kernel's own fp32 state before that step, and the counter advances by one per call.
  Bounds from the kernel's expressions, U32 per operation: m' = b1*m + (1-b1)*g (4 operations), v' = b2*v + (1-b2)*g*g
  (5), denom = sqrt(v')*k + eps (3, plus v's error through the square root), p' = p - s*(m'/denom) (3)."""
  from iic_amd import _lib
  rng = np.random.default_rng(11)
  sizes = [1, 257, 70001]
  p = [rnd(rng, n).to(dev()) for n in sizes]
  m = [(rnd(rng, n) * 0.1).to(dev()) for n in sizes]
  v = [(rnd(rng, n) ** 2 * 0.01).to(dev()) for n in sizes]
  lr, b1, b2, eps = [float(np.float32(t)) for t in (1e-3, 0.9, 0.999, 1e-8)]
  steps = torch.full((1,), 4, dtype=torch.int32, device=dev())
  VP, LP = ctypes.c_void_p * len(sizes), ctypes.c_long * len(sizes)
  for it in range(2):
    g = [rnd(rng, n).to(dev()) for n in sizes]
    before = [[t.cpu().double() for t in grp] for grp in (p, g, m, v)]
    _lib.check(_lib.lib().iic_adam_step_dev(len(sizes), VP(*[t.data_ptr() for t in p]), VP(*[t.data_ptr() for t in g]), None,
                                            VP(*[t.data_ptr() for t in m]), VP(*[t.data_ptr() for t in v]), LP(*sizes),
                                            lr, b1, b2, eps, steps.data_ptr(), _lib.stream_ptr()), "iic_adam_step_dev")
    torch.cuda.synchronize()
    step = 5 + it
    assert int(steps) == step
    s, k = lr / (1 - b1 ** step), 1 / np.sqrt(1 - b2 ** step)
    for i in range(len(sizes)):
      p0, g0, m0, v0 = (before[j][i] for j in range(4))
      m1, v1 = b1 * m0 + (1 - b1) * g0, b2 * v0 + (1 - b2) * g0 * g0
      tm, tv = 4 * U32 * (m0.abs() + g0.abs()), 5 * U32 * (v0 + g0 * g0)
      assert_within(m[i], m1, tm, "exp_avg")
      assert_within(v[i], v1, tv, "exp_avg_sq")
      den = v1.sqrt() * k + eps
      tden = k * tv / (2 * (v1 - tv).clamp_min(1e-300).sqrt()) + 4 * U32 * den
      upd = s * m1 / den
      tupd = s * (tm / (den - tden).clamp_min(1e-300) + m1.abs() * tden / (den - tden).clamp_min(1e-300) ** 2) + 3 * U32 * upd.abs()
      assert_within(p[i], p0 - upd, tupd + U32 * (p0.abs() + upd.abs()), "parameter")
