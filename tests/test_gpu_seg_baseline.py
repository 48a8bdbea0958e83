"""The Isola / Doersch segmentation baselines on the GPU: the patch sampler (iic_seg_patch_sample_fwd / _bwd,
csrc/seg_patches.hip), the joint Linear (iic_pair_weight_prep, iic_pair_linear_fwd_nsplit, iic_pair_linear_fwd,
iic_pair_linear_bwd_dx, iic_pair_linear_wgrad, csrc/sup_head.hip), the losses (iic_isola_loss, iic_doersch_loss,
csrc/seg_baseline_loss.hip) and the whole nets (iic_amd/archs/seg_baselines.py, iic_amd/seg_baselines.py) against the
oracle.  Cases, float64 restatements and bounds: tests/seg_baseline_cases.py (proved on the CPU by
tests/test_seg_baseline_cpu.py)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import parity
from tests import seg_baseline_cases as bc
from tests import sup_head_cases as sc
from tests.parity import assert_bits, assert_border, assert_in_bracket, assert_within, dev

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
P3 = bc.P_TRUNK


def _coords(case_or_pts, label=0):
  from iic_amd.archs.seg_baselines import coords_block
  centre, other = case_or_pts if isinstance(case_or_pts, tuple) and len(case_or_pts) == 2 else bc.points(case_or_pts)
  return coords_block(centre, other, label, dev())


# ======================================================================================================================
# 1. sampler
# ======================================================================================================================
def _sample(case, x, dtype, fill=parity.SENTINEL):
  """patches [2 N, p + 2, p + 2, C] of the kernel for features x [N, C, Hl, Hl]; the source's border holds `fill` (read
  by nothing) and the output starts from a sentinel (the kernel writes all of it, border included)."""
  pt = bc.to_pt(x, P3, dtype, fill=fill).to(dev())
  out = torch.full((2 * case.N, case.p + 2, case.p + 2, case.C), parity.SENTINEL, dtype=dtype, device=dev())
  parity.ok("iic_seg_patch_sample_fwd", pt, int(dtype == F32), _coords(case), out, case.N, case.Hl, case.Hl,
            case.Hl + 2 * P3, case.Hl + 2 * P3, P3, case.C, case.S, case.p)
  return pt, out


def _adjoint(case, g, dtype):
  """dx_pt of the kernel for g [2 N, C, p, p]; the gradients' borders hold a sentinel (not read), dx_pt starts from one
  everywhere: the interior must be written completely, the border not at all."""
  gp = bc.to_pt(g, 1, dtype, fill=parity.SENTINEL).to(dev())
  dx = torch.full((case.N, case.Hl + 2 * P3, case.Hl + 2 * P3, case.C), parity.SENTINEL, dtype=dtype, device=dev())
  parity.ok("iic_seg_patch_sample_bwd", gp[:case.N], gp[case.N:], int(dtype == F32), _coords(case), dx, case.N, case.Hl,
            case.Hl, case.Hl + 2 * P3, case.Hl + 2 * P3, P3, case.C, case.S, case.p)
  return dx


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", bc.LATTICE_CASES, ids=lambda c: c.name)
def test_sampler_exact_lattice(case, dtype):
  x, g = bc.lattice_features(case), bc.lattice_grads(case)
  ref = bc.sample64(x, case)
  _, out = _sample(case, x, dtype)
  assert_bits(out[:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous(), torch.from_numpy(ref).to(dtype),
              "forward %s" % case.name)
  assert_border(out, 1, 0.0, "patches %s" % case.name)          # the kernel zeroes the border
  dx64, _, T = bc.adjoint64(g, case)
  dx = _adjoint(case, g, dtype)
  got = dx[:, P3:-P3, P3:-P3].permute(0, 3, 1, 2).contiguous()
  want = parity.bf16_rne(torch.from_numpy(dx64)).to(BF16) if dtype == BF16 else torch.from_numpy(dx64).float()
  assert_bits(got, want, "adjoint %s" % case.name)
  assert_border(dx, P3, parity.SENTINEL, "dx_pt %s" % case.name)      # never written
  assert bool((got.float().cpu()[:, :, torch.from_numpy(T == 0)] == 0).all())      # zeros outside both footprints
  if dtype == F32:      # <fwd x, g> == <x, bwd g>, exactly: every product and sum is an integer multiple of 1/16
    fwd = out[:, 1:-1, 1:-1].permute(0, 3, 1, 2).double().cpu().numpy()
    assert float((fwd * g).sum()) == float((x * got.double().cpu().numpy()).sum())
  # two calls give equal bits
  assert_bits(_adjoint(case, g, dtype), dx, "adjoint, second call")
  assert_bits(_sample(case, x, dtype)[1], out, "forward, second call")


@pytest.mark.parametrize("case", bc.RATIO_CASES, ids=lambda c: c.name)
def test_sampler_real_ratio(case):
  """Hl = S / 2 - 4, weights with full mantissas: the forward is bf16(iic_seg_feat_sample) bit for bit (the numbers
  iic_bilinear_fwd stores), the adjoint stays inside its derived bound."""
  from iic_amd import seg_kmeans
  x, g = bc.mantissa_features(case), bc.mantissa_grads(case)
  pt, out = _sample(case, x, BF16, fill=0.0)
  d = case.p // 2
  rows = []
  for (cy, cx) in bc.points(case):
    for n in range(case.N):
      for i in range(case.p):
        for j in range(case.p):
          rows.append((n, cy - d + i, cx - d + j))
  feats = seg_kmeans.feat_sample(pt, np.asarray(rows, dtype=np.int32), case.S)      # [2 N p p, C] fp32
  want = feats.view(2 * case.N, case.p, case.p, case.C).to(BF16)
  assert_bits(out[:, 1:-1, 1:-1].contiguous(), want, "forward %s" % case.name)
  assert_border(out, 1, 0.0, "patches %s" % case.name)
  # and the float64 restatement agrees with what the kernel computed, to fp32 accuracy
  ref = bc.sample64(x, case)
  assert float(np.abs(out[:, 1:-1, 1:-1].permute(0, 3, 1, 2).double().cpu().numpy() - ref).max()) <= 2.0 ** -8
  dx64, A, T = bc.adjoint64(g, case)
  b = torch.from_numpy(bc.adjoint_bound(A, T))
  dx = _adjoint(case, g, BF16)
  lo, hi = parity.bf16_bracket(torch.from_numpy(dx64), b)
  assert_in_bracket(dx[:, P3:-P3, P3:-P3].permute(0, 3, 1, 2).contiguous(), lo, hi, "adjoint %s" % case.name,
                    family="patch_adjoint", ref=torch.from_numpy(dx64), b=b)
  assert_border(dx, P3, parity.SENTINEL, "dx_pt %s" % case.name)
  dxf = _adjoint(case, g, F32)
  assert_within(dxf[:, P3:-P3, P3:-P3].permute(0, 3, 1, 2), torch.from_numpy(dx64), b, "fp32 adjoint %s" % case.name,
                family="patch_adjoint_f32")
  # the fp32 flavour of the forward: the rows of iic_seg_feat_sample themselves
  ptf, outf = _sample(case, x, F32, fill=0.0)
  assert_bits(outf[:, 1:-1, 1:-1].contiguous(),
              seg_kmeans.feat_sample(ptf, np.asarray(rows, dtype=np.int32), case.S).view(2 * case.N, case.p, case.p, case.C),
              "fp32 forward %s" % case.name)
  print("worst:", {k: v for k, v in parity.WORST.items() if k.startswith("patch_")})


def test_sampler_clamps_and_refuses():
  """Coordinates are device data: a centre outside [d, S - 1 - d] is clamped by the kernel (the wrapper refuses it on the
  host); an even patch side or an odd channel count is refused before a launch."""
  case = bc.LATTICE_CASES[0]
  x = bc.lattice_features(case)
  pt = bc.to_pt(x, P3, BF16).to(dev())
  out = torch.empty((2 * case.N, case.p + 2, case.p + 2, case.C), dtype=BF16, device=dev())
  args = (case.N, case.Hl, case.Hl, case.Hl + 2 * P3, case.Hl + 2 * P3, P3, case.C, case.S)
  parity.ok("iic_seg_patch_sample_fwd", pt, 0, _coords(((-5, 100), (0, 15))), out, *args, case.p)
  clamped = case._replace(centre=(1, 14), other=(1, 14))
  assert_bits(out, _sample(clamped, x, BF16, fill=0.0)[1], "clamped centres")
  assert parity.call("iic_seg_patch_sample_fwd", pt, 0, _coords(case), out, *args, 4) == -3
  assert parity.call("iic_seg_patch_sample_fwd", pt, 0, _coords(case), out, case.N, case.Hl, case.Hl, case.Hl + 2 * P3,
                     case.Hl + 2 * P3, P3, 63, case.S, 3) == -3
  assert parity.call("iic_seg_patch_sample_bwd", out[:case.N], out[case.N:], 0, _coords(case), pt, *args, 2) == -3


# ======================================================================================================================
# 2. joint Linear
# ======================================================================================================================
def _pair_products(case, t, border=0.0):
  from iic_amd import _lib
  K = bc.pair_K(case)
  S = _lib.lib().iic_pair_linear_fwd_nsplit(case.N, case.F, case.C, case.p)
  assert S >= 1
  a0, a1 = sc.to_pt(t["a0"], fill=border).to(dev()), sc.to_pt(t["a1"], fill=border).to(dev())
  wb = torch.empty((case.F, 2 * K), dtype=BF16, device=dev())
  wt = torch.empty((2 * K, case.F), dtype=BF16, device=dev())
  parity.ok("iic_pair_weight_prep", t["w"].to(dev()), wb, wt, case.F, case.C, case.p)
  y = torch.empty((case.N, case.F), dtype=F32, device=dev())
  ws = torch.empty(max(1, S * case.N * case.F), dtype=F32, device=dev())
  parity.ok("iic_pair_linear_fwd", a0, a1, wb, t["b"].to(dev()), y, ws, case.N, case.F, case.C, case.p)
  Np = (case.N + 63) // 64 * 64
  dyb = torch.empty((case.N, case.F), dtype=BF16, device=dev())
  dyt = torch.empty((case.F, Np), dtype=BF16, device=dev())
  parity.ok("iic_sup_dy_cast", t["dy"].to(dev()), dyb, dyt, case.N, case.F)
  dx0, dx1 = torch.zeros_like(a0), torch.zeros_like(a1)
  parity.ok("iic_pair_linear_bwd_dx", dyb, wt, dx0, dx1, case.N, case.F, case.C, case.p)
  dW = torch.full((case.F, 2 * K), parity.SENTINEL, dtype=F32, device=dev())
  parity.ok("iic_pair_linear_wgrad", dyt, a0, a1, dW, case.N, case.F, case.C, case.p)
  return S, y, dW, dx0, dx1, wb, wt


@pytest.mark.parametrize("case", bc.PAIR_CASES, ids=lambda c: c.name)
def test_pair_linear_exact_lattice(case):
  from iic_amd.semisup import permute_columns
  t = bc.pair_lattice(case)
  y64, Ay, dW64, AdW, dx0, dx1, Adx0, Adx1 = bc.pair_products64(t["a0"], t["a1"], t["w"], t["b"], t["dy"])
  assert float(max(Ay.max(), AdW.max(), Adx0.max(), Adx1.max())) < 2 ** 24      # every partial sum exact in fp32
  S, y, dW, g0, g1, wb, wt = _pair_products(case, t, border=parity.SENTINEL)
  if case.C == 1024:
    assert S > 1      # the K split is exercised
  K = bc.pair_K(case)
  perm = torch.from_numpy(permute_columns(case.C, case.p, case.p))
  perm2 = torch.cat([perm, perm + K])      # both halves, each in the PT interior order
  assert_bits(wb, t["w"][:, perm2].to(BF16), "wb")
  assert_bits(wt, t["w"][:, perm2].t().contiguous().to(BF16), "wt")
  # (+ 0.0: a float64 sum of one product can be -0; the kernels' accumulators start from +0)
  assert_bits(y, (y64 + 0.0).float(), "forward")
  assert_bits(dW, (dW64 + 0.0).float(), "dW: parameter order, both halves in their places")
  assert not torch.equal(dW64[:, :K], dW64[:, K:])
  assert_bits(sc.from_pt(g0).to(BF16), parity.bf16_rne(dx0 + 0.0).to(BF16), "dx, centre")
  assert_bits(sc.from_pt(g1).to(BF16), parity.bf16_rne(dx1 + 0.0).to(BF16), "dx, other")
  assert_border(g0, 1, 0.0, "dx0")
  assert_border(g1, 1, 0.0, "dx1")


@pytest.mark.parametrize("case", bc.PAIR_CASES, ids=lambda c: c.name)
def test_pair_linear_within_f64_brackets(case):
  t = bc.pair_mantissa(case)
  b16 = lambda v: v.to(BF16).float()
  y64, Ay, dW64, AdW, dx0, dx1, Adx0, Adx1 = bc.pair_products64(t["a0"], t["a1"], b16(t["w"]), t["b"], b16(t["dy"]))
  S, y, dW, g0, g1, _, _ = _pair_products(case, t)
  assert_within(y, y64, bc.pair_forward_bound(case, Ay, S), "forward", family="pair_fwd")
  assert_within(dW, dW64, bc.pair_wgrad_bound(case, AdW), "dW", family="pair_dW")
  for name, got, ref, A in (("centre", g0, dx0, Adx0), ("other", g1, dx1, Adx1)):
    b, lo, hi = bc.pair_dx_bracket(case, ref, A)
    assert_in_bracket(sc.from_pt(got), lo, hi, "dx %s" % name, family="pair_dx", ref=ref, b=b)
    assert_border(got, 1, 0.0, "dx %s" % name)
  print("nsplit %d; worst:" % S, {k: v for k, v in parity.WORST.items() if k.startswith("pair_")})


def test_pair_linear_reproducible_and_unsupported():
  from iic_amd import linear
  case = bc.PAIR_CASES[-2]      # N = 3, C = 1024, F = 1024: K split
  t = bc.pair_mantissa(case)
  _, y1, dW1, a1, b1, wb, wt = _pair_products(case, t)
  junk = torch.randn(1024, 1024, device=dev())
  for _ in range(4):
    junk = junk @ junk * 1e-3      # other work queued in front of the second run, through the wrappers this time
  a0p, a1p = sc.to_pt(t["a0"]).to(dev()), sc.to_pt(t["a1"]).to(dev())
  wb2, wt2 = linear.pt_weight_prep(t["w"].to(dev()), case.C, case.p, case.p, 2)
  y2 = linear.pt_linear_forward((a0p, a1p), wb2, t["b"].to(dev()), case.F)
  dyb, dyt = linear.dy_cast(t["dy"].to(dev()))
  a2, b2 = linear.pt_linear_bwd_dx(dyb, wt2, (torch.zeros_like(a0p), torch.zeros_like(a1p)))
  dW2 = linear.pt_linear_wgrad(dyt, (a0p, a1p))
  torch.cuda.synchronize()
  for name, u, v in (("y", y1, y2), ("dW", dW1, dW2), ("dx0", a1, a2), ("dx1", b1, b2), ("wb", wb, wb2), ("wt", wt, wt2)):
    assert_bits(u, v, name + " second run")
  assert linear.pt_linear_nsplit(case.N, case.F, case.C, case.p, case.p, 2) > 1
  z = torch.zeros(16, device=dev())
  for F_, C_, p_ in ((100, 64, 3), (64, 96, 3), (64, 64, 2)):      # refused before a launch
    assert linear.pt_linear_nsplit(4, F_, C_, p_, p_, 2) == 0
    assert parity.call("iic_pair_weight_prep", z, z, z, F_, C_, p_) == -3
    assert parity.call("iic_pair_linear_fwd", z, z, z, z, z, z, 4, F_, C_, p_) == -3
    assert parity.call("iic_pair_linear_bwd_dx", z, z, z, z, 4, F_, C_, p_) == -3
    assert parity.call("iic_pair_linear_wgrad", z, z, z, z, 4, F_, C_, p_) == -3


def _sup_forward(a, wb_half, bias, case):
  """iic_sup_linear_fwd of one activation against one [F, K] operand, H = W = p."""
  from iic_amd import _lib
  S = _lib.lib().iic_sup_fwd_nsplit(case.N, case.F, case.C, case.p, case.p)
  assert S >= 1
  y = torch.empty((case.N, case.F), dtype=F32, device=dev())
  ws = torch.empty(max(1, S * case.N * case.F), dtype=F32, device=dev())
  parity.ok("iic_sup_linear_fwd", a, wb_half, bias, y, ws, case.N, case.F, case.C, case.p, case.p)
  return y


@pytest.mark.parametrize("case", [c for c in bc.PAIR_CASES if c.name in ("N3_C64_p3_F128", "N130_C64_p3_F64",
                                                                        "N3_C1024_p3_F1024")], ids=lambda c: c.name)
def test_pair_entries_are_the_single_operand_entries_per_half(case):
  """iic_pair_* is iic_sup_* (H = W = p) applied to each column half of the weight, bit for bit: the operands, dx and dW
  on the full-mantissa draw; the forward on the lattice, where every partial sum is an integer below 2^24 and the sum of
  the two halves' results is exact."""
  K = bc.pair_K(case)
  t = bc.pair_mantissa(case)
  S, _, dW, g0, g1, wb, wt = _pair_products(case, t)
  if case.C == 1024:
    assert S > 1      # the K split is on
  a = [sc.to_pt(t["a0"]).to(dev()), sc.to_pt(t["a1"]).to(dev())]
  Np = (case.N + 63) // 64 * 64
  dyb = torch.empty((case.N, case.F), dtype=BF16, device=dev())
  dyt = torch.empty((case.F, Np), dtype=BF16, device=dev())
  parity.ok("iic_sup_dy_cast", t["dy"].to(dev()), dyb, dyt, case.N, case.F)
  for q in (0, 1):
    wq = t["w"][:, q * K:(q + 1) * K].contiguous().to(dev())
    wbq = torch.empty((case.F, K), dtype=BF16, device=dev())
    wtq = torch.empty((K, case.F), dtype=BF16, device=dev())
    parity.ok("iic_sup_weight_prep", wq, wbq, wtq, case.F, case.C, case.p, case.p)
    assert_bits(wb[:, q * K:(q + 1) * K], wbq, "wb, half %d" % q)
    assert_bits(wt[q * K:(q + 1) * K], wtq, "wt, half %d" % q)
    dx = torch.zeros_like(a[q])
    parity.ok("iic_sup_linear_bwd_dx", dyb, wt[q * K:(q + 1) * K].contiguous(), dx, case.N, case.F, case.C, case.p, case.p)
    assert_bits((g0, g1)[q], dx, "dx, half %d" % q)
    dWq = torch.full((case.F, K), parity.SENTINEL, dtype=F32, device=dev())
    parity.ok("iic_sup_linear_wgrad", dyt, a[q], dWq, case.N, case.F, case.C, case.p, case.p)
    assert_bits(dW[:, q * K:(q + 1) * K], dWq, "dW, half %d" % q)
  # forward, on the lattice
  t = bc.pair_lattice(case)
  _, y, _, _, _, wb, _ = _pair_products(case, t)
  a = [sc.to_pt(t["a0"]).to(dev()), sc.to_pt(t["a1"]).to(dev())]
  bias = [t["b"].to(dev()), torch.zeros(case.F, dtype=F32, device=dev())]
  halves = [_sup_forward(a[q], wb[:, q * K:(q + 1) * K].contiguous(), bias[q], case) for q in (0, 1)]
  assert_bits(y, halves[0] + halves[1], "forward: the sum of the halves")


# ======================================================================================================================
# 3. losses
# ======================================================================================================================
def _loss_setup(N, mode):
  mask, m = bc.loss_mask(N, mode)
  return torch.from_numpy(mask).to(dev()), m


@pytest.mark.parametrize("adjacent", [True, False], ids=["adjacent", "apart"])
@pytest.mark.parametrize("mode", ["mixed", "all"])
@pytest.mark.parametrize("N", bc.LOSS_NS)
def test_isola_loss_vs_float64(N, mode, adjacent):
  from iic_amd import seg_baselines as sb
  mask, m = _loss_setup(N, mode)
  p = bc.isola_probs(N)
  loss64, dp64, mag, drop = bc.isola_ref(p, m, adjacent)
  (c, o) = (np.asarray(v) for v in bc.LOSS_POINTS)
  pred = torch.from_numpy(p).to(dev()).view(N, 1).requires_grad_(True)
  loss = sb.isola_loss(pred, c, o, adjacent, mask)
  assert loss.shape == ()
  (loss * 3.0).backward()
  if m.sum() == 0:
    assert bool(torch.isnan(loss)) and bool(torch.isnan(pred.grad).all())
    return
  tl, tg = bc.isola_bounds(loss64, dp64, mag, N)
  print("N %d %s adjacent %s: loss %.9e (float64 %.9e, bound %.2e)" % (N, mode, adjacent, float(loss.detach()), loss64, tl))
  assert_within(loss.detach().view(1), torch.tensor([loss64]), torch.tensor([tl]), "loss", family="isola_loss")
  raw, dp = sb.isola_loss_raw(pred.detach().view(-1), mask, _coords(bc.LOSS_POINTS, int(adjacent)))
  assert_bits(raw, loss.detach(), "loss, second call")
  assert_within(dp, torch.from_numpy(dp64), torch.from_numpy(tg), "dp", family="isola_dp")
  assert bool((dp.cpu()[torch.from_numpy(drop)] == 0).all())          # dropped rows: exactly 0
  assert_bits(pred.grad.view(-1), dp * 3.0, "autograd scales by the upstream factor")


@pytest.mark.parametrize("label", range(9))
def test_doersch_loss_every_label(label):
  from iic_amd import seg_baselines as sb
  N = 5
  mask, m = _loss_setup(N, "mixed")
  x = bc.doersch_logits(N)
  loss64, dl64, mag, gmag = bc.doersch_ref(x, m, label)
  tl, tg = bc.doersch_bounds(loss64, dl64, mag, gmag, N, 9)
  (c, o) = (np.asarray(v) for v in bc.LOSS_POINTS)
  lg = torch.from_numpy(x).to(dev()).requires_grad_(True)
  loss = sb.doersch_loss(lg, c, o, label, mask, crossent=None, verbose=False)
  (loss * 0.5).backward()
  assert_within(loss.detach().view(1), torch.tensor([loss64]), torch.tensor([tl]), "loss", family="doersch_loss")
  raw, dl = sb.doersch_loss_raw(lg.detach(), mask, _coords(bc.LOSS_POINTS, label))
  assert_within(dl, torch.from_numpy(dl64), torch.from_numpy(tg), "dlogits", family="doersch_dl")
  assert_bits(raw, loss.detach(), "loss, second call")
  assert_bits(lg.grad, dl * 0.5, "autograd scales by the upstream factor")


@pytest.mark.parametrize("mode", ["mixed", "all"])
@pytest.mark.parametrize("N", bc.LOSS_NS)
def test_doersch_loss_vs_float64(N, mode):
  from iic_amd import seg_baselines as sb
  mask, m = _loss_setup(N, mode)
  x = bc.doersch_logits(N)
  raw, dl = sb.doersch_loss_raw(torch.from_numpy(x).to(dev()), mask, _coords(bc.LOSS_POINTS, 7))
  loss64, dl64, mag, gmag = bc.doersch_ref(x, m, 7)
  if m.sum() == 0:
    assert bool(torch.isnan(raw)) and bool(torch.isnan(dl).all())
    return
  tl, tg = bc.doersch_bounds(loss64, dl64, mag, gmag, N, 9)
  assert_within(raw.view(1), torch.tensor([loss64]), torch.tensor([tl]), "loss", family="doersch_loss")
  assert_within(dl, torch.from_numpy(dl64), torch.from_numpy(tg), "dlogits", family="doersch_dl")
  print("worst:", {k: v for k, v in parity.WORST.items() if k.startswith(("isola_", "doersch_"))})


def test_losses_norm_zero_is_nan_and_k_limit():
  from iic_amd import seg_baselines as sb
  mask, m = _loss_setup(5, "none")
  assert m.sum() == 0
  loss, dp = sb.isola_loss_raw(torch.from_numpy(bc.isola_probs(5)).to(dev()), mask, _coords(bc.LOSS_POINTS, 1))
  assert bool(torch.isnan(loss)) and bool(torch.isnan(dp).all())
  loss, dl = sb.doersch_loss_raw(torch.from_numpy(bc.doersch_logits(5)).to(dev()), mask, _coords(bc.LOSS_POINTS, 2))
  assert bool(torch.isnan(loss)) and bool(torch.isnan(dl).all())
  z = torch.zeros((5, 33), device=dev())
  assert parity.call("iic_doersch_loss", z, mask, _coords(bc.LOSS_POINTS, 2), z, z, 5, 33, bc.S_MASK) == -3
  with pytest.raises(ValueError):
    sb.doersch_loss(z, np.asarray(bc.LOSS_POINTS[0]), np.asarray(bc.LOSS_POINTS[1]), 2, mask)
  # k = 32 is served
  x = torch.from_numpy(bc.doersch_logits(5, 32)).to(dev())
  mk, m = _loss_setup(5, "all")
  loss, dl = sb.doersch_loss_raw(x, mk, _coords(bc.LOSS_POINTS, 31))
  l64, d64, mag, gmag = bc.doersch_ref(x.cpu().numpy(), m, 31)
  tl, tg = bc.doersch_bounds(l64, d64, mag, gmag, 5, 32)
  assert_within(loss.view(1), torch.tensor([l64]), torch.tensor([tl]), "loss k = 32")
  assert_within(dl, torch.from_numpy(d64), torch.from_numpy(tg), "dlogits k = 32")


# ======================================================================================================================
# 4. whole nets
# ======================================================================================================================
S_NET, P_NET, N_NET, IN_CH = 24, 3, 4, 3
CENTRE, OTHER = np.array([7, 12], dtype=np.int32), np.array([10, 15], dtype=np.int32)


def _net_params(kind, seed):
  """Reference-named parameters: the oracle's 10a trunk (oracle.net_oracle.make_net10a_params) plus seeded head weights."""
  from oracle import net_oracle
  tp = net_oracle.make_net10a_params(IN_CH, 3, 1, True, seed=seed, randomize_bn=True)
  params = {"features." + k[len("trunk."):]: v for k, v in tp.items() if k.startswith("trunk.")}
  rng = np.random.default_rng([51, seed])
  f = lambda shape, s: torch.from_numpy((rng.standard_normal(shape) * s).astype(np.float32))
  h = kind + "_head."
  nout = 1 if kind == "isola" else 9
  params[h + "siamese_branch.0.weight"] = f((1024, 512, 3, 3), (2.0 / (512 * 9)) ** 0.5)
  params[h + "siamese_branch.1.weight"] = 1.0 + f((1024,), 0.1)
  params[h + "siamese_branch.1.bias"] = f((1024,), 0.1)
  params[h + "siamese_branch.1.running_mean"] = f((1024,), 0.1)
  params[h + "siamese_branch.1.running_var"] = 1.0 + f((1024,), 0.1).abs()
  params[h + "siamese_branch.1.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
  params[h + "joint.0.weight"] = f((1024, 2 * 1024 * P_NET * P_NET), 0.01)
  params[h + "joint.0.bias"] = f((1024,), 0.05)
  params[h + "joint.3.weight"] = f((nout, 1024), 0.05)
  params[h + "joint.3.bias"] = f((nout,), 0.05)
  return params


def _inputs(seed):
  from oracle import net_oracle
  x, _ = net_oracle.make_paired_batch(N_NET * IN_CH, S_NET, 1, seed=seed)      # smoothed noise, one plane per channel
  x = x.view(N_NET, IN_CH, S_NET, S_NET)
  rng = np.random.default_rng([52, seed])
  keep = torch.from_numpy((rng.uniform(size=(N_NET, 1024)) >= 0.5).astype(np.float32))
  mask = torch.ones((N_NET, S_NET, S_NET), dtype=torch.uint8)
  mask[1] = 0      # one image outside the relevancy mask at both points: norm = N - 1
  return x.contiguous(), keep, mask


def _oracle_forward(kind, params, x, keep, training=True):
  """oracle.net_oracle.vgg_trunk, F.interpolate, the slices of general.py:4-18 and torch modules, on the CPU.  Running
  statistics are updated in `params` in place, the siamese BatchNorm twice: centre images, then other images."""
  from oracle import net_oracle
  tp = {"trunk." + k[len("features."):]: v for k, v in params.items() if k.startswith("features.")}
  f = net_oracle.vgg_trunk(tp, x, net_oracle.NET10A_CFG, 3, 1, training)
  for k, v in tp.items():
    params["features." + k[len("trunk."):]] = v
  up = F.interpolate(f, size=S_NET, mode="bilinear", align_corners=False)
  d, h = P_NET // 2, kind + "_head."
  outs = []
  for pt in (CENTRE, OTHER):
    patch = up[:, :, pt[0] - d:pt[0] + d + 1, pt[1] - d:pt[1] + d + 1]
    y = F.conv2d(patch, params[h + "siamese_branch.0.weight"], padding=1)
    if training:
      params[h + "siamese_branch.1.num_batches_tracked"] += 1
    y = F.batch_norm(y, params[h + "siamese_branch.1.running_mean"], params[h + "siamese_branch.1.running_var"],
                     params[h + "siamese_branch.1.weight"], params[h + "siamese_branch.1.bias"], training, 0.1, 1e-5)
    outs.append(F.relu(y).reshape(x.shape[0], -1))
  hdn = F.relu(F.linear(torch.cat(outs, dim=1), params[h + "joint.0.weight"], params[h + "joint.0.bias"]))
  if training:
    hdn = hdn * keep * 2.0
  out = F.linear(hdn, params[h + "joint.3.weight"], params[h + "joint.3.bias"])
  return torch.sigmoid(out) if kind == "isola" else out


def _oracle_loss(kind, out, mask, gt):
  """isola_utils.py:27-72 / doersch_utils.py:55-66 in torch on the CPU."""
  m = ((mask[:, CENTRE[0], CENTRE[1]].int() + mask[:, OTHER[0], OTHER[1]].int()) > 0).float()
  norm = float(m.sum())
  if kind == "isola":
    t = out.squeeze(1) if gt else 1.0 - out.squeeze(1)
    keep = (t >= bc.EPS).float()
    return -(1.0 / norm) * (m * keep * torch.log(torch.where(t < bc.EPS, torch.full_like(t, bc.EPS), t))).sum()
  tgt = torch.ones(out.shape[0], dtype=torch.int64) * gt
  return (m * torch.nn.CrossEntropyLoss(reduction="none")(out, tgt)).sum() / norm


def _make(kind, params):
  from iic_amd import archs
  cfg = types.SimpleNamespace(in_channels=IN_CH, input_sz=S_NET, batchnorm_track=True, isola_patch_side=P_NET,
                              doersch_patch_side=P_NET)
  cls = archs.SegmentationNet10aIsola if kind == "isola" else archs.SegmentationNet10aDoersch
  net = cls(cfg)
  net.load_state_dict({k: v.clone() for k, v in params.items()}, strict=True)
  return net.to(dev()).train()


def _loss_of(kind, out, gt, mask):
  from iic_amd import seg_baselines as sb
  if kind == "isola":
    return sb.isola_loss(out, CENTRE, OTHER, bool(gt), mask)
  return sb.doersch_loss(out, CENTRE, OTHER, gt, mask)


@pytest.mark.parametrize("kind,gt", [("isola", True), ("isola", False), ("doersch", 5)])
def test_step_vs_oracle(kind, gt):
  from iic_amd import ops
  params = _net_params(kind, 3)
  x, keep, mask = _inputs(4)
  rp = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone())
        for k, v in params.items()}
  ref_out = _oracle_forward(kind, rp, x, keep)
  ref_loss = _oracle_loss(kind, ref_out, mask, gt)
  ref_loss.backward()
  h = kind + "_head.siamese_branch.1."
  assert int(rp[h + "num_batches_tracked"]) == 2
  # ---- the exact-fp32 tier, at the tolerances test_gpu_triplets.py::_check_step cites
  net = _make(kind, params)
  net.dropout_keep = keep.to(dev())
  with ops.fp32_mode():
    out = net(x.to(dev()), centre=CENTRE, other=OTHER)
    loss = _loss_of(kind, out, gt, mask.to(dev()))
    loss.backward()
  torch.cuda.synchronize()
  dmax = (out.detach().cpu() - ref_out.detach()).abs().max().item()
  scale = max(1.0, ref_out.detach().abs().max().item())
  print("%s fp32: max |out - ref| = %.3e (scale %.3f); loss %.8e, reference %.8e" % (
    kind, dmax, scale, float(loss.detach()), float(ref_loss.detach())))
  assert out.shape == ref_out.shape and dmax <= 2e-4 * scale, (dmax, scale)
  assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 5e-4 * abs(float(ref_loss.detach())) + 1e-7
  for n, p in net.named_parameters():
    gn = float(rp[n].grad.double().norm())
    assert abs(float(p.grad.double().norm()) - gn) <= 1e-2 * max(gn, 1e-6) + 1e-9, (n, float(p.grad.double().norm()), gn)
  sd = net.state_dict()
  assert int(sd[h + "num_batches_tracked"]) == 2
  for name in ("running_mean", "running_var"):      # after its two calls, in the oracle's order
    assert_within(sd[h + name], rp[h + name].detach(), 1e-5 + 1e-4 * rp[h + name].detach().abs().double(), h + name)
  # ---- the bf16 path: finite gradients, two steps from the same state give equal bits; the gap is printed, not asserted
  res = []
  for _ in range(2):
    nb = _make(kind, params)
    nb.dropout_keep = keep.to(dev())
    ob = nb(x.to(dev()), centre=CENTRE, other=OTHER)
    lb = _loss_of(kind, ob, gt, mask.to(dev()))
    lb.backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in nb.parameters())
    res.append((ob.detach(), lb.detach(), [p.grad.clone() for p in nb.parameters()], nb.state_dict()))
  assert_bits(res[0][0], res[1][0], "bf16 outputs, second step")
  assert_bits(res[0][1], res[1][1], "bf16 loss, second step")
  for (n, _), a, b in zip(nb.named_parameters(), res[0][2], res[1][2]):
    assert_bits(a, b, "bf16 grad %s, second step" % n)
  print("%s bf16: max |out - oracle| = %.3e, loss %.8e (oracle %.8e, rel %.2e)" % (
    kind, (res[0][0].cpu() - ref_out.detach()).abs().max().item(), float(res[0][1]), float(ref_loss.detach()),
    abs(float(res[0][1]) - float(ref_loss.detach())) / abs(float(ref_loss.detach()))))


def test_eval_mode_and_train_step():
  """eval(): dropout is the identity and the siamese stage uses its running statistics; train_step runs the scripts'
  loop body with iic_amd.optim.Adam and returns a device scalar."""
  from iic_amd import ops, seg_baselines as sb
  from iic_amd.optim import Adam
  params = _net_params("doersch", 5)
  x, keep, mask = _inputs(6)
  net = _make("doersch", params).eval()
  net.dropout_keep = torch.zeros_like(keep).to(dev())      # would zero everything if it were applied
  with ops.fp32_mode(), torch.no_grad():
    out = net(x.to(dev()), centre=CENTRE, other=OTHER)
  ref = _oracle_forward("doersch", {k: v.clone() for k, v in params.items()}, x, keep, training=False)
  d = (out.cpu() - ref).abs().max().item()
  assert d <= 2e-4 * max(1.0, ref.abs().max().item()), d
  assert int(net.state_dict()["doersch_head.siamese_branch.1.num_batches_tracked"]) == 0
  for kind in ("isola", "doersch"):
    net = _make(kind, _net_params(kind, 7))
    opt = Adam(net.parameters(), lr=1e-4)
    before = [p.detach().clone() for p in net.parameters()]
    loss = sb.train_step(net, opt, x.to(dev()), mask.to(dev()), kind, rng=np.random.RandomState(1))
    torch.cuda.synchronize()
    assert loss.is_cuda and loss.shape == () and bool(torch.isfinite(loss))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    loss2 = sb.train_step(net, opt, x.to(dev()), mask.to(dev()), kind, rng=np.random.RandomState(2))
    assert bool(torch.isfinite(loss2))      # the refreshed bf16 operands of the joint Linear are in use
  with pytest.raises(ValueError):
    net(x.to(dev()), centre=np.array([0, 5]), other=OTHER)
  with pytest.raises(ValueError):
    net(x, centre=CENTRE, other=OTHER)


def test_kmeans_eval_and_trunk_checkpoint_on_an_isola_net():
  """The section-5i evaluation twins accept the subclass unchanged, and load_trunk_state_dict reads its checkpoint."""
  from iic_amd import archs, kmeans, seg_kmeans
  from iic_amd.archs import seg as seg_archs
  from tests.test_gpu_seg_kmeans import _Loader, _e2e_config
  config = _e2e_config(isola_patch_side=P_NET)
  torch.manual_seed(0)
  net = archs.SegmentationNet10aIsola(config).to(dev())
  S, gt_k, n_img, bs = config.input_sz, config.gt_k, 5, 2
  rng = np.random.RandomState(12)
  imgs = rng.random_sample((n_img, 3, S, S)).astype(np.float32)
  targets = rng.randint(0, gt_k, (n_img, S, S)).astype(np.int32)
  mask = rng.random_sample((n_img, S, S)) < 0.85
  batches = [(torch.from_numpy(imgs[i:i + bs]), torch.from_numpy(targets[i:i + bs]), torch.from_numpy(mask[i:i + bs]))
             for i in range(0, n_img, bs)]
  np.random.seed(3)
  acc, nmi, ari, masses = seg_kmeans.kmeans_segmentation_eval(config, net, _Loader(batches, n_img), sampling="uniform",
                                                              kmeans=kmeans.MiniBatchKMeans(gt_k, seed=1))
  assert 0.0 < acc <= 1.0 and (nmi, ari) == (-1., -1.) and abs(float(masses.sum()) - 1.0) < 1e-9 and not net.training
  with torch.no_grad():
    up = net(torch.from_numpy(imgs[:2]).to(dev()), penultimate=True)      # inherited
  assert tuple(up.shape) == (2, 512, S, S)
  feats = archs.SegmentationNet10aFeatures(config).to(dev())
  seg_archs.load_trunk_state_dict(feats, net.state_dict())
  for (n, a), (_, b) in zip(feats.features.state_dict().items(), net.features.state_dict().items()):
    assert torch.equal(a, b), n
  other = archs.SegmentationNet10aIsola(config).to(dev())
  seg_archs.load_trunk_state_dict(other, net.state_dict())
  assert torch.equal(other.features.features[0].weight, net.features.features[0].weight)
