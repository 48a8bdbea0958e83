"""The Isola / Doersch baselines without a GPU: the patch-selection twins against the reference's recorded draws, the
float64 restatements of the losses against torch autograd of the reference's expressions, state_dict keys and shapes,
the launch plans of the siamese stage, the argument checks, and the proof that every derived bound of
tests/seg_baseline_cases.py admits correct arithmetic and rejects a seeded defect."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import seg_baseline_cases as bc
from tests.parity import bf16_rne

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
  with open(os.path.join(GOLDEN, name)) as f:
    return json.load(f)


# ---- patch selection ---------------------------------------------------------------------------------------------------
def test_set_patches_twins_reproduce_the_reference_draws():
  from iic_amd import seg_baselines as sb
  g = _golden("seg_baseline_patches.json")
  assert sorted((c["S"], c["p"]) for c in g["cases"]) == [(24, 3), (128, 11), (200, 11)]
  for c in g["cases"]:
    for key, fn in (("isola", sb.isola_set_patches), ("doersch", sb.doersch_set_patches)):
      np.random.seed(g["seed"])                                   # the global stream, as the reference uses it
      rng = np.random.RandomState(g["seed"])                      # and an explicit one
      assert len(c[key]) == g["draws"] == 64
      for want in c[key]:
        for r in (None, rng):
          centre, other, gt = fn(c["S"], c["p"], rng=r)
          assert [int(v) for v in centre] + [int(v) for v in other] + [int(gt)] == want, (key, c["S"], c["p"])
          d = c["p"] // 2
          assert all(d <= int(v) <= c["S"] - 1 - d for v in list(centre) + list(other))
      # both streams consumed the same number of draws
      assert np.random.rand() == rng.rand()
  centre, other, adjacent = sb.isola_set_patches(24, 3, rng=np.random.RandomState(0))
  assert isinstance(adjacent, bool) and centre.dtype == np.int32 and other.dtype == np.int32
  centre, other, pos = sb.doersch_set_patches(24, 3, rng=np.random.RandomState(0))
  assert other.dtype == np.int32 and 0 <= int(pos) < 9


# ---- losses: the restatements against torch autograd of the reference's expressions ----------------------------------
def _torch_isola(p, m, adjacent):
  """isola_utils.py:27-72 in float64 torch, expression for expression (the EPS replacement is an in-place indexed
  assignment there: the gradient of a replaced entry is cut)."""
  pred = torch.tensor(np.asarray(p, dtype=np.float32), dtype=torch.float64, requires_grad=True)
  mt = torch.from_numpy(m)
  norm = float(mt.sum())
  if adjacent:
    t = pred.clone()
  else:
    # the net's output is fp32: 1 - p is rounded to fp32 there; the rounding is a constant shift for autograd
    t32 = (np.float32(1.0) - np.asarray(p, dtype=np.float32)).astype(np.float64)
    t = (1.0 - pred) + torch.from_numpy(t32 - (1.0 - np.asarray(p, dtype=np.float64)))
  lt = (t < bc.EPS)
  keep = 1.0 - lt.double()
  t = torch.where(lt, torch.full_like(t, bc.EPS), t)        # (a constant where replaced)
  loss = -(1.0 / norm) * (mt * keep * torch.log(t)).sum()
  loss.backward()
  return float(loss.detach()), pred.grad.numpy()


@pytest.mark.parametrize("adjacent", [True, False])
@pytest.mark.parametrize("N", bc.LOSS_NS)
def test_isola_restatement_equals_float64_autograd(N, adjacent):
  p = bc.isola_probs(N)
  _, m = bc.loss_mask(N, "mixed" if N > 1 else "all")
  loss, dp, mag, drop = bc.isola_ref(p, m, adjacent)
  tl, tg = _torch_isola(p, m, adjacent)
  assert abs(loss - tl) <= 1e-13 * max(1.0, mag)
  np.testing.assert_allclose(dp, tg, rtol=1e-13, atol=0)
  assert bool((dp[drop] == 0).all())
  if N >= 5:      # the special rows: p = 0 and EPS / 2 are dropped when adjacent, p = 1 (and 1 - 2^-24: fl32(1 - p) = 2^-24,
    #               kept) when not; 2 EPS is kept either way
    assert drop.tolist()[:5] == ([True, True, False, False, False] if adjacent else [False, False, False, False, True])


@pytest.mark.parametrize("label", range(9))
def test_doersch_restatement_equals_float64_autograd(label):
  N = 5
  x = bc.doersch_logits(N)
  _, m = bc.loss_mask(N, "mixed")
  loss, dl, mag, gmag = bc.doersch_ref(x, m, label)
  xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
  mt = torch.from_numpy(m)
  gt = torch.ones(N, dtype=torch.int64) * label
  tl = (mt * torch.nn.CrossEntropyLoss(reduction="none")(xt, gt)).sum() / float(mt.sum())      # doersch_utils.py:61-66
  tl.backward()
  assert abs(loss - float(tl.detach())) <= 1e-13 * mag
  np.testing.assert_allclose(dl, xt.grad.numpy(), rtol=0, atol=1e-14)


def test_norm_zero_is_nan():
  _, m = bc.loss_mask(5, "none")
  assert m.sum() == 0
  loss, dp, _, _ = bc.isola_ref(bc.isola_probs(5), m, True)
  assert np.isnan(loss) and np.isnan(dp).all()
  loss, dl, _, _ = bc.doersch_ref(bc.doersch_logits(5), m, 3)
  assert np.isnan(loss) and np.isnan(dl).all()


# ---- state_dict ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls", [("isola", "SegmentationNet10aIsola"), ("doersch", "SegmentationNet10aDoersch")])
def test_state_keys_and_shapes_match_the_reference(name, cls):
  from iic_amd import archs
  g = _golden("seg_baseline_state_keys.json")[name]
  assert g["class"] == cls
  net = getattr(archs, cls)(types.SimpleNamespace(**g["config"]))
  assert isinstance(net, archs.SegmentationNet10aFeatures)
  assert [[n, list(t.shape)] for n, t in net.state_dict().items()] == g["state"]
  head = getattr(net, name + "_head")
  # vgg.py:42-54: BatchNorm weight 1 / bias 0, Linear bias 0 and N(0, 0.01) weights
  assert float(head.siamese_branch[1].weight.min()) == 1.0 and float(head.siamese_branch[1].bias.abs().max()) == 0.0
  assert float(head.joint[0].bias.abs().max()) == 0.0 and 0.005 < float(head.joint[0].weight.std()) < 0.02
  assert head.joint[2].p == 0.5


# ---- launch plans of the siamese stage ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
  from iic_amd import _lib
  dbg = os.path.join(os.path.dirname(_lib.LIB_PATH), "libiic_hip_dbg.so")
  assert os.path.exists(dbg), "build it: make -C iic_amd/csrc dbg"
  h = ctypes.CDLL(dbg)
  h.iic_conv_igemm_frag_supported.restype = ctypes.c_int
  h.iic_debug_conv_plan.restype = None
  h.iic_debug_wgrad_plan.restype = None
  return h


@pytest.mark.parametrize("N", [4, 75, 120])
@pytest.mark.parametrize("p", [3, 5, 11])
def test_launch_plans_serve_the_siamese_stage(L, N, p):
  """conv 3x3 512 -> 1024 on p x p patches with border 1: the weights-direct kernels serve the forward and the
  backward-data geometry, and the weight gradient has a plan."""
  from iic_amd import geom
  from tests.test_conv_dispatch_cpu import FIELDS, WFIELDS
  spec = geom.ConvSpec(512, 1024, 3, 1, 1, 1)
  geoms = [geom.fwd_geom(spec, N, p, p, 1, 1)] + geom.bwd_data_geoms(spec, N, p, p, 1, 1)
  assert len(geoms) == 2 and geoms[0].ntaps == 9 and geoms[1].ntaps == 9
  for g in geoms:
    out = (ctypes.c_int * len(FIELDS))()
    L.iic_debug_conv_plan(ctypes.byref(g), out)
    plan = dict(zip(FIELDS, out))
    assert plan["kernel"] != 0 and plan["grid"] >= 1 and 0 < plan["lds"] <= 160 * 1024, plan
    assert L.iic_conv_igemm_frag_supported(ctypes.byref(g)) == 1
  out = (ctypes.c_int * len(WFIELDS))()
  L.iic_debug_wgrad_plan(ctypes.byref(geoms[0]), 1, out)
  wplan = dict(zip(WFIELDS, out))
  assert wplan["kernel"] != 0 and 0 < wplan["lds"] <= 160 * 1024 and wplan["nsplit"] >= 1, wplan


def test_pair_linear_host_queries():
  from iic_amd import linear
  pair_fwd_nsplit = lambda N, F, C, p: linear.pt_linear_nsplit(N, F, C, p, p, 2)
  assert pair_fwd_nsplit(75, 1024, 1024, 11) == 64       # 8 column tiles, 3872 K-tiles: two workgroups per CU
  assert pair_fwd_nsplit(4, 1024, 1024, 3) > 1
  assert pair_fwd_nsplit(1, 64, 64, 3) >= 1
  for bad in ((4, 100, 64, 3), (4, 64, 96, 3), (4, 64, 64, 4), (0, 64, 64, 3)):      # F, C, even p, N
    assert pair_fwd_nsplit(*bad) == 0


def test_pair_forward_k_split_counts_are_pinned():
  """iic_pair_linear_fwd_nsplit at 256 CUs (the count without a device, and the MI355X's): two workgroups per CU over the
  row x column tiles, at least 8 K-tiles per slice, at most 64 slices."""
  from iic_amd import _lib
  L = _lib.lib()
  assert L.iic_pair_linear_fwd_nsplit(75, 1024, 1024, 11) == 64      # 8 tiles -> 64 wanted; 3872 K-tiles; the cap
  assert L.iic_pair_linear_fwd_nsplit(3, 1024, 1024, 3) == 36        # 8 tiles -> 64 wanted; 288 K-tiles / 8 = 36


# ---- argument checks ---------------------------------------------------------------------------------------------------
def test_argument_checks():
  from iic_amd import archs, seg_baselines as sb
  from iic_amd.archs import seg_baselines as ab
  with pytest.raises(ValueError):
    ab.check_patches((5, 5), (9, 9), 24, 4)                   # even patch side
  with pytest.raises(ValueError):
    ab.check_patches(np.array([0, 5]), np.array([9, 9]), 24, 3)      # the patch leaves the map
  with pytest.raises(ValueError):
    ab.check_patches(np.array([5, 5]), np.array([9, 23]), 24, 3)
  with pytest.raises(ValueError):
    ab.check_patches(np.array([5.0, 5.0]), np.array([9, 9]), 24, 3)      # not integers
  with pytest.raises(ValueError):
    ab.check_patches(np.array([5, 5]), None, 24, 3)
  assert ab.check_patches(np.array([1, 22]), np.array([22, 1]), 24, 3) == (1, 22, 22, 1)
  cfg = types.SimpleNamespace(in_channels=3, input_sz=24, batchnorm_track=True, isola_patch_side=3)
  net = archs.SegmentationNet10aIsola(cfg)
  with pytest.raises(ValueError):                             # CPU tensors: no fallback, nothing enqueued
    net(torch.zeros(2, 3, 24, 24), centre=np.array([5, 5]), other=np.array([9, 9]))
  with pytest.raises(ValueError):
    archs.SegmentationNet10aIsola(types.SimpleNamespace(in_channels=3, input_sz=24, batchnorm_track=True,
                                                        isola_patch_side=4))
  c, o = np.array([5, 5]), np.array([9, 9])
  mask = torch.ones(2, 24, 24, dtype=torch.uint8)
  with pytest.raises(ValueError):
    sb.isola_loss(torch.full((2, 1), 0.5), c, o, True, mask)
  with pytest.raises(ValueError):
    sb.doersch_loss(torch.zeros(2, 9), c, o, 3, mask)
  with pytest.raises(ValueError):
    sb.train_step(net, None, torch.zeros(2, 3, 24, 24), mask, "other")


# ---- the bounds admit correct arithmetic and reject seeded defects ---------------------------------------------------
@pytest.mark.parametrize("case", bc.LATTICE_CASES[:6], ids=lambda c: c.name)
def test_sampler_lattice_is_exact_and_rejects_a_swapped_tap(case):
  x = bc.lattice_features(case)
  ref = bc.sample64(x, case)
  assert np.array_equal(ref * 16, np.round(ref * 16)) and float(np.abs(ref).max()) <= 8      # exact in fp32 and in bf16
  assert np.array_equal(bf16_rne(torch.from_numpy(ref)).numpy(), ref)
  bad = bc.sample64(x, case, swap=True)
  assert float((bad != ref).mean()) > 0.3
  # the adjoint: the fp32 emulation in the kernel's order is exact on the lattice, and <fwd x, g> == <x, bwd g> exactly
  g = bc.lattice_grads(case)
  dx, A, T = bc.adjoint64(g, case)
  assert np.array_equal(bc.emu_adjoint_f32(g, case).astype(np.float64), dx)
  assert float((ref * g).sum()) == float((x * dx).sum())
  if case.name in ("adjacent_p3", "same_p3"):
    assert int(((bc.adjoint64(g, case, patches=(0,))[2] > 0) & (bc.adjoint64(g, case, patches=(1,))[2] > 0)).sum()) > 0


@pytest.mark.parametrize("case", bc.RATIO_CASES, ids=lambda c: c.name)
def test_adjoint_bound_admits_fp32_and_rejects_a_missing_patch(case):
  g = bc.mantissa_grads(case)
  dx, A, T = bc.adjoint64(g, case)
  tol = bc.adjoint_bound(A, T)
  got = bc.emu_adjoint_f32(g, case).astype(np.float64)
  touched = np.broadcast_to((T > 0)[None, None], dx.shape)
  assert bool((np.abs(got - dx) <= tol).all())
  assert bool((got[~touched] == 0).all()) and bool((tol[~touched] == 0).all())
  worst = float((np.abs(got - dx)[touched] / tol[touched]).max())
  assert 0 < worst < 1
  # defect: the other patch left out of the gather
  bad = bc.emu_adjoint_f32(g, case, patches=(0,)).astype(np.float64)
  only_other = np.broadcast_to(((bc.adjoint64(g, case, patches=(1,))[2] > 0))[None, None], dx.shape)
  assert float((np.abs(bad - dx) > tol)[only_other].mean()) > 0.95


def test_pair_bounds_admit_fp32_and_reject_exchanged_halves():
  case = bc.PAIR_CASES[1]      # N = 3, C = 64, p = 3, F = 64
  t = bc.pair_mantissa(case)
  wb, dyb = t["w"].to(torch.bfloat16).float(), t["dy"].to(torch.bfloat16).float()
  y, Ay, dW, AdW, dx0, dx1, Adx0, Adx1 = bc.pair_products64(t["a0"], t["a1"], wb, t["b"], dyb)
  for chunks in (1, 2, 18):
    got = bc.emu_pair_forward(t["a0"], t["a1"], wb, t["b"], chunks).double()
    assert bool(((got - y).abs() <= bc.pair_forward_bound(case, Ay, chunks)).all())
  yx = bc.pair_products64(t["a0"], t["a1"], wb, t["b"], dyb, exchange=True)
  assert float(((yx[0] - y).abs() > bc.pair_forward_bound(case, Ay, 18)).double().mean()) > 0.99
  assert float(((yx[4] - dx0).abs() > bc.pair_dx_bracket(case, dx0, Adx0)[0]).double().mean()) > 0.99
  # dW with its halves exchanged is dW of the exchanged activations
  K = bc.pair_K(case)
  swapped = torch.cat([dW[:, K:], dW[:, :K]], dim=1)
  assert float(((swapped - dW).abs() > bc.pair_wgrad_bound(case, AdW)).double().mean()) > 0.99
  # the lattice is exact in fp32
  t = bc.pair_lattice(case)
  y = bc.pair_products64(t["a0"], t["a1"], t["w"], t["b"], t["dy"])
  assert float(max(y[1].max(), y[3].max(), y[6].max(), y[7].max())) < 2 ** 24
  assert torch.equal(bc.emu_pair_forward(t["a0"], t["a1"], t["w"], t["b"], 2).double(), y[0])


@pytest.mark.parametrize("N", [7, 257])
def test_loss_bounds_admit_fp32_rounding_and_reject_norm_n(N):
  mask, m = bc.loss_mask(N, "mixed")
  assert 0 < m.sum() < N
  for adjacent in (True, False):
    p = bc.isola_probs(N)
    loss, dp, mag, drop = bc.isola_ref(p, m, adjacent)
    tl, tg = bc.isola_bounds(loss, dp, mag, N)
    assert abs(float(np.float32(loss)) - loss) <= tl and bool((np.abs(dp.astype(np.float32) - dp) <= tg).all())
    # defect: norm = N instead of sum m
    bad = loss * m.sum() / N
    assert abs(bad - loss) > 1e3 * tl
    assert bool((np.abs(dp * m.sum() / N - dp) > tg)[(m > 0) & ~drop].all())
  x = bc.doersch_logits(N)
  loss, dl, mag, gmag = bc.doersch_ref(x, m, 4)
  tl, tg = bc.doersch_bounds(loss, dl, mag, gmag, N, 9)
  assert abs(float(np.float32(loss)) - loss) <= tl and bool((np.abs(dl.astype(np.float32) - dl) <= tg).all())
  bl, bdl, _, _ = bc.doersch_ref(x, m, 4, norm=float(N))
  assert abs(bl - loss) > 1e3 * tl
  assert bool((np.abs(bdl - dl) > tg)[m > 0].all())
