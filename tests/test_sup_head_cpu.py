"""CPU proof of what tests/test_gpu_sup_head.py asks of the kernels (tests/sup_head_cases.py): the ten-crop boxes against
PIL, the weight-column permutation, the float64 bounds of the three products on a numpy / torch emulation -- correct
arithmetic in several orders passes, seeded defects are rejected -- the decisive-share condition of the committed draws,
and the BatchNorm1d / cross-entropy bounds on an fp32 emulation of the kernels' arithmetic.  No GPU."""
import numpy as np
import pytest
import torch

from tests import sup_head_cases as sc
from tests.parity import assert_in_bracket, assert_within, outside_share


def _outside(got, ref, tol):
  return float((~((got.double() - ref.double()).abs() <= tol)).double().mean())


# ---- ten-crop boxes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,S", [(96, 96, 64), (97, 95, 64), (96, 96, 96), (33, 40, 32)])
def test_ten_crop_params_vs_pil(W, H, S):
  """torchvision 0.2.1 TenCrop(S): five_crop(img) + five_crop(hflip(img)), F.center_crop's int(round(.)) -- on even and odd
  H - S, W - S.  A row (idx, x, y, flip) means: crop the image at (x, y), then mirror the crop if flip."""
  from PIL import Image
  from iic_amd.semisup import ten_crop_params
  from iic_amd.augment import FPARAMS, IPARAMS
  rng = np.random.default_rng(1)
  img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
  pil = Image.fromarray(img)

  def five(im):
    w, h = im.size
    i, j = int(round((h - S) / 2.)), int(round((w - S) / 2.))
    return [im.crop((0, 0, S, S)), im.crop((w - S, 0, w, S)), im.crop((0, h - S, S, h)), im.crop((w - S, h - S, w, h)),
            im.crop((j, i, j + S, i + S))]
  want = five(pil) + five(pil.transpose(Image.FLIP_LEFT_RIGHT))
  ip, fp = ten_crop_params([7, 2], W, H, S)
  assert ip.shape == (20, IPARAMS) and ip.dtype == np.int32 and fp.shape == (20, FPARAMS) and not fp.any()
  assert list(ip[:, 0]) == [7] * 10 + [2] * 10
  assert not ip[:, 4:].any()                        # no jitter, table 0, no rotation, no cutout
  for rows in (ip[:10], ip[10:]):
    for (_, x, y, flip), w_img in zip(rows[:, :4], want):
      got = img[y:y + S, x:x + S]
      if flip:
        got = got[:, ::-1]
      assert np.array_equal(got, np.asarray(w_img)), (x, y, flip)


# ---- the weight operand's column order -------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", [(64, 3, 3), (4, 2, 3), (256, 5, 5)])
def test_column_permutation_and_inverse(C, H, W):
  from iic_amd.semisup import permute_columns, unpermute_columns
  K = C * H * W
  perm, inv = permute_columns(C, H, W), unpermute_columns(C, H, W)
  assert sorted(perm) == list(range(K)) and np.array_equal(perm[inv], np.arange(K)) and np.array_equal(inv[perm], np.arange(K))
  x = np.arange(K).reshape(1, C, H, W)                         # distinct integers, NCHW
  param_order = x.reshape(1, -1)                               # net5g.py:56
  pt_order = x.transpose(0, 2, 3, 1).reshape(1, -1)            # the PT interior, row by row
  assert np.array_equal(param_order[:, perm], pt_order)
  assert np.array_equal(pt_order[:, inv], param_order)


def test_lattice_preconditions():
  for case in sc.LATTICE_CASES:
    t = sc.lattice_inputs(case)
    assert sc.columns_distinct(t["w"])
    _, Ay, _, AdW, _, Adx = sc.products64(t["x"], t["w"], t["b"], t["dy"])
    assert float(max(Ay.max(), AdW.max(), Adx.max())) < 2 ** 24
    for v in t.values():
      assert torch.equal(sc.bf16(v), v)


# ---- the forward's K split ---------------------------------------------------------------------------------------------
def test_forward_k_split_counts_are_pinned():
  """iic_sup_fwd_nsplit at 256 CUs (the count without a device, and the MI355X's): two workgroups per CU over the
  row x column tiles, at least 8 K-tiles per slice, at most 16 slices; 0 for a shape the kernels do not serve."""
  from iic_amd import _lib
  L = _lib.lib()
  for (N, F, C, H, W), want in (((37, 192, 64, 3, 3), 1),           # 2 tiles; 9 K-tiles: no slice has 8
                                ((12, 2048, 256, 5, 5), 12),        # 16 tiles -> 32 wanted; 100 K-tiles / 8 = 12
                                ((150, 64, 64, 2, 3), 1),           # 6 K-tiles
                                ((3, 64, 64, 9, 8), 9),             # 1 tile -> 512 wanted; 72 K-tiles / 8 = 9
                                ((700, 2048, 256, 9, 9), 6)):       # 96 tiles -> 6 wanted; 324 K-tiles
    assert L.iic_sup_fwd_nsplit(N, F, C, H, W) == want, (N, F, C, H, W)
  u = sc.UNSUPPORTED
  assert L.iic_sup_fwd_nsplit(u.N, u.F, u.C, u.H, u.W) == 0


# ---- the three products: correct arithmetic passes, defects are rejected -------------------------------------------
@pytest.mark.parametrize("draw", sc.DRAWS)
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_correct_arithmetic_passes(case, draw):
  t = sc.inputs(case, draw)
  y64, Ay, dW64, AdW, dx64, Adx = sc.refs(case, draw)
  wb, dyb = sc.bf16(t["w"]), sc.bf16(t["dy"])
  for chunks, order in ((1, None), (12, None), (12, list(range(11, -1, -1))), (5, [2, 0, 4, 1, 3])):
    y = sc.emu_forward(t["x"], wb, t["b"], chunks, order)
    assert_within(y, y64, sc.forward_bound(case, Ay, chunks), "forward, %d slices" % chunks)
  for chunks, order in ((1, None), (4, None), (3, [2, 0, 1])):
    assert_within(sc.emu_wgrad(t["x"], dyb, chunks, order), dW64, sc.wgrad_bound(case, AdW), "dW, %d slices" % chunks)
  b, lo, hi = sc.dx_bracket(case, dx64, Adx)
  for chunks, order in ((1, None), (8, None), (3, [1, 2, 0])):
    assert_in_bracket(sc.store_rne(sc.emu_dx_acc(t["x"].shape, dyb, wb, chunks, order)), lo, hi, "dx, %d slices" % chunks)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_seeded_defects_are_rejected(case):
  from iic_amd.semisup import permute_columns
  t = sc.inputs(case, "pos")
  y64, Ay, dW64, AdW, dx64, Adx = sc.refs(case, "pos")
  wb, dyb = sc.bf16(t["w"]), sc.bf16(t["dy"])
  S = 12
  fb, wgb = sc.forward_bound(case, Ay, S), sc.wgrad_bound(case, AdW)
  b, lo, hi = sc.dx_bracket(case, dx64, Adx)
  acc = sc.emu_dx_acc(t["x"].shape, dyb, wb)
  assert outside_share(sc.store_rne(acc), lo, hi) == 0.0
  # 1. a truncating store
  assert outside_share(sc.store_truncating(acc), lo, hi) > 0.3
  # 2. a value rounded twice: the fp32 results staged through bf16; dx's partial sums stored as bf16 between K slices
  assert _outside(sc.store_rne(sc.emu_forward(t["x"], wb, t["b"])), y64, fb) > 0.5
  assert _outside(sc.store_rne(sc.emu_wgrad(t["x"], dyb)), dW64, wgb) > 0.5
  # (four partials a quarter of the result's size: their roundings are a quarter of its spacing, so they move the final
  # rounding of every seventh element or so -- any one of them fails the GPU test)
  assert outside_share(sc.store_rne(sc.emu_dx_acc(t["x"].shape, dyb, wb, 4, on_part=sc.store_rne)), lo, hi) > 0.05
  # 3. one K-tile of 64 dropped (a wrong loop bound), in the forward and in dx (64 of the F terms)
  K = sc.K_of(case)
  assert _outside(sc.emu_forward(t["x"], wb, t["b"], drop_tile=(K - 64, K)), y64, fb) > 0.9
  short = sc.emu_dx_acc(t["x"].shape, dyb[:, :case.F - 64], wb[:case.F - 64])
  assert outside_share(sc.store_rne(short), lo, hi) > 0.9
  # 4. the (h, w, c) operand order used against the parameter's (c, h, w) columns
  perm = torch.from_numpy(permute_columns(case.C, case.H, case.W))
  tm = sc.inputs(case, "mixed")
  ym64, Aym = sc.refs(case, "mixed")[:2]
  assert _outside(sc.emu_forward(tm["x"], sc.bf16(tm["w"]), tm["b"], columns=perm), ym64, sc.forward_bound(case, Aym, S)) > 0.9
  # ... and a weight gradient left in the operand's order
  dWm64, AdWm = sc.refs(case, "mixed")[2:4]
  assert _outside(sc.emu_wgrad(tm["x"], sc.bf16(tm["dy"]))[:, perm], dWm64, sc.wgrad_bound(case, AdWm)) > 0.9


@pytest.mark.parametrize("draw", sc.DRAWS)
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_decisive_share_of_the_committed_draws(case, draw):
  """The condition of the dx check, on the reference alone: a weak case cannot hide behind a wide bracket."""
  _, _, _, _, dx64, Adx = sc.refs(case, draw)
  _, lo, hi = sc.dx_bracket(case, dx64, Adx)
  floor = sc.decisive_floor(case, draw)
  share = sc.decisive_share(lo, hi)
  if draw == "pos":
    assert floor == sc.POS_DECISIVE_FLOOR == 0.85
  if floor is not None:
    assert share >= floor, (case.name, draw, share, floor)


# ---- BatchNorm1d + ReLU: an fp32 emulation of the kernels' arithmetic ----------------------------------------------
f32 = lambda v: torch.as_tensor(v, dtype=torch.float64).float()


def emu_bn(t, training, biased_running=False):
  x, N = t["x"], t["x"].shape[0]
  if training:
    xs = x.double()
    m64 = xs.mean(0).double()
    v64 = ((xs - xs.mean(0)) ** 2).mean(0).double()
    rm = f32(0.9 * t["rm"].double() + 0.1 * m64)
    rv = f32(0.9 * t["rv"].double() + 0.1 * v64 * (1.0 if biased_running else N / (N - 1.0)))
  else:
    m64, v64, rm, rv = t["rm"].double(), t["rv"].double(), t["rm"], t["rv"]
  mean, inv = f32(m64), f32(1.0 / torch.sqrt(v64 + sc.BN_EPS))
  xh = (x - mean) * inv
  y = torch.relu(xh * t["gamma"] + t["beta"])
  gz = torch.where(y > 0, t["dout"], torch.zeros_like(y))
  S1, S2 = gz.double().sum(0), (gz.double() * xh.double()).sum(0)
  k = t["gamma"] * inv
  m1, m2 = (f32(S1 / N), f32(S2 / N)) if training else (torch.zeros_like(k), torch.zeros_like(k))
  dx = k * (gz - m1 - xh * m2)
  return dict(y=y, rm=rm, rv=rv, dgamma=f32(S2), dbeta=f32(S1), dx=dx)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("N,F", [(37, 192), (12, 2048), (2, 64)])
def test_bn_bounds_on_the_emulation(N, F, training):
  t = sc.bn_inputs(N, F, 1)
  r = sc.bn_ref(t, training)
  assert not bool(sc.bn_ambiguous(t, r).any()), "a pre-activation of the committed draw lies within its own bound of 0"
  e = emu_bn(t, training)
  _, ez = sc.bn_fwd_bound(t, r)
  tdx, tdg, tdb = sc.bn_bwd_bounds(t, r, training)
  assert_within(e["y"], r["y"], ez, "y")
  assert_within(e["dgamma"], r["dgamma"], tdg, "dgamma")
  assert_within(e["dbeta"], r["dbeta"], tdb, "dbeta")
  assert_within(e["dx"], r["dx"], tdx, "dx")
  if training:
    uv = t["x"].double().var(0, unbiased=True)
    assert_within(e["rm"], r["rm1"], sc.bn_running_bound(t["rm"], [r["mean"]], N), "running_mean")
    assert_within(e["rv"], r["rv1"], sc.bn_running_bound(t["rv"], [uv], N), "running_var")
    # defect: the biased variance in the running update
    bad = emu_bn(t, True, biased_running=True)
    assert _outside(bad["rv"], r["rv1"], sc.bn_running_bound(t["rv"], [uv], N)) > 0.99
  # defect: an output staged through bf16
  assert _outside(sc.store_rne(e["y"]), r["y"], ez) > 0.3


# ---- cross-entropy: an fp32 emulation ------------------------------------------------------------------------------
def emu_ce(logits, targets):
  x = logits.numpy().astype(np.float32)
  N, k = x.shape
  m = x.max(1, keepdims=True)
  e = np.exp(x - m, dtype=np.float32)
  s = np.zeros((N, 1), np.float32)
  for j in range(k):
    s = s + e[:, j:j + 1]
  oh = np.eye(k, dtype=np.float32)[targets.numpy()]
  dl = (e * (np.float32(1) / s) - oh) * (np.float32(1) / np.float32(N))
  xt = np.take_along_axis(x, targets.numpy()[:, None], 1)
  rows = np.log(s, dtype=np.float32) - (xt - m)
  return torch.tensor([np.float32(rows.astype(np.float64).mean())]), torch.from_numpy(dl)


@pytest.mark.parametrize("N,k", [(37, 10), (1, 10), (300, 3)])
def test_cross_entropy_bounds_on_the_emulation(N, k):
  logits, targets = sc.ce_inputs(N, k, 1)
  assert float(logits[N // 2].max() - logits[N // 2].min()) == 160.0
  loss64, dl64 = sc.ce_ref(logits, targets)
  tol_loss, tol_dl = sc.ce_bounds(logits, targets)
  loss, dl = emu_ce(logits, targets)
  assert_within(loss, loss64.view(1), tol_loss.view(1), "loss")
  assert_within(dl, dl64, tol_dl, "dlogits")
  # without the max subtraction the wide row overflows: the reference is finite, so the bound rejects it
  with np.errstate(over="ignore"):
    naive = np.exp(logits.numpy().astype(np.float32) * np.float32(2))
  assert not np.isfinite(naive).all()
  # defect: dlogits not divided by N
  if N > 1:
    assert _outside(dl * N, dl64, tol_dl) > 0.9


# ---- ten-crop count -------------------------------------------------------------------------------------------------
def test_tencrop_special_rows_and_restatement():
  k = 10
  lg = sc.tencrop_logits(7, k, 1)
  im = lg.reshape(7, 10, k)
  assert im[0, :, 2].sum() == im[0, :, 5].sum() and im[0].astype(np.float64).sum(0).argmax() == 2
  acc32 = np.zeros(k, np.float32)
  for q in range(10):
    acc32 = acc32 + im[1, q]
  assert acc32.argmax() == 3 and im[1].astype(np.float64).sum(0).argmax() == 1
  tg = im.astype(np.float64).sum(1).argmax(1)
  assert sc.assess_acc_block_np([lg], [tg]) == (7, 7)
  tg2 = tg.copy()
  tg2[1] = 3
  assert sc.assess_acc_block_np([lg[:30], lg[30:]], [tg2[:3], tg2[3:]]) == (6, 7)
