"""csrc/seg_augment.hip through the C ABI (iic_amd/seg_augment.py) against
  * the reference-generated fixture tests/golden/seg_augment.npz (tools/gen_golden_seg_augment.py: the reference's
    own `_prepare_train` of the Potsdam and COCO-Stuff datasets, every draw recorded) -- img1, mask_img1,
    affine2_to_1 and img2 without random affine bit-identical, every pixel compared; img2 with random affine within
    the tolerance tests/test_gpu_seg_loss.py::test_affine_warp_matches_grid_sample applies to the same warp kernel
    (2e-5 absolute on values in [0, 1]);
  * a numpy + PIL restatement of `_prepare_train` (below) at the real batch shapes, bit-identical;
  * one end-to-end training step.
Grey (no_sobel=False) is OpenCV 3.x's fixed-point RGB2GRAY restated from its source on every side -- cv2 itself is
not available; see iic_amd/seg_augment.py."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "seg_augment.npz")
WARP_TOL = 2e-5      # test_affine_warp_matches_grid_sample's bound for iic_affine_warp_fwd


def dev():
  return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------
# numpy + PIL restatement of _prepare_train without random affine (potsdam.py:95-216, cocostuff.py:104-230),
# one image at a time like the reference; torchvision 0.2.1's adjust_* are the PIL calls of oracle/tv021_shim.py
# ------------------------------------------------------------------------------------------
def restate_prepare_train(img, label, relevance, ip, fp, S, no_sobel, include_rgb):
  from PIL import Image
  from iic_amd import seg_augment as sa
  from oracle import tv021_shim as tv
  h, w, cs = img.shape
  new_h, new_w, oy, ox = sa.pad_offsets(h, w, S)
  pad = np.zeros((new_h, new_w, cs), np.uint8)
  pad[oy:oy + h, ox:ox + w] = img
  x0, y0 = int(ip[1]), int(ip[2])
  crop = pad[y0:y0 + S, x0:x0 + S]
  if label is None:
    mask = np.ones((S, S), np.uint8)
  else:
    lpad = np.zeros((new_h, new_w), np.uint8)            # padded label pixels are fine-label 0
    lpad[oy:oy + h, ox:ox + w] = label
    mask = relevance[lpad[y0:y0 + S, x0:x0 + S]]
  img1 = Image.fromarray(np.ascontiguousarray(crop[:, :, :3]))
  img2 = img1
  for o in range(int(ip[4])):
    op = int(ip[5 + o])
    f = float(fp[op])
    assert op != 3 or int(f * 255) % 256 == int(ip[9])      # the uint8 hue increment the kernel was given
    img2 = (tv.adjust_brightness, tv.adjust_contrast, tv.adjust_saturation, tv.adjust_hue)[op](img2, f)
  views = []
  for v in (np.array(img1), np.array(img2)):
    if not no_sobel:
      grey = sa.cv_grey(v)[:, :, None]
      v = np.concatenate([v, grey], axis=2) if include_rgb else grey
    v = v.astype(np.float32) / 255.
    if cs == 4:
      v = np.concatenate([v, (crop[:, :, 3].astype(np.float32) / 255.)[:, :, None]], axis=2)
    views.append(np.ascontiguousarray(v.transpose(2, 0, 1)))
  aff = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
  if ip[3] & 1:
    views[1] = np.ascontiguousarray(views[1][:, :, ::-1])
    aff[0, :] *= np.float32(-1.)
  return views[0], views[1], aff, mask


def _params_from_fixture(g, key, meta, S):
  """iparams / fparams / affine1_to_2 from the RECORDED draws of the reference run."""
  from iic_amd import seg_augment as sa
  n = len(g[key + "/seeds"])
  ip = np.zeros((n, sa.IPARAMS), np.int32)
  fp = np.zeros((n, sa.FPARAMS), np.float32)
  half = int(S / 2.)
  affine = meta["config"]["use_random_affine"]
  a12 = g[key + "/a12"].astype(np.float32) if affine else None
  for i in range(n):
    h_c, w_c = g[key + "/coords"][i]
    nj = int(g[key + "/jit_n"][i])
    ip[i, :5] = (i, w_c - half, h_c - half, g[key + "/rands"][i][-1] > meta["config"]["flip_p"], nj)
    ip[i, 5:5 + nj] = g[key + "/jit_ops"][i][:nj]
    fp[i, :4] = g[key + "/jit_f"][i]
    ip[i, 9] = int(float(g[key + "/jit_f"][i][3]) * 255) % 256
    m21 = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    if affine:
      full = np.concatenate([a12[i], np.array([[0, 0, 1]], np.float32)], 0)
      m21 = np.linalg.inv(full).astype(np.float32)[:2]      # transforms.py:119
    fp[i, 4:10] = m21.reshape(6)
  return dict(iparams=ip, fparams=fp, affine1_to_2=a12)


def _fixture_cases():
  g = np.load(G)
  return [(str(n), int(s)) for n in g["names"] for s in g["sizes"]]


@pytest.mark.parametrize("name,size", _fixture_cases())
def test_fixture_bit_identical(name, size):
  from iic_amd import seg_augment as sa
  g = np.load(G)
  meta = json.loads(str(g[name + "/meta"]))
  key = "%s/%d" % (name, size)
  cfg = types.SimpleNamespace(**meta["config"])
  imgs = torch.from_numpy(g[key + "/images"]).to(dev())
  labels = rel = None
  if meta["kind"] != "potsdam":
    labels = torch.from_numpy(g[key + "/labels"].astype(np.int64) % 256).to(torch.uint8).to(dev())
    rel = g[name + "/relevance"]
  aug = sa.SegPairedAugmenter(imgs, cfg, labels_u8=labels, relevance=rel)
  params = _params_from_fixture(g, key, meta, aug.S)
  img1, img2, aff, mask = (t.cpu().numpy() for t in aug.apply(params))
  assert img1.shape == g[key + "/img1"].shape and img2.shape == g[key + "/img2"].shape
  assert mask.dtype == np.uint8 and aff.dtype == np.float32
  assert img1.tobytes() == g[key + "/img1"].tobytes(), np.abs(img1 - g[key + "/img1"]).max()
  assert mask.tobytes() == g[key + "/mask"].tobytes()
  assert aff.tobytes() == g[key + "/aff"].tobytes(), (aff, g[key + "/aff"])
  err = float(np.abs(img2.astype(np.float64) - g[key + "/img2"].astype(np.float64)).max())
  print("%s: C %d, max |img2 - reference| %.3e%s" % (key, img1.shape[1], err,
                                                     " (random affine)" if cfg.use_random_affine else ""))
  if cfg.use_random_affine:
    assert err <= WARP_TOL, err
  else:
    assert img2.tobytes() == g[key + "/img2"].tobytes(), err
  # two calls with the same parameters give identical bytes (no atomics on this path)
  again = [t.cpu().numpy() for t in aug.apply(params)]
  for a, b in zip((img1, img2, aff, mask), again):
    assert a.tobytes() == b.tobytes()


def test_fixture_covers_every_channel_layout_and_both_flips():
  g = np.load(G)
  layouts, flips = set(), set()
  for name, size in _fixture_cases():
    key = "%s/%d" % (name, size)
    layouts.add(g[key + "/img1"].shape[1])
    flips.update(bool(v) for v in (g[key + "/aff"][:, 0, 0] < 0))
  assert layouts == {1, 2, 3, 4, 5} and flips == {True, False}


REAL = [  # name, batch, dataset size, H, W, Cs, S, no_sobel, include_rgb, jitter, labels
  ("potsdam3", 75, 24, 200, 200, 4, 200, True, False, (0.1, 0.1, 0.1, 0.1), False),
  ("coco3", 120, 24, 141, 187, 3, 128, False, True, (0.4, 0.4, 0.4, 0.125), True),
]


def real_case(name, batch, B, H, W, cs, S, no_sobel, include_rgb, jitter, with_labels, affine=False, seed=0):
  """Random content at a published batch shape; returns (augmenter, host images, host labels, relevance, config)."""
  from iic_amd import seg_augment as sa
  rng = np.random.default_rng(1234 + S)
  imgs = rng.integers(0, 256, (B, H, W, cs), dtype=np.uint8)
  imgs[1, :, :, :3] = np.repeat(imgs[1][:, :, :1], 3, 2)     # a grey image: hue / saturation degenerate
  imgs[2], imgs[3] = 255, 0
  labels = rel = None
  if with_labels:
    labels = rng.integers(0, 183, (B, H, W)).astype(np.uint8)
    labels[labels == 182] = 255                               # unlabelled
    rel = (np.arange(256) >= 91).astype(np.uint8)
    rel[182:] = 0
  cfg = types.SimpleNamespace(input_sz=S, no_sobel=no_sobel, include_rgb=include_rgb, jitter_brightness=jitter[0],
                              jitter_contrast=jitter[1], jitter_saturation=jitter[2], jitter_hue=jitter[3], flip_p=0.5,
                              use_random_affine=affine, use_random_scale=False, pre_scale_all=name == "coco3",
                              aff_min_rot=-30., aff_max_rot=30., aff_min_shear=-10., aff_max_shear=10.,
                              aff_min_scale=0.8, aff_max_scale=1.2)
  aug = sa.SegPairedAugmenter(torch.from_numpy(imgs).to(dev()), cfg,
                              labels_u8=None if labels is None else torch.from_numpy(labels).to(dev()),
                              relevance=rel, seed=seed)
  return aug, imgs, labels, rel, cfg


@pytest.mark.parametrize("case", REAL, ids=[c[0] for c in REAL])
def test_real_batch_shape_bit_identical_to_restatement(case):
  aug, imgs, labels, rel, cfg = real_case(*case)
  batch = case[1]
  idx = np.random.default_rng(5).integers(0, imgs.shape[0], batch)
  p = aug.draw(idx)
  got = [t.cpu().numpy() for t in aug.apply(p)]
  assert got[0].shape == (batch, aug.out_channels, aug.S, aug.S)
  assert len(set(map(tuple, p["iparams"][:, 1:3]))) > 1 or case[3] == aug.S    # crops are actually random
  bad = []
  for i in range(batch):
    src = int(p["iparams"][i, 0])
    want = restate_prepare_train(imgs[src], None if labels is None else labels[src], rel, p["iparams"][i],
                                 p["fparams"][i], aug.S, cfg.no_sobel, cfg.include_rgb)
    for k in range(4):
      if got[k][i].tobytes() != want[k].tobytes():
        bad.append((i, k))
  assert not bad, bad[:8]
  assert set(p["iparams"][:, 3]) == {0, 1}


@pytest.mark.parametrize("kind", ["potsdam", "coco"])
def test_end_to_end_step(kind):
  """paired_batch -> sobel_process where configured -> SegmentationNet10aTwoHead -> uncollapsed loss -> backward."""
  from iic_amd import archs, seg_augment as sa, seg_losses
  from iic_amd.transforms import sobel_process
  torch.manual_seed(0)
  S, n = 48, 6
  rng = np.random.default_rng(3)
  if kind == "potsdam":
    imgs = rng.integers(0, 256, (8, 56, 56, 4), dtype=np.uint8)
    no_sobel, in_ch, labels, rel = True, 4, None, None
  else:
    imgs = rng.integers(0, 256, (8, 50, 60, 3), dtype=np.uint8)
    no_sobel, in_ch = False, 5
    labels = torch.from_numpy(rng.integers(60, 182, (8, 50, 60)).astype(np.uint8)).to(dev())
    rel = (np.arange(256) >= 91).astype(np.uint8)
  cfg = types.SimpleNamespace(input_sz=S, no_sobel=no_sobel, include_rgb=True, jitter_brightness=0.4, jitter_contrast=0.4,
                              jitter_saturation=0.4, jitter_hue=0.125, flip_p=0.5, use_random_affine=False,
                              use_random_scale=False, pre_scale_all=False)
  aug = sa.SegPairedAugmenter(torch.from_numpy(imgs).to(dev()), cfg, labels_u8=labels, relevance=rel, seed=11)
  p = aug.draw(np.arange(n))
  assert set(p["iparams"][:, 3]) == {0, 1}
  img1, img2, aff, mask = aug.apply(p)
  if not no_sobel:
    img1, img2 = sobel_process(img1, True, using_IR=False), sobel_process(img2, True, using_IR=False)
  assert img1.shape == (n, in_ch, S, S)
  ncfg = types.SimpleNamespace(in_channels=in_ch, input_sz=S, batchnorm_track=True, num_sub_heads=1, output_k_A=9,
                               output_k_B=3)
  net = archs.SegmentationNet10aTwoHead(ncfg).to(dev()).train()
  x1, x2 = net(img1, head="B"), net(img2, head="B")
  loss, loss_nl = seg_losses.IID_segmentation_loss_uncollapsed(
    x1[0], x2[0], all_affine2_to_1=aff, all_mask_img1=mask.to(torch.float32), lamb=1.0, half_T_side_dense=1,
    half_T_side_sparse_min=0, half_T_side_sparse_max=0)
  loss.backward()
  assert np.isfinite(loss.item()) and np.isfinite(loss_nl.item())
  gn = sum(float(q.grad.norm()) for q in net.parameters() if q.grad is not None)
  assert np.isfinite(gn) and gn > 0
  flips = seg_losses._flips_from_affine(aff)
  assert flips is not None
  assert list(flips[:, 0].numpy()) == list(p["iparams"][:, 3]) and not flips[:, 1].any()
