"""Host logic of iic_amd/seg_augment.py against the reference-generated fixture tests/golden/seg_augment.npz
(tools/gen_golden_seg_augment.py: the reference's own `_prepare_train` with every random draw recorded).
No GPU: draws, crop arithmetic, affine matrices, refusals and the dataloader list."""
import json
import os
import types

import numpy as np
import pytest
import torch

from iic_amd import seg_augment as sa

G = os.path.join(os.path.dirname(__file__), "golden", "seg_augment.npz")


def _fixture():
  return np.load(G)


def _cases(g):
  for name in g["names"]:
    meta = json.loads(str(g[str(name) + "/meta"]))
    for size in g["sizes"]:
      yield str(name), int(size), meta


def _augmenter(g, name, size, meta, device="cpu"):
  key = "%s/%d" % (name, size)
  cfg = types.SimpleNamespace(**meta["config"])
  imgs = torch.from_numpy(g[key + "/images"]).to(device)
  labels = rel = None
  if meta["kind"] != "potsdam":
    labels = torch.from_numpy(g[key + "/labels"].astype(np.int64) % 256).to(torch.uint8).to(device)     # -1 -> 255
    rel = g[name + "/relevance"]
  return sa.SegPairedAugmenter(imgs, cfg, labels_u8=labels, relevance=rel), key


def test_draw_replays_the_reference_draws():
  """Seeded like numpy's global generator was for the fixture, `draw` makes the reference's draws in the
  reference's order: crop centre, jitter factors and op order, random_affine's matrices, flip."""
  g = _fixture()
  n_checked = 0
  for name, size, meta in _cases(g):
    aug, key = _augmenter(g, name, size, meta)
    for i, seed in enumerate(g[key + "/seeds"]):
      aug.rng = np.random.RandomState(int(seed))
      p = aug.draw([i])
      assert tuple(p["coords"][0]) == tuple(g[key + "/coords"][i]), (key, i)
      nj = int(g[key + "/jit_n"][i])
      assert p["iparams"][0, 4] == nj
      assert list(p["iparams"][0, 5:5 + nj]) == list(g[key + "/jit_ops"][i][:nj])
      f = g[key + "/jit_f"][i]
      assert np.array_equal(p["fparams"][0, :4], f.astype(np.float32))
      assert p["hue"][0] == f[3] and p["iparams"][0, 9] == int(f[3] * 255) % 256
      flip = g[key + "/rands"][i][-1] > meta["config"]["flip_p"]
      assert bool(p["iparams"][0, 3]) == bool(flip)
      if meta["config"]["use_random_affine"]:
        assert np.array_equal(p["affine1_to_2"][0], g[key + "/a12"][i])
      else:
        assert p["affine1_to_2"] is None
      # affine2_to_1 as the kernel writes it: fparams[4:10], top row negated when flipped -- bit-equal
      a21 = p["fparams"][0, 4:10].reshape(2, 3).copy()
      if flip:
        a21[0, :] *= np.float32(-1.)
      assert a21.tobytes() == g[key + "/aff"][i].tobytes(), (key, i, a21, g[key + "/aff"][i])
      n_checked += 1
  assert n_checked == len(g["names"]) * len(g["sizes"]) * 2


@pytest.mark.parametrize("sz", [31, 32])
@pytest.mark.parametrize("h,w", [(24, 24), (20, 40), (32, 32), (33, 47), (48, 31)])
def test_crop_arithmetic_odd_even_and_too_small(sz, h, w):
  """pad_if_too_small / pad_and_or_crop (transforms.py:23-88) restated line by line here."""
  if not (h >= sz and w >= sz):
    new_h, new_w = max(h, sz), max(w, sz)
    h_start, w_start = int(new_h / 2.) - int(h / 2.), int(new_w / 2.) - int(w / 2.)
  else:
    new_h, new_w, h_start, w_start = h, w, 0, 0
  assert sa.pad_offsets(h, w, sz) == (new_h, new_w, h_start, w_start)
  lo = int(sz / 2.)
  hi_h = (new_h - 1 - int(sz / 2.)) if sz % 2 == 1 else (new_h - int(sz / 2.))
  hi_w = (new_w - 1 - int(sz / 2.)) if sz % 2 == 1 else (new_w - int(sz / 2.))
  assert sa.crop_centre_range(new_h, new_w, sz) == (lo, hi_h + 1, lo, hi_w + 1)
  # every centre of the range gives a crop inside the padded image
  for c, full in ((lo, new_h), (hi_h, new_h), (lo, new_w), (hi_w, new_w)):
    assert 0 <= c - int(sz / 2.) and c - int(sz / 2.) + sz <= full


def test_crop_origins_equal_the_fixture_coords():
  g = _fixture()
  for name, size, meta in _cases(g):
    aug, key = _augmenter(g, name, size, meta)
    half = int(aug.S / 2.)
    for i, seed in enumerate(g[key + "/seeds"]):
      aug.rng = np.random.RandomState(int(seed))
      p = aug.draw([i])
      h_c, w_c = g[key + "/coords"][i]
      assert (p["iparams"][0, 2], p["iparams"][0, 1]) == (h_c - half, w_c - half)
      # the crop the reference cut, restated with numpy on the padded image, is what those origins select
      new_h, new_w, oy, ox = sa.pad_offsets(size, size, aug.S)
      pad = np.zeros((new_h, new_w, meta["channels"]), np.uint8)
      pad[oy:oy + size, ox:ox + size] = g[key + "/images"][i]
      crop = pad[h_c - half:h_c - half + aug.S, w_c - half:w_c - half + aug.S]
      if meta["config"]["no_sobel"]:
        want = g[key + "/img1"][i][:3]
        assert np.array_equal(crop[..., :3].transpose(2, 0, 1).astype(np.float32) / 255., want)


def test_affine_pair_matches_random_affine():
  g = _fixture()
  seen = 0
  for name, size, meta in _cases(g):
    c = meta["config"]
    if not c["use_random_affine"]:
      continue
    key = "%s/%d" % (name, size)
    for i in range(len(g[key + "/seeds"])):
      ua, ush, usc, uf = g[key + "/rands"][i]
      a = np.radians(ua * (c["aff_max_rot"] - c["aff_min_rot"]) + c["aff_min_rot"])
      sh = np.radians(ush * (c["aff_max_shear"] - c["aff_min_shear"]) + c["aff_min_shear"])
      sc = usc * (c["aff_max_scale"] - c["aff_min_scale"]) + c["aff_min_scale"]
      m12, m21 = sa.affine_pair(a, sh, sc)
      assert m12.tobytes() == g[key + "/a12"][i].tobytes()
      if uf > c["flip_p"]:
        m21 = m21.copy()
        m21[0, :] *= np.float32(-1.)
      assert m21.tobytes() == g[key + "/aff"][i].tobytes()
      seen += 1
  assert seen == 12


def test_warp_matrices_fold_the_flip():
  """A flipped sample's warp reads M (S - 1 - ox, oy, 1): same source pixel as warping, then mirroring."""
  from iic_amd import seg_losses
  S = 32
  m12, _ = sa.affine_pair(0.3, -0.1, 1.1)
  a12 = np.stack([m12, m12])
  M = sa.warp_matrices(a12, np.array([0, 1]), S).double().numpy()
  base = seg_losses._pixel_matrices(torch.from_numpy(a12), S, S).double().numpy()
  assert np.array_equal(M[0], base[0])
  for ox, oy in ((0, 0), (5, 9), (31, 31)):
    for row in (0, 3):
      got = M[1][row] * ox + M[1][row + 1] * oy + M[1][row + 2]
      want = base[1][row] * (S - 1 - ox) + base[1][row + 1] * oy + base[1][row + 2]
      assert abs(got - want) < 1e-4


def _cfg(**kw):
  c = dict(input_sz=32, no_sobel=True, include_rgb=False, jitter_brightness=0.1, jitter_contrast=0.1,
           jitter_saturation=0.1, jitter_hue=0.1, flip_p=0.5, use_random_affine=False, use_random_scale=False,
           pre_scale_all=False)
  c.update(kw)
  return types.SimpleNamespace(**c)


def test_not_implemented_paths_name_their_flag():
  imgs = torch.zeros(2, 40, 40, 3, dtype=torch.uint8)
  with pytest.raises(NotImplementedError, match="use_random_scale"):
    sa.SegPairedAugmenter(imgs, _cfg(use_random_scale=True))
  with pytest.raises(NotImplementedError, match="pre_scale_all"):
    sa.SegPairedAugmenter(imgs, _cfg(pre_scale_all=True), prescaled=False)
  sa.SegPairedAugmenter(imgs, _cfg(pre_scale_all=True))           # the resident images are the pre-scaled ones
  with pytest.raises(AssertionError):
    sa.SegPairedAugmenter(imgs, _cfg(mask_input=True))             # cocostuff.py:63
  with pytest.raises(ValueError):
    sa.SegPairedAugmenter(torch.zeros(2, 6, 6, 3, dtype=torch.uint8), _cfg())   # implausible for input_sz 32
  with pytest.raises(AssertionError):
    sa.SegPairedAugmenter(imgs, _cfg(), labels_u8=torch.zeros(2, 40, 40, dtype=torch.uint8))   # no relevance table
  aug = sa.SegPairedAugmenter(imgs, _cfg())
  with pytest.raises(AssertionError, match="resident on the GPU"):
    aug.apply(aug.draw([0, 1]))                                     # no CPU path


def test_relevance_table_of_a_filter_label():
  def filter_label(label):                                          # cocostuff.py:645-656, stuff-only fine labels
    mask = label >= 91
    return label - 91, mask
  t = sa.relevance_table(filter_label)
  assert t.dtype == np.uint8 and t.shape == (256,)
  assert t[:91].sum() == 0 and t[91:182].all() and t[182:].sum() == 0


def test_dataloader_list_length_order_and_ragged_last_batch():
  imgs = torch.zeros(11, 40, 40, 4, dtype=torch.uint8)
  aug = sa.SegPairedAugmenter(imgs, _cfg())
  calls = []

  def stub_apply(params):
    calls.append(params["iparams"][:, 0].copy())
    n = params["iparams"].shape[0]
    return torch.zeros(n, 4, 32, 32), torch.zeros(n, 4, 32, 32), torch.zeros(n, 2, 3), torch.ones(n, 32, 32)
  aug.apply = stub_apply
  loaders = sa.seg_paired_dataloaders(aug, 4, 3)
  assert len(loaders) == 3 and all(len(d) == 3 for d in loaders)
  seen = []
  for tup in zip(*loaders):                                         # as segmentation_twohead.py:262 zips them
    assert len(tup) == 3
    for img1, img2, aff, mask in tup:
      assert img1.shape[0] == img2.shape[0] == aff.shape[0] == mask.shape[0]
    seen.append(tup[0][0].shape[0])
  assert seen == [4, 4, 3]
  assert [list(c) for c in calls[:3]] == [[0, 1, 2, 3]] * 3          # every loader over the same samples
  assert list(calls[-1]) == [8, 9, 10]


def test_exported_from_the_package():
  import iic_amd
  assert iic_amd.SegPairedAugmenter is sa.SegPairedAugmenter
  assert iic_amd.seg_paired_dataloaders is sa.seg_paired_dataloaders
