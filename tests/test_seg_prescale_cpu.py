"""Host logic of pre_scale_all on the device (iic_amd/seg_prescale.py, SegRaggedAugmenter(source="original")) against the
reference-generated fixture tests/golden/seg_prescale.npz (tools/gen_golden_seg_prescale.py: the reference's own
`_prepare_train` with pre_scale_all on, every draw recorded).  No GPU, numpy only: extents, the two-stage tap tables the
kernel reads, draws, the host pipeline the GPU tests compare against, refusals.  Every comparison is of bytes."""
import types

import numpy as np
import pytest
import torch

from iic_amd import seg_augment as sa
from iic_amd import seg_prescale as sp
from iic_amd import seg_ragged as sr
from tests import seg_prescale_cases as cases


def test_prescaled_sizes_are_scaled_len_and_round_half_to_even():
  sizes = np.array([[50, 150], [150, 50], [61, 150], [185, 121], [1, 2], [97, 130]])
  got = sp.prescaled_sizes(sizes, 0.33)
  assert got.dtype == np.int64 and got.shape == sizes.shape
  assert np.array_equal(got, sr.scaled_len(sizes, 0.33))
  assert 50 * 0.33 == 16.5 and 150 * 0.33 == 49.5                       # exact halves in float64
  assert [list(r) for r in got[:2]] == [[16, 50], [50, 16]]             # 16.5 -> 16, 49.5 -> 50: half to even
  assert list(got[4]) == [1, 1]                                          # at least 1
  for factor in (0.33, 0.5, 0.9):
    for h, w in sizes:
      img = np.zeros((h, w, 3), np.uint8)
      out, lab = sp.prescale_host(img, np.zeros((h, w), np.uint8), factor)
      assert out.shape[:2] == lab.shape == tuple(sp.prescaled_sizes([[h, w]], factor)[0])


def _reference_crop(img, lab, factor, scale, S, y0, x0):
  """resize_linear_host(resize_linear_host(img, f), s) cropped and padded by pad_offsets, truncated."""
  crop, lab = cases.resized_crop(img, lab, [factor, scale], S, y0, x0)
  return crop.astype(np.uint8), lab


@pytest.mark.parametrize("shape", [(7, 5), (61, 150), (185, 121)])
@pytest.mark.parametrize("factor", [0.33, 0.5])
@pytest.mark.parametrize("scale", [0.6, 1.0, 1.4])
def test_crop_taps2_reproduces_two_resizes_in_a_row(shape, factor, scale):
  """The kernel's formula evaluated from crop_taps2's tables gives the bytes of two host resizes, for every crop origin
  class: the first, the last, one in between -- with S = 32 most of these crops lie partly in the padding."""
  rs = np.random.RandomState(shape[0] * 7 + int(scale * 10))
  S = 32
  img = rs.randint(0, 256, shape + (4,)).astype(np.uint8)
  lab = rs.randint(0, 256, shape).astype(np.uint8)
  ext = sr.scaled_len(sr.scaled_len(np.array(shape), factor), scale)
  padded = np.maximum(ext, S)
  padding_seen = False
  for y0 in sorted({0, int(padded[0] - S) // 2, int(padded[0] - S)}):
    for x0 in sorted({0, int(padded[1] - S) // 2, int(padded[1] - S)}):
      ty = sr.crop_taps2([shape[0]], factor, [scale], [y0], S)[0]
      tx = sr.crop_taps2([shape[1]], factor, [scale], [x0], S)[0]
      val, got_lab = cases.emulate_taps2(img, lab, ty, tx)
      want, want_lab = _reference_crop(img, lab, factor, scale, S, y0, x0)
      assert val.astype(np.uint8).tobytes() == want.tobytes(), (shape, factor, scale, y0, x0)
      assert got_lab.tobytes() == want_lab.tobytes()
      # IR is compared untruncated
      assert val[:, :, 3].tobytes() == cases.resized_crop(img, None, [factor, scale], S, y0, x0)[0][:, :, 3].tobytes()
      padding_seen |= not (ty["inside"].all() and tx["inside"].all())
  assert padding_seen or min(ext) >= S
  assert sr.TAP2_DTYPE.itemsize == 48


def test_a_truncated_intermediate_image_does_not_match():
  """The seeded defect: the same emulation with the pre-scaled pixels truncated to uint8 -- what a resident pre-scaled
  image amounts to -- changes about half of the final bytes (49 % here), so the comparison above can see it."""
  rs = np.random.RandomState(0)
  h, w, factor, scale = 97, 130, 0.33, 1.37
  img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
  eh, ew = (int(v) for v in sr.scaled_len(sr.scaled_len(np.array([h, w]), factor), scale))
  S = 44
  assert (eh, ew) == (44, 59)
  ty = sr.crop_taps2([h], factor, [scale], [0], S)[0]
  tx = sr.crop_taps2([w], factor, [scale], [7], S)[0]
  want = _reference_crop(img, None, factor, scale, S, 0, 7)[0]
  good = cases.emulate_taps2(img, None, ty, tx)[0].astype(np.uint8)
  bad = cases.emulate_taps2(img, None, ty, tx, truncate_between=True)[0].astype(np.uint8)
  assert good.tobytes() == want.tobytes()
  share = float((bad != want).mean())
  print("bytes changed by truncating the intermediate image: %.1f %%" % (100 * share))
  assert bad.tobytes() != want.tobytes()


@pytest.mark.parametrize("name", cases.names())
def test_host_pipeline_reproduces_the_reference_tensors(name):
  """Every fixture case: prescale / resize restatements + the host restatements of crop, grey, jitter, warp and flip,
  from the ORIGINAL image and the recorded draws, against img1, img2, affine2_to_1 and mask_img1, bit for bit."""
  cfg = cases.config(name)
  imgs, labels, rel = cases.images(name)
  params = cases.recorded_params(name, cfg.input_sz)
  assert cfg.pre_scale_all and cfg.pre_scale_factor == 0.33
  got = cases.host_pipeline(imgs, labels, rel, cfg, params, cfg.pre_scale_factor)
  assert len(got) == len(imgs)
  for i, g in enumerate(got):
    want = cases.expected(name, i)
    for k, what in enumerate(("img1", "img2", "affine2_to_1", "mask")):
      assert g[k].shape == want[k].shape and g[k].dtype == want[k].dtype, (name, i, what)
      assert g[k].tobytes() == want[k].tobytes(), (name, i, what)


@pytest.mark.parametrize("name", [n for n in cases.names() if not cases.meta(n)["config"]["use_random_scale"]])
def test_without_random_scale_the_resident_prescaled_image_gives_the_same_tensors(name):
  """prescale_host's truncated image through the plain (no resize) pipeline equals the reference for Cs = 3: truncation
  and cropping commute.  For Cs = 4 the IR channel differs (the reference never truncates it) and nothing else does."""
  cfg = cases.config(name)
  imgs, labels, rel = cases.images(name)
  params = cases.recorded_params(name, cfg.input_sz)
  small = [sp.prescale_host(im[:, :, :3], None if labels is None else labels[i], 0.33) for i, im in enumerate(imgs)]
  if imgs[0].shape[2] == 4:
    small = [(np.concatenate([s[0], sr.resize_linear_host(im[:, :, 3].astype(np.float32), 0.33).astype(np.uint8)[:, :, None]],
                             2), s[1]) for s, im in zip(small, imgs)]
  got = cases.host_pipeline([s[0] for s in small], None if labels is None else [s[1] for s in small], rel, cfg, params, None)
  for i, g in enumerate(got):
    want = cases.expected(name, i)
    if imgs[0].shape[2] == 3:
      assert all(g[k].tobytes() == want[k].tobytes() for k in range(4)), (name, i)
    else:
      assert g[0][:3].tobytes() == want[0][:3].tobytes() and g[0][3].tobytes() != want[0][3].tobytes()
      assert np.abs(g[0][3] - want[0][3]).max() < 1 / 255.


def test_fixture_covers_the_layouts_flags_and_half_way_sides():
  g = cases.fixture()
  seen = set()
  for name in cases.names():
    m = cases.meta(name)
    cfg = m["config"]
    assert (cfg["pre_scale_all"], cfg["pre_scale_factor"], cfg["input_sz"]) == (True, 0.33, 32)
    seen.add((m["kind"] == "potsdam", cfg["no_sobel"], cfg["include_rgb"], cfg["use_random_scale"]))
    flips = set(bool(v) for v in (g[name + "/rands"][:, -1] > cfg["flip_p"]))
    assert flips == {True, False}, name
    pre = sp.prescaled_sizes(g[name + "/sizes"], 0.33)
    if cfg["use_random_scale"]:
      assert np.array_equal(g[name + "/extent"], sr.scaled_len(pre, g[name + "/scale"].reshape(-1, 1)))
    else:
      assert np.array_equal(g[name + "/extent"], pre)
  for potsdam, no_sobel, include_rgb in ((False, False, False), (False, False, True), (True, True, False)):
    assert (potsdam, no_sobel, include_rgb, False) in seen and (potsdam, no_sobel, include_rgb, True) in seen
  assert any(cases.meta(n)["config"]["use_random_affine"] for n in cases.names())
  sides = set(int(v) for v in g["coco_sobel/sizes"].reshape(-1))
  assert {50, 150} <= sides
  ext = sp.prescaled_sizes(g["coco_sobel/sizes"], 0.33)
  assert (ext < 32).any() and (ext > 32).any() and (ext == 32).any()      # the extents straddle input_sz


@pytest.mark.parametrize("name", cases.names())
def test_draw_replays_the_reference_draws(name):
  g = cases.fixture()
  cfg = cases.meta(name)["config"]
  aug = cases.augmenter(name)
  rp = cases.recorded_params(name, aug.S)
  for i, seed in enumerate(g[name + "/seeds"]):
    aug.rng = np.random.RandomState(int(seed))
    p = aug.draw([i])
    if cfg["use_random_scale"]:
      assert p["scale"][0] == g[name + "/scale"][i]
    else:
      assert p["scale"] is None
    assert tuple(p["extent"][0]) == tuple(g[name + "/extent"][i]), (name, i)
    assert tuple(p["coords"][0]) == tuple(g[name + "/coords"][i]), (name, i)
    one = cases.take(rp, [i])
    assert np.array_equal(one["iparams"], p["iparams"]) and one["fparams"].tobytes() == p["fparams"].tobytes()
    if cfg["use_random_affine"]:
      assert np.array_equal(p["affine1_to_2"][0], g[name + "/a12"][i])


def _cfg(**kw):
  c = dict(input_sz=32, no_sobel=True, include_rgb=False, jitter_brightness=0.1, jitter_contrast=0.1,
           jitter_saturation=0.1, jitter_hue=0.1, flip_p=0.5, use_random_affine=False, use_random_scale=False,
           pre_scale_all=True, pre_scale_factor=0.33, scale_min=0.6, scale_max=1.4)
  c.update(kw)
  return types.SimpleNamespace(**c)


def test_draw_from_the_originals_equals_draw_over_the_prescaled_images():
  """Same seed, same config, no random scale: source="original" draws exactly what a resident augmenter over the
  pre-scaled images draws."""
  rs = np.random.RandomState(4)
  shapes = [(50, 72), (61, 150), (150, 61), (97, 97), (100, 142), (185, 121)]
  imgs = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in shapes]
  small = [sp.prescale_host(im, None, 0.33)[0] for im in imgs]
  a = sr.SegRaggedAugmenter(imgs, _cfg(), seed=9, device="cpu", source="original")
  b = sr.SegRaggedAugmenter(small, _cfg(), seed=9, device="cpu")
  idx = [5, 0, 1, 1, 4, 3, 2]
  pa, pb = a.draw(idx), b.draw(idx)
  assert pa.keys() == pb.keys()
  for k in pa:
    assert (pa[k] is None and pb[k] is None) or np.asarray(pa[k]).tobytes() == np.asarray(pb[k]).tobytes(), k
  assert np.array_equal(pa["extent"], sp.prescaled_sizes(shapes, 0.33)[idx])
  # with the random scale the extent is scaled_len of scaled_len, the scale drawn first
  c = sr.SegRaggedAugmenter(imgs, _cfg(use_random_scale=True), seed=9, device="cpu", source="original")
  first = np.random.RandomState(9).rand() * (1.4 - 0.6) + 0.6
  pc = c.draw(idx)
  assert pc["scale"][0] == first
  assert np.array_equal(pc["extent"], sr.scaled_len(sp.prescaled_sizes(shapes, 0.33)[idx], pc["scale"].reshape(-1, 1)))


def test_source_keyword_refusals():
  imgs = [np.zeros((40, 30, 3), np.uint8)]
  R = sr.SegRaggedAugmenter
  with pytest.raises(ValueError, match="source='original' is for pre_scale_all"):
    R(imgs, _cfg(pre_scale_all=False), device="cpu", source="original")
  with pytest.raises(ValueError, match=r"pre_scale_factor.*\(0, 1\)"):
    R(imgs, _cfg(pre_scale_factor=1.0), device="cpu", source="original")
  with pytest.raises(ValueError, match=r"pre_scale_factor.*\(0, 1\)"):
    R(imgs, _cfg(pre_scale_factor=0.0), device="cpu", source="original")
  with pytest.raises(ValueError, match="source: 'both'"):
    R(imgs, _cfg(), device="cpu", source="both")
  # the default keeps today's refusals
  with pytest.raises(NotImplementedError, match="untruncated float image"):
    R(imgs, _cfg(use_random_scale=True), device="cpu")
  with pytest.raises(NotImplementedError, match="pre_scale_all inside the kernel"):
    R(imgs, _cfg(), prescaled=False, device="cpu")
  # Cs 3 and 4, with and without the random scale, are accepted from the originals
  for cs in (3, 4):
    for scale in (False, True):
      aug = R([np.zeros((40, 30, cs), np.uint8)], _cfg(use_random_scale=scale), device="cpu", source="original")
      assert aug.pre_factor == 0.33 and tuple(aug.base_extent[0]) == (13, 10)
      with pytest.raises(AssertionError, match="resident on the GPU"):
        aug.apply(aug.draw([0]))                                          # no CPU path


def test_prescale_dataset_refusals():
  P = sp.prescale_dataset
  imgs = [np.zeros((40, 30, 3), np.uint8), np.zeros((20, 50, 3), np.uint8)]
  labs = [np.zeros((40, 30), np.uint8), np.zeros((20, 50), np.uint8)]
  packed = torch.zeros(100, 3, dtype=torch.uint8)
  for bad in (0.0, 1.0, 1.5, -0.33):
    with pytest.raises(ValueError, match=r"factor: .*must lie within \(0, 1\)"):
      P(imgs, factor=bad, device="cpu")
  with pytest.raises(ValueError, match="factor: required"):
    P(imgs, device="cpu")
  with pytest.raises(ValueError, match="layout: 'planar'"):
    P(imgs, factor=0.33, layout="planar", device="cpu")
  with pytest.raises(ValueError, match=r"Cs = 4 .*source=\"original\""):
    P([np.zeros((8, 8, 4), np.uint8)], factor=0.33, device="cpu")
  with pytest.raises(ValueError, match=r"Cs = 4 .*source=\"original\""):
    P(torch.zeros(64, 4, dtype=torch.uint8), sizes=[[8, 8]], factor=0.33)
  with pytest.raises(TypeError, match=r"images\[1\].*uint8"):
    P([imgs[0], imgs[1].astype(np.int32)], factor=0.33, device="cpu")
  with pytest.raises(ValueError, match=r"images\[0\]: shape .*expected \[h, w, 3\]"):
    P([np.zeros((8, 8), np.uint8)], factor=0.33, device="cpu")
  with pytest.raises(ValueError, match="images: the list is empty"):
    P([], factor=0.33, device="cpu")
  with pytest.raises(ValueError, match="labels: 1 maps for 2 images"):
    P(imgs, labels=labs[:1], factor=0.33, device="cpu")
  with pytest.raises(ValueError, match="sizes / offsets describe an already packed tensor"):
    P(imgs, sizes=[[40, 30], [20, 50]], factor=0.33, device="cpu")
  with pytest.raises(ValueError, match="chunk_px: must be positive"):
    P(imgs, factor=0.33, chunk_px=0, device="cpu")
  with pytest.raises(TypeError, match="images: a list of uint8"):
    P(torch.zeros(100, 3, dtype=torch.float32), sizes=[[10, 10]], factor=0.33)
  with pytest.raises(ValueError, match=r"images: packed shape \[total, 3\]"):
    P(torch.zeros(10, 10, 3, dtype=torch.uint8), sizes=[[10, 10]], factor=0.33)
  with pytest.raises(ValueError, match="sizes: required"):
    P(packed, factor=0.33)
  with pytest.raises(ValueError, match=r"sizes: must be an integer array \[B, 2\]"):
    P(packed, sizes=[10, 10], factor=0.33)
  with pytest.raises(ValueError, match=r"sizes: every h and w must lie within 1\.\.16384"):
    P(packed, sizes=[[0, 10]], factor=0.33)
  with pytest.raises(ValueError, match="offsets: image 1 leaves the packed array of 100 pixels"):
    P(packed, sizes=[[5, 10], [5, 11]], factor=0.33)
  with pytest.raises(ValueError, match="offsets: image 0 leaves"):
    P(packed, sizes=[[5, 10]], offsets=[-1], factor=0.33)
  with pytest.raises(ValueError, match="offsets: images overlap"):
    P(packed, sizes=[[5, 10], [5, 10]], offsets=[0, 49], factor=0.33)
  with pytest.raises(ValueError, match=r"offsets: must be an integer array \[2\]"):
    P(packed, sizes=[[5, 10], [5, 10]], offsets=[0], factor=0.33)
  with pytest.raises(ValueError, match="labels: one byte per pixel"):
    P(packed, sizes=[[10, 10]], labels=torch.zeros(99, dtype=torch.uint8), factor=0.33)
  with pytest.raises(TypeError, match="labels: the packed uint8"):
    P(packed, sizes=[[10, 10]], labels=torch.zeros(100, dtype=torch.int64), factor=0.33)
  with pytest.raises(AssertionError, match="must be on the GPU"):
    P(packed, sizes=[[10, 10]], factor=0.33)                              # no CPU path


def test_work_list_and_chunks_cover_every_row_and_image_once():
  nsz = np.array([[1, 2], [8, 3], [9, 3], [61, 40], [16, 1]])
  w = sp.work_list(nsz)
  assert w.dtype == np.int32 and w.shape[1] == 3
  rows = [set() for _ in nsz]
  for img, first, count in w:
    assert 1 <= count <= sp.ROWS_PER_ITEM
    new = set(range(first, first + count))
    assert not (rows[img] & new)
    rows[img] |= new
  assert [sorted(r) for r in rows] == [list(range(h)) for h in nsz[:, 0]]
  assert sp._chunks([10, 10, 10, 50, 5, 5], 20) == [(0, 2), (2, 3), (3, 4), (4, 6)]
  assert sp._chunks([10, 10], 1000) == [(0, 2)]


def test_exported_from_the_package_and_bound():
  import iic_amd
  from iic_amd import _lib
  assert iic_amd.prescale_dataset is sp.prescale_dataset
  assert "iic_seg_prescale" in _lib.EXPORTED_SYMBOLS and "iic_seg_augment_ragged_prescaled" in _lib.EXPORTED_SYMBOLS
