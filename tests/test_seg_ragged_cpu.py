"""Host logic of iic_amd/seg_ragged.py (SegRaggedAugmenter: segmentation batches from images of different sizes) against
the reference-generated fixture tests/golden/seg_augment_ragged.npz (tools/gen_golden_seg_augment_ragged.py: the
reference's own `_prepare_train` on images of different sizes, every random draw recorded).  No GPU: draws, per-image
crop arithmetic, packing, the resampling tables the kernel reads, refusals, and the shuffled dataloader list."""
import numpy as np
import pytest
import torch

from iic_amd import seg_augment as sa
from iic_amd import seg_ragged as sr
from tests import seg_ragged_cases as cases


def test_draw_replays_the_reference_draws_case_by_case():
  """Seeded like numpy's global generator was for the fixture, `draw` makes the reference's draws in the reference's
  order on every image's own extent: [scale,] crop centre, jitter, [random_affine,] flip."""
  g = cases.fixture()
  checked = 0
  for name in cases.names():
    cfg = cases.meta(name)["config"]
    aug = cases.augmenter(name)
    for i, seed in enumerate(g[name + "/seeds"]):
      aug.rng = np.random.RandomState(int(seed))
      p = aug.draw([i])
      key = (name, i)
      if cfg["use_random_scale"]:
        assert p["scale"][0] == g[name + "/scale"][i], key
      else:
        assert p["scale"] is None
      assert tuple(p["extent"][0]) == tuple(g[name + "/extent"][i]), key        # the (scaled) image the crop is drawn on
      assert tuple(p["coords"][0]) == tuple(g[name + "/coords"][i]), key
      half = int(aug.S / 2.)
      assert (p["iparams"][0, 2], p["iparams"][0, 1]) == tuple(g[name + "/coords"][i] - half)
      nj = int(g[name + "/jit_n"][i])
      assert p["iparams"][0, 4] == nj
      assert list(p["iparams"][0, 5:5 + nj]) == list(g[name + "/jit_ops"][i][:nj])
      f = g[name + "/jit_f"][i]
      assert np.array_equal(p["fparams"][0, :4], f.astype(np.float32))
      assert p["hue"][0] == f[3] and p["iparams"][0, 9] == int(f[3] * 255) % 256
      flip = g[name + "/rands"][i][-1] > cfg["flip_p"]
      assert bool(p["iparams"][0, 3]) == bool(flip)
      if cfg["use_random_affine"]:
        assert np.array_equal(p["affine1_to_2"][0], g[name + "/a12"][i])
      else:
        assert p["affine1_to_2"] is None
      a21 = p["fparams"][0, 4:10].reshape(2, 3).copy()
      if flip:
        a21[0, :] *= np.float32(-1.)
      assert a21.tobytes() == g[name + "/aff"][i].tobytes(), key
      # and the recorded-parameter dictionary the GPU tests replay is the same one
      rp = cases.take(cases.recorded_params(name, aug.S), [i])
      assert np.array_equal(rp["iparams"], p["iparams"]) and rp["fparams"].tobytes() == p["fparams"].tobytes()
      checked += 1
  assert checked == 48


def _host_views(aug, imgs, labels, rel, params):
  """img1 and mask_img1 as the kernel computes them, in numpy, from the SAME inputs the kernel gets: the crop origin and
  the image's own extent, or (use_random_scale) the tap tables of crop_taps."""
  S = aug.S
  ip, scale = params["iparams"], params["scale"]
  out = []
  for k in range(ip.shape[0]):
    src = int(ip[k, 0])
    img = imgs[src]
    h, w, cs = img.shape
    if scale is None:
      new_h, new_w, oy, ox = sa.pad_offsets(h, w, S)
      pad = np.zeros((new_h, new_w, cs), np.uint8)
      pad[oy:oy + h, ox:ox + w] = img
      crop = pad[ip[k, 2]:ip[k, 2] + S, ip[k, 1]:ip[k, 1] + S]
      lab = None
      if labels is not None:
        lpad = np.zeros((new_h, new_w), np.uint8)
        lpad[oy:oy + h, ox:ox + w] = labels[src]
        lab = lpad[ip[k, 2]:ip[k, 2] + S, ip[k, 1]:ip[k, 1] + S]
    else:
      ty = sr.crop_taps([h], [scale[k]], [ip[k, 2]], S)[0]
      tx = sr.crop_taps([w], [scale[k]], [ip[k, 1]], S)[0]
      v = img.astype(np.float32)
      top = v[ty["i0"]][:, tx["i0"]] * tx["a0"][None, :, None] + v[ty["i0"]][:, tx["i1"]] * tx["a1"][None, :, None]
      bot = v[ty["i1"]][:, tx["i0"]] * tx["a0"][None, :, None] + v[ty["i1"]][:, tx["i1"]] * tx["a1"][None, :, None]
      val = top * ty["a0"][:, None, None] + bot * ty["a1"][:, None, None]
      assert val.dtype == np.float32
      inside = (ty["inside"][:, None] & tx["inside"][None, :]).astype(bool)
      crop = np.where(inside[:, :, None], val.astype(np.uint8), np.uint8(0))
      lab = None
      if labels is not None:
        lab = np.where(inside, labels[src][ty["nearest"]][:, tx["nearest"]], np.uint8(0))
    v = crop[:, :, :3]
    if not aug.no_sobel:
      grey = sa.cv_grey(v)[:, :, None]
      v = np.concatenate([v, grey], axis=2) if aug.include_rgb else grey
    v = v.astype(np.float32) / 255.
    if cs == 4:                  # IR is never truncated (potsdam.py:148-151, :170): after a resize it is not an integer
      ir = crop[:, :, 3].astype(np.float32) if scale is None else np.where(inside, val[:, :, 3], np.float32(0))
      v = np.concatenate([v, (ir / np.float32(255.))[:, :, None]], axis=2)
    mask = np.ones((S, S), np.uint8) if lab is None else np.asarray(rel, np.uint8)[lab]
    out.append((np.ascontiguousarray(v.transpose(2, 0, 1)), mask))
  return out


@pytest.mark.parametrize("name", cases.names())
def test_crop_and_tables_reproduce_the_reference_img1_and_mask(name):
  """What the host hands the kernel -- per-image pad offsets and crop origins, or the resampling tables -- selects
  exactly the pixels and labels the reference cut: img1 and mask_img1 of every fixture sample, bit for bit."""
  aug = cases.augmenter(name)
  imgs, labels, rel = cases.images(name)
  params = cases.recorded_params(name, aug.S)
  for i, (img1, mask) in enumerate(_host_views(aug, imgs, labels, rel, params)):
    want = cases.expected(name, i)
    assert img1.shape == want[0].shape
    assert img1.tobytes() == want[0].tobytes(), (name, i, np.abs(img1 - want[0]).max() * 255)
    assert mask.tobytes() == want[3].tobytes(), (name, i)


def test_grid_warp_restatement_reproduces_the_reference_img2():
  """random_affine + flip of the reference, from the tensor it received (img2_pre) to the img2 it returned: the host
  restatement of iic_seg_augment_warp's arithmetic is bit-identical on every random-affine sample of the fixture."""
  g = cases.fixture()
  seen = 0
  for name in cases.names():
    cfg = cases.meta(name)["config"]
    if not cfg["use_random_affine"]:
      continue
    for i in range(len(g[name + "/seeds"])):
      flip = bool(g[name + "/rands"][i][-1] > cfg["flip_p"])
      got = sr.grid_warp_host(g["%s/%d/img2_pre" % (name, i)], g[name + "/a12"][i], flip)
      want = cases.expected(name, i)[1]
      assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (name, i, np.abs(got - want).max())
      seen += 1
  assert seen == 8


def test_fixture_covers_the_sizes_layouts_flips_and_flags():
  g = cases.fixture()
  sizes32 = {(20, 24), (20, 50), (50, 20), (32, 32), (33, 47), (61, 40)}
  layouts, affine, scaled = {}, 0, 0
  for name in cases.names():
    m = cases.meta(name)
    cfg = m["config"]
    flips = set(bool(v) for v in (g[name + "/rands"][:, -1] > cfg["flip_p"]))
    assert flips == {True, False}, name
    affine += cfg["use_random_affine"]
    scaled += cfg["use_random_scale"]
    if not cfg["use_random_affine"] and not cfg["use_random_scale"]:
      key = (m["kind"] == "potsdam", cfg["no_sobel"], cfg["include_rgb"], cfg["input_sz"])
      layouts[key] = set(map(tuple, g[name + "/sizes"]))
    if cfg["use_random_scale"]:
      assert (cfg["scale_min"], cfg["scale_max"], cfg["pre_scale_all"]) == (0.6, 1.4, False)
      assert (g[name + "/extent"] != g[name + "/sizes"]).any()
  for coco_layout in ((True, False), (False, True), (False, False)):
    assert layouts[(False,) + coco_layout + (32,)] == sizes32
    assert layouts[(False,) + coco_layout + (36,)] == {(35, 37)}
  assert layouts[(True, True, False, 32)] == sizes32 and layouts[(True, True, False, 36)] == {(35, 37)}
  assert affine >= 1 and scaled >= 2


def test_packing_round_trips():
  rs = np.random.RandomState(0)
  shapes = [(5, 7), (1, 1), (16, 3), (9, 9)]
  for cs in (3, 4):
    imgs = [rs.randint(0, 256, s + (cs,)).astype(np.uint8) for s in shapes]
    labs = [rs.randint(0, 256, s).astype(np.uint8) for s in shapes]
    pixels, packed_labels, sizes, offsets = sr.pack_images(imgs, labs)
    assert pixels.shape == (sum(h * w for h, w in shapes), cs) and pixels.dtype == np.uint8
    assert sizes.dtype == np.int32 and offsets.dtype == np.int64
    assert list(offsets) == [0, 35, 36, 84] and [tuple(s) for s in sizes] == shapes
    back, back_labs = sr.unpack_images(pixels, sizes, offsets, packed_labels)
    assert all(np.array_equal(a, b) for a, b in zip(imgs, back))
    assert all(np.array_equal(a, b) for a, b in zip(labs, back_labs))
    # the augmenter holds the same pack, from a list or from the packed tensors
    rel = np.ones(256, np.uint8)
    a = sr.SegRaggedAugmenter(imgs, _cfg(), labels=labs, relevance=rel, device="cpu")
    b = sr.SegRaggedAugmenter(torch.from_numpy(pixels), _cfg(), labels=torch.from_numpy(packed_labels), relevance=rel,
                              sizes=sizes, offsets=offsets)
    c = sr.SegRaggedAugmenter(torch.from_numpy(pixels), _cfg(), sizes=sizes)          # offsets default: back to back
    for aug in (a, b, c):
      assert aug.B == 4 and aug.Cs == cs and aug.total == pixels.shape[0]
      assert np.array_equal(aug.images.numpy(), pixels)
      assert np.array_equal(aug.offsets.numpy(), offsets) and aug.offsets.dtype == torch.int64
      assert np.array_equal(aug.sizes.numpy(), sizes) and aug.sizes.dtype == torch.int32
    assert np.array_equal(a.labels.numpy(), packed_labels) and c.labels is None


def _cfg(**kw):
  c = dict(input_sz=32, no_sobel=True, include_rgb=False, jitter_brightness=0.1, jitter_contrast=0.1,
           jitter_saturation=0.1, jitter_hue=0.1, flip_p=0.5, use_random_affine=False, use_random_scale=False,
           pre_scale_all=False, scale_min=0.6, scale_max=1.4)
  c.update(kw)
  import types
  return types.SimpleNamespace(**c)


def test_every_validation_refuses_with_its_message():
  imgs = [np.zeros((40, 30, 3), np.uint8), np.zeros((20, 50, 3), np.uint8)]
  labs = [np.zeros((40, 30), np.uint8), np.zeros((20, 50), np.uint8)]
  rel = np.ones(256, np.uint8)
  R = sr.SegRaggedAugmenter
  with pytest.raises(TypeError, match=r"images\[1\].*uint8"):
    R([imgs[0], imgs[1].astype(np.int32)], _cfg(), device="cpu")
  with pytest.raises(TypeError, match=r"labels\[0\].*uint8"):
    R(imgs, _cfg(), labels=[labs[0].astype(np.int32), labs[1]], relevance=rel, device="cpu")
  with pytest.raises(ValueError, match=r"labels\[1\].*shape"):
    R(imgs, _cfg(), labels=[labs[0], labs[0]], relevance=rel, device="cpu")
  with pytest.raises(ValueError, match="Cs must be 3"):
    R([np.zeros((8, 8, 2), np.uint8)], _cfg(), device="cpu")
  with pytest.raises(ValueError, match="Cs must be 3"):
    R(torch.zeros(64, 5, dtype=torch.uint8), _cfg(), sizes=[[8, 8]])
  with pytest.raises(ValueError, match="one Cs for the whole list"):
    R([imgs[0], np.zeros((8, 8, 4), np.uint8)], _cfg(), device="cpu")
  with pytest.raises(TypeError, match="images"):
    R(torch.zeros(64, 3, dtype=torch.float32), _cfg(), sizes=[[8, 8]])
  packed = torch.zeros(100, 3, dtype=torch.uint8)
  with pytest.raises(ValueError, match="sizes: required"):
    R(packed, _cfg())
  with pytest.raises(ValueError, match=r"sizes: must be an integer array \[B, 2\]"):
    R(packed, _cfg(), sizes=[10, 10])
  with pytest.raises(ValueError, match="sizes: must be an integer array"):
    R(packed, _cfg(), sizes=np.array([[10., 10.]]))
  with pytest.raises(ValueError, match=r"sizes: every h and w must lie within 1\.\.16384"):
    R(packed, _cfg(), sizes=[[0, 10]])
  with pytest.raises(ValueError, match=r"sizes: every h and w must lie within 1\.\.16384"):
    R(packed, _cfg(), sizes=[[1, 16385]])
  with pytest.raises(ValueError, match="offsets: image 1 leaves the packed array of 100 pixels"):
    R(packed, _cfg(), sizes=[[5, 10], [5, 11]])                         # 50 + 55 > 100: sizes against the total length
  with pytest.raises(ValueError, match="offsets: image 0 leaves"):
    R(packed, _cfg(), sizes=[[5, 10]], offsets=[-1])
  with pytest.raises(ValueError, match="offsets: images overlap"):
    R(packed, _cfg(), sizes=[[5, 10], [5, 10]], offsets=[0, 49])
  with pytest.raises(ValueError, match=r"offsets: must be an integer array \[2\]"):
    R(packed, _cfg(), sizes=[[5, 10], [5, 10]], offsets=[0])
  R(packed, _cfg(), sizes=[[5, 10], [5, 10]], offsets=[50, 0])          # any order, gaps allowed
  with pytest.raises(ValueError, match="labels and relevance go together"):
    R(imgs, _cfg(), labels=labs, device="cpu")
  with pytest.raises(ValueError, match="labels and relevance go together"):
    R(imgs, _cfg(), relevance=rel, device="cpu")
  with pytest.raises(ValueError, match="labels: one byte per pixel"):
    R(packed, _cfg(), sizes=[[10, 10]], labels=torch.zeros(99, dtype=torch.uint8), relevance=rel)
  with pytest.raises(TypeError, match="labels: the packed uint8"):
    R(packed, _cfg(), sizes=[[10, 10]], labels=torch.zeros(100, dtype=torch.int64), relevance=rel)
  with pytest.raises(ValueError, match="relevance: the 256-entry table"):
    R(imgs, _cfg(), labels=labs, relevance=np.ones(10, np.uint8), device="cpu")
  with pytest.raises(NotImplementedError, match="input_sz must be a multiple of 4"):
    R(imgs, _cfg(input_sz=30), device="cpu")
  with pytest.raises(AssertionError, match="mask_input"):
    R(imgs, _cfg(mask_input=True), device="cpu")
  with pytest.raises(NotImplementedError, match="pre_scale_all inside the kernel"):
    R(imgs, _cfg(pre_scale_all=True), prescaled=False, device="cpu")
  R(imgs, _cfg(pre_scale_all=True), device="cpu")                       # the resident images are the pre-scaled ones
  with pytest.raises(ValueError, match="scale_min / scale_max"):
    R(imgs, _cfg(use_random_scale=True, scale_min=1.5, scale_max=1.0), device="cpu")
  aug = R(imgs, _cfg(), device="cpu")
  with pytest.raises(AssertionError, match="source index out of range"):
    aug.draw([2])
  p = aug.draw([0, 1])
  with pytest.raises(AssertionError, match="resident on the GPU"):
    aug.apply(p)                                                        # no CPU path
  bad = dict(p, iparams=p["iparams"].copy())
  bad["iparams"][1, 2] = 1                                              # image 1 is 20 high: padded to 32, origin 0 only
  with pytest.raises(AssertionError, match="crop outside"):
    aug.apply(bad)
  bad["iparams"][:, 0] = (0, 2)
  with pytest.raises(AssertionError, match="source index out of range"):
    aug.apply(bad)


def test_pre_scale_all_with_random_scale_names_both_flags_and_the_reason():
  imgs = [np.zeros((40, 30, 3), np.uint8)]
  with pytest.raises(NotImplementedError) as e:
    sr.SegRaggedAugmenter(imgs, _cfg(pre_scale_all=True, use_random_scale=True), device="cpu")
  msg = str(e.value)
  assert "pre_scale_all" in msg and "use_random_scale" in msg and "untruncated float image" in msg
  # and the uniform augmenter keeps refusing the flag altogether
  with pytest.raises(NotImplementedError, match="use_random_scale"):
    sa.SegPairedAugmenter(torch.zeros(2, 40, 40, 3, dtype=torch.uint8), _cfg(use_random_scale=True))


def test_resize_at_scale_one_is_the_identity():
  rs = np.random.RandomState(1)
  for shape in ((33, 47, 3), (1, 1, 4), (20, 24), (2, 61, 3)):
    img = rs.randint(0, 256, shape).astype(np.float32)
    out = sr.resize_linear_host(img, 1.0)
    assert out.dtype == np.float32 and out.tobytes() == img.tobytes()
    lab = rs.randint(-1, 182, shape[:2]).astype(np.int32)
    assert np.array_equal(sr.resize_nearest_host(lab, 1.0), lab)
  t = sr.crop_taps([20, 47], [1.0, 1.0], [0, 9], 32)
  assert np.array_equal(t["i0"][1], np.arange(9, 41)) and (t["a0"] == 1).all() and (t["a1"] == 0).all()
  assert list(t["inside"][0]) == [0] * 6 + [1] * 20 + [0] * 6           # 20 centred in 32: offset 16 - 10
  assert np.array_equal(t["nearest"][1], np.arange(9, 41)) and t["inside"][1].all()


def _bilinear_f64(img, scale):
  """cv2's INTER_LINEAR sampling positions, (d + 0.5) / scale - 0.5 clamped to the image, evaluated in float64."""
  h, w = img.shape[:2]
  nh, nw = int(sr.scaled_len(h, scale)), int(sr.scaled_len(w, scale))
  y = np.clip((np.arange(nh) + 0.5) / scale - 0.5, 0, h - 1)
  x = np.clip((np.arange(nw) + 0.5) / scale - 0.5, 0, w - 1)
  y0, x0 = np.minimum(np.floor(y).astype(int), h - 1), np.minimum(np.floor(x).astype(int), w - 1)
  y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
  fy, fx = (y - y0)[:, None, None], (x - x0)[None, :, None]
  v = img.astype(np.float64).reshape(h, w, -1)
  return ((v[y0][:, x0] * (1 - fx) + v[y0][:, x1] * fx) * (1 - fy) + (v[y1][:, x0] * (1 - fx) + v[y1][:, x1] * fx) * fy)


@pytest.mark.parametrize("scale", [0.6, 0.7310585786, 1.0, 1.25, 1.4])
def test_resize_matches_a_float64_bilinear_evaluation(scale):
  rs = np.random.RandomState(2)
  img = rs.randint(0, 256, (33, 47, 3)).astype(np.float32)
  got = sr.resize_linear_host(img, scale)
  want = _bilinear_f64(img, scale)
  assert got.shape == want.shape == (int(round(33 * scale)), int(round(47 * scale)), 3)
  err = float(np.abs(got.astype(np.float64) - want).max())
  print("scale %.4f: max |float32 restatement - float64 bilinear| = %.3e grey levels" % (scale, err))
  assert err <= 0.5
  assert got.min() >= 0 and got.max() <= 255
  lab = rs.randint(-1, 182, (33, 47)).astype(np.int32)
  near = sr.resize_nearest_host(lab, scale)
  ys = np.minimum(np.floor(np.arange(near.shape[0]) / scale).astype(int), 32)
  xs = np.minimum(np.floor(np.arange(near.shape[1]) / scale).astype(int), 46)
  assert near.shape == got.shape[:2] and np.array_equal(near, lab[ys][:, xs])


def test_scaled_len_rounds_half_to_even_and_stays_positive():
  assert [int(sr.scaled_len(n, 0.5)) for n in (1, 3, 5, 7, 200)] == [1, 2, 2, 4, 100]       # 0.5 -> 0 -> 1; 1.5 -> 2; 2.5 -> 2
  assert int(sr.scaled_len(1, 0.1)) == 1


def _stub_apply(aug, calls):
  def stub(params):
    calls.append(params)
    n = params["iparams"].shape[0]
    return torch.zeros(n, 3, 32, 32), torch.zeros(n, 3, 32, 32), torch.zeros(n, 2, 3), torch.ones(n, 32, 32)
  aug.apply = stub


def _ragged(n=11, seed=0):
  rs = np.random.RandomState(5)
  imgs = [np.zeros((int(h), int(w), 3), np.uint8) for h, w in rs.randint(20, 60, (n, 2))]
  return sr.SegRaggedAugmenter(imgs, _cfg(), seed=seed, device="cpu")


def test_shuffle_false_keeps_the_sequential_order():
  aug, calls = _ragged(), []
  _stub_apply(aug, calls)
  loaders = sa.seg_paired_dataloaders(aug, 4, 2)
  assert [len(d) for d in loaders] == [3, 3]
  for _ in range(2):                                                    # two epochs, the same order
    del calls[:]
    shapes = [tup[0][0].shape[0] for tup in zip(*loaders)]
    assert shapes == [4, 4, 3]
    order = [list(c["iparams"][:, 0]) for c in calls]
    assert order == [[0, 1, 2, 3]] * 2 + [[4, 5, 6, 7]] * 2 + [[8, 9, 10]] * 2


def test_shuffle_visits_every_sample_once_in_the_same_order_for_every_loader():
  aug, calls = _ragged(), []
  _stub_apply(aug, calls)
  loaders = sa.seg_paired_dataloaders(aug, 4, 3, shuffle=True)
  epochs = []
  for _ in range(3):
    del calls[:]
    assert [tup[0][0].shape[0] for tup in zip(*loaders)] == [4, 4, 3]
    per_loader = [np.concatenate([c["iparams"][:, 0] for c in calls[k::3]]) for k in range(3)]
    assert sorted(per_loader[0]) == list(range(11))                     # every sample once per epoch
    assert all(np.array_equal(per_loader[0], p) for p in per_loader[1:])    # one order for the whole list
    epochs.append(tuple(per_loader[0]))
  assert len(set(epochs)) == 3 and epochs[0] != tuple(range(11))        # a fresh permutation every epoch
  again = sa.seg_paired_dataloaders(_ragged(), 4, 1, shuffle=True)[0]
  assert tuple(again.order.permutation(0)) == epochs[0]                 # reproducible from shuffle_seed


def test_shuffle_leaves_the_augmentation_draws_of_a_seed_unchanged():
  """The permutation comes from a generator of its own: the k-th draw of the augmenter's generator is the same with and
  without shuffling (on equal-sized images, where the draws do not depend on which sample is drawn)."""
  imgs = [np.zeros((40, 50, 3), np.uint8)] * 9
  draws = {}
  for shuffle in (False, True):
    aug, calls = sr.SegRaggedAugmenter(imgs, _cfg(use_random_scale=True), seed=123, device="cpu"), []
    _stub_apply(aug, calls)
    for _ in zip(*sa.seg_paired_dataloaders(aug, 4, 2, shuffle=shuffle)):
      pass
    draws[shuffle] = calls
  assert len(draws[False]) == len(draws[True]) == 6
  assert any(not np.array_equal(a["iparams"][:, 0], b["iparams"][:, 0]) for a, b in zip(draws[False], draws[True]))
  for a, b in zip(draws[False], draws[True]):
    assert np.array_equal(a["iparams"][:, 1:], b["iparams"][:, 1:]) and a["fparams"].tobytes() == b["fparams"].tobytes()
    assert np.array_equal(a["scale"], b["scale"]) and np.array_equal(a["coords"], b["coords"])


def test_exported_from_the_package_and_bound():
  import iic_amd
  from iic_amd import _lib
  assert iic_amd.SegRaggedAugmenter is sr.SegRaggedAugmenter
  assert "iic_seg_augment_ragged" in _lib.EXPORTED_SYMBOLS
  assert sr.TAP_DTYPE.itemsize == 24                                    # iic_seg_resample_tap
