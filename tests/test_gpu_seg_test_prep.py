"""csrc/seg_augment.hip::seg_prepare_test_kernel through the C ABI (iic_seg_prepare_test, iic_amd/seg_augment.py
SegTestPreparer / seg_mapping_dataloader) against
  * the reference-generated fixture tests/golden/seg_test_prep.npz (tools/gen_golden_seg_test_prep.py: the reference's
    own `_prepare_test` of the Potsdam and COCO-Stuff datasets) -- imgs, targets and mask bit-identical, every case,
    size, sample and pixel, once with each size as its own uniform resident array and once with all sizes of a case
    packed top-left into one 48 x 48 slab array with `sizes`;
  * the numpy restatement `prepare_test_host` (tests/test_seg_test_prep_cpu.py holds it to the same fixture) over a
    sweep of source sizes around input_sz and at the two real batch shapes, bit-identical;
  * seg_eval.segmentation_eval fed by the device loader and by host-prepared batches: equal statistics, equal counts,
    and no copy of the loader's uint8 tensors on the way into the count kernel.
Grey (no_sobel=False) is OpenCV 3.x's fixed-point RGB2GRAY restated from its source on every side -- cv2 itself is
not available; see iic_amd/seg_augment.py."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden", "seg_test_prep.npz")
MODES = {"nosobel": (True, False), "sobel_rgb": (False, True), "sobel": (False, False)}


def dev():
  return torch.device("cuda:0")


def _cfg(S, no_sobel, include_rgb, **kw):
  c = dict(input_sz=S, no_sobel=no_sobel, include_rgb=include_rgb, pre_scale_all=False, mask_input=False)
  c.update(kw)
  return types.SimpleNamespace(**c)


def _u8_labels(lab_i16):
  return (lab_i16.astype(np.int64) % 256).astype(np.uint8)         # -1 -> 255, the resident form


def _names():
  return [str(n) for n in np.load(G)["names"]]


def _case(g, name):
  meta = json.loads(str(g[name + "/meta"]))
  rel = g[name + "/relevance"] if meta["kind"] != "potsdam" else None
  cfg = _cfg(**{k: meta["config"][k] for k in ("no_sobel", "include_rgb")}, S=meta["config"]["input_sz"])
  return meta, cfg, g[name + "/targets_table"], rel


def _pack(images, labels, H, W, fill):
  """Images of different sizes top-left in [H][W] slabs; the rest of every slab holds `fill`, which no output may
  show.  Returns (slab images, slab labels, sizes)."""
  B, cs = len(images), images[0].shape[2]
  im = np.full((B, H, W, cs), fill, np.uint8)
  lb = np.full((B, H, W), fill, np.uint8)
  sizes = np.zeros((B, 2), np.int32)
  for i, (a, l) in enumerate(zip(images, labels)):
    h, w = l.shape
    im[i, :h, :w], lb[i, :h, :w], sizes[i] = a, l, (h, w)
  return im, lb, sizes


def _run(images, labels, cfg, ttab, rel, sizes=None, idx=None):
  from iic_amd import seg_augment as sa
  prep = sa.SegTestPreparer(torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev()), cfg, ttab,
                            relevance=rel, sizes=sizes)
  out = prep.batch(np.arange(images.shape[0]) if idx is None else idx)
  assert out[0].dtype == torch.float32 and out[1].dtype == torch.uint8 and out[2].dtype == torch.uint8
  assert all(t.is_cuda and t.is_contiguous() for t in out)
  return prep, [t.cpu().numpy() for t in out]


def _assert_fixture(g, keys_rows, got, name):
  """got: the three outputs over the samples listed in keys_rows [(fixture key, sample)], in that order."""
  for j, (key, i) in enumerate(keys_rows):
    want = g[key + "/imgs"][i]
    assert got[0][j].shape == want.shape, (key, got[0][j].shape, want.shape)
    assert got[0][j].tobytes() == want.tobytes(), (key, i, float(np.abs(got[0][j] - want).max()))
    assert np.array_equal(got[1][j], g[key + "/targets"][i].astype(np.uint8)), (key, i)
    assert np.array_equal(got[2][j], g[key + "/mask"][i]), (key, i)


@pytest.mark.parametrize("name", _names())
def test_fixture_bit_identical_uniform_arrays(name):
  g = np.load(G)
  meta, cfg, ttab, rel = _case(g, name)
  n = 0
  for h, w in g["sizes"]:
    key = "%s/%dx%d" % (name, h, w)
    prep, got = _run(g[key + "/images"], _u8_labels(g[key + "/labels"]), cfg, ttab, rel)
    _assert_fixture(g, [(key, i) for i in range(got[0].shape[0])], got, name)
    again = [t.cpu().numpy() for t in prep.batch(np.arange(got[0].shape[0]))]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))        # no atomics: identical bytes
    n += got[0].shape[0]
  assert n == 2 * len(g["sizes"])                                    # every size and sample, nothing skipped


@pytest.mark.parametrize("name", _names())
def test_fixture_bit_identical_packed_slabs_with_sizes(name):
  """All sizes of a case -- the two non-square sources included -- in one 48 x 48 slab array: the per-image extent
  path.  The slabs are filled with 173 outside the images (a stuff class, a bright pixel): nothing of it may show."""
  g = np.load(G)
  meta, cfg, ttab, rel = _case(g, name)
  rows = [("%s/%dx%d" % (name, h, w), i) for h, w in g["sizes"] for i in range(2)]
  assert {(24, 48), (48, 24)} <= {tuple(s) for s in g["sizes"]}
  im, lb, sizes = _pack([g[k + "/images"][i] for k, i in rows], [_u8_labels(g[k + "/labels"][i]) for k, i in rows],
                        48, 48, 173)
  order = np.random.default_rng(3).permutation(len(rows))           # idx is not the identity
  prep, got = _run(im, lb, cfg, ttab, rel, sizes=sizes, idx=order)
  _assert_fixture(g, [rows[j] for j in order], got, name)
  assert got[0].shape[0] == len(rows) == 12


def _random_tables(rng):
  ttab = rng.integers(0, 256, 256).astype(np.uint8)
  rel = rng.integers(0, 2, 256).astype(np.uint8)
  return ttab, rel


def _random_labels(rng, shape):
  lab = rng.integers(0, 183, shape).astype(np.uint8)
  lab[lab == 182] = 255                                              # unlabelled
  return lab


def _host(images, labels, cfg, ttab, rel):
  from iic_amd import seg_augment as sa
  res = [sa.prepare_test_host(a, l, cfg.input_sz, cfg.no_sobel, cfg.include_rgb, ttab, rel)
         for a, l in zip(images, labels)]
  return [np.stack([r[k] for r in res]) for k in range(3)]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("cs", [3, 4])
@pytest.mark.parametrize("S", [8, 32])
def test_geometry_sweep_against_the_restatement(S, cs, mode):
  """Every (h, w) with h, w in {1, S - 1, S, S + 1, 2 S + 3}: each side padded to the limit, padded by one, exact,
  cropped by one (odd) and cropped by more than a full window -- both parities of int(h / 2.) on either side of S.
  Each size once as its own uniform array and all 25 once in one slab array with `sizes`."""
  no_sobel, include_rgb = MODES[mode]
  cfg = _cfg(S, no_sobel, include_rgb)
  rng = np.random.default_rng(1000 * S + 10 * cs + len(mode))
  ttab, rel = _random_tables(rng)
  rel = rel if cs == 3 else None                                     # Cs 4 as Potsdam: mask of ones
  ext = (1, S - 1, S, S + 1, 2 * S + 3)
  images, labels = [], []
  for h in ext:
    for w in ext:
      a, l = rng.integers(0, 256, (2, h, w, cs), dtype=np.uint8), _random_labels(rng, (2, h, w))
      _, got = _run(a, l, cfg, ttab, rel)
      want = _host(a, l, cfg, ttab, rel)
      for k in range(3):
        assert got[k].tobytes() == want[k].tobytes(), ("uniform", h, w, k)
      images.append(a[0])
      labels.append(l[0])
  im, lb, sizes = _pack(images, labels, 2 * S + 3, 2 * S + 3, 201)
  _, got = _run(im, lb, cfg, ttab, rel, sizes=sizes)
  want = _host(images, labels, cfg, ttab, rel)
  bad = [(i, k) for i in range(len(images)) for k in range(3) if got[k][i].tobytes() != want[k][i].tobytes()]
  assert not bad, ("packed", [tuple(sizes[i]) for i, _ in bad[:6]], bad[:6])
  if rel is None:
    assert bool((got[2] == 1).all())


def real_case(name):
  """Random content at a published evaluation shape; returns (preparer, host images, host labels, sizes, tables, cfg,
  batch size).  potsdam: 100 images of 200 x 200 x 4, S 200, no_sobel, batches of 75; coco: 150 images with (h, w)
  drawn between 96 and 160 in 160 x 160 slabs, S 128, sobel + include_rgb, label masks, batches of 120."""
  from iic_amd import seg_augment as sa
  rng = np.random.default_rng(77)
  if name == "potsdam":
    B, H, W, cs, S, batch, cfg = 100, 200, 200, 4, 200, 75, _cfg(200, True, False)
    sizes = None
    ttab = np.zeros(256, np.uint8)
    ttab[:6] = [0, 1, 2, 2, 0, 1]
    rel = None
    labels = rng.integers(0, 6, (B, H, W)).astype(np.uint8)
  else:
    B, H, W, cs, S, batch, cfg = 150, 160, 160, 3, 128, 120, _cfg(128, False, True, pre_scale_all=True)
    sizes = rng.integers(96, 161, (B, 2)).astype(np.int32)
    sizes[0], sizes[1], sizes[2] = (96, 160), (160, 96), (128, 128)
    rel = ((np.arange(256) >= 91) & (np.arange(256) < 182)).astype(np.uint8)
    ttab = ((np.arange(256) % 15) * rel + 255 * (1 - rel)).astype(np.uint8)
    labels = _random_labels(rng, (B, H, W))
  images = rng.integers(0, 256, (B, H, W, cs), dtype=np.uint8)
  images[3], images[4] = 255, 0
  prep = sa.SegTestPreparer(torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev()), cfg, ttab,
                            relevance=rel, sizes=sizes)
  return prep, images, labels, sizes, ttab, rel, cfg, batch


@pytest.mark.parametrize("name", ["potsdam", "coco"])
def test_real_batch_shape_bit_identical_to_restatement(name):
  from iic_amd import seg_augment as sa
  prep, images, labels, sizes, ttab, rel, cfg, batch = real_case(name)
  loader = sa.seg_mapping_dataloader(prep, batch)
  B = images.shape[0]
  assert len(loader) == 2 and B % batch != 0
  lo, bad = 0, []
  for imgs, targets, mask in loader:                                 # a full batch, then the ragged last one
    n = imgs.shape[0]
    assert n == min(batch, B - lo) and tuple(imgs.shape) == (n, prep.out_channels, prep.S, prep.S)
    assert tuple(targets.shape) == tuple(mask.shape) == (n, prep.S, prep.S)
    got = [t.cpu().numpy() for t in (imgs, targets, mask)]
    again = [t.cpu().numpy() for t in prep.batch(np.arange(lo, lo + n))]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))        # two calls: identical bytes
    for j in range(n):
      i = lo + j
      h, w = (images.shape[1:3] if sizes is None else sizes[i])
      want = sa.prepare_test_host(images[i, :h, :w], labels[i, :h, :w], cfg.input_sz, cfg.no_sobel, cfg.include_rgb,
                                  ttab, rel)
      bad += [(i, k) for k in range(3) if got[k][j].tobytes() != want[k].tobytes()]
    lo += n
  assert lo == B and not bad, bad[:8]


def test_c_abi_refuses_what_the_kernel_cannot_serve():
  """iic_seg_prepare_test returns an error code and launches nothing: S % 4, a channel count it has no kernel for,
  missing arrays."""
  from iic_amd._lib import lib, stream_ptr
  z = torch.zeros(4096, dtype=torch.uint8, device=dev())
  f = torch.zeros(4096, dtype=torch.float32, device=dev())
  i = torch.zeros(4, dtype=torch.int32, device=dev())
  p = z.data_ptr()

  def call(S=8, cs=3, labels=p, ttab=p, n=1):
    return lib().iic_seg_prepare_test(p, 1, 8, 8, cs, labels, None, ttab, None, i.data_ptr(), n, S, 1, 0, f.data_ptr(),
                                      f.data_ptr(), p, p, stream_ptr())
  assert call(S=6) == -3 and call(cs=2) == -3 and call(n=65536) == -3
  assert call(labels=None) == -1 and call(ttab=None) == -1 and call(n=0) == -1


def _stats_equal(a, b):
  assert set(a) == set(b)
  for k in a:
    if k == "best_train_sub_head_match":
      assert a[k] == b[k]
    else:
      assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (k, a[k], b[k])


def test_segmentation_eval_fed_by_the_device_loader(monkeypatch):
  """segmentation_eval over seg_mapping_dataloader == over host-prepared batches (prepare_test_host per image, stacked,
  as the reference's DataLoader collates them): equal dicts, integer-equal count matrices; and the loader's targets
  and mask reach iic_seg_contingency_acc as they are -- uint8, contiguous, the same device pointers."""
  from iic_amd import archs, seg_augment as sa, seg_eval
  S, B, gt_k, k = 32, 10, 3, 6
  rng = np.random.default_rng(12)
  sizes = rng.integers(20, 49, (B, 2)).astype(np.int32)
  sizes[0], sizes[1] = (24, 48), (48, 24)
  images = rng.integers(0, 256, (B, 48, 48, 4), dtype=np.uint8)
  labels = _random_labels(rng, (B, 48, 48))
  rel = ((np.arange(256) >= 91) & (np.arange(256) < 182)).astype(np.uint8)
  ttab = ((np.arange(256) % gt_k) * rel + 255 * (1 - rel)).astype(np.uint8)
  cfg = _cfg(S, True, False)
  prep = sa.SegTestPreparer(torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev()), cfg, ttab,
                            relevance=rel, sizes=sizes)
  torch.manual_seed(4)
  ncfg = types.SimpleNamespace(in_channels=4, input_sz=S, batchnorm_track=True, num_sub_heads=2, output_k=k)
  net = archs.SegmentationNet10a(ncfg).to(dev()).train()
  config = types.SimpleNamespace(in_channels=4, input_sz=S, num_sub_heads=2, output_k=k, gt_k=gt_k, batch_sz=4,
                                 eval_mode="orig", mode="IID+", include_rgb=False, mapping_assignment_partitions=["a"],
                                 mapping_test_partitions=["b"], epoch_stats=[], epoch_acc=[], epoch_avg_subhead_acc=[])

  def host_loader(batch_sz):
    out = []
    for lo in range(0, B, batch_sz):
      res = [sa.prepare_test_host(images[i, :sizes[i, 0], :sizes[i, 1]], labels[i, :sizes[i, 0], :sizes[i, 1]], S, True,
                                  False, ttab, rel) for i in range(lo, min(B, lo + batch_sz))]
      out.append(tuple(torch.from_numpy(np.stack([r[j] for r in res])) for j in range(3)))
    return out

  dev_assign, dev_test = sa.seg_mapping_dataloader(prep, 4), sa.seg_mapping_dataloader(prep, 3)
  assert len(dev_assign) == 3 and len(dev_test) == 4
  want = seg_eval.segmentation_eval(config, net, host_loader(4), host_loader(3), sobel=False, return_only=True)

  yielded, seen = [], []
  orig_batch, orig_u8, orig_add = prep.batch, seg_eval._u8, seg_eval.SegEvalAccumulator.add

  def batch(idx):
    out = orig_batch(idx)
    yielded.append((out[1].data_ptr(), out[2].data_ptr()))
    return out

  def add(self, label_maps, flat_targets, mask=None):
    seen.append(("add", flat_targets.dtype, flat_targets.is_contiguous(), flat_targets.data_ptr(), mask.dtype,
                 mask.is_contiguous(), mask.data_ptr()))
    return orig_add(self, label_maps, flat_targets, mask)

  def u8(t, device, is_mask=False):
    out = orig_u8(t, device, is_mask=is_mask)
    seen.append(("u8", t.data_ptr(), out.data_ptr()))
    return out
  prep.batch = batch
  monkeypatch.setattr(seg_eval.SegEvalAccumulator, "add", add)
  monkeypatch.setattr(seg_eval, "_u8", u8)
  got = seg_eval.segmentation_eval(config, net, dev_assign, dev_test, sobel=False, return_only=True)
  monkeypatch.undo()
  prep.batch = orig_batch
  _stats_equal(got, want)
  adds = [s for s in seen if s[0] == "add"]
  assert len(adds) == len(yielded) == 7
  for (tp, mp), a in zip(yielded, adds):
    assert a[1] == torch.uint8 and a[2] and a[4] == torch.uint8 and a[5]
    assert (a[3], a[6]) == (tp, mp)                                  # what the loader yielded, not a copy of it
  u8s = [s for s in seen if s[0] == "u8"]
  assert len(u8s) == 14 and all(s[1] == s[2] for s in u8s)           # _u8 returned a view of its argument
  assert sorted(s[1] for s in u8s) == sorted(p for pair in yielded for p in pair)

  # the count matrices themselves, integer-equal
  net.eval()
  for dl, hl in ((dev_assign, host_loader(4)), (dev_test, host_loader(3))):
    c_dev, n_dev = seg_eval._stream_counts(config, net, dl, False, False)
    c_host, n_host = seg_eval._stream_counts(config, net, hl, False, False)
    assert c_dev.dtype == np.int64 and np.array_equal(c_dev, c_host) and n_dev == n_host
    assert n_dev == sum(int(b[2].sum()) for b in hl) > 0              # the selected pixels: the host masks' ones
  net.train()
