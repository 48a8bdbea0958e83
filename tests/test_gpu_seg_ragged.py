"""csrc/seg_augment.hip::seg_augment_ragged_kernel through the C ABI (`iic_seg_augment_ragged`, iic_amd/seg_ragged.py):
segmentation training batches from images of different sizes, against
  * the reference-generated fixture tests/golden/seg_augment_ragged.npz (tools/gen_golden_seg_augment_ragged.py: the
    reference's own `_prepare_train` on images of seven sizes, every draw recorded), bit for bit.  The use_random_scale
    cases pin the pixels to the restatement of OpenCV's resize (iic_amd/seg_ragged.py), not to a cv2 binary;
  * the uniform kernel (`iic_seg_augment`, pinned by tests/test_gpu_seg_augment.py) on datasets of one size;
  * itself: a mixed batch against one-image packs, two calls, black samples for indices outside the dataset;
  * one end-to-end training step.
Fixture shapes only (images up to 61 x 40, input_sz 32 / 36 / 48): the whole file runs in a few seconds."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tests import seg_ragged_cases as cases   # noqa: E402

pytestmark = pytest.mark.gpu
WARP_TOL = 2e-5      # tests/test_gpu_seg_loss.py::test_affine_warp_matches_grid_sample's bound for iic_affine_warp_fwd


def dev():
  return torch.device("cuda:0")


def _np(outs):
  return [t.cpu().numpy() for t in outs]


def _same(a, b):
  return all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a, b))


@pytest.mark.parametrize("name", cases.names())
def test_fixture_bit_identical(name):
  """Every fixture case -- one launch over the case's images of different sizes -- against the reference's outputs:
  img1, img2, affine2_to_1, mask_img1, bit for bit.
  With use_random_affine img2 is the kernel's img2 passed through iic_seg_augment_warp, the restatement of
  F.affine_grid + F.grid_sample in the operation order of torch's CPU kernels, which produced the fixture."""
  aug = cases.augmenter(name, device=dev())
  params = cases.recorded_params(name, aug.S)
  img1, img2, aff, mask = _np(aug.apply(params))
  assert mask.dtype == np.uint8 and aff.dtype == np.float32
  n = img1.shape[0]
  want = [cases.expected(name, i) for i in range(n)]
  for i in range(n):
    assert img1[i].shape == want[i][0].shape
    assert img1[i].tobytes() == want[i][0].tobytes(), (name, i, np.abs(img1[i] - want[i][0]).max())
    assert mask[i].tobytes() == want[i][3].tobytes(), (name, i)
    assert aff[i].tobytes() == want[i][2].tobytes(), (name, i, aff[i], want[i][2])
  err = max(float(np.abs(img2[i].astype(np.float64) - want[i][1]).max()) for i in range(n))
  print("%s: %d images, C %d, max |img2 - reference| %.3e" % (name, n, img1.shape[1], err))
  for i in range(n):
    assert img2[i].tobytes() == want[i][1].tobytes(), (name, i, err)


@pytest.mark.parametrize("name", [n for n in cases.names() if cases.meta(n)["config"]["use_random_affine"]])
def test_fixture_affine_img2_before_the_warp_bit_identical(name):
  """What the new kernel itself contributes to img2 in the random-affine cases -- the jittered view before warp and flip
  -- against the tensor the reference's `random_affine` received, bit for bit."""
  plain = cases.augmenter(name, device=dev(), use_random_affine=False)
  params = dict(cases.recorded_params(name, plain.S), affine1_to_2=None)
  params["iparams"][:, 3] = 0                                  # the reference flips after the warp
  img2 = plain.apply(params)[1].cpu().numpy()
  g = cases.fixture()
  for i in range(img2.shape[0]):
    assert img2[i].tobytes() == g["%s/%d/img2_pre" % (name, i)].tobytes(), (name, i)


@pytest.mark.parametrize("S,C", [(36, 4), (48, 5), (128, 1)])
def test_warp_equals_its_host_restatement_and_the_library_warp(S, C):
  """iic_seg_augment_warp at sizes the fixture does not hold (not powers of two among them), flipped and not: the bytes
  of seg_ragged.grid_warp_host -- which the CPU tests hold to the reference's img2 -- and, within that kernel's 2e-5,
  the values of the uniform augmenter's iic_affine_warp_fwd, so that both augmenters warp alike."""
  from iic_amd import _lib, seg_augment as sa, seg_ragged as sr
  rs = np.random.RandomState(S)
  n = 4
  img = (rs.randint(0, 256, (n, C, S, S)) / 255.).astype(np.float32)
  a12 = np.stack([sa.affine_pair(np.radians(rs.uniform(-30, 30)), np.radians(rs.uniform(-10, 10)), rs.uniform(0.8, 1.2))[0]
                  for _ in range(n)])
  flips = np.array([0, 1, 1, 0], np.int32)
  aug = sr.SegRaggedAugmenter([np.zeros((S, S, 3), np.uint8)], _cfg(S=S), device=dev())
  x = torch.from_numpy(img).to(dev())
  got = aug._grid_warp(x, a12, flips).cpu().numpy()
  for i in range(n):
    want = sr.grid_warp_host(img[i], a12[i], bool(flips[i]))
    assert got[i].tobytes() == want.tobytes(), (i, np.abs(got[i] - want).max())
  mats = sa.warp_matrices(a12, flips, S).to(dev())
  old = torch.empty_like(x)
  _lib.check(_lib.lib().iic_affine_warp_fwd(x.data_ptr(), mats.data_ptr(), old.data_ptr(), n, C, S, S, 0, 0,
                                            _lib.stream_ptr()), "iic_affine_warp_fwd")
  assert float(np.abs(old.cpu().numpy() - got).max()) <= WARP_TOL


def _cfg(S=32, no_sobel=True, include_rgb=False, **kw):
  c = dict(input_sz=S, no_sobel=no_sobel, include_rgb=include_rgb, jitter_brightness=0.4, jitter_contrast=0.4,
           jitter_saturation=0.4, jitter_hue=0.125, flip_p=0.5, use_random_affine=False, use_random_scale=False,
           pre_scale_all=False, scale_min=0.6, scale_max=1.4, aff_min_rot=-30., aff_max_rot=30., aff_min_shear=-10.,
           aff_max_shear=10., aff_min_scale=0.8, aff_max_scale=1.2)
  c.update(kw)
  return types.SimpleNamespace(**c)


LAYOUTS = [(True, False), (False, True), (False, False)]      # no_sobel, include_rgb


@pytest.mark.parametrize("h,w", [(24, 41), (41, 53)])
@pytest.mark.parametrize("no_sobel,include_rgb", LAYOUTS)
@pytest.mark.parametrize("cs", [3, 4])
def test_uniform_dataset_gives_the_bytes_of_the_uniform_kernel(cs, no_sobel, include_rgb, h, w):
  """Images of one size through SegRaggedAugmenter, with the draws SegPairedAugmenter made, give what iic_seg_augment
  gives on the stacked array: the new kernel is tied to the one tests/test_gpu_seg_augment.py pins."""
  from iic_amd import seg_augment as sa, seg_ragged as sr
  rng = np.random.default_rng(100 * cs + h)
  B = 5
  imgs = rng.integers(0, 256, (B, h, w, cs), dtype=np.uint8)
  imgs[1, :, :, :3] = imgs[1][:, :, :1]                      # a grey image: hue / saturation degenerate
  labels = rng.integers(0, 183, (B, h, w)).astype(np.uint8)
  labels[labels == 182] = 255
  rel = (np.arange(256) >= 91).astype(np.uint8)
  rel[182:] = 0
  cfg = _cfg(no_sobel=no_sobel, include_rgb=include_rgb)
  uni = sa.SegPairedAugmenter(torch.from_numpy(imgs).to(dev()), cfg, labels_u8=torch.from_numpy(labels).to(dev()),
                              relevance=rel, seed=7)
  rag = sr.SegRaggedAugmenter(list(imgs), cfg, labels=list(labels), relevance=rel, device=dev())
  p = uni.draw([4, 0, 1, 1, 3, 2, 4])
  assert set(p["iparams"][:, 3]) == {0, 1}
  assert _same(_np(uni.apply(p)), _np(rag.apply(dict(p, scale=None))))


def _mixed_images(cs):
  """Every fixture size in one dataset, the 35 x 37 image last."""
  name, name36 = ("coco_sobel_rgb", "coco_sobel_rgb_s36") if cs == 3 else ("potsdam_nosobel", "potsdam_nosobel_s36")
  imgs, labels, rel = cases.images(name)
  imgs36, labels36, _ = cases.images(name36)
  imgs = imgs + imgs36[:1]
  labels = None if labels is None else labels + labels36[:1]
  assert [im.shape[:2] for im in imgs] == [(20, 24), (20, 50), (50, 20), (32, 32), (33, 47), (61, 40), (35, 37)]
  return imgs, labels, rel


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("cs", [3, 4])
def test_mixed_batch_with_repeats_equals_the_per_sample_results(cs, scale):
  """All the fixture sizes in one launch, indices repeated and out of order, the last image of the pack among them:
  every sample equals what a pack holding only its image (offset 0) gives -- a wrong row pitch or pixel offset shows."""
  from iic_amd import seg_ragged as sr
  imgs, labels, rel = _mixed_images(cs)
  cfg = _cfg(no_sobel=False, include_rgb=True, use_random_scale=scale)
  aug = sr.SegRaggedAugmenter(imgs, cfg, labels=labels, relevance=rel, seed=3, device=dev())
  assert aug.total == sum(im.shape[0] * im.shape[1] for im in imgs) and int(aug.offsets[-1]) + 35 * 37 == aug.total
  idx = [6, 0, 3, 3, 5, 1, 6, 2, 4, 0, 6]
  p = aug.draw(idx)
  got = _np(aug.apply(p))
  assert got[0].shape == (len(idx), aug.out_channels, 32, 32)
  assert _same(got, _np(aug.apply(p)))                         # determinism: no atomics on this path
  for k, src in enumerate(idx):
    one = sr.SegRaggedAugmenter([imgs[src]], cfg, labels=None if labels is None else [labels[src]], relevance=rel,
                                device=dev())
    pk = cases.take(p, [k])
    pk["iparams"][:, 0] = 0
    want = _np(one.apply(pk))
    for a, b in zip(got, want):
      assert a[k].tobytes() == b[0].tobytes(), (k, src)


def test_two_calls_give_identical_bytes():
  for name in ("coco_sobel_rgb", "potsdam_nosobel_scale", "coco_sobel_scale_affine"):
    aug = cases.augmenter(name, device=dev())
    params = cases.recorded_params(name, aug.S)
    assert _same(_np(aug.apply(params)), _np(aug.apply(params)))


def _launch(aug, ip, fp, taps=None, sizes=None):
  """iic_seg_augment_ragged directly: parameters the host API refuses."""
  from iic_amd import _lib
  n, S, C = ip.shape[0], aug.S, aug.out_channels
  d = aug.images.device
  ipd, fpd = torch.from_numpy(ip).to(d), torch.from_numpy(fp).to(d)
  sizes = aug.sizes if sizes is None else torch.from_numpy(sizes).to(d)
  outs = (torch.full((n, C, S, S), 7., device=d), torch.full((n, C, S, S), 7., device=d),
          torch.full((n, 2, 3), 7., device=d), torch.full((n, S, S), 7, device=d, dtype=torch.uint8))
  _lib.check(_lib.lib().iic_seg_augment_ragged(
    aug.images.data_ptr(), aug.offsets.data_ptr(), sizes.data_ptr(), aug.B, aug.total, aug.Cs, _lib.ptr(aug.labels),
    _lib.ptr(aug.relevance), ipd.data_ptr(), fpd.data_ptr(), _lib.ptr(taps), n, S, int(aug.no_sobel),
    int(aug.include_rgb), aug.lut.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[3].data_ptr(),
    outs[2].data_ptr(), _lib.stream_ptr()), "iic_seg_augment_ragged")
  torch.cuda.synchronize()
  return _np((outs[0], outs[1], outs[2], outs[3]))


def test_index_outside_the_dataset_reads_as_a_black_image():
  """Built directly in iparams (draw and apply refuse one): a black sample, fine label 0 everywhere, no fault; so does an
  image whose recorded extent would leave the pack.  The neighbouring valid samples are untouched."""
  from iic_amd import seg_ragged as sr
  imgs, labels, _ = _mixed_images(3)
  rel = np.zeros(256, np.uint8)
  rel[0] = 1                                                   # label 0 (the padding's) is relevant, nothing else
  labels = [np.maximum(l, 1) for l in labels]
  cfg = _cfg(no_sobel=False, include_rgb=True)
  aug = sr.SegRaggedAugmenter(imgs, cfg, labels=labels, relevance=rel, seed=5, device=dev())
  p = aug.draw([5, 6, 6, 2, 6])
  ip, fp = p["iparams"].copy(), p["fparams"]
  ip[1, 0], ip[3, 0] = aug.B, -1
  got = _launch(aug, ip, fp)
  valid = _np(aug.apply(cases.take(p, [0, 2, 4])))
  for a, b in zip(got, valid):
    assert a[[0, 2, 4]].tobytes() == b.tobytes()
  for k in (1, 3):
    assert not got[0][k].any() and (got[3][k] == 1).all()
    assert got[2][k].tobytes() == _np(aug.apply(cases.take(p, [k])))[2][0].tobytes()     # affine2_to_1 is still written
  # img2 of a black sample: the jitter of a black image, whatever the ops
  black = sr.SegRaggedAugmenter([np.zeros((40, 40, 3), np.uint8)], cfg, labels=[np.zeros((40, 40), np.uint8)],
                                relevance=rel, device=dev())
  pb = cases.take(p, [1])
  pb["iparams"][:, :3] = 0
  assert got[1][1].tobytes() == _np(black.apply(pb))[1][0].tobytes()
  # the last image claims more rows than the pack holds: black, not a read past the end
  sizes = aug.sizes_host.astype(np.int32)
  sizes[6, 0] += 1
  got = _launch(aug, p["iparams"], fp, sizes=sizes)
  assert not got[0][[1, 2, 4]].any() and (got[3][[1, 2, 4]] == 1).all()
  assert got[0][[0, 3]].tobytes() == _np(aug.apply(cases.take(p, [0, 3])))[0].tobytes()


@pytest.mark.parametrize("name", ["coco_sobel_rgb_scale", "potsdam_nosobel_scale", "coco_sobel_scale_affine"])
def test_scale_one_equals_the_unscaled_path(name):
  """scale_min = scale_max = 1.0: the tables are the identity (weights 1 and 0), and the resampling kernel gives the
  bytes of the plain one for the same remaining draws."""
  scaled = cases.augmenter(name, device=dev(), scale_min=1.0, scale_max=1.0)
  plain = cases.augmenter(name, device=dev(), use_random_scale=False)
  scaled.rng = np.random.RandomState(17)
  p = scaled.draw([3, 0, 2, 1, 0])
  assert (p["scale"] == 1.0).all() and np.array_equal(p["extent"], scaled.sizes_host[[3, 0, 2, 1, 0]])
  assert _same(_np(scaled.apply(p)), _np(plain.apply(dict(p, scale=None))))


@pytest.mark.parametrize("kind", ["potsdam", "coco", "coco_scale"])
def test_end_to_end_step(kind):
  """ragged paired_batch -> sobel_process where configured -> SegmentationNet10aTwoHead -> uncollapsed loss -> backward,
  as tests/test_gpu_seg_augment.py::test_end_to_end_step does for the uniform augmenter."""
  from iic_amd import archs, seg_losses, seg_ragged as sr
  from iic_amd.transforms import sobel_process
  torch.manual_seed(0)
  S, n = 48, 6
  rng = np.random.default_rng(3)
  shapes = [(56, 56), (40, 70), (48, 48), (61, 45), (30, 33), (50, 60), (49, 90), (64, 47)]
  cs = 4 if kind == "potsdam" else 3
  imgs = [rng.integers(0, 256, s + (cs,), dtype=np.uint8) for s in shapes]
  if kind == "potsdam":
    no_sobel, in_ch, labels, rel = True, 4, None, None
  else:
    no_sobel, in_ch = False, 5
    labels = [rng.integers(60, 182, s).astype(np.uint8) for s in shapes]
    rel = (np.arange(256) >= 91).astype(np.uint8)
  cfg = _cfg(S=S, no_sobel=no_sobel, include_rgb=True, use_random_scale=(kind == "coco_scale"))
  aug = sr.SegRaggedAugmenter(imgs, cfg, labels=labels, relevance=rel, seed=11, device=dev())
  img1, img2, aff, mask = aug.paired_batch(np.arange(n))
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
