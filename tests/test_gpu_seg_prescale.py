"""pre_scale_all on the device: csrc/seg_prescale.hip (`iic_seg_prescale`, iic_amd/seg_prescale.py) and the two-stage
instantiation of seg_augment_ragged_kernel (`iic_seg_augment_ragged_prescaled`, SegRaggedAugmenter(source="original")),
against
  * seg_prescale.prescale_host and the host pipeline of tests/seg_prescale_cases.py (which tests/test_seg_prescale_cpu.py
    holds to the fixture), byte for byte;
  * the reference-generated fixture tests/golden/seg_prescale.npz (tools/gen_golden_seg_prescale.py), bit for bit;
  * each other: the augmenter over the originals against the resident augmenter over prescale_dataset's output.
No tolerance anywhere.  Fixture-sized shapes only: the whole file runs in a few seconds."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tests import seg_prescale_cases as cases   # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(1, 5), (3, 2), (2, 2), (33, 47), (61, 150), (185, 121)]
FACTORS = [0.33, 0.5, 0.9]
LAYOUTS = [(True, False), (False, True), (False, False)]      # no_sobel, include_rgb


def dev():
  return torch.device("cuda:0")


_SOURCES = {}


def sources():
  """The six source images and label maps (255 among the labels), made once."""
  if not _SOURCES:
    rs = np.random.RandomState(11)
    _SOURCES["imgs"] = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in SHAPES]
    labs = [rs.randint(0, 183, s).astype(np.uint8) for s in SHAPES]
    for l in labs:
      l[l == 182] = 255
    _SOURCES["labs"] = labs
    _SOURCES["host"] = {}
  return _SOURCES["imgs"], _SOURCES["labs"]


def host(factor):
  """prescale_host of every source at `factor`, computed once per factor."""
  from iic_amd import seg_prescale as sp
  imgs, labs = sources()
  if factor not in _SOURCES["host"]:
    _SOURCES["host"][factor] = [sp.prescale_host(im, l, factor) for im, l in zip(imgs, labs)]
  return _SOURCES["host"][factor]


def _unpack(pixels, labels, sizes, offsets):
  from iic_amd import seg_ragged as sr
  return sr.unpack_images(pixels.cpu().numpy(), sizes.numpy(), offsets.numpy(), None if labels is None else labels.cpu().numpy())


def test_small_sources_become_the_expected_extents():
  from iic_amd import seg_prescale as sp
  assert [tuple(v) for v in sp.prescaled_sizes(SHAPES[:2], 0.33)] == [(1, 2), (1, 1)]


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("factor", FACTORS)
def test_prescale_equals_the_host_restatement_in_both_layouts(factor, with_labels):
  """iic_seg_prescale over a pack of six images -- 1 x 5 and 3 x 2 among them -- against prescale_host, byte for byte;
  packed and slab layout from the same sources; a second call gives identical bytes."""
  from iic_amd import seg_prescale as sp, seg_ragged as sr
  imgs, labs = sources()
  px, lab, sizes, offsets = sr.pack_images(imgs, labs)
  dpx = torch.from_numpy(px).to(dev())
  dlab = torch.from_numpy(lab).to(dev()) if with_labels else None
  out, olab, nsz, noff = sp.prescale_dataset(dpx, sizes=sizes, labels=dlab, factor=factor)
  assert out.dtype == torch.uint8 and out.dim() == 2 and out.shape[1] == 3 and nsz.dtype == torch.int32
  assert np.array_equal(nsz.numpy(), sp.prescaled_sizes(SHAPES, factor)) and noff.dtype == torch.int64
  assert int(noff[-1]) + int(nsz[-1, 0]) * int(nsz[-1, 1]) == out.shape[0]
  assert (olab is None) == (not with_labels)
  got, got_lab = _unpack(out, olab, nsz, noff)
  want = host(factor)
  for i in range(len(imgs)):
    assert got[i].shape == want[i][0].shape
    assert got[i].tobytes() == want[i][0].tobytes(), (factor, SHAPES[i], int((got[i] != want[i][0]).sum()))
    if with_labels:
      assert got_lab[i].tobytes() == want[i][1].tobytes(), (factor, SHAPES[i])
  again = sp.prescale_dataset(dpx, sizes=sizes, labels=dlab, factor=factor)
  assert again[0].cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
  # the slab: every image in the top-left corner of its slab, zeros elsewhere
  slab, slab_lab, ssz = sp.prescale_dataset(dpx, sizes=sizes, labels=dlab, factor=factor, layout="slab")
  assert tuple(slab.shape) == (len(imgs), int(nsz[:, 0].max()), int(nsz[:, 1].max()), 3) and np.array_equal(ssz, nsz)
  s, sl = slab.cpu().numpy(), (slab_lab.cpu().numpy() if with_labels else None)
  for i, (h, w) in enumerate(nsz.numpy()):
    assert s[i, :h, :w].tobytes() == got[i].tobytes(), (factor, i)
    rest = s[i].copy()
    rest[:h, :w] = 0
    assert not rest.any()
    if with_labels:
      assert sl[i, :h, :w].tobytes() == got_lab[i].tobytes()
      rest = sl[i].copy()
      rest[:h, :w] = 0
      assert not rest.any()


def test_source_offsets_with_gaps_and_any_order():
  from iic_amd import seg_prescale as sp
  imgs, labs = sources()
  order = [3, 0, 5, 1, 4, 2]
  area = [im.shape[0] * im.shape[1] for im in imgs]
  offsets, pos = np.zeros(len(imgs), np.int64), 5
  for i in order:
    offsets[i] = pos
    pos += area[i] + 7 + i
  px = np.full((pos, 3), 201, np.uint8)
  lab = np.full(pos, 77, np.uint8)
  for i, im in enumerate(imgs):
    px[offsets[i]:offsets[i] + area[i]] = im.reshape(-1, 3)
    lab[offsets[i]:offsets[i] + area[i]] = labs[i].reshape(-1)
  out, olab, nsz, noff = sp.prescale_dataset(torch.from_numpy(px).to(dev()), sizes=SHAPES, offsets=offsets,
                                             labels=torch.from_numpy(lab).to(dev()), factor=0.33)
  got, got_lab = _unpack(out, olab, nsz, noff)
  for i, (wi, wl) in enumerate(host(0.33)):
    assert got[i].tobytes() == wi.tobytes() and got_lab[i].tobytes() == wl.tobytes(), i


@pytest.mark.parametrize("factor", [0.33, 0.9, 0.001])
def test_rows_wider_than_the_staging_buffer_are_done_in_column_chunks(factor):
  """The kernel stages at most 2048 source pixels of a row in LDS: wider rows take the column-chunk loop (at 0.33 from
  693 output columns on, at 0.9 from 1840; at 0.001 a chunk is two output columns).  Few rows, so the images stay small."""
  from iic_amd import seg_prescale as sp
  rs = np.random.RandomState(7)
  shapes = [(3, 2100), (2, 4100), (5, 2049)]
  imgs = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in shapes]
  labs = [rs.randint(0, 256, s).astype(np.uint8) for s in shapes]
  assert int(sp.prescaled_sizes(shapes, 0.33)[0, 1]) == 693 and int(sp.prescaled_sizes(shapes, 0.9)[2, 1]) == 1844
  got, got_lab = _unpack(*sp.prescale_dataset(imgs, labels=labs, factor=factor, device=dev()))
  for i in range(len(imgs)):
    wi, wl = sp.prescale_host(imgs[i], labs[i], factor)
    assert got[i].shape == wi.shape and got[i].tobytes() == wi.tobytes(), (factor, shapes[i])
    assert got_lab[i].tobytes() == wl.tobytes(), (factor, shapes[i])


def _raw(src, lab, sizes, offsets, total_px, factor, dst_ptr, dst_lab_ptr, doff, pitch, nsz, out_px):
  """iic_seg_prescale directly: tables and extents the host API would refuse."""
  from iic_amd import _lib, seg_prescale as sp
  d = src.device
  up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(d)      # noqa: E731
  work = sp.work_list(np.maximum(np.asarray(nsz), 1))
  t = (up(offsets, np.int64), up(sizes, np.int32), up(doff, np.int64), up(pitch, np.int32), up(nsz, np.int32),
       up(work, np.int32))
  _lib.check(_lib.lib().iic_seg_prescale(
    src.data_ptr(), None if lab is None else lab.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), len(sizes), int(total_px),
    float(factor), dst_ptr, dst_lab_ptr, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), int(out_px), t[5].data_ptr(),
    int(work.shape[0]), _lib.stream_ptr()), "iic_seg_prescale")
  torch.cuda.synchronize()


def test_nothing_is_written_outside_the_destination():
  """The ABI called directly on a destination with 64 sentinel bytes on either side, pixels and labels."""
  from iic_amd import seg_prescale as sp, seg_ragged as sr
  imgs, labs = sources()
  px, lab, sizes, offsets = sr.pack_images(imgs, labs)
  nsz = sp.prescaled_sizes(SHAPES, 0.33)
  area = nsz[:, 0] * nsz[:, 1]
  doff = np.concatenate([[0], np.cumsum(area)[:-1]])
  out_px = int(area.sum())
  buf = torch.full((out_px * 3 + 128,), 0xA5, dtype=torch.uint8, device=dev())
  lbuf = torch.full((out_px + 128,), 0x5A, dtype=torch.uint8, device=dev())
  _raw(torch.from_numpy(px).to(dev()), torch.from_numpy(lab).to(dev()), sizes, offsets, px.shape[0], 0.33,
       buf.data_ptr() + 64, lbuf.data_ptr() + 64, doff, nsz[:, 1], nsz, out_px)
  b, lb = buf.cpu().numpy(), lbuf.cpu().numpy()
  assert (b[:64] == 0xA5).all() and (b[-64:] == 0xA5).all() and (lb[:64] == 0x5A).all() and (lb[-64:] == 0x5A).all()
  want = host(0.33)
  assert b[64:-64].tobytes() == b"".join(w[0].tobytes() for w in want)
  assert lb[64:-64].tobytes() == b"".join(w[1].tobytes() for w in want)


def test_list_input_in_three_chunks_equals_one_chunk():
  from iic_amd import seg_prescale as sp
  imgs, labs = sources()
  area = np.array([im.shape[0] * im.shape[1] for im in imgs])
  chunk_px = int(area[-2])                                     # the four small ones; 61 x 150; 185 x 121 (larger: alone)
  assert len(sp._chunks(area, chunk_px)) == 3
  one = sp.prescale_dataset(imgs, labels=labs, factor=0.5, device=dev())
  three = sp.prescale_dataset(imgs, labels=labs, factor=0.5, chunk_px=chunk_px, device=dev())
  for a, b in zip(one, three):
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
  got, got_lab = _unpack(*three)
  for i, (wi, wl) in enumerate(host(0.5)):
    assert got[i].tobytes() == wi.tobytes() and got_lab[i].tobytes() == wl.tobytes(), i
  slab1 = sp.prescale_dataset(imgs, labels=labs, factor=0.5, layout="slab", device=dev())
  slab3 = sp.prescale_dataset(imgs, labels=labs, factor=0.5, layout="slab", chunk_px=chunk_px, device=dev())
  for a, b in zip(slab1, slab3):
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_an_image_whose_extent_leaves_its_pack_is_skipped():
  """Source side: the last image claims one more row than the pack holds.  Destination side: an image whose rows would
  end past out_px.  Neither is written at all (the destination keeps its fill value); the others are.  Both allocations
  are larger than the extents the kernel is told, so even a wrong kernel would stay inside them."""
  from iic_amd import seg_prescale as sp, seg_ragged as sr
  imgs, labs = sources()
  px, lab, sizes, offsets = sr.pack_images(imgs, labs)
  total = px.shape[0]
  slack = 2 * 121
  dpx = torch.from_numpy(np.concatenate([px, np.zeros((slack, 3), np.uint8)])).to(dev())
  dlab = torch.from_numpy(np.concatenate([lab, np.zeros(slack, np.uint8)])).to(dev())
  nsz = sp.prescaled_sizes(SHAPES, 0.33)
  area = nsz[:, 0] * nsz[:, 1]
  doff = np.concatenate([[0], np.cumsum(area)[:-1]])
  out_px = int(area.sum())
  want = host(0.33)

  def run(sizes_told, nsz_told, out_px_told):
    buf = torch.full(((out_px + 4096) * 3,), 9, dtype=torch.uint8, device=dev())
    lbuf = torch.full((out_px + 4096,), 9, dtype=torch.uint8, device=dev())
    _raw(dpx, dlab, sizes_told, offsets, total, 0.33, buf.data_ptr(), lbuf.data_ptr(), doff, nsz_told[:, 1], nsz_told,
         out_px_told)
    return buf.cpu().numpy(), lbuf.cpu().numpy()

  def check(b, lb, skipped):
    for i in range(len(imgs)):
      lo, hi = int(doff[i]), int(doff[i] + area[i])
      if i in skipped:
        assert (b[lo * 3:hi * 3] == 9).all() and (lb[lo:hi] == 9).all(), i
      else:
        assert b[lo * 3:hi * 3].tobytes() == want[i][0].tobytes() and lb[lo:hi].tobytes() == want[i][1].tobytes(), i
    assert (b[out_px * 3:] == 9).all() and (lb[out_px:] == 9).all()
  bad = sizes.copy()
  bad[5, 0] += 1                                               # 186 rows of 121: one row past total_px
  check(*run(bad, nsz, out_px), skipped={5})
  check(*run(sizes, nsz, out_px - 1), skipped={5})             # the last destination image ends one pixel past out_px
  tall = nsz.copy()
  tall[4, 0] = 20000                                           # an extent outside 1..16384
  check(*run(sizes, tall, out_px), skipped={4})


@pytest.mark.parametrize("name", cases.names())
def test_fixture_bit_identical_from_the_originals(name):
  """Every fixture case: SegRaggedAugmenter over the ORIGINAL images with source="original" and the recorded draws
  against the reference's img1, img2, affine2_to_1 and mask_img1, bit for bit.  With use_random_affine img2 goes through
  iic_seg_augment_warp, as in tests/test_gpu_seg_ragged.py."""
  aug = cases.augmenter(name, device=dev())
  params = cases.recorded_params(name, aug.S)
  img1, img2, aff, mask = [t.cpu().numpy() for t in aug.apply(params)]
  assert mask.dtype == np.uint8 and aff.dtype == np.float32
  for i in range(img1.shape[0]):
    want = cases.expected(name, i)
    assert img1[i].shape == want[0].shape
    assert img1[i].tobytes() == want[0].tobytes(), (name, i, np.abs(img1[i] - want[0]).max() * 255)
    assert img2[i].tobytes() == want[1].tobytes(), (name, i, np.abs(img2[i] - want[1]).max() * 255)
    assert aff[i].tobytes() == want[2].tobytes(), (name, i)
    assert mask[i].tobytes() == want[3].tobytes(), (name, i)
  again = [t.cpu().numpy() for t in aug.apply(params)]
  assert all(a.tobytes() == b.tobytes() for a, b in zip((img1, img2, aff, mask), again))


@pytest.mark.parametrize("name", ["coco_sobel", "coco_sobel_rgb"])
def test_originals_equal_the_resident_augmenter_over_the_prescaled_pack(name):
  """The tie between the two halves, Cs = 3, no random scale: source="original" gives the bytes of the resident augmenter
  over prescale_dataset's output for the same draws."""
  from iic_amd import seg_prescale as sp, seg_ragged as sr
  imgs, labels, rel = cases.images(name)
  cfg = cases.config(name)
  orig = cases.augmenter(name, device=dev())
  px, lab, nsz, noff = sp.prescale_dataset(imgs, labels=labels, factor=cfg.pre_scale_factor, device=dev())
  res = sr.SegRaggedAugmenter(px, cfg, labels=lab, relevance=rel, sizes=nsz, offsets=noff, seed=21)
  orig.rng = np.random.RandomState(21)
  idx = [2, 0, 1, 1, 2, 0, 2] if len(imgs) == 3 else [5, 0, 3, 3, 1, 4, 2, 5]
  p, q = orig.draw(idx), res.draw(idx)
  assert np.array_equal(p["iparams"], q["iparams"]) and p["fparams"].tobytes() == q["fparams"].tobytes()
  assert set(p["iparams"][:, 3]) == {0, 1}
  for a, b in zip(orig.apply(p), res.apply(q)):
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _cfg(S, no_sobel, include_rgb, **kw):
  c = dict(input_sz=S, no_sobel=no_sobel, include_rgb=include_rgb, jitter_brightness=0.4, jitter_contrast=0.4,
           jitter_saturation=0.4, jitter_hue=0.125, flip_p=0.5, use_random_affine=False, use_random_scale=True,
           pre_scale_all=True, pre_scale_factor=0.33, scale_min=0.6, scale_max=1.4)
  c.update(kw)
  return types.SimpleNamespace(**c)


def _big_sources(cs):
  rs = np.random.RandomState(50 + cs)
  shapes = [(97, 130), (150, 61), (185, 121), (61, 150), (50, 72)]
  imgs = [rs.randint(0, 256, s + (cs,)).astype(np.uint8) for s in shapes]
  if cs == 4:
    return imgs, None, None
  labels = [rs.randint(0, 183, s).astype(np.uint8) for s in shapes]
  for l in labels:
    l[l == 182] = 255
  rel = (np.arange(256) >= 91).astype(np.uint8)
  rel[182:] = 0
  return imgs, labels, rel


@pytest.mark.parametrize("no_sobel,include_rgb", LAYOUTS)
@pytest.mark.parametrize("cs", [3, 4])
@pytest.mark.parametrize("S", [36, 48])
def test_two_stage_kernel_equals_the_host_pipeline(S, cs, no_sobel, include_rgb):
  """iic_seg_augment_ragged_prescaled at input sizes the fixture lacks, scales 0.6, 1.0 and 1.4, every channel layout,
  with and without IR: the four tensors of the host pipeline (two resizes of the float image, crop, truncate), byte
  for byte."""
  from iic_amd import seg_ragged as sr
  imgs, labels, rel = _big_sources(cs)
  cfg = _cfg(S, no_sobel, include_rgb)
  aug = sr.SegRaggedAugmenter(imgs, cfg, labels=labels, relevance=rel, seed=S + cs, device=dev(), source="original")
  for scale in (0.6, 1.0, 1.4):
    aug.scale_min = aug.scale_max = scale
    p = aug.draw([4, 0, 2, 1, 3, 0])
    assert (p["scale"] == scale).all()
    got = [t.cpu().numpy() for t in aug.apply(p)]
    want = cases.host_pipeline(imgs, labels, rel, cfg, p, 0.33)
    for k, w in enumerate(want):
      for j, what in enumerate(("img1", "img2", "affine2_to_1", "mask")):
        assert got[j][k].shape == w[j].shape and got[j][k].dtype == w[j].dtype
        assert got[j][k].tobytes() == w[j].tobytes(), (S, cs, scale, k, what)


def test_two_stage_index_outside_the_dataset_reads_as_a_black_image():
  """Built directly in iparams (draw and apply refuse one): a black sample with the mask of fine label 0, no fault; the
  valid samples beside it are untouched."""
  from iic_amd import _lib, seg_ragged as sr
  imgs, labels, _ = _big_sources(3)
  rel = np.zeros(256, np.uint8)
  rel[0] = 1                                                   # only label 0 (the padding's) is relevant
  labels = [np.maximum(l, 1) for l in labels]
  cfg = _cfg(36, False, True)
  aug = sr.SegRaggedAugmenter(imgs, cfg, labels=labels, relevance=rel, seed=2, device=dev(), source="original")
  p = aug.draw([0, 1, 2, 3])
  valid = [t.cpu().numpy() for t in aug.apply(p)]
  ip = p["iparams"].copy()
  ip[1, 0], ip[3, 0] = aug.B, -1
  n, S, C, d = 4, aug.S, aug.out_channels, dev()
  src = aug.sizes_host[p["iparams"][:, 0]]
  t = np.stack([sr.crop_taps2(src[:, 0], 0.33, p["scale"], ip[:, 2], S), sr.crop_taps2(src[:, 1], 0.33, p["scale"], ip[:, 1], S)], 1)
  taps2 = torch.from_numpy(np.ascontiguousarray(t).view(np.int32).reshape(n, 2, S, 12)).to(d)
  ipd, fpd = torch.from_numpy(ip).to(d), torch.from_numpy(p["fparams"]).to(d)
  outs = (torch.full((n, C, S, S), 7., device=d), torch.full((n, C, S, S), 7., device=d),
          torch.full((n, S, S), 7, device=d, dtype=torch.uint8), torch.full((n, 2, 3), 7., device=d))
  _lib.check(_lib.lib().iic_seg_augment_ragged_prescaled(
    aug.images.data_ptr(), aug.offsets.data_ptr(), aug.sizes.data_ptr(), aug.B, aug.total, aug.Cs, aug.labels.data_ptr(),
    aug.relevance.data_ptr(), ipd.data_ptr(), fpd.data_ptr(), taps2.data_ptr(), n, S, int(aug.no_sobel),
    int(aug.include_rgb), aug.lut.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
    outs[3].data_ptr(), _lib.stream_ptr()), "iic_seg_augment_ragged_prescaled")
  torch.cuda.synchronize()
  img1, img2, mask, aff = [o.cpu().numpy() for o in outs]
  for k in (0, 2):
    assert img1[k].tobytes() == valid[0][k].tobytes() and img2[k].tobytes() == valid[1][k].tobytes()
    assert mask[k].tobytes() == valid[3][k].tobytes()
  for k in (1, 3):
    assert not img1[k].any() and (mask[k] == 1).all()
    assert aff[k].tobytes() == valid[2][k].tobytes()           # affine2_to_1 is still written


def test_test_preparer_over_the_slab_output():
  """SegTestPreparer(slab, sizes') against prepare_test_host over prescale_host's outputs."""
  from iic_amd import seg_augment as sa, seg_prescale as sp
  imgs, labs = sources()
  slab, slab_lab, nsz = sp.prescale_dataset(imgs, labels=labs, factor=0.33, layout="slab", device=dev())
  targets = (np.arange(256) % 27).astype(np.uint8)
  rel = (np.arange(256) >= 91).astype(np.uint8)
  rel[182:] = 0
  cfg = types.SimpleNamespace(input_sz=32, no_sobel=False, include_rgb=True, pre_scale_all=True, pre_scale_factor=0.33)
  prep = sa.SegTestPreparer(slab, slab_lab, cfg, targets, relevance=rel, sizes=nsz)
  got = [t.cpu().numpy() for t in prep.batch(np.arange(len(imgs)))]
  for i, (wi, wl) in enumerate(host(0.33)):
    want = sa.prepare_test_host(wi, wl, 32, False, True, targets, rel)
    for j in range(3):
      assert got[j][i].tobytes() == want[j].tobytes(), (i, j)
