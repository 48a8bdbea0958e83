"""Paired augmentation of the segmentation datasets on the GPU.

Host side of csrc/seg_augment.hip.  `SegPairedAugmenter` returns, for a whole batch in one launch,
what the training `__getitem__` of the reference's segmentation datasets returns per image
(/root/reference/code/datasets/segmentation/potsdam.py:95-216 `_Potsdam._prepare_train`,
cocostuff.py:104-230 `_Coco._prepare_train`):

  img1          the random S x S crop (zero-padded when the source is smaller), / 255.
  img2          the same crop after ColorJitter (RGB only, never IR), optionally random_affine,
                optionally a horizontal flip
  affine2_to_1  identity / inverse of the random affine, top row negated when flipped
  mask_img1     ones (Potsdam) or `_filter_label`'s mask of the cropped label map (COCO-Stuff)

with the channel layout of `custom_greyscale_numpy` (code/utils/segmentation/transforms.py:7-20):
no_sobel R,G,B(,IR); else R,G,B,grey(,IR) with include_rgb, grey(,IR) without -- what
`sobel_process(..., using_IR)` expects downstream.

The random parameters are drawn on the host in the reference's order and from its distributions
(`np.random.randint` crop centres, torchvision 0.2.1 `ColorJitter.get_params`, `random_affine`'s three
uniforms, `rand() > flip_p`), a few dozen bytes per image; `draw` exposes them so that callers and tests
can replay a recorded sequence.

Grey is OpenCV's 8-bit COLOR_RGB2GRAY in its 3.x fixed-point form, (R 4899 + G 9617 + B 1868 + 8192) >> 14,
restated from OpenCV's source and NOT compared against a cv2 binary (cv2 is not available where this
is built and tested; newer OpenCV builds use a 15-bit variant that can differ by one grey level).
Every published Potsdam command is --no_sobel and never reaches it; the COCO commands do.

Test time.  `SegTestPreparer` is the evaluation twin: what `_prepare_test` (potsdam.py:295-350,
cocostuff.py:309-358) returns per image -- the centre crop in the same channel layout, `_filter_label`'s label map
and its mask -- for a whole batch in one launch (csrc/seg_augment.hip::seg_prepare_test_kernel), and
`seg_mapping_dataloader` what `_create_mapping_loader` (code/utils/segmentation/data.py:129-149) yields.  Labels and
mask leave the kernel as uint8, the form seg_eval.SegEvalAccumulator consumes without a copy.  One more caveat on
grey: `_prepare_test` hands cv2.cvtColor the float32 image (it never truncates to uint8 as the training path does),
so a real OpenCV takes its float path there, 0.299 R + 0.587 G + 0.114 B unrounded; the kernel and the fixture's
stand-in use the rounded fixed-point grey above, within half a grey level of it.
"""
import math

import numpy as np
import torch

from . import _lib
from .augment import OP_BRIGHTNESS, OP_CONTRAST, OP_HUE, OP_SATURATION, hue_shift

IPARAMS, FPARAMS = 12, 10
GREY_R, GREY_G, GREY_B, GREY_SHIFT = 4899, 9617, 1868, 14     # csrc/seg_augment.hip SEG_GREY_*


def cv_grey(rgb_u8):
  """The kernel's grey on a uint8 [..., 3] array (host restatement for tests and tools)."""
  v = rgb_u8.astype(np.int64)
  return ((v[..., 0] * GREY_R + v[..., 1] * GREY_G + v[..., 2] * GREY_B + (1 << (GREY_SHIFT - 1)))
          >> GREY_SHIFT).astype(np.uint8)


def pad_offsets(h, w, sz):
  """pad_if_too_small (transforms.py:23-49): (padded h, padded w, row offset, column offset) of the source
  inside the zero image, with the reference's int(x / 2.) arithmetic."""
  new_h, new_w = max(h, sz), max(w, sz)
  return new_h, new_w, int(new_h / 2.) - int(h / 2.), int(new_w / 2.) - int(w / 2.)


def crop_centre_range(h, w, sz):
  """pad_and_or_crop mode 'random' (transforms.py:67-79): inclusive-exclusive randint bounds of the crop
  centre, (h_lo, h_hi, w_lo, w_hi), on the padded h x w image."""
  half = int(sz / 2.)
  if sz % 2 == 1:
    return half, h - 1 - half + 1, half, w - 1 - half + 1
  return half, h - half + 1, half, w - half + 1


def relevance_table(filter_label):
  """`_filter_label` (cocostuff.py:629-657, :734-760) as the 256-entry uint8 table the kernel reads:
  entry l is the mask of fine label l, entry 255 that of -1.  filter_label: the bound method (or any
  callable) taking an int32 label array and returning (labels, mask)."""
  fine = np.arange(256, dtype=np.int32)
  fine[255] = -1
  fine[182:255] = -1                       # not fine labels: treated as unlabelled
  _, mask = filter_label(fine.reshape(1, 256).copy())
  return np.ascontiguousarray(np.asarray(mask).reshape(256).astype(np.uint8))


def _flag(config, name, default=False):
  return getattr(config, name, default)


class _SegDraws(object):
  """What SegPairedAugmenter and seg_ragged.SegRaggedAugmenter share: the reference's flags, its jitter and
  random_affine draws from self.rng, the channel layout, and the warp of img2 that follows either kernel."""

  def _read_flags(self, config, seed, device):
    self.no_sobel, self.include_rgb = bool(config.no_sobel), bool(config.include_rgb)
    self.jitter = tuple(float(getattr(config, "jitter_" + n)) for n in ("brightness", "contrast", "saturation", "hue"))
    self.flip_p = float(config.flip_p)
    self.use_random_affine = bool(_flag(config, "use_random_affine"))
    if self.use_random_affine:
      self.aff = tuple(float(getattr(config, "aff_" + n)) for n in
                       ("min_rot", "max_rot", "min_shear", "max_shear", "min_scale", "max_scale"))
    self.rng = np.random.RandomState(seed)
    self.lut = (torch.arange(256, dtype=torch.float32) / 255).to(device)               # astype(float32) / 255.

  @property
  def out_channels(self):
    return (3 if self.no_sobel else (4 if self.include_rgb else 1)) + (1 if self.Cs == 4 else 0)

  def _jitter_draws(self, ip, fp):
    """torchvision 0.2.1 ColorJitter.get_params: one uniform per non-zero strength, in the order brightness,
    contrast, saturation, hue, then np.random.shuffle of the op list."""
    r = self.rng
    b, c, s, h = self.jitter
    ops = []
    if b > 0:
      fp[OP_BRIGHTNESS] = r.uniform(max(0, 1 - b), 1 + b)
      ops.append(OP_BRIGHTNESS)
    if c > 0:
      fp[OP_CONTRAST] = r.uniform(max(0, 1 - c), 1 + c)
      ops.append(OP_CONTRAST)
    if s > 0:
      fp[OP_SATURATION] = r.uniform(max(0, 1 - s), 1 + s)
      ops.append(OP_SATURATION)
    hue = 0.0
    if h > 0:
      hue = r.uniform(-h, h)
      fp[OP_HUE] = hue
      ops.append(OP_HUE)
    r.shuffle(ops)
    ip[4] = len(ops)
    ip[5:5 + len(ops)] = ops
    ip[9] = hue_shift(float(hue))
    return hue

  def _affine_draw(self):
    """random_affine (transforms.py:111-121): the three uniforms, affine1_to_2 and its float32 inverse."""
    min_rot, max_rot, min_shear, max_shear, min_scale, max_scale = self.aff
    r = self.rng
    a = np.radians(r.rand() * (max_rot - min_rot) + min_rot)
    shear = np.radians(r.rand() * (max_shear - min_shear) + min_shear)
    scale = r.rand() * (max_scale - min_scale) + min_scale
    return affine_pair(a, shear, scale)

  def _warp_img2(self, img2, a12, iparams):
    """img2 = flip(perform_affine_tf(img2, affine1_to_2)) as one iic_affine_warp_fwd launch."""
    n, C, S = int(img2.shape[0]), int(img2.shape[1]), self.S
    mats = warp_matrices(a12, iparams[:, 3] & 1, S).to(img2.device, non_blocking=True)
    warped = torch.empty_like(img2)
    _lib.check(_lib.lib().iic_affine_warp_fwd(img2.data_ptr(), mats.data_ptr(), warped.data_ptr(), n, C, S, S,
                                              0, 0, _lib.stream_ptr()), "iic_affine_warp_fwd")
    return warped


class SegPairedAugmenter(_SegDraws):
  """images_u8: uint8 [B, H, W, Cs] on the GPU, Cs = 3 (COCO-Stuff, RGB) or 4 (Potsdam, RGB + IR);
  labels_u8: uint8 [B, H, W] fine labels with 255 for the reference's -1, and relevance: the 256-entry
  table of `relevance_table` -- both or neither (neither: mask_img1 is all ones, as for Potsdam).
  config carries the reference's flags: input_sz, include_rgb, no_sobel, jitter_brightness / _contrast /
  _saturation / _hue, flip_p, use_random_affine (+ aff_min/max_rot, _shear, _scale), use_random_scale,
  pre_scale_all, mask_input.

  pre_scale_all: the reference resizes every image on every access (cv2.resize INTER_LINEAR on the float
  image, labels with INTER_NEAREST) and truncates to uint8 only after the crop.  Truncation is elementwise,
  so it commutes with the crop and the zero padding: the resident dataset here IS the pre-scaled, truncated
  images (and NEAREST-pre-scaled labels), prepared once by the caller.  The constructor only checks that
  H, W are plausible for input_sz; prescaled=False with config.pre_scale_all asks for the resize inside
  the kernel, which is not built.

  Not built (NotImplementedError): use_random_scale (a per-sample cv2.resize of a float image; no published
  command uses it).  mask_input is asserted false, as the reference does (cocostuff.py:63).

  draw(idx) -> params; apply(params) -> (img1, img2, affine2_to_1, mask_img1); paired_batch(idx) = both.
  With use_random_affine, img2 is warped by the library's affine warp (csrc/warp.hip, the grid convention
  of seg_losses.ALIGN_CORNERS, so img2 and the affine2_to_1 the loss consumes stay consistent); the flip
  is folded into the warp's matrix."""

  def __init__(self, images_u8, config, labels_u8=None, relevance=None, seed=0, prescaled=True):
    assert not _flag(config, "mask_input"), "cocostuff.py:63"
    if _flag(config, "use_random_scale"):
      raise NotImplementedError("use_random_scale (a per-sample cv2.resize of the float image) is not built")
    if _flag(config, "pre_scale_all") and not prescaled:
      raise NotImplementedError("pre_scale_all inside the kernel is not built: keep the pre-scaled, truncated "
                                "images (labels: NEAREST) resident and pass those")
    assert images_u8.dtype == torch.uint8 and images_u8.is_contiguous()
    assert images_u8.dim() == 4 and images_u8.shape[3] in (3, 4), "[B, H, W, 3] (RGB) or [B, H, W, 4] (RGB + IR) uint8"
    self.images = images_u8
    self.B, self.H, self.W, self.Cs = (int(v) for v in images_u8.shape)
    self.S = int(config.input_sz)
    if self.S % 4 != 0:
      raise NotImplementedError("input_sz must be a multiple of 4 (16-byte stores); the published runs use 128 and 200")
    if not (1 <= self.H <= 16384 and 1 <= self.W <= 16384):
      raise ValueError("implausible image size %d x %d" % (self.H, self.W))
    if 4 * max(self.H, self.W) < self.S:
      raise ValueError("images of %d x %d for input_sz %d would be almost all padding (scaled twice?)"
                       % (self.H, self.W, self.S))
    assert (labels_u8 is None) == (relevance is None), "labels_u8 and relevance go together"
    self.labels = labels_u8
    self.relevance = None
    if labels_u8 is not None:
      assert labels_u8.dtype == torch.uint8 and labels_u8.is_contiguous()
      assert tuple(labels_u8.shape) == (self.B, self.H, self.W) and labels_u8.device == images_u8.device
      rel = np.ascontiguousarray(np.asarray(relevance.cpu() if torch.is_tensor(relevance) else relevance,
                                            dtype=np.uint8).reshape(-1))
      assert rel.shape == (256,)
      self.relevance = torch.from_numpy(rel).to(images_u8.device)
    self._read_flags(config, seed, images_u8.device)

  def draw(self, idx):
    """The reference's draws for the samples `idx`, per sample in its order: crop centre (h, w), jitter,
    [random_affine's a, shear, scale], flip.  Returns a dict: iparams int32 [n, 12] and fparams float32
    [n, 10] as iic_seg_augment reads them, coords int [n, 2] (the crop centre h_c, w_c pad_and_or_crop
    returns), hue float64 [n] (the hue factor before its uint8 truncation), affine1_to_2 float32 [n, 2, 3]
    (None without use_random_affine; fparams[:, 4:10] holds its fp32 inverse)."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    n = idx.shape[0]
    ip = np.zeros((n, IPARAMS), np.int32)
    fp64 = np.zeros((n, 4), np.float64)
    fp = np.zeros((n, FPARAMS), np.float32)
    coords = np.zeros((n, 2), np.int64)
    hue = np.zeros(n, np.float64)
    a12 = np.zeros((n, 2, 3), np.float32) if self.use_random_affine else None
    new_h, new_w, _, _ = pad_offsets(self.H, self.W, self.S)
    h_lo, h_hi, w_lo, w_hi = crop_centre_range(new_h, new_w, self.S)
    half = int(self.S / 2.)
    r = self.rng
    ip[:, 0] = idx
    fp[:, 4], fp[:, 8] = 1.0, 1.0                               # identity affine2_to_1
    for i in range(n):
      h_c = r.randint(low=h_lo, high=h_hi)
      w_c = r.randint(low=w_lo, high=w_hi)
      coords[i] = (h_c, w_c)
      ip[i, 1], ip[i, 2] = w_c - half, h_c - half
      hue[i] = self._jitter_draws(ip[i], fp64[i])
      if self.use_random_affine:
        m12, m21 = self._affine_draw()
        a12[i] = m12
        fp[i, 4:10] = m21.reshape(6)
      ip[i, 3] = 1 if r.rand() > self.flip_p else 0
    fp[:, :4] = fp64
    return dict(iparams=ip, fparams=fp, coords=coords, hue=hue, affine1_to_2=a12)

  def apply(self, params):
    iparams = np.ascontiguousarray(params["iparams"], dtype=np.int32)
    fparams = np.ascontiguousarray(params["fparams"], dtype=np.float32)
    a12 = params.get("affine1_to_2")
    n = int(iparams.shape[0])
    assert iparams.shape == (n, IPARAMS) and fparams.shape == (n, FPARAMS)
    assert n > 0 and iparams[:, 0].min() >= 0 and iparams[:, 0].max() < self.B, "source index out of range"
    new_h, new_w, _, _ = pad_offsets(self.H, self.W, self.S)
    assert (iparams[:, 1] >= 0).all() and (iparams[:, 1] + self.S <= new_w).all(), "crop outside the (padded) image"
    assert (iparams[:, 2] >= 0).all() and (iparams[:, 2] + self.S <= new_h).all(), "crop outside the (padded) image"
    assert (iparams[:, 4] >= 0).all() and (iparams[:, 4] <= 4).all()
    assert (iparams[:, 5:9] >= 0).all() and (iparams[:, 5:9] <= 3).all()
    assert ((iparams[:, 3] & ~1) == 0).all(), "flip is one bit"
    assert self.images.is_cuda, "the dataset must be resident on the GPU (there is no CPU path)"
    assert (a12 is not None) == self.use_random_affine
    dev = self.images.device
    S, C = self.S, self.out_channels
    if a12 is not None:
      iparams = iparams.copy()
      iparams[:, 3] |= 2                   # the mirror of img2 is folded into the warp below
    ip = torch.from_numpy(iparams).to(dev, non_blocking=True)
    fp = torch.from_numpy(fparams).to(dev, non_blocking=True)
    img1 = torch.empty(n, C, S, S, device=dev, dtype=torch.float32)
    img2 = torch.empty(n, C, S, S, device=dev, dtype=torch.float32)
    mask = torch.empty(n, S, S, device=dev, dtype=torch.uint8)
    aff = torch.empty(n, 2, 3, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().iic_seg_augment(
      self.images.data_ptr(), self.B, self.H, self.W, self.Cs, _lib.ptr(self.labels), _lib.ptr(self.relevance),
      ip.data_ptr(), fp.data_ptr(), n, S, int(self.no_sobel), int(self.include_rgb), self.lut.data_ptr(),
      img1.data_ptr(), img2.data_ptr(), mask.data_ptr(), aff.data_ptr(), _lib.stream_ptr()), "iic_seg_augment")
    if a12 is not None:
      img2 = self._warp_img2(img2, a12, iparams)
    return img1, img2, aff, mask

  def paired_batch(self, idx):
    """What one iteration of ONE of the reference's paired dataloaders yields
    (code/scripts/segmentation/segmentation_twohead.py:283): img1, img2, affine2_to_1, mask_img1."""
    return self.apply(self.draw(idx))


def affine_pair(a, shear, scale):
  """random_affine's matrices (transforms.py:115-121): affine1_to_2 float32 [2, 3] and affine2_to_1 =
  np.linalg.inv of the float32 3 x 3, as float32 [2, 3]."""
  m12 = np.array([[np.cos(a) * scale, - np.sin(a + shear) * scale, 0.],
                  [np.sin(a) * scale, np.cos(a + shear) * scale, 0.],
                  [0., 0., 1.]], dtype=np.float32)
  m21 = np.linalg.inv(m12).astype(np.float32)
  return m12[:2, :], m21[:2, :]


def warp_matrices(affine1_to_2, flips, S):
  """Pixel-space rows [n, 6] for iic_affine_warp_fwd: img2 = flip(perform_affine_tf(img2, affine1_to_2)).
  The warp's source pixel of output (ox, oy) is M (ox, oy, 1) (seg_losses._pixel_matrices, the grid
  convention of seg_losses.ALIGN_CORNERS); a flipped sample reads M (S - 1 - ox, oy, 1) instead."""
  from . import seg_losses
  M = seg_losses._pixel_matrices(torch.from_numpy(np.ascontiguousarray(affine1_to_2, dtype=np.float32)), S, S).double()
  f = torch.from_numpy(np.asarray(flips).astype(np.bool_))
  Mf = M.clone()
  Mf[:, 2] = M[:, 0] * (S - 1) + M[:, 2]
  Mf[:, 0] = -M[:, 0]
  Mf[:, 5] = M[:, 3] * (S - 1) + M[:, 5]
  Mf[:, 3] = -M[:, 3]
  return torch.where(f[:, None], Mf, M).float().contiguous()


class _SegPairedLoader(object):
  """One element of the list `_create_dataloaders` returns (code/utils/segmentation/data.py:86-126):
  iterating yields (img1, img2, affine2_to_1, mask_img1) batches, the last one ragged (drop_last=False); every loader
  of the list draws its own augmentation of the same samples.  order: None for sequential sample order, else the
  `_EpochOrder` the loaders of one list share."""

  def __init__(self, augmenter, batch_sz, order=None):
    self.aug, self.batch_sz, self.n, self.order = augmenter, int(batch_sz), int(augmenter.B), order
    self.epoch = 0
    assert self.batch_sz > 0

  def __len__(self):
    return (self.n + self.batch_sz - 1) // self.batch_sz

  def __iter__(self):
    perm = np.arange(self.n) if self.order is None else self.order.permutation(self.epoch)
    self.epoch += 1
    for lo in range(0, self.n, self.batch_sz):
      yield self.aug.paired_batch(perm[lo:min(self.n, lo + self.batch_sz)])


class _EpochOrder(object):
  """The sample order of epoch e, the same for every loader that asks: a permutation seeded by (seed, e) alone,
  from a generator that serves nothing else, so the augmenter's draws are what they would be without shuffling."""

  def __init__(self, n, seed):
    self.n, self.seed = int(n), int(seed)

  def permutation(self, epoch):
    return np.random.RandomState([self.seed, int(epoch)]).permutation(self.n)


def seg_paired_dataloaders(augmenter, batch_sz, num_dataloaders, shuffle=False, shuffle_seed=0):
  """Drop-in for the list of DataLoaders the segmentation scripts zip
  (code/scripts/segmentation/segmentation_twohead.py:262-300): num_dataloaders loaders over the same
  samples, each yielding the four tensors of `_prepare_train` per batch, already on the GPU.  augmenter: a
  SegPairedAugmenter or a seg_ragged.SegRaggedAugmenter.

  shuffle=False (default): sequential sample order.  shuffle=True: every epoch (every iteration of the loaders)
  visits the samples in a fresh permutation, the same one for every loader of the list, drawn from a generator of
  its own (shuffle_seed) so that the augmentation draws do not shift.  The reference shuffles when
  num_dataloaders == 1 (code/utils/segmentation/data.py:90) with torch's randperm; that permutation is NOT
  reproduced here, only the property that each epoch is a permutation."""
  assert int(num_dataloaders) >= 1
  order = _EpochOrder(augmenter.B, shuffle_seed) if shuffle else None
  return [_SegPairedLoader(augmenter, batch_sz, order) for _ in range(int(num_dataloaders))]


# ------------------------------------------------------------------------------------------
# test time: _prepare_test
# ------------------------------------------------------------------------------------------
def _fine_labels():
  fine = np.arange(256, dtype=np.int32)
  fine[182:] = -1                          # 255 is -1; 182..254 are not fine labels: treated as unlabelled
  return fine


def label_table(filter_label):
  """Companion of `relevance_table`: `_filter_label`'s returned LABEL (potsdam.py:429-439, cocostuff.py:629-657,
  :734-760) as the 256-entry uint8 table the test kernel reads.  Entry l is the low 8 bits of the reference's int32
  value for fine label l (entry 255: for -1), so a map looked up here equals `ref_label.astype(np.uint8)` in masked-out
  pixels too, negatives included.  filter_label: the bound method (or any callable) taking an int32 label array and
  returning the labels alone (Potsdam) or (labels, mask) (COCO-Stuff); it may work in place.  The table is whatever
  the method returns, quirks included: _CocoFew starts its map from zeros, so -1 comes back as class 0 with mask 1.
  A method that refuses the whole range (Potsdam fine: `assert label.max() < gt_k`) is asked one label at a time;
  the labels it refuses get 255."""
  def labels_of(fine):
    res = filter_label(fine.copy())
    return np.asarray(res[0] if isinstance(res, tuple) else res).astype(np.int64).reshape(-1)
  fine = _fine_labels()
  try:
    lab = labels_of(fine.reshape(1, 256))
  except AssertionError:
    lab = np.full(256, -1, np.int64)
    for i in range(256):
      try:
        lab[i] = labels_of(fine[i:i + 1].reshape(1, 1))[0]
      except AssertionError:
        pass
  return np.ascontiguousarray((lab & 255).astype(np.uint8))


def prepare_test_host(img, label, input_sz, no_sobel, include_rgb, targets, relevance=None):
  """`_prepare_test` (potsdam.py:295-350, cocostuff.py:309-358) for one image, in numpy: the host restatement for
  tests and tools.  img uint8 [h, w, 3 or 4], label uint8 [h, w] fine labels (255 for -1), targets / relevance the
  tables of `label_table` / `relevance_table` (relevance None: Potsdam, mask of ones).
  Returns (img float32 [C, S, S], targets uint8 [S, S], mask uint8 [S, S])."""
  S = int(input_sz)
  h, w, cs = img.shape
  assert label.shape == (h, w) and img.dtype == np.uint8 and label.dtype == np.uint8
  new_h, new_w, oy, ox = pad_offsets(h, w, S)
  pad = np.zeros((new_h, new_w, cs), np.uint8)
  pad[oy:oy + h, ox:ox + w] = img
  lpad = np.zeros((new_h, new_w), np.uint8)                # pad_if_too_small zero-fills: fine label 0
  lpad[oy:oy + h, ox:ox + w] = label
  y0, x0 = int(new_h / 2.) - int(S / 2.), int(new_w / 2.) - int(S / 2.)       # pad_and_or_crop mode "centre"
  crop, lab = pad[y0:y0 + S, x0:x0 + S], lpad[y0:y0 + S, x0:x0 + S]
  v = crop[:, :, :3]
  if not no_sobel:
    grey = cv_grey(v)[:, :, None]
    v = np.concatenate([v, grey], axis=2) if include_rgb else grey
  v = v.astype(np.float32) / 255.
  if cs == 4:
    v = np.concatenate([v, (crop[:, :, 3].astype(np.float32) / 255.)[:, :, None]], axis=2)
  mask = np.ones((S, S), np.uint8) if relevance is None else np.asarray(relevance, np.uint8)[lab]
  return np.ascontiguousarray(v.transpose(2, 0, 1)), np.asarray(targets, np.uint8)[lab], np.ascontiguousarray(mask)


def _table(t, device):
  t = np.ascontiguousarray(np.asarray(t.cpu() if torch.is_tensor(t) else t, dtype=np.uint8).reshape(-1))
  assert t.shape == (256,)
  return torch.from_numpy(t).to(device)


class SegTestPreparer(object):
  """images_u8: uint8 [B, H, W, Cs] and labels_u8: uint8 [B, H, W] (fine labels, 255 for -1) on the GPU -- the
  partitions of a mapping loader concatenated by the caller; targets: the table of `label_table`; relevance: the table
  of `relevance_table`, or None (Potsdam: mask of ones).  sizes: int [B, 2], the (h, w) of every image when they differ
  (COCO-Stuff): image i occupies the top-left h x w of its slab and is centre-cropped by its own extent, as the
  reference crops each image; None: every image is H x W.  config is read for input_sz, include_rgb, no_sobel,
  pre_scale_all and mask_input (asserted false).  pre_scale_all as for SegPairedAugmenter: the resident arrays ARE the
  pre-scaled images and NEAREST-pre-scaled labels (and sizes their extents); prescaled=False asks for the resize
  inside the kernel, which is not built.

  batch(idx) -> (imgs float32 [n, C, S, S], targets uint8 [n, S, S], mask uint8 [n, S, S]) on the device."""

  def __init__(self, images_u8, labels_u8, config, targets, relevance=None, sizes=None, prescaled=True):
    assert not _flag(config, "mask_input"), "cocostuff.py:348"
    if _flag(config, "pre_scale_all") and not prescaled:
      raise NotImplementedError("pre_scale_all inside the kernel is not built: keep the pre-scaled, truncated "
                                "images (labels: NEAREST) resident and pass those")
    assert images_u8.dtype == torch.uint8 and images_u8.is_contiguous()
    assert images_u8.dim() == 4 and images_u8.shape[3] in (3, 4), "[B, H, W, 3] (RGB) or [B, H, W, 4] (RGB + IR) uint8"
    self.images = images_u8
    self.B, self.H, self.W, self.Cs = (int(v) for v in images_u8.shape)
    self.S = int(config.input_sz)
    if self.S % 4 != 0:
      raise NotImplementedError("input_sz must be a multiple of 4 (16-byte stores); the published runs use 128 and 200")
    if not (1 <= self.H <= 16384 and 1 <= self.W <= 16384):
      raise ValueError("implausible image size %d x %d" % (self.H, self.W))
    assert labels_u8.dtype == torch.uint8 and labels_u8.is_contiguous()
    assert tuple(labels_u8.shape) == (self.B, self.H, self.W) and labels_u8.device == images_u8.device
    self.labels = labels_u8
    dev = images_u8.device
    self.targets = _table(targets, dev)
    self.relevance = None if relevance is None else _table(relevance, dev)
    self.sizes = None
    if sizes is not None:
      sz = np.ascontiguousarray(np.asarray(sizes.cpu() if torch.is_tensor(sizes) else sizes).astype(np.int64))
      if sz.shape != (self.B, 2):
        raise ValueError("sizes must be [%d, 2], one (h, w) per image" % self.B)
      if (sz < 1).any() or (sz[:, 0] > self.H).any() or (sz[:, 1] > self.W).any():
        raise ValueError("sizes out of range: every (h, w) must lie within 1..%d x 1..%d" % (self.H, self.W))
      self.sizes = torch.from_numpy(sz.astype(np.int32)).to(dev)
    self.no_sobel, self.include_rgb = bool(config.no_sobel), bool(config.include_rgb)
    self.lut = (torch.arange(256, dtype=torch.float32) / 255).to(dev)                  # astype(float32) / 255.

  @property
  def out_channels(self):
    return (3 if self.no_sobel else (4 if self.include_rgb else 1)) + (1 if self.Cs == 4 else 0)

  def batch(self, idx):
    idx = np.ascontiguousarray(np.asarray(idx).reshape(-1), dtype=np.int32)
    n = int(idx.shape[0])
    assert n > 0 and idx.min() >= 0 and idx.max() < self.B, "source index out of range"
    assert self.images.is_cuda, "the dataset must be resident on the GPU (there is no CPU path)"
    dev = self.images.device
    S = self.S
    didx = torch.from_numpy(idx).to(dev, non_blocking=True)
    imgs = torch.empty(n, self.out_channels, S, S, device=dev, dtype=torch.float32)
    targets = torch.empty(n, S, S, device=dev, dtype=torch.uint8)
    mask = torch.empty(n, S, S, device=dev, dtype=torch.uint8)
    _lib.check(_lib.lib().iic_seg_prepare_test(
      self.images.data_ptr(), self.B, self.H, self.W, self.Cs, self.labels.data_ptr(), _lib.ptr(self.sizes),
      self.targets.data_ptr(), _lib.ptr(self.relevance), didx.data_ptr(), n, S, int(self.no_sobel),
      int(self.include_rgb), self.lut.data_ptr(), imgs.data_ptr(), targets.data_ptr(), mask.data_ptr(),
      _lib.stream_ptr()), "iic_seg_prepare_test")
    return imgs, targets, mask


class _SegMappingLoader(object):
  """What `_create_mapping_loader` returns (code/utils/segmentation/data.py:129-149, shuffle=False, drop_last=False):
  iterating yields (imgs, flat_targets, mask) batches in sequential sample order, the last one ragged."""

  def __init__(self, preparer, batch_sz):
    self.prep, self.batch_sz, self.n = preparer, int(batch_sz), int(preparer.B)
    assert self.batch_sz > 0

  def __len__(self):
    return (self.n + self.batch_sz - 1) // self.batch_sz

  def __iter__(self):
    for lo in range(0, self.n, self.batch_sz):
      yield self.prep.batch(np.arange(lo, min(self.n, lo + self.batch_sz)))


def seg_mapping_dataloader(preparer, batch_sz):
  """Drop-in for mapping_assignment_dataloader / mapping_test_dataloader of the segmentation scripts
  (code/utils/segmentation/data.py:58-83, code/scripts/segmentation/segmentation_twohead.py:163): consumed by iic_amd.seg_eval.segmentation_eval and by
  the reference's own _segmentation_get_data alike, every tensor already on the GPU."""
  return _SegMappingLoader(preparer, batch_sz)
