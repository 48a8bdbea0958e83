"""Paired augmentation of a segmentation dataset whose images differ in size, on the GPU.

Host side of csrc/seg_augment.hip::seg_augment_ragged_kernel (C ABI `iic_seg_augment_ragged`), the sibling of
seg_augment.SegPairedAugmenter for COCO-Stuff: every published COCO-Stuff command (examples/commands.txt:74-97) trains
on images of many sizes, and the reference pads and crops each by ITS OWN extent -- `pad_if_too_small` +
`pad_and_or_crop(mode="random")` (code/utils/segmentation/transforms.py:23-88) from `_Coco._prepare_train`
(code/datasets/segmentation/cocostuff.py:133-135).  The crop-centre range, the padding offsets and which pixels are
padding all follow from the image's (h, w).  The dataset is kept PACKED: the images concatenated without padding,
image i being uint8 [h_i, w_i, Cs] at pixel offset offsets[i]; labels one byte per pixel at the same offsets.

`SegRaggedAugmenter` returns the four tensors of `_prepare_train` -- img1, img2, affine2_to_1, mask_img1 -- with the
draws, the parameter dictionary and the methods of SegPairedAugmenter (whose docstring describes them); the two share
their draw code (seg_augment._SegDraws) and `seg_paired_dataloaders` takes either.

use_random_scale (cocostuff.py:123-130, potsdam.py:109-114): the reference draws one scale per sample BEFORE the crop
centre, resizes the float32 image with cv2.resize(fx = fy = scale, INTER_LINEAR) and the labels with INTER_NEAREST, and
crops the scaled image; RGB is truncated to uint8 afterwards (`img.astype(np.uint8)` for PIL), Potsdam's IR plane never
(potsdam.py:148-151, :170), so after a resize IR leaves the kernel as value / 255. without truncation.
`resize_linear_host` / `resize_nearest_host` restate OpenCV 3.x's `resize` for float32 / int32 input from its source
(modules/imgproc/src/resize.cpp: the destination size is cvRound(len * scale), the inverse scale 1. / scale in double, coefficients in float32, a horizontal pass then a vertical one, no fused multiply-add); they are
NOT compared against a cv2 binary -- cv2 is not available where this is built and tested -- exactly as for the grey
conversion of seg_augment.  All coefficient arithmetic happens here on the host: `apply` hands the kernel, per sample,
the taps of the S crop rows and S crop columns, and the kernel multiplies and adds.

pre_scale_all (cocostuff.py:113-120, potsdam.py:103-106) comes in two forms.  source="resident" (the default): the
resident pack holds the PRE-SCALED, truncated images -- seg_prescale.prescale_dataset makes it on the device -- and the
flag changes nothing here; use_random_scale cannot be combined with it, because the reference resizes the untruncated
float image a second time.  source="original": the resident pack holds the original-resolution images and every
sample is pre-scaled inside the kernel: without use_random_scale that is the resampling above with scale =
pre_scale_factor; with it, `crop_taps2` composes the taps of both resizes and iic_seg_augment_ragged_prescaled keeps the
intermediate image in float32 (sixteen source pixels per output pixel).  Cs = 4 is served by source="original" only.

use_random_affine: img2 is warped by iic_seg_augment_warp, F.affine_grid + F.grid_sample + flip in the operation order of
torch's CPU kernels (`grid_warp_host` is its host restatement), so that img2 equals the reference's bit for bit; the
uniform augmenter's iic_affine_warp_fwd computes the same warp within 2e-6.
"""
import numpy as np
import torch

from . import _lib
from .seg_augment import FPARAMS, IPARAMS, _SegDraws, _flag, crop_centre_range, pad_offsets

MAX_SIDE = 16384
SOURCES = ("resident", "original")
# iic_seg_resample_tap (include/iic_hip.h)
TAP_DTYPE = np.dtype([("i0", "<i4"), ("i1", "<i4"), ("a0", "<f4"), ("a1", "<f4"), ("nearest", "<i4"), ("inside", "<i4")])
# iic_seg_resample_tap2: [k] = the first resize's taps that produce the second resize's tap k
TAP2_DTYPE = np.dtype([("i0", "<i4", (2,)), ("i1", "<i4", (2,)), ("a0", "<f4", (2,)), ("a1", "<f4", (2,)),
                       ("b0", "<f4"), ("b1", "<f4"), ("nearest", "<i4"), ("inside", "<i4")])


# ------------------------------------------------------------------------------------------
# cv2.resize(dsize=None, fx=scale, fy=scale) restated (OpenCV 3.x, float32 image / int32 labels)
# ------------------------------------------------------------------------------------------
def scaled_len(length, scale):
  """Destination side of cv2.resize: cvRound(len * scale) (round half to even), at least 1."""
  v = np.rint(np.asarray(length, np.float64) * np.asarray(scale, np.float64)).astype(np.int64)
  return np.maximum(v, 1)


def linear_taps(src_len, scale, d):
  """INTER_LINEAR along one side: for destination indices d (any integer array; src_len and scale broadcast against
  it) the tap indices (i0, i1) and their float32 weights (a0, a1)."""
  d = np.asarray(d, np.float64)
  src_len = np.broadcast_to(np.asarray(src_len, np.int64), d.shape)
  inv = 1.0 / np.asarray(scale, np.float64)
  f = ((d + 0.5) * inv - 0.5).astype(np.float32)            # the product and the difference in float64
  s = np.floor(f)
  f = (f - s).astype(np.float32)
  s = s.astype(np.int64)
  lo = s < 0
  s = np.where(lo, 0, s)
  f = np.where(lo, np.float32(0), f)
  hi = s >= src_len - 1
  s = np.where(hi, src_len - 1, s)
  f = np.where(hi, np.float32(0), f).astype(np.float32)
  return s, np.minimum(s + 1, src_len - 1), (np.float32(1) - f).astype(np.float32), f


def nearest_index(src_len, scale, d):
  """INTER_NEAREST along one side: min(floor(d / scale), len - 1), the division as a product with 1. / scale."""
  inv = 1.0 / np.asarray(scale, np.float64)
  s = np.floor(np.asarray(d, np.float64) * inv).astype(np.int64)
  return np.minimum(s, np.asarray(src_len, np.int64) - 1)


def resize_linear_host(img, scale):
  """cv2.resize(img float32 [h, w] or [h, w, c], dsize=None, fx=scale, fy=scale, interpolation=INTER_LINEAR):
  (p00 ax0 + p01 ax1) by0 + (p10 ax0 + p11 ax1) by1, every product and sum rounded to float32."""
  img = np.asarray(img)
  assert img.dtype == np.float32 and img.ndim in (2, 3)
  v = img.reshape(img.shape[0], img.shape[1], -1)
  h, w = v.shape[:2]
  nh, nw = int(scaled_len(h, scale)), int(scaled_len(w, scale))
  x0, x1, ax0, ax1 = linear_taps(w, scale, np.arange(nw))
  y0, y1, by0, by1 = linear_taps(h, scale, np.arange(nh))
  rows = v[:, x0] * ax0[None, :, None] + v[:, x1] * ax1[None, :, None]
  out = rows[y0] * by0[:, None, None] + rows[y1] * by1[:, None, None]
  assert out.dtype == np.float32
  return np.ascontiguousarray(out.reshape((nh, nw) + img.shape[2:]))


def resize_nearest_host(label, scale):
  """cv2.resize(label [h, w], dsize=None, fx=scale, fy=scale, interpolation=INTER_NEAREST)."""
  label = np.asarray(label)
  assert label.ndim == 2
  h, w = label.shape
  ys = nearest_index(h, scale, np.arange(int(scaled_len(h, scale))))
  xs = nearest_index(w, scale, np.arange(int(scaled_len(w, scale))))
  return np.ascontiguousarray(label[ys][:, xs])


def crop_taps(src_len, scale, origin, S):
  """The kernel's table for one side of n samples: the taps of crop positions 0..S-1, TAP_DTYPE [n, S].
  src_len int [n], scale float64 [n], origin int [n]: the crop origin in the padded scaled side."""
  src_len = np.asarray(src_len, np.int64).reshape(-1, 1)
  scale = np.asarray(scale, np.float64).reshape(-1, 1)
  dst_len = scaled_len(src_len, scale)
  pad = np.maximum(dst_len, S) // 2 - dst_len // 2                  # pad_offsets' int(x / 2.) on non-negative ints
  d = np.asarray(origin, np.int64).reshape(-1, 1) + np.arange(S)[None, :] - pad
  inside = (d >= 0) & (d < dst_len)
  d = np.clip(d, 0, dst_len - 1)
  t = np.zeros(d.shape, TAP_DTYPE)
  t["i0"], t["i1"], t["a0"], t["a1"] = linear_taps(src_len, scale, d)
  t["nearest"] = nearest_index(src_len, scale, d)
  t["inside"] = inside
  return t


def crop_taps2(src_len, factor, scale, origin, S):
  """crop_taps for two resizes in a row -- by `factor` (pre_scale_all), then by `scale` (use_random_scale) -- of a side
  of src_len pixels, TAP2_DTYPE [n, S]: the second resize's two taps and weights (b0, b1) on the pre-scaled side and,
  for each of the two, the first resize's taps on the source side; nearest of nearest for the label.  factor: one
  float; src_len int [n], scale float64 [n], origin int [n]: the crop origin in the padded twice-scaled side."""
  src_len = np.asarray(src_len, np.int64).reshape(-1, 1)
  scale = np.asarray(scale, np.float64).reshape(-1, 1)
  factor = np.float64(factor)
  mid_len = scaled_len(src_len, factor)
  dst_len = scaled_len(mid_len, scale)
  pad = np.maximum(dst_len, S) // 2 - dst_len // 2
  d = np.asarray(origin, np.int64).reshape(-1, 1) + np.arange(S)[None, :] - pad
  inside = (d >= 0) & (d < dst_len)
  d = np.clip(d, 0, dst_len - 1)
  t = np.zeros(d.shape, TAP2_DTYPE)
  m0, m1, t["b0"], t["b1"] = linear_taps(mid_len, scale, d)
  for k, m in enumerate((m0, m1)):
    i0, i1, a0, a1 = linear_taps(src_len, factor, m)
    t["i0"][..., k], t["i1"][..., k], t["a0"][..., k], t["a1"][..., k] = i0, i1, a0, a1
  t["nearest"] = nearest_index(src_len, factor, nearest_index(mid_len, scale, d))
  t["inside"] = inside
  return t


# ------------------------------------------------------------------------------------------
# random_affine's warp restated (perform_affine_tf, transforms.py:131-143, on a CPU): what iic_seg_augment_warp computes
# ------------------------------------------------------------------------------------------
def _fma(a, b, c):
  """float32 fused multiply-add: the product of two float32 is exact in float64."""
  return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def grid_warp_host(img, affine1_to_2, flip=False):
  """flip(F.grid_sample(img, F.affine_grid(affine1_to_2)))) for one float32 [C, S, S] image, bilinear, zero padding,
  align_corners false, in the operation order of torch's CPU kernels (bit-identical to them on the fixture's cases,
  and at input_sz 36, 48, 128 and 200 when compared with the installed torch):
  the host restatement of csrc/seg_augment.hip::seg_grid_warp_kernel for tests and tools."""
  one, half_px = np.float32(1), np.float32(0.5)
  img = np.asarray(img, np.float32)
  C, S, _ = img.shape
  t = np.asarray(affine1_to_2, np.float32).reshape(6)
  base = (torch.linspace(-1, 1, S) * (S - 1) / S).numpy()
  xb, yb = np.meshgrid(base[::-1] if flip else base, base)
  gx = _fma(yb, t[1], xb * t[0]) + t[2]
  gy = _fma(yb, t[4], xb * t[3]) + t[5]
  half = np.float32(S) / np.float32(2)
  fx, fy = _fma(gx + one, half, -half_px), _fma(gy + one, half, -half_px)
  xw, yn = np.floor(fx), np.floor(fy)
  w, n = fx - xw, fy - yn
  e, s = one - w, one - n
  ix, iy = xw.astype(np.int64), yn.astype(np.int64)

  def tap(yy, xx):
    inside = (yy >= 0) & (yy < S) & (xx >= 0) & (xx < S)
    return np.where(inside[None], img[:, np.clip(yy, 0, S - 1), np.clip(xx, 0, S - 1)], np.float32(0))
  r = tap(iy, ix) * (s * e)[None]
  r = _fma(tap(iy, ix + 1), (s * w)[None], r)
  r = _fma(tap(iy + 1, ix), (n * e)[None], r)
  return _fma(tap(iy + 1, ix + 1), (n * w)[None], r)


# ------------------------------------------------------------------------------------------
# packing
# ------------------------------------------------------------------------------------------
def pack_images(images, labels=None):
  """A list of uint8 [h_i, w_i, Cs] arrays (and of uint8 [h_i, w_i] label maps, 255 for -1) as the packed layout:
  (pixels uint8 [total, Cs], labels uint8 [total] or None, sizes int32 [B, 2], offsets int64 [B])."""
  if len(images) == 0:
    raise ValueError("images: the list is empty")
  arrs = [np.asarray(a.cpu() if torch.is_tensor(a) else a) for a in images]
  for i, a in enumerate(arrs):
    if a.dtype != np.uint8:
      raise TypeError("images[%d]: dtype %s, expected uint8" % (i, a.dtype))
    if a.ndim != 3 or a.shape[2] != arrs[0].shape[2]:
      raise ValueError("images[%d]: shape %s, expected [h, w, Cs] with one Cs for the whole list" % (i, a.shape))
  sizes = np.array([a.shape[:2] for a in arrs], np.int32)
  offsets = np.concatenate([[0], np.cumsum(sizes[:, 0].astype(np.int64) * sizes[:, 1])[:-1]]).astype(np.int64)
  pixels = np.ascontiguousarray(np.concatenate([a.reshape(-1, a.shape[2]) for a in arrs], 0))
  packed_labels = None
  if labels is not None:
    if len(labels) != len(arrs):
      raise ValueError("labels: %d maps for %d images" % (len(labels), len(arrs)))
    labs = [np.asarray(a.cpu() if torch.is_tensor(a) else a) for a in labels]
    for i, a in enumerate(labs):
      if a.dtype != np.uint8:
        raise TypeError("labels[%d]: dtype %s, expected uint8 (255 for -1)" % (i, a.dtype))
      if a.shape != arrs[i].shape[:2]:
        raise ValueError("labels[%d]: shape %s, its image is %s" % (i, a.shape, arrs[i].shape[:2]))
    packed_labels = np.ascontiguousarray(np.concatenate([a.reshape(-1) for a in labs], 0))
  return pixels, packed_labels, sizes, offsets


def unpack_images(pixels, sizes, offsets, labels=None):
  """Inverse of pack_images on host arrays: the list of images (and the list of label maps, or None)."""
  imgs, labs = [], []
  for (h, w), o in zip(np.asarray(sizes), np.asarray(offsets)):
    imgs.append(pixels[o:o + h * w].reshape(h, w, -1))
    if labels is not None:
      labs.append(labels[o:o + h * w].reshape(h, w))
  return imgs, (labs if labels is not None else None)


def _host(t):
  return np.asarray(t.cpu() if torch.is_tensor(t) else t)


def check_pack(total, sizes, offsets=None):
  """sizes and offsets of a pack of `total` pixels as int64 arrays ([B, 2], [B]), or the ValueError that names what is
  wrong with them.  offsets None: the images back to back."""
  sz = _host(sizes)
  if sz.dtype.kind not in "iu" or sz.ndim != 2 or sz.shape[1] != 2 or sz.shape[0] < 1:
    raise ValueError("sizes: must be an integer array [B, 2], one (h, w) per image")
  sz = sz.astype(np.int64)
  if (sz < 1).any() or (sz > MAX_SIDE).any():
    raise ValueError("sizes: every h and w must lie within 1..%d" % MAX_SIDE)
  B = int(sz.shape[0])
  area = sz[:, 0] * sz[:, 1]
  if offsets is None:
    off = np.concatenate([[0], np.cumsum(area)[:-1]]).astype(np.int64)
  else:
    off = _host(offsets)
    if off.dtype.kind not in "iu" or off.shape != (B,):
      raise ValueError("offsets: must be an integer array [%d], the pixel offset of every image" % B)
    off = off.astype(np.int64)
  if (off < 0).any() or (off + area > total).any():
    raise ValueError("offsets: image %d leaves the packed array of %d pixels"
                     % (int(np.argmax((off < 0) | (off + area > total))), total))
  order = np.argsort(off, kind="stable")
  if (off[order][1:] < (off + area)[order][:-1]).any():
    raise ValueError("offsets: images overlap -- offsets are not consistent with sizes")
  return sz, off


class SegRaggedAugmenter(_SegDraws):
  """images: a list of uint8 [h_i, w_i, Cs] arrays (packed and uploaded to `device`, with labels: the list of uint8
  [h_i, w_i] fine-label maps, 255 for -1), OR the packed uint8 [total, Cs] tensor already on the device, with sizes
  int [B, 2] = (h_i, w_i), offsets int [B] (pixel offset of every image; default: the images back to back) and labels
  the packed uint8 [total] tensor.  Cs = 3 (RGB) or 4 (RGB + IR).  relevance: the table of
  seg_augment.relevance_table, given exactly when labels are (neither: mask_img1 is all ones).

  config: the flags SegPairedAugmenter reads, plus use_random_scale with scale_min / scale_max.  pre_scale_all keeps
  its meaning there: the resident images ARE the pre-scaled, truncated ones (labels NEAREST).  Refused
  (NotImplementedError): pre_scale_all together with use_random_scale -- the reference resizes the untruncated float
  image a second time, which a resident uint8 image cannot reproduce; pre_scale_all with prescaled=False; input_sz
  not a multiple of 4.  mask_input is asserted false (cocostuff.py:63).

  source="original": the resident pack holds the ORIGINAL-resolution images, and pre_scale_all / pre_scale_factor are
  honoured inside the kernel, with or without use_random_scale (the module docstring says how); ValueError without
  pre_scale_all or with a factor outside (0, 1) (cocostuff.py:114).  The default, source="resident", is described above.

  draw(idx) -> params: SegPairedAugmenter's dictionary, the crop origin in each sample's own padded (scaled) image,
  plus scale float64 [n] (None without use_random_scale) and extent int [n, 2], the (h, w) the crop was drawn on
  (source="original": cvRound(len * pre_scale_factor) per side, then cvRound(that * scale)).
  Per sample the reference's order: [scale], crop centre h then w, jitter, [random_affine's three], flip.
  apply(params) -> (img1, img2, affine2_to_1, mask_img1); paired_batch(idx) = both."""

  def __init__(self, images, config, labels=None, relevance=None, sizes=None, offsets=None, seed=0, prescaled=True,
               device=None, source="resident"):
    assert not _flag(config, "mask_input"), "mask_input is not built (cocostuff.py:63 asserts it false)"
    if source not in SOURCES:
      raise ValueError("source: %r, expected one of %s" % (source, ", ".join(repr(v) for v in SOURCES)))
    self.use_random_scale = bool(_flag(config, "use_random_scale"))
    self.pre_factor = None
    if source == "original":
      if not _flag(config, "pre_scale_all"):
        raise ValueError("source='original' is for pre_scale_all: without the flag the resident images are the ones "
                         "the crop is cut from (source='resident')")
      self.pre_factor = float(config.pre_scale_factor)
      if not 0 < self.pre_factor < 1:
        raise ValueError("pre_scale_factor: %r, must lie within (0, 1) (cocostuff.py:114 asserts < 1.)"
                         % (config.pre_scale_factor,))
    elif _flag(config, "pre_scale_all") and self.use_random_scale:
      raise NotImplementedError("pre_scale_all with use_random_scale is not built: the reference resizes the untruncated "
                                "float image a second time, which the resident uint8 (pre-scaled, truncated) image "
                                "cannot reproduce")
    if source == "resident" and _flag(config, "pre_scale_all") and not prescaled:
      raise NotImplementedError("pre_scale_all inside the kernel is not built: keep the pre-scaled, truncated "
                                "images (labels: NEAREST) resident and pass those")
    self.S = int(config.input_sz)
    if self.S % 4 != 0:
      raise NotImplementedError("input_sz must be a multiple of 4 (16-byte stores); the published runs use 128 and 200")
    if (labels is None) != (relevance is None):
      raise ValueError("labels and relevance go together: give both (COCO-Stuff) or neither (mask of ones)")
    if isinstance(images, (list, tuple)):
      if sizes is not None or offsets is not None:
        raise ValueError("sizes / offsets describe an already packed tensor; a list of images carries its own")
      if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
      pixels, lab, sizes, offsets = pack_images(images, labels)
      images = torch.from_numpy(pixels).to(device)
      labels = None if lab is None else torch.from_numpy(lab).to(device)
    else:
      if not torch.is_tensor(images) or images.dtype != torch.uint8:
        raise TypeError("images: a list of uint8 [h, w, Cs] arrays or the packed uint8 [total, Cs] tensor")
      if sizes is None:
        raise ValueError("sizes: required with a packed images tensor, int [B, 2] = (h, w) of every image")
    if images.dim() != 2 or int(images.shape[1]) not in (3, 4) or not images.is_contiguous():
      raise ValueError("images: Cs must be 3 (RGB) or 4 (RGB + IR) -- packed shape [total, Cs], contiguous; got %s"
                       % (tuple(images.shape),))
    self.images = images
    self.total, self.Cs = int(images.shape[0]), int(images.shape[1])
    sz, off = check_pack(self.total, sizes, offsets)
    self.B = int(sz.shape[0])
    self.sizes_host, self.offsets_host = sz, off
    # (h, w) before the random scale: the stored extent, or the pre-scaled one
    self.base_extent = sz if self.pre_factor is None else scaled_len(sz, self.pre_factor)
    dev = images.device
    self.sizes = torch.from_numpy(sz.astype(np.int32)).to(dev)
    self.offsets = torch.from_numpy(off).to(dev)
    self.labels = self.relevance = None
    if labels is not None:
      if not torch.is_tensor(labels) or labels.dtype != torch.uint8:
        raise TypeError("labels: the packed uint8 [total] tensor (255 for -1)")
      if tuple(labels.shape) != (self.total,) or labels.device != dev or not labels.is_contiguous():
        raise ValueError("labels: one byte per pixel of images, shape [%d] on %s" % (self.total, dev))
      rel = np.ascontiguousarray(_host(relevance).astype(np.uint8).reshape(-1))
      if rel.shape != (256,):
        raise ValueError("relevance: the 256-entry table of relevance_table")
      self.labels = labels
      self.relevance = torch.from_numpy(rel).to(dev)
    if self.use_random_scale:
      self.scale_min, self.scale_max = float(config.scale_min), float(config.scale_max)
      if not 0 < self.scale_min <= self.scale_max:
        raise ValueError("scale_min / scale_max: need 0 < scale_min <= scale_max")
    self._read_flags(config, seed, dev)
    # F.affine_grid's base grid for align_corners=False, made by torch itself (linear_grid: linspace * (n - 1) / n)
    self.base_grid = (torch.linspace(-1, 1, self.S) * (self.S - 1) / self.S).to(dev)

  def extents(self, idx, scale=None):
    """(h, w) the crop is drawn on, int64 [n, 2]: the image's own (source="original": its pre-scaled extent), or
    cvRound(len * scale) per side of that."""
    ext = self.base_extent[np.asarray(idx, np.int64).reshape(-1)]
    return ext if scale is None else scaled_len(ext, np.asarray(scale, np.float64).reshape(-1, 1))

  def draw(self, idx):
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    n = idx.shape[0]
    assert n > 0 and idx.min() >= 0 and idx.max() < self.B, "source index out of range"
    S, r = self.S, self.rng
    ip = np.zeros((n, IPARAMS), np.int32)
    fp64 = np.zeros((n, 4), np.float64)
    fp = np.zeros((n, FPARAMS), np.float32)
    coords = np.zeros((n, 2), np.int64)
    extent = np.zeros((n, 2), np.int64)
    hue = np.zeros(n, np.float64)
    scale = np.ones(n, np.float64) if self.use_random_scale else None
    a12 = np.zeros((n, 2, 3), np.float32) if self.use_random_affine else None
    half = int(S / 2.)
    ip[:, 0] = idx
    fp[:, 4], fp[:, 8] = 1.0, 1.0                               # identity affine2_to_1
    for i in range(n):
      h, w = (int(v) for v in self.base_extent[idx[i]])
      if self.use_random_scale:
        scale[i] = r.rand() * (self.scale_max - self.scale_min) + self.scale_min
        h, w = int(scaled_len(h, scale[i])), int(scaled_len(w, scale[i]))
      extent[i] = (h, w)
      new_h, new_w, _, _ = pad_offsets(h, w, S)
      h_lo, h_hi, w_lo, w_hi = crop_centre_range(new_h, new_w, S)
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
    return dict(iparams=ip, fparams=fp, coords=coords, hue=hue, affine1_to_2=a12, scale=scale, extent=extent)

  def apply(self, params):
    iparams = np.ascontiguousarray(params["iparams"], dtype=np.int32)
    fparams = np.ascontiguousarray(params["fparams"], dtype=np.float32)
    a12, scale = params.get("affine1_to_2"), params.get("scale")
    n, S = int(iparams.shape[0]), self.S
    assert iparams.shape == (n, IPARAMS) and fparams.shape == (n, FPARAMS)
    assert n > 0 and iparams[:, 0].min() >= 0 and iparams[:, 0].max() < self.B, "source index out of range"
    assert (scale is not None) == self.use_random_scale, "params['scale'] goes with use_random_scale"
    if scale is not None:
      scale = np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
      assert scale.shape == (n,) and (scale > 0).all() and np.isfinite(scale).all()
    ext = self.extents(iparams[:, 0], scale)
    padded = np.maximum(ext, S)
    assert (iparams[:, 1] >= 0).all() and (iparams[:, 1] + S <= padded[:, 1]).all(), "crop outside the (padded) image"
    assert (iparams[:, 2] >= 0).all() and (iparams[:, 2] + S <= padded[:, 0]).all(), "crop outside the (padded) image"
    assert (iparams[:, 4] >= 0).all() and (iparams[:, 4] <= 4).all()
    assert (iparams[:, 5:9] >= 0).all() and (iparams[:, 5:9] <= 3).all()
    assert ((iparams[:, 3] & ~1) == 0).all(), "flip is one bit"
    assert self.images.is_cuda, "the dataset must be resident on the GPU (there is no CPU path)"
    assert (a12 is not None) == self.use_random_affine
    dev = self.images.device
    C = self.out_channels
    if a12 is not None:
      iparams = iparams.copy()
      iparams[:, 3] |= 2                   # the mirror of img2 is folded into the warp below
    taps = taps2 = None
    src = self.sizes_host[iparams[:, 0]]
    if self.pre_factor is not None and scale is not None:         # two resizes: pre_scale_all, then the random scale
      t = np.stack([crop_taps2(src[:, 0], self.pre_factor, scale, iparams[:, 2], S),
                    crop_taps2(src[:, 1], self.pre_factor, scale, iparams[:, 1], S)], 1)
      taps2 = torch.from_numpy(np.ascontiguousarray(t).view(np.int32).reshape(n, 2, S, 12)).to(dev, non_blocking=True)
    elif self.pre_factor is not None or scale is not None:        # one resize: by pre_scale_factor, or by the random scale
      one = np.full(n, self.pre_factor, np.float64) if scale is None else scale
      t = np.stack([crop_taps(src[:, 0], one, iparams[:, 2], S), crop_taps(src[:, 1], one, iparams[:, 1], S)], 1)
      taps = torch.from_numpy(np.ascontiguousarray(t).view(np.int32).reshape(n, 2, S, 6)).to(dev, non_blocking=True)
    ip = torch.from_numpy(iparams).to(dev, non_blocking=True)
    fp = torch.from_numpy(fparams).to(dev, non_blocking=True)
    img1 = torch.empty(n, C, S, S, device=dev, dtype=torch.float32)
    img2 = torch.empty(n, C, S, S, device=dev, dtype=torch.float32)
    mask = torch.empty(n, S, S, device=dev, dtype=torch.uint8)
    aff = torch.empty(n, 2, 3, device=dev, dtype=torch.float32)
    entry, name = ((_lib.lib().iic_seg_augment_ragged, "iic_seg_augment_ragged") if taps2 is None else
                   (_lib.lib().iic_seg_augment_ragged_prescaled, "iic_seg_augment_ragged_prescaled"))
    _lib.check(entry(
      self.images.data_ptr(), self.offsets.data_ptr(), self.sizes.data_ptr(), self.B, self.total, self.Cs,
      _lib.ptr(self.labels), _lib.ptr(self.relevance), ip.data_ptr(), fp.data_ptr(), _lib.ptr(taps if taps2 is None else taps2),
      n, S, int(self.no_sobel), int(self.include_rgb), self.lut.data_ptr(), img1.data_ptr(), img2.data_ptr(),
      mask.data_ptr(), aff.data_ptr(), _lib.stream_ptr()), name)
    if a12 is not None:
      img2 = self._grid_warp(img2, a12, iparams[:, 3] & 1)
    return img1, img2, aff, mask

  def _grid_warp(self, img2, a12, flips):
    """img2 = flip(perform_affine_tf(img2, affine1_to_2)) as one iic_seg_augment_warp launch: F.affine_grid +
    F.grid_sample restated in torch's CPU operation order, bit-identical to the reference on the fixture (the uniform
    augmenter's iic_affine_warp_fwd is within 2e-6 of it)."""
    n, C = int(img2.shape[0]), int(img2.shape[1])
    dev = img2.device
    theta = torch.from_numpy(np.ascontiguousarray(a12, dtype=np.float32).reshape(n, 6)).to(dev, non_blocking=True)
    fl = torch.from_numpy(np.ascontiguousarray(flips, dtype=np.int32)).to(dev, non_blocking=True)
    warped = torch.empty_like(img2)
    _lib.check(_lib.lib().iic_seg_augment_warp(img2.data_ptr(), theta.data_ptr(), fl.data_ptr(), self.base_grid.data_ptr(),
                                               warped.data_ptr(), n, C, self.S, _lib.stream_ptr()), "iic_seg_augment_warp")
    return warped

  def paired_batch(self, idx):
    """What one iteration of ONE of the reference's paired dataloaders yields
    (code/scripts/segmentation/segmentation_twohead.py:283): img1, img2, affine2_to_1, mask_img1."""
    return self.apply(self.draw(idx))
