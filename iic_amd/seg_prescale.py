"""pre_scale_all of a segmentation dataset as a pass on the GPU, made once.

Host side of csrc/seg_prescale.hip (C ABI `iic_seg_prescale`).  Every published COCO-Stuff command sets
`--pre_scale_all --pre_scale_factor 0.33` (examples/commands.txt 2.1, 2.2), and the reference shrinks each image on
EVERY access: cv2.resize(fx = fy = factor) with INTER_LINEAR on the float image and INTER_NEAREST on the labels
(code/datasets/segmentation/cocostuff.py:113-120, :242-249, :321-328; potsdam.py:103-106).  `prescale_dataset` does it
once for the whole set and returns what the resident-data classes take:

    pixels, labels, sizes, offsets = prescale_dataset(originals, labels=label_maps, factor=0.33)        # packed
    aug = SegRaggedAugmenter(pixels, config, labels=labels, relevance=rel, sizes=sizes, offsets=offsets)
    images, labels, sizes = prescale_dataset(originals, labels=label_maps, factor=0.33, layout="slab")
    prep = SegTestPreparer(images, labels, config, targets, relevance=rel, sizes=sizes)

The image is truncated toward zero to uint8, which is what `img.astype(np.uint8)` does to the training crop
(cocostuff.py:170; truncation and cropping commute), so a SegRaggedAugmenter over the result gives the reference's
training tensors bit for bit as long as use_random_scale is off.  With use_random_scale the reference resizes the
UNTRUNCATED image again: that is SegRaggedAugmenter(originals, ..., source="original"), which keeps the originals
resident instead.  Test time: `_prepare_test` does not truncate after the resize and converts floats to grey; the
preparer works on the truncated image, at most 1/255 per channel below the reference's float.

The resize is OpenCV 3.x's, restated in seg_ragged.py (scaled_len, linear_taps, nearest_index) and NOT compared against a
cv2 binary; `prescale_host` is the numpy form of what the kernel computes, for tests and tools.
"""
import numpy as np
import torch

from . import _lib
from .seg_ragged import (check_pack, pack_images, resize_linear_host, resize_nearest_host, scaled_len)

LAYOUTS = ("packed", "slab")
ROWS_PER_ITEM = 8                 # output rows one workgroup resamples
CHUNK_PX = 1 << 26                # source pixels uploaded per launch from a list of host arrays (192 MiB of RGB)


def prescaled_sizes(sizes, factor):
  """(h', w') of every image after cv2.resize(fx = fy = factor), int64 [B, 2]: cvRound(len * factor) per side -- round
  half to even -- and at least 1."""
  return scaled_len(np.asarray(sizes, np.int64).reshape(-1, 2), factor)


def prescale_host(img_u8, label_u8, factor):
  """What the kernel computes for one image, in numpy: (uint8 [h', w', 3], uint8 [h', w'] or None)."""
  img_u8 = np.asarray(img_u8)
  assert img_u8.dtype == np.uint8 and img_u8.ndim == 3
  out = resize_linear_host(img_u8.astype(np.float32), factor).astype(np.uint8)
  return out, (None if label_u8 is None else resize_nearest_host(np.asarray(label_u8), factor))


def _check_factor(factor):
  factor = float(factor)
  if not 0 < factor < 1:
    raise ValueError("factor: %r, must lie within (0, 1) (cocostuff.py:114 asserts pre_scale_factor < 1.)" % (factor,))
  return factor


def _refuse_ir(cs):
  if cs == 4:
    raise ValueError("images: Cs = 4 (RGB + IR) cannot be pre-scaled to uint8 -- the reference never truncates the IR "
                     "plane after a resize (potsdam.py:148-151, :170); keep the originals resident and use "
                     "SegRaggedAugmenter(..., source=\"original\")")


def work_list(out_sizes, rows_per_item=ROWS_PER_ITEM):
  """The kernel's flat work list int32 [n, 3] = (image, first output row, row count): every image cut into runs of
  rows_per_item output rows."""
  nh = np.asarray(out_sizes, np.int64)[:, 0]
  per = (nh + rows_per_item - 1) // rows_per_item
  img = np.repeat(np.arange(nh.shape[0], dtype=np.int64), per)
  first = (np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)) * rows_per_item
  return np.ascontiguousarray(np.stack([img, first, np.minimum(rows_per_item, nh[img] - first)], 1).astype(np.int32))


def _launch(src, src_labels, src_sizes, src_offsets, factor, dst, dst_labels, dst_offsets, dst_pitch, dst_sizes):
  """One iic_seg_prescale launch: the B images of the source pack (device tensors, host tables) into their places."""
  dev = src.device
  assert src.is_cuda, "the dataset must be on the GPU (there is no CPU path)"
  work = work_list(dst_sizes)
  up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev, non_blocking=True)   # noqa: E731
  t = (up(src_offsets, np.int64), up(src_sizes, np.int32), up(dst_offsets, np.int64), up(dst_pitch, np.int32),
       up(dst_sizes, np.int32), up(work, np.int32))
  _lib.check(_lib.lib().iic_seg_prescale(
    src.data_ptr(), _lib.ptr(src_labels), t[0].data_ptr(), t[1].data_ptr(), int(src_sizes.shape[0]), int(src.shape[0]),
    factor, dst.data_ptr(), _lib.ptr(dst_labels), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
    int(dst_labels.numel() if dst_labels is not None else dst.numel() // 3), t[5].data_ptr(), int(work.shape[0]),
    _lib.stream_ptr()), "iic_seg_prescale")


def _chunks(area, chunk_px):
  """Runs [lo, hi) of consecutive images holding at most chunk_px source pixels (a larger image is a run of its own)."""
  lo, acc, runs = 0, 0, []
  for i, a in enumerate(area):
    if i > lo and acc + a > chunk_px:
      runs.append((lo, i))
      lo, acc = i, 0
    acc += int(a)
  runs.append((lo, len(area)))
  return runs


def prescale_dataset(images, sizes=None, offsets=None, labels=None, factor=None, layout="packed", chunk_px=None,
                     device=None):
  """The whole dataset resized by `factor` on the GPU (see the module docstring).

  images: the packed uint8 [total, 3] tensor on the device with sizes int [B, 2] and optional offsets int [B] (gaps
  allowed) and labels the packed uint8 [total] tensor, exactly as SegRaggedAugmenter takes them -- one launch; OR a list
  of uint8 [h_i, w_i, 3] host arrays with labels a list of uint8 [h_i, w_i] maps (255 for -1): uploaded in runs of at
  most chunk_px source pixels, one launch per run, each writing into its final place of ONE destination allocation, so
  that the original-resolution set is never resident as a whole.
  layout="packed" -> (pixels uint8 [total', 3], labels uint8 [total'] or None, sizes' int32 [B, 2], offsets' int64 [B]),
  the images back to back; layout="slab" -> (images uint8 [B, H', W', 3], labels uint8 [B, H', W'] or None, sizes'),
  image i in the top-left h'_i x w'_i of its slab, zeros elsewhere.  sizes' and offsets' are host tensors."""
  if factor is None:
    raise ValueError("factor: required, the reference's pre_scale_factor")
  factor = _check_factor(factor)
  if layout not in LAYOUTS:
    raise ValueError("layout: %r, expected one of %s" % (layout, ", ".join(repr(v) for v in LAYOUTS)))
  from_list = isinstance(images, (list, tuple))
  if from_list:
    if sizes is not None or offsets is not None:
      raise ValueError("sizes / offsets describe an already packed tensor; a list of images carries its own")
    if len(images) == 0:
      raise ValueError("images: the list is empty")
    if labels is not None and len(labels) != len(images):
      raise ValueError("labels: %d maps for %d images" % (len(labels), len(images)))
    for i, a in enumerate(images):
      if np.asarray(a.cpu() if torch.is_tensor(a) else a).dtype != np.uint8:
        raise TypeError("images[%d]: dtype %s, expected uint8" % (i, getattr(a, "dtype", type(a))))
      if getattr(a, "ndim", 0) == 3:
        _refuse_ir(int(a.shape[2]))
      if getattr(a, "ndim", 0) != 3 or int(a.shape[2]) != 3:
        raise ValueError("images[%d]: shape %s, expected [h, w, 3]" % (i, tuple(getattr(a, "shape", ()))))
    sz, _ = check_pack(sum(int(a.shape[0]) * int(a.shape[1]) for a in images), [a.shape[:2] for a in images])
    if device is None:
      device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    dev = torch.device(device)
    chunk_px = CHUNK_PX if chunk_px is None else int(chunk_px)
    if chunk_px < 1:
      raise ValueError("chunk_px: must be positive")
  else:
    if not torch.is_tensor(images) or images.dtype != torch.uint8:
      raise TypeError("images: a list of uint8 [h, w, 3] arrays or the packed uint8 [total, 3] tensor")
    if sizes is None:
      raise ValueError("sizes: required with a packed images tensor, int [B, 2] = (h, w) of every image")
    if images.dim() == 2:
      _refuse_ir(int(images.shape[1]))
    if images.dim() != 2 or int(images.shape[1]) != 3 or not images.is_contiguous():
      raise ValueError("images: packed shape [total, 3], contiguous; got %s" % (tuple(images.shape),))
    total = int(images.shape[0])
    sz, off = check_pack(total, sizes, offsets)
    dev = images.device
    if labels is not None:
      if not torch.is_tensor(labels) or labels.dtype != torch.uint8:
        raise TypeError("labels: the packed uint8 [total] tensor (255 for -1)")
      if tuple(labels.shape) != (total,) or labels.device != dev or not labels.is_contiguous():
        raise ValueError("labels: one byte per pixel of images, shape [%d] on %s" % (total, dev))
  B = int(sz.shape[0])
  nsz = prescaled_sizes(sz, factor)
  if layout == "packed":
    pitch = nsz[:, 1].copy()
    area = nsz[:, 0] * nsz[:, 1]
    doff = np.concatenate([[0], np.cumsum(area)[:-1]]).astype(np.int64)
    out = torch.empty(int(area.sum()), 3, device=dev, dtype=torch.uint8)
    out_labels = None if labels is None else torch.empty(int(area.sum()), device=dev, dtype=torch.uint8)
  else:
    H, W = int(nsz[:, 0].max()), int(nsz[:, 1].max())
    pitch = np.full(B, W, np.int64)
    doff = np.arange(B, dtype=np.int64) * (H * W)
    out = torch.zeros(B, H, W, 3, device=dev, dtype=torch.uint8)
    out_labels = None if labels is None else torch.zeros(B, H, W, device=dev, dtype=torch.uint8)
  if from_list:
    for lo, hi in _chunks(sz[:, 0] * sz[:, 1], chunk_px):
      px, lab, csz, coff = pack_images(images[lo:hi], None if labels is None else labels[lo:hi])
      _launch(torch.from_numpy(px).to(dev), None if lab is None else torch.from_numpy(lab).to(dev), csz, coff, factor,
              out, out_labels, doff[lo:hi], pitch[lo:hi], nsz[lo:hi])
  else:
    _launch(images, labels, sz, off, factor, out, out_labels, doff, pitch, nsz)
  sizes_out = torch.from_numpy(nsz.astype(np.int32))
  if layout == "packed":
    return out, out_labels, sizes_out, torch.from_numpy(doff)
  return out, out_labels, sizes_out
