"""The reference-generated fixture tests/golden/seg_prescale.npz (tools/gen_golden_seg_prescale.py: the reference's own
`_prepare_train` with pre_scale_all on, ORIGINAL-resolution sources) as augmenters and parameter dictionaries, plus the
host pipeline both tests/test_seg_prescale_cpu.py and tests/test_gpu_seg_prescale.py compare against.  The fixture has
the keys of the ragged one, so its accessors are tests/seg_ragged_cases.py's, bound to the other file."""
import importlib.util
import os

import numpy as np

from tests import seg_ragged_cases as _ragged

# a second instance of the accessor module, reading this fixture (the module keeps its file name and cache in globals)
_spec = importlib.util.spec_from_file_location("tests._seg_prescale_fixture", _ragged.__file__)
_fx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_fx)
_fx.G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_prescale.npz")

fixture, names, meta, config, images, expected, recorded_params, take = (
  _fx.fixture, _fx.names, _fx.meta, _fx.config, _fx.images, _fx.expected, _fx.recorded_params, _fx.take)


def augmenter(name, device="cpu", **overrides):
  """SegRaggedAugmenter over the case's ORIGINAL images: the kernel pre-scales."""
  from iic_amd import seg_ragged
  imgs, labels, rel = images(name)
  return seg_ragged.SegRaggedAugmenter(imgs, config(name, **overrides), labels=labels, relevance=rel, device=device,
                                       source="original")


# ------------------------------------------------------------------------------------------
# the host pipeline: `_prepare_train` from the original image to the four tensors, in numpy / PIL
# ------------------------------------------------------------------------------------------
def jitter_host(rgb_u8, ops, factors, hue_delta):
  """torchvision 0.2.1 ColorJitter on one uint8 [S, S, 3] crop, through PIL as the reference runs it: ops in application
  order (0 brightness, 1 contrast, 2 saturation, 3 hue), factors indexed by op, the hue shift as its uint8 delta."""
  from PIL import Image, ImageEnhance
  img = Image.fromarray(np.ascontiguousarray(rgb_u8))
  for op in ops:
    if op == 0:
      img = ImageEnhance.Brightness(img).enhance(float(factors[0]))
    elif op == 1:
      img = ImageEnhance.Contrast(img).enhance(float(factors[1]))
    elif op == 2:
      img = ImageEnhance.Color(img).enhance(float(factors[2]))
    else:
      h, s, v = img.convert("HSV").split()
      h = Image.fromarray(((np.array(h, dtype=np.uint8).astype(np.int64) + int(hue_delta)) % 256).astype(np.uint8), "L")
      img = Image.merge("HSV", (h, s, v)).convert("RGB")
  return np.asarray(img)


def resized_crop(img_u8, label_u8, factors, S, y0, x0):
  """cv2.resize by every factor in turn on the FLOAT image (labels NEAREST), pad_if_too_small, the S x S crop at (y0, x0)
  of the padded image: (float32 [S, S, Cs] untruncated, uint8 [S, S] labels or None)."""
  from iic_amd import seg_augment as sa, seg_ragged as sr
  img, lab = img_u8.astype(np.float32), label_u8
  for f in factors:
    img = sr.resize_linear_host(img, f)
    lab = None if lab is None else sr.resize_nearest_host(lab, f)
  h, w, cs = img.shape
  new_h, new_w, oy, ox = sa.pad_offsets(h, w, S)
  pad = np.zeros((new_h, new_w, cs), np.float32)
  pad[oy:oy + h, ox:ox + w] = img
  crop = pad[y0:y0 + S, x0:x0 + S]
  if lab is not None:
    lpad = np.zeros((new_h, new_w), np.uint8)
    lpad[oy:oy + h, ox:ox + w] = lab
    lab = lpad[y0:y0 + S, x0:x0 + S]
  assert crop.shape[:2] == (S, S)
  return crop, lab


def host_pipeline(imgs, labels, rel, cfg, params, pre_factor):
  """[(img1, img2, affine2_to_1, mask_img1)] per sample of `params`, the way the reference computes them: resize by
  pre_factor (None: not at all), then by params["scale"], crop, truncate RGB (never IR), jitter, grey, / 255., random
  affine, flip."""
  from iic_amd import seg_augment as sa, seg_ragged as sr
  S = int(cfg.input_sz)
  ip, fp, scale, a12 = params["iparams"], params["fparams"], params.get("scale"), params.get("affine1_to_2")
  out = []
  for k in range(ip.shape[0]):
    src = int(ip[k, 0])
    factors = ([] if pre_factor is None else [pre_factor]) + ([] if scale is None else [float(scale[k])])
    crop, lab = resized_crop(imgs[src], None if labels is None else labels[src], factors, S, int(ip[k, 2]), int(ip[k, 1]))
    rgb = crop[:, :, :3].astype(np.uint8)
    nj = int(ip[k, 4])
    rgb2 = jitter_host(rgb, [int(o) for o in ip[k, 5:5 + nj]], fp[k, :3], int(ip[k, 9]))

    def layout(v):
      if not cfg.no_sobel:
        grey = sa.cv_grey(v)[:, :, None]
        v = np.concatenate([v, grey], axis=2) if cfg.include_rgb else grey
      v = v.astype(np.float32) / 255.
      if crop.shape[2] == 4:
        v = np.concatenate([v, (crop[:, :, 3] / np.float32(255.))[:, :, None]], axis=2)
      return np.ascontiguousarray(v.transpose(2, 0, 1))
    img1, img2 = layout(rgb), layout(rgb2)
    flip = bool(ip[k, 3] & 1)
    if a12 is not None:
      img2 = sr.grid_warp_host(img2, a12[k], flip)
    elif flip:
      img2 = np.ascontiguousarray(img2[:, :, ::-1])
    aff = fp[k, 4:10].reshape(2, 3).copy()
    if flip:
      aff[0, :] *= np.float32(-1.)
    mask = np.ones((S, S), np.uint8) if lab is None else np.asarray(rel, np.uint8)[lab]
    out.append((img1, img2, aff, np.ascontiguousarray(mask)))
  return out


def emulate_taps2(img_u8, label_u8, ty, tx, truncate_between=False):
  """csrc/seg_augment.hip's two-stage fetch in numpy, from one sample's row and column tables (TAP2_DTYPE [S] each):
  (float32 [S, S, Cs] before truncation, zero in the padding; uint8 [S, S] labels or None).  truncate_between: the
  DEFECT a resident pre-scaled uint8 image would introduce -- the intermediate pixels truncated to uint8."""
  v = img_u8.astype(np.float32)

  def stage1(i, j):      # the pre-scaled image at the second stage's tap (i of the rows, j of the columns)
    y0, y1, x0, x1 = ty["i0"][:, i], ty["i1"][:, i], tx["i0"][:, j], tx["i1"][:, j]
    ax0, ax1 = tx["a0"][None, :, j, None], tx["a1"][None, :, j, None]
    by0, by1 = ty["a0"][:, i, None, None], ty["a1"][:, i, None, None]
    top = v[y0][:, x0] * ax0 + v[y0][:, x1] * ax1
    bot = v[y1][:, x0] * ax0 + v[y1][:, x1] * ax1
    m = top * by0 + bot * by1
    assert m.dtype == np.float32
    return m.astype(np.uint8).astype(np.float32) if truncate_between else m
  bx0, bx1 = tx["b0"][None, :, None], tx["b1"][None, :, None]
  top = stage1(0, 0) * bx0 + stage1(0, 1) * bx1
  bot = stage1(1, 0) * bx0 + stage1(1, 1) * bx1
  val = top * ty["b0"][:, None, None] + bot * ty["b1"][:, None, None]
  assert val.dtype == np.float32
  inside = (ty["inside"][:, None] & tx["inside"][None, :]).astype(bool)
  val = np.where(inside[:, :, None], val, np.float32(0))
  lab = None if label_u8 is None else np.where(inside, label_u8[ty["nearest"]][:, tx["nearest"]], np.uint8(0))
  return val, lab
