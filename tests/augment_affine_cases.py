"""RandomAffine of sobel_make_transforms (code/utils/cluster/transforms.py:152-161) for the tests of
csrc/augment_affine.hip: the matrix, the pixel arithmetic as a numpy specification, Pillow's own transform, the case
list, and the oracle composed from them and oracle/augment_oracle.py (TEST INFRASTRUCTURE, never imported by iic_amd/).

torchvision is absent here.  Its 0.2.1 RandomAffine is restated below over PIL: RandomApply(p) +
RandomAffine.get_params (angle, np.round-ed translations, scale, shear), F._get_inverse_affine_matrix with
center = (w * 0.5 + 0.5, h * 0.5 + 0.5), then img.transform(img.size, Image.AFFINE, matrix, Image.BILINEAR, fillcolor=0).

PINNING.  `pil_affine` calls the Pillow installed here (12.2.0); the reference's environment pins Pillow 5.2.0
(package_versions.txt), which is not available offline, and the torchvision restatement is from the 0.2.1 sources, not
executed: with respect to both, this part stays "parity unpinned", as oracle/augment_oracle.py says of the other
operations.  What IS checked: np_affine_bilinear == Pillow's transform bit for bit on the whole case list
(tests/test_augment_affine_cpu.py), and the kernel == the composed PIL oracle (tests/test_gpu_augment_affine.py).

The case list has two families, because each catches what the other cannot (test_augment_affine_cpu.py seeds the
defects and counts): reference-distribution draws on natural / random crops flip under fused or float32 COORDINATES,
crops of 0 / 255 pixels under translations n + j / 255 flip under a fused INTERPOLATION (255 * (j / 255) sits on the
truncation's edge).  The fused operation is emulated in 80-bit long double: an 8-bit difference times a double is exact
there, so the emulation differs from a true fma only by the final double rounding of the sum.
"""
import math
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from oracle import augment_oracle as ao   # noqa: E402

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
DEFECTS = ("fused_interpolation", "fused_coordinates", "float32_coordinates", "round_to_nearest_store",
           "range_test_after_shift", "neighbours_beyond_crop", "no_row_below_rule")


# ------------------------------------------------------------------------------------------
# torchvision 0.2.1 on PIL
# ------------------------------------------------------------------------------------------
def inverse_affine_matrix(center, angle, translate, scale, shear):
  """F._get_inverse_affine_matrix (torchvision 0.2.1), Python doubles."""
  angle = math.radians(angle)
  shear = math.radians(shear)
  scale = 1.0 / scale
  d = math.cos(angle + shear) * math.cos(angle) + math.sin(angle + shear) * math.sin(angle)
  matrix = [math.cos(angle + shear), math.sin(angle + shear), 0, -math.sin(angle), math.cos(angle), 0]
  matrix = [scale / d * m for m in matrix]
  matrix[2] += matrix[0] * (-center[0] - translate[0]) + matrix[1] * (-center[1] - translate[1])
  matrix[5] += matrix[3] * (-center[0] - translate[0]) + matrix[4] * (-center[1] - translate[1])
  matrix[2] += center[0]
  matrix[5] += center[1]
  return matrix


def crop_center(crop):
  """F.affine: center = (img.size[0] * 0.5 + 0.5, img.size[1] * 0.5 + 0.5)."""
  return (crop * 0.5 + 0.5, crop * 0.5 + 0.5)


def random_affine_params(rng, crop, degrees=18, translate=(0.1, 0.1), scale=(0.9, 1.1), shear=10):
  """RandomAffine.get_params with img_size = (crop, crop)."""
  angle = rng.uniform(-degrees, degrees)
  tx = np.round(rng.uniform(-translate[0] * crop, translate[0] * crop))
  ty = np.round(rng.uniform(-translate[1] * crop, translate[1] * crop))
  return float(angle), (float(tx), float(ty)), float(rng.uniform(scale[0], scale[1])), float(rng.uniform(-shear, shear))


def pil_affine(crop_u8, m):
  """Pillow's own img.transform(img.size, AFFINE, m, BILINEAR, fillcolor=0) of an HWC uint8 RGB crop."""
  img = Image.fromarray(np.ascontiguousarray(crop_u8))
  out = img.transform(img.size, Image.AFFINE, tuple(float(v) for v in m), Image.BILINEAR, fillcolor=0)
  return np.asarray(out)


# ------------------------------------------------------------------------------------------
# the same arithmetic, step by step (specification of aug_affine_bilinear in csrc/aug_stages.h)
# ------------------------------------------------------------------------------------------
def _fma(a, b, c):
  """a * b + c rounded once (80-bit emulation, see the module docstring)."""
  ld = np.longdouble
  return (np.asarray(a, ld) * np.asarray(b, ld) + np.asarray(c, ld)).astype(np.float64)


def np_affine_bilinear(crop_u8, m, defect=None, source=None, origin=None):
  """Geometry.c: ImagingGenericTransform + affine_transform + bilinear_filter32RGB, IEEE double, every multiply and add
  on its own.  crop_u8 HWC uint8 (square or not), m the six inverse coefficients.  defect: None, or one of DEFECTS --
  a deliberately WRONG variant, for the tests that show the case list can tell.  'neighbours_beyond_crop' needs the
  dataset image `source` (HWC) and the crop's `origin` (x0, y0) in it."""
  assert defect is None or defect in DEFECTS
  h, w = crop_u8.shape[:2]
  p = crop_u8.astype(np.int64)
  m0, m1, m2, m3, m4, m5 = (float(v) for v in m)
  y, x = np.mgrid[0:h, 0:w]
  xin, yin = x + 0.5, y + 0.5
  if defect == "fused_coordinates":
    X = _fma(m0, xin, _fma(m1, yin, m2))
    Y = _fma(m3, xin, _fma(m4, yin, m5))
  elif defect == "float32_coordinates":
    f = np.float32
    X = ((f(m0) * xin.astype(f) + f(m1) * yin.astype(f)) + f(m2)).astype(np.float64)
    Y = ((f(m3) * xin.astype(f) + f(m4) * yin.astype(f)) + f(m5)).astype(np.float64)
  else:
    X = (m0 * xin + m1 * yin) + m2
    Y = (m3 * xin + m4 * yin) + m5
  if defect == "range_test_after_shift":
    inside = (X - 0.5 >= 0) & (X - 0.5 < w) & (Y - 0.5 >= 0) & (Y - 0.5 < h)
  else:
    inside = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)          # tested BEFORE the half-pixel shift
  X, Y = np.where(inside, X, 0.5) - 0.5, np.where(inside, Y, 0.5) - 0.5
  xf, yf = np.floor(X), np.floor(Y)
  dx, dy = X - xf, Y - yf
  xf, yf = xf.astype(np.int64), yf.astype(np.int64)             # may be -1

  if defect == "neighbours_beyond_crop":
    # the neighbours of an edge pixel taken from the dataset image around the crop instead of the clamped crop
    ox, oy = origin
    sp = source.astype(np.int64)
    sh, sw = sp.shape[:2]

    def px(yy, xx):
      return sp[np.clip(oy + yy, 0, sh - 1), np.clip(ox + xx, 0, sw - 1)]
    below = np.ones_like(inside)
  else:
    def px(yy, xx):
      return p[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
    below = (yf + 1 >= 0) & (yf + 1 < h)

  def lerp(a, b, d):
    if defect == "fused_interpolation":
      return _fma((b - a).astype(np.float64), d[..., None], a.astype(np.float64))
    return a + (b - a) * d[..., None]
  v1 = lerp(px(yf, xf), px(yf, xf + 1), dx)
  if defect == "no_row_below_rule":
    # the absent row below the last one read as fill (zero) instead of v2 = v1.  (Clamping it to the last row gives
    # v2 == v1 as well: that variant is no defect.)
    v2 = np.where(below[..., None], lerp(px(yf + 1, xf), px(yf + 1, xf + 1), dx), 0.0)
  else:
    v2 = np.where(below[..., None], lerp(px(yf + 1, xf), px(yf + 1, xf + 1), dx), v1)
  if defect == "fused_interpolation":
    v = _fma(v2 - v1, dy[..., None], v1)
  else:
    v = v1 + (v2 - v1) * dy[..., None]
  if defect == "round_to_nearest_store":
    v = np.floor(v + 0.5)
  out = v.astype(np.int64)                                      # (UINT8) v: truncation, 0 <= v <= 255
  return np.where(inside[..., None], out, 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------
# dataset and case list
# ------------------------------------------------------------------------------------------
N_IMAGES = 8
BINARY_IMAGES = (3, 4)       # 0 / 255 pixels: the structured family's sources


def dataset(H, W, seed=0):
  """uint8 [8, H, W, 3]: noise, a smooth image, a grey one, two of 0 / 255 pixels, white, noise, a ramp."""
  rng = np.random.default_rng(1000 + seed)
  imgs = rng.integers(0, 256, (N_IMAGES, H, W, 3), dtype=np.uint8)
  y, x = np.mgrid[0:H, 0:W]
  imgs[1] = np.clip(np.stack([127 + 120 * np.sin(x / 9.0 + y / 17.0), 127 + 120 * np.cos(x / 5.0),
                              (x * y) % 256], -1), 0, 255).astype(np.uint8)
  imgs[2] = np.repeat(imgs[2][:, :, :1], 3, 2)
  imgs[3] = np.repeat(rng.integers(0, 2, (H, W, 1), dtype=np.uint8) * 255, 3, 2)
  imgs[4] = rng.integers(0, 2, (H, W, 3), dtype=np.uint8) * 255
  imgs[5] = 255
  imgs[7] = np.stack([(x * 7 + y) % 256, (x + y * 5) % 256, (x * 3 + y * 3) % 256], -1).astype(np.uint8)
  return imgs


def case_list(crop, H, W, seed, n_draws=24, n_structured=14):
  """Rows of one launch for crops of side `crop` out of H x W images: list of dicts with
  src (image index), xy (crop origin), m (six floats, or None: a plain row, no affine), name.
  Family (i): reference-distribution draws; family (ii): 0 / 255 crops under translations n + j / 255; hand-made rows."""
  rng = np.random.default_rng(seed)
  c = crop_center(crop)
  rows = []

  def add(name, m, src=None):
    src = int(rng.integers(0, N_IMAGES)) if src is None else src
    xy = (int(rng.integers(0, W - crop + 1)), int(rng.integers(0, H - crop + 1)))
    rows.append(dict(name=name, src=src, xy=xy, m=None if m is None else tuple(float(v) for v in m)))
  for i in range(n_draws):                                    # (i)
    add("draw%d" % i, inverse_affine_matrix(c, *random_affine_params(rng, crop)),
        src=(0, 1, 6, 7, 2)[i % 5])
  for i in range(n_structured):                               # (ii)
    n, j = int(rng.integers(-3, 4)), int(rng.integers(1, 255))
    n2, j2 = int(rng.integers(-3, 4)), int(rng.integers(1, 255))
    ty = (0.0, n2 + j2 / 255.0, float(n2))[i % 3]
    add("structured%d" % i, (1.0, 0.0, n + j / 255.0, 0.0, 1.0, ty), src=BINARY_IMAGES[i % 2])
  add("identity", IDENTITY)
  add("identity_draw", inverse_affine_matrix(c, 0.0, (0.0, 0.0), 1.0, 0.0))
  add("shift_int", (1.0, 0.0, 2.0, 0.0, 1.0, -3.0))
  add("shift_half_up", (1.0, 0.0, 0.5, 0.0, 1.0, 0.5), src=0)      # X exactly w at the last column
  add("shift_half_down", (1.0, 0.0, -0.5, 0.0, 1.0, -0.5), src=0)  # X exactly 0 at the first column
  add("shift_edge", (1.0, 0.0, float(crop - 1), 0.0, 1.0, float(1 - crop)), src=1)
  add("all_out", (1.0, 0.0, float(crop + 1), 0.0, 1.0, 0.0), src=5)
  add("scale_half", inverse_affine_matrix(c, 0.0, (0.0, 0.0), 0.5, 0.0), src=1)
  add("scale_two", inverse_affine_matrix(c, 0.0, (0.0, 0.0), 2.0, 0.0), src=0)
  add("plain", None)
  return rows


# (H, W, crop, S, include_rgb) of the launches, CPU and GPU tests alike
SHAPES = [(40, 40, 36, 24, True), (32, 32, 20, 24, False), (40, 48, 36, 40, True), (96, 96, 84, 96, True)]


def shape_cases(shape):
  H, W, crop, S, include_rgb = shape
  return dataset(H, W, seed=crop + S), case_list(crop, H, W, seed=H * 1000 + W * 10 + S)


# ------------------------------------------------------------------------------------------
# kernel parameters and the composed oracle
# ------------------------------------------------------------------------------------------
def jitter_rows(rng, n, jitter=(0.4, 0.4, 0.4, 0.125)):
  """flip, op order and factors per row: RandomHorizontalFlip + ColorJitter.get_params, full jitter."""
  out = []
  for _ in range(n):
    b, c, s, h = jitter
    factors = {ao.OP_BRIGHTNESS: float(np.float32(rng.uniform(1 - b, 1 + b))),
               ao.OP_CONTRAST: float(np.float32(rng.uniform(1 - c, 1 + c))),
               ao.OP_SATURATION: float(np.float32(rng.uniform(1 - s, 1 + s))),
               ao.OP_HUE: float(np.float32(rng.uniform(-h, h)))}
    out.append(dict(flip=bool(rng.random() < 0.5), order=[int(o) for o in rng.permutation(4)], factors=factors))
  return out


def kernel_params(rows, jit, table=0, cutout_boxes=None):
  """(iparams int32 [n, 20], fparams float32 [n, 4], aparams float64 [n, 6]) of the rows, as iic_augment_affine reads
  them (include/iic_hip.h)."""
  n = len(rows)
  ip, fp, ap = np.zeros((n, 20), np.int32), np.zeros((n, 4), np.float32), np.zeros((n, 6), np.float64)
  for i, (r, j) in enumerate(zip(rows, jit)):
    ip[i, 0], ip[i, 1], ip[i, 2], ip[i, 3] = r["src"], r["xy"][0], r["xy"][1], int(j["flip"])
    ip[i, 4] = len(j["order"])
    ip[i, 5:5 + len(j["order"])] = j["order"]
    for op, f in j["factors"].items():
      fp[i, op] = f
    ip[i, 9] = ao.hue_delta(float(fp[i, 3]))
    ip[i, 10] = table if np.isscalar(table) else table[i]
    if r["m"] is not None:
      ip[i, 11] |= 2
      ap[i] = r["m"]
    if cutout_boxes is not None and cutout_boxes[i] is not None:
      l, u, rr, lo = cutout_boxes[i]
      ip[i, 18], ip[i, 19] = l | (u << 16), rr | (lo << 16)
  return ip, fp, ap


def composed_oracle(img_u8, xy, crop, S, include_rgb, m, jit, angle=None, cutout_box=None, norm=None):
  """tf2 with the affine for one row: [rotate the whole image, PIL NEAREST] -> crop -> pil_affine -> the existing
  oracle on the affined crop (the crop of a crop-sized image is the identity): cutout, Resize, flip, ColorJitter,
  custom_greyscale_to_tensor, Normalize."""
  img = Image.fromarray(img_u8)
  if angle is not None:
    img = img.rotate(angle, Image.NEAREST, False, None)
  x0, y0 = xy
  a = np.asarray(img.crop((x0, y0, x0 + crop, y0 + crop)))
  if m is not None:
    a = pil_affine(a, m)
  return ao.pil_pipeline(a, (0, 0), crop, S, include_rgb, jit["flip"], jit["order"], jit["factors"],
                         cutout_box=cutout_box, norm=norm)
