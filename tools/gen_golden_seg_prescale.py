"""Generates tests/golden/seg_prescale.npz by EXECUTING the reference's own training `_prepare_train`
(code/datasets/segmentation/cocostuff.py:104-230, potsdam.py:95-216) with pre_scale_all ON, on small synthetic images of
different sizes.  Run where the reference tree exists (IIC_REFERENCE):

    python tools/gen_golden_seg_prescale.py

The recipe is tools/gen_golden_seg_augment_ragged.py's, imported: its stub modules, synthetic content, draw recording,
per-sample keys and metadata.  Only the case table differs: pre_scale_factor 0.33 (every published COCO-Stuff command,
examples/commands.txt 2.1 and 2.2) at input_sz 32, on source sizes whose pre-scaled extents straddle 32 --
50 x 72 -> 16 x 24, 61 x 150 -> 20 x 50, 150 x 61 -> 50 x 20, 97 x 97 -> 32 x 32, 100 x 142 -> 33 x 47,
185 x 121 -> 61 x 40 (all six in the published layout, three each in the other cases).  Sides 50 and 150 are among
them on purpose: 50 * 0.33 and 150 * 0.33 land on exact halves (16.5,
49.5), which cvRound rounds to even (16, 50).  Cases: COCO-Stuff-3 sobel (the published layout), COCO sobel + rgb, Potsdam
no-sobel with 4 channels, each with and without use_random_scale 0.6 .. 1.4; the scaled COCO sobel case also uses
use_random_affine.

WHAT THE FIXTURE DOES NOT VALIDATE.  cv2 is not installable here: `cv2.cvtColor` is OpenCV 3.x's 8-bit RGB2GRAY restated,
and `cv2.resize` is iic_amd.seg_ragged.resize_linear_host / resize_nearest_host, the project's restatement of OpenCV
3.x's resize -- the same one the kernels' coefficients come from.  The fixture therefore pins the ORDER of the
reference's operations (pre-scale, random scale, crop, truncate; IR never truncated), the extents the crop range is
computed on, the draw order (the scale first) and everything downstream -- ColorJitter, grey, channel layout, random
affine, flip, affine2_to_1, masks -- to the reference's own code.  The resampled PIXELS are pinned to the restatement
only, on both sides.

Per case and sample: the ORIGINAL-resolution source image (and label map), numpy's seed, every random draw and the four
returned tensors, under the keys of the ragged fixture ("<case>/<i>/<key>"; `extent` is the twice-scaled (h, w) the crop
was drawn on).  Arrays only.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import gen_golden_seg_augment_ragged as ragged  # noqa: E402  (installs the shims and the Python-2 hook)

FACTOR = 0.33
SIZES = ((50, 72), (61, 150), (150, 61), (97, 97), (100, 142), (185, 121))
# the sources are noise-like and do not compress: only the published layout carries all six, so that the file stays
# under 1 MB
SIZES_RGB = ((50, 72), (61, 150), (100, 142))
SIZES_IR = ((50, 72), (150, 61), (97, 97))
SIZES_SCALE = ((50, 72), (61, 150), (150, 61))
PJ, DJ = ragged.PJ, ragged.DJ


def _cfg(jitter, no_sobel, include_rgb, affine=False, scale=False):
  c = ragged._cfg(32, jitter, no_sobel, include_rgb, affine=affine, scale=scale)
  c.update(pre_scale_all=True, pre_scale_factor=FACTOR)
  return c


# name -> (dataset, config, ORIGINAL image sizes)
CASES = {
  "coco_sobel": ("coco_few", _cfg(DJ, False, False), SIZES),                                 # C = 1 (published)
  "coco_sobel_rgb": ("coco_full", _cfg(DJ, False, True), SIZES_RGB),                             # C = 4
  "potsdam_nosobel": ("potsdam", _cfg(PJ, True, False), SIZES_IR),                              # C = 4, IR untruncated
  "coco_sobel_scale_affine": ("coco_few", _cfg(DJ, False, False, affine=True, scale=True), SIZES_SCALE),
  "coco_sobel_rgb_scale": ("coco_full", _cfg(DJ, False, True, scale=True), SIZES_SCALE),
  "potsdam_nosobel_scale": ("potsdam", _cfg(PJ, True, False, scale=True), SIZES_SCALE),
}


if __name__ == "__main__":
  ragged.main(CASES, os.path.join(ROOT, "tests", "golden", "seg_prescale.npz"))
