"""Generates tests/golden/seg_test_prep.npz by EXECUTING the reference's own test-time `_prepare_test`
(/root/reference/code/datasets/segmentation/potsdam.py:295-350, cocostuff.py:309-358, with
code/utils/segmentation/transforms.py underneath and each dataset's own `_filter_label`) on small synthetic
images.  Run in the build container, where /root/reference exists:

    python tools/gen_golden_seg_test_prep.py

Same recipe as tools/gen_golden_seg_augment.py: the reference is imported read-only through the Python-2 hook
(iic_amd.py2compat) and oracle/ref_import.py's stub modules; `_Potsdam` / `Potsdam`, `_CocoFew` and `_CocoFull`
instances are made with object.__new__ plus the fields `_prepare_test` and `_filter_label` read (their __init__
walks a dataset directory).  Nothing random happens at test time, so there are no draws to record.

WHAT THE FIXTURE DOES NOT VALIDATE: cv2 is not installable here, so for the no_sobel=False cases this generator
installs OpenCV 3.x's documented 8-bit RGB2GRAY, (R 4899 + G 9617 + B 1868 + 8192) >> 14, as `cv2.cvtColor` in the
stub module.  `_prepare_test` calls it on the float32 image (unlike `_prepare_train` it never truncates to uint8
first); every value of that image is an integer in 0..255 here (no pre_scale_all), and the stand-in applies the
8-bit formula to them.  A real OpenCV would take its float path on such an input -- 0.299 R + 0.587 G + 0.114 B,
unrounded -- which lies within half a grey level of the value stored here.  The fixture therefore pins the padding
and centre-crop arithmetic, the channel layout, the scaling, the label filtering and the masks -- EXCEPT grey.

Per case and source size the fixture stores the source images, the fine label maps (int16), and the three returned
tensors (image float32, label int16, mask uint8); per case the two 256-entry tables (`_filter_label`'s label and
mask as functions of the fine label, -1 at entries 182..255) taken from the reference's own method.  Arrays only.
"""
import importlib
import io
import json
import os
import pickle
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("IIC_REFERENCE", "/root/reference")

from oracle import ref_import  # noqa: E402

ref_import._shim()                         # xrange + an empty `cv2` module
from iic_amd import py2compat  # noqa: E402

py2compat.enable(REF)

INPUT_SZ = 32
# (h, w): smaller, equal, odd-larger and larger than input_sz -- both parities of int(h / 2.) -- and two sources
# of which one axis pads while the other crops
SIZES = ((24, 24), (32, 32), (37, 37), (48, 48), (24, 48), (48, 24))
SAMPLES = 2
# name -> (dataset, gt_k, use_coarse_labels, no_sobel, include_rgb): every channel layout C = 1..5
CASES = {
  "potsdam_coarse_nosobel": ("potsdam", 3, True, True, False),        # C = 4 (published Potsdam-3)
  "potsdam_coarse_sobel": ("potsdam", 3, True, False, False),         # C = 2
  "potsdam_fine_sobel_rgb": ("potsdam", 6, False, False, True),       # C = 5
  "coco_few_sobel": ("coco_few", 3, True, False, False),              # C = 1 (published COCO-Stuff-3)
  "coco_fine_nosobel": ("coco_full", 91, False, True, False),         # C = 3
  "coco_coarse_sobel_rgb": ("coco_full", 15, True, False, True),      # C = 4 (published COCO-Stuff: 15 classes)
}


def seed_for(ci, zi, si):
  return 9000011 * (ci + 1) + 10007 * zi + si


def _packages():
  """The reference's package __init__ files import every dataset and script dependency; only the two dataset
  modules are wanted, so their parent packages are registered empty (sub-modules still come from disk)."""
  for name in ("code", "code.datasets", "code.datasets.segmentation", "code.datasets.segmentation.util", "code.utils",
               "code.utils.segmentation"):
    pkg = types.ModuleType(name)
    pkg.__path__ = [os.path.join(REF, *name.split("."))]
    sys.modules[name] = pkg


def grey_fixed_point(img, code):
  """Stand-in for cv2.cvtColor(img, cv2.COLOR_RGB2GRAY) (see the header): the 8-bit formula on a float32 image
  whose values are all integers in 0..255."""
  assert code == "RGB2GRAY" and img.dtype == np.float32 and img.shape[2] == 3
  v = img.astype(np.int64)
  assert np.array_equal(v, img) and v.min() >= 0 and v.max() <= 255
  return ((v[..., 0] * 4899 + v[..., 1] * 9617 + v[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def make_image(rs, h, w, channels):
  """Natural-image-like content: low-frequency colour blobs + texture + a few saturated pixels."""
  yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
  yy, xx = yy / h, xx / w
  img = np.zeros((h, w, channels))
  for c in range(channels):
    a, b, ph = rs.uniform(1, 4), rs.uniform(1, 4), rs.uniform(0, 6.28)
    img[..., c] = 0.5 + 0.35 * np.sin(a * 6.28 * xx + ph) * np.cos(b * 6.28 * yy + 0.7 * c)
  img += rs.normal(0, 0.08, img.shape)
  img = np.clip(img, 0, 1)
  ky, kx = rs.randint(0, h, 8), rs.randint(0, w, 8)
  img[ky, kx] = rs.randint(0, 2, (8, channels))
  return (img * 255).round().astype(np.uint8)


def make_labels(rs, h, w, pool):
  """Fine labels in 4 x 4 blocks drawn from `pool`, plus six single pixels of its first entry."""
  pool = np.asarray(pool, np.int32)
  blocks = pool[rs.randint(0, len(pool), (h // 4 + 1, w // 4 + 1))]
  lab = np.kron(blocks, np.ones((4, 4), np.int32))[:h, :w]
  lab[rs.randint(0, h, 6), rs.randint(0, w, 6)] = pool[0]
  return np.ascontiguousarray(lab.astype(np.int32))


COCO_POOL = (-1, 0, 1, 17, 90, 91, 95, 105, 123, 141, 156, 168, 181)    # unlabelled, things (0..90), stuff (91..181)
POTSDAM_POOL = (0, 1, 2, 3, 4, 5)


def tables(filter_label):
  """(label, mask) of `_filter_label` per fine label, -1 at entries 182..255, as two uint8 [256] arrays (the label's
  low 8 bits; mask None where the method returns the labels alone).  Asked one label at a time where the method
  refuses the whole range (Potsdam fine asserts label.max() < gt_k): a refused label gets -1."""
  fine = np.arange(256, dtype=np.int32)
  fine[182:] = -1

  def ask(a):
    res = filter_label(a.copy())
    if isinstance(res, tuple):
      return np.asarray(res[0]).reshape(-1).astype(np.int64), np.asarray(res[1]).reshape(-1).astype(np.uint8)
    return np.asarray(res).reshape(-1).astype(np.int64), None
  try:
    lab, mask = ask(fine.reshape(1, 256))
  except AssertionError:
    lab, mask = np.full(256, -1, np.int64), None
    for i in range(256):
      try:
        one, m = ask(fine[i:i + 1].reshape(1, 1))
        assert m is None
        lab[i] = one[0]
      except AssertionError:
        pass
  return (lab & 255).astype(np.uint8), mask


def main():
  import cv2
  cv2.COLOR_RGB2GRAY = "RGB2GRAY"
  cv2.cvtColor = grey_fixed_point
  cv2.setNumThreads = lambda n: None
  _packages()
  potsdam = importlib.import_module("code.datasets.segmentation.potsdam")
  with redirect_stdout(io.StringIO()):
    coco = importlib.import_module("code.datasets.segmentation.cocostuff")
  f2c_mod = importlib.import_module("code.datasets.segmentation.util.cocostuff_fine_to_coarse")

  # the reference's own fine -> coarse table, generated by its own function (cwd = the reference tree)
  import yaml
  yaml_load = yaml.load
  yaml.load = lambda f, Loader=yaml.SafeLoader: yaml_load(f, Loader)     # PyYAML >= 6 wants the loader named
  cwd = os.getcwd()
  tmp = tempfile.mkdtemp()
  try:
    os.chdir(REF)
    with redirect_stdout(io.StringIO()):
      f2c_mod.generate_fine_to_coarse(os.path.join(tmp, "f2c.pickle"))
  finally:
    os.chdir(cwd)
    yaml.load = yaml_load
  with open(os.path.join(tmp, "f2c.pickle"), "rb") as f:
    fine_to_coarse = pickle.load(f)["fine_index_to_coarse_index"]

  def instance(kind, gt_k, coarse, no_sobel, include_rgb):
    cls = {"potsdam": potsdam.Potsdam, "coco_few": coco._CocoFew, "coco_full": coco._CocoFull}[kind]
    ds = object.__new__(cls)
    ds.pre_scale_all, ds.pre_scale_factor, ds.input_sz = False, 1.0, INPUT_SZ
    ds.include_rgb, ds.no_sobel, ds.mask_input, ds.gt_k = include_rgb, no_sobel, False, gt_k
    if kind == "potsdam":
      ds.use_coarse_labels = coarse
      ds._fine_to_coarse_dict = {0: 0, 4: 0, 1: 1, 5: 1, 2: 2, 3: 2}     # potsdam.py:418-421 (set in __init__)
    elif kind == "coco_few":            # COCO-Stuff-3: sky, plant, ground (cocostuff.py:667-722)
      ds._fine_to_coarse_dict = fine_to_coarse
      ds.include_things_labels, ds.incl_animal_things = False, False
      ds.label_names = ["sky-stuff", "plant-stuff", "ground-stuff"]
      with redirect_stdout(io.StringIO()):
        ds._fine_to_few_dict = ds._make_fine_to_few_dict()
    else:                               # COCO-Stuff, stuff classes only: fine (91) or coarse (15), cocostuff.py:629-656
      ds._fine_to_coarse_dict = fine_to_coarse
      ds.use_coarse_labels, ds.include_things_labels = coarse, False
    ds._check_gt_k()
    return ds

  out = {}
  names = sorted(CASES)
  for ci, name in enumerate(names):
    kind, gt_k, coarse, no_sobel, include_rgb = CASES[name]
    ds = instance(kind, gt_k, coarse, no_sobel, include_rgb)
    cs = 4 if kind == "potsdam" else 3
    seen = set()
    for zi, (h, w) in enumerate(SIZES):
      key = "%s/%dx%d" % (name, h, w)
      cols = {k: [] for k in ("images", "labels", "imgs", "targets", "mask")}
      for si in range(SAMPLES):
        rs = np.random.RandomState(seed_for(ci, zi, si))
        img = make_image(rs, h, w, cs)
        lab = make_labels(rs, h, w, POTSDAM_POOL if kind == "potsdam" else COCO_POOL)
        seen.update(int(v) for v in np.unique(lab))
        res_img, res_lab, res_mask = ds._prepare_test(si, img.copy(), lab.copy())
        assert res_img.dtype == torch.float32 and res_mask.dtype == torch.uint8
        assert tuple(res_lab.shape) == tuple(res_mask.shape) == (INPUT_SZ, INPUT_SZ)
        cols["images"].append(img)
        cols["labels"].append(lab.astype(np.int16))
        cols["imgs"].append(res_img.numpy().astype(np.float32))
        cols["targets"].append(res_lab.numpy().astype(np.int16))
        cols["mask"].append(res_mask.numpy())
      for k, v in cols.items():
        out[key + "/" + k] = np.stack(v)
    if kind != "potsdam":               # -1, thing classes and stuff classes all occur
      assert -1 in seen and any(0 <= v <= 90 for v in seen) and any(v >= 91 for v in seen), seen
    meta = dict(kind=kind, channels=cs, gt_k=gt_k, use_coarse_labels=coarse,
                config=dict(input_sz=INPUT_SZ, no_sobel=no_sobel, include_rgb=include_rgb, pre_scale_all=False,
                            mask_input=False))
    out[name + "/meta"] = np.array(json.dumps(meta))
    ttab, rtab = tables(ds._filter_label)
    out[name + "/targets_table"] = ttab
    assert (rtab is None) == (kind == "potsdam")
    if rtab is not None:
      out[name + "/relevance"] = rtab
  out["names"] = np.array(names)
  out["sizes"] = np.array(SIZES)
  path = os.path.join(ROOT, "tests", "golden", "seg_test_prep.npz")
  np.savez_compressed(path, **out)
  print("wrote", path, os.path.getsize(path), "bytes;", len(names), "cases x", len(SIZES), "sizes x", SAMPLES, "samples")


if __name__ == "__main__":
  main()
