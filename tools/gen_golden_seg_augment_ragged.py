"""Generates tests/golden/seg_augment_ragged.npz by EXECUTING the reference's own training `_prepare_train`
(code/datasets/segmentation/cocostuff.py:104-230, potsdam.py:95-216, with code/utils/segmentation/transforms.py
underneath) on small synthetic images of DIFFERENT sizes.  Run where the reference tree exists (IIC_REFERENCE):

    python tools/gen_golden_seg_augment_ragged.py

Same recipe as tools/gen_golden_seg_augment.py, whose stub modules, synthetic content, draw recording and metadata
keys it shares: the Python-2 hook, oracle/ref_import.py's stubs, oracle/tv021_shim.py, instances made with
object.__new__, everything on the CPU.

Per image size the crop-centre range, the padding offsets and which pixels are padding differ; the sizes are
20 x 24 (both sides padded), 20 x 50 and 50 x 20 (one side padded), 32 x 32, 33 x 47 (odd), 61 x 40 at input_sz 32,
and 35 x 37 at input_sz 36 (a multiple of 4 whose half image is odd-sized).

WHAT THE FIXTURE DOES NOT VALIDATE.  cv2 is not installable here.
  * Grey (no_sobel=False): OpenCV 3.x's 8-bit RGB2GRAY is installed as `cv2.cvtColor`, as in the uniform generator.
    The cases WITHOUT use_random_scale use no other stand-in: they pin the per-image crop and padding arithmetic,
    draw order, ColorJitter, channel layout, random affine, flip, affine2_to_1 and masks to the reference's own code.
  * use_random_scale (the `*_scale` cases, scale 0.6 .. 1.4, no pre_scale_all): `cv2.resize` in the stub module is
    iic_amd.seg_ragged.resize_linear_host / resize_nearest_host, the restatement of OpenCV 3.x's resize the kernel's
    tables are built from.  Those cases pin the draw order (the scale is drawn first), the scaled extents the crop
    range is computed on, and the crop coordinates to the reference; the resampled PIXELS are pinned to the
    restatement only, on both sides.

Per case and sample the fixture stores the source image (and label map), numpy's seed, every random draw and the four
returned tensors (with use_random_affine also img2 as `random_affine` receives it, before the warp), so that tests/test_seg_ragged_cpu.py and tests/test_gpu_seg_ragged.py replay identical draws.
Images of one case differ in size, so per-sample arrays are stored under "<case>/<i>/<key>".  Arrays only.
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

from tools import gen_golden_seg_augment as base  # noqa: E402  (installs the shims and the Python-2 hook)
from oracle import tv021_shim  # noqa: E402
from iic_amd import seg_ragged  # noqa: E402

REF = base.REF
NS = types.SimpleNamespace
AFFINE = base.AFFINE
SIZES_32 = ((20, 24), (20, 50), (50, 20), (32, 32), (33, 47), (61, 40))
SIZES_36 = ((35, 37), (35, 37))            # two samples: both flip outcomes
SIZES_SUB = ((20, 24), (33, 47), (61, 40), (32, 32))


def _cfg(input_sz, jitter, no_sobel, include_rgb, affine=False, scale=False):
  return dict(input_sz=input_sz, no_sobel=no_sobel, include_rgb=include_rgb, jitter_brightness=jitter[0],
              jitter_contrast=jitter[1], jitter_saturation=jitter[2], jitter_hue=jitter[3], flip_p=0.5,
              use_random_affine=affine, use_random_scale=scale, scale_min=0.6, scale_max=1.4, pre_scale_all=False,
              pre_scale_factor=1.0, **AFFINE)


PJ, DJ = base.POTSDAM_JITTER, base.DEFAULT_JITTER
# name -> (dataset, config, image sizes)
CASES = {
  "coco_nosobel": ("coco_full", _cfg(32, PJ, True, False), SIZES_32),                       # C = 3
  "coco_sobel_rgb": ("coco_full", _cfg(32, DJ, False, True), SIZES_32),                     # C = 4
  "coco_sobel": ("coco_few", _cfg(32, DJ, False, False), SIZES_32),                         # C = 1 (published)
  "potsdam_nosobel": ("potsdam", _cfg(32, PJ, True, False), SIZES_32),                      # C = 4
  "coco_nosobel_s36": ("coco_full", _cfg(36, PJ, True, False), SIZES_36),
  "coco_sobel_rgb_s36": ("coco_full", _cfg(36, DJ, False, True), SIZES_36),
  "coco_sobel_s36": ("coco_few", _cfg(36, DJ, False, False), SIZES_36),
  "potsdam_nosobel_s36": ("potsdam", _cfg(36, PJ, True, False), SIZES_36),
  "coco_sobel_affine": ("coco_few", _cfg(32, DJ, False, False, affine=True), SIZES_SUB),
  "coco_sobel_rgb_scale": ("coco_full", _cfg(32, DJ, False, True, scale=True), SIZES_SUB),
  "potsdam_nosobel_scale": ("potsdam", _cfg(32, PJ, True, False, scale=True), SIZES_SUB),
  "coco_sobel_scale_affine": ("coco_few", _cfg(32, DJ, False, False, affine=True, scale=True), SIZES_SUB),
}


def seed_for(ci, si, salt):
  return 9000011 * (ci + 1) + 10007 * si + 101 * salt


def make_image(rs, h, w, channels):
  """The content of the uniform generator's make_image on an h x w image."""
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


def make_labels(rs, h, w):
  side = max(h, w)
  return np.ascontiguousarray(base.make_labels(rs, side)[:h, :w])


def resize_stand_in(img, dsize=None, fx=None, fy=None, interpolation=None):
  """Stand-in for cv2.resize(dsize=None, fx=fy=scale) (see the header)."""
  assert dsize is None and fx == fy
  if interpolation == "LINEAR":
    assert img.dtype == np.float32
    return seg_ragged.resize_linear_host(img, fx)
  assert interpolation == "NEAREST" and img.dtype == np.int32
  return seg_ragged.resize_nearest_host(img, fx)


def main(cases=None, path=None):
  """cases / path: another case table and fixture file (tools/gen_golden_seg_prescale.py); the defaults are this tool's."""
  cases = CASES if cases is None else cases
  import cv2
  cv2.COLOR_RGB2GRAY = "RGB2GRAY"
  cv2.cvtColor = base.grey_fixed_point
  cv2.INTER_LINEAR, cv2.INTER_NEAREST = "LINEAR", "NEAREST"
  cv2.resize = resize_stand_in
  cv2.setNumThreads = lambda n: None
  base._packages()
  potsdam = importlib.import_module("code.datasets.segmentation.potsdam")
  with redirect_stdout(io.StringIO()):
    coco = importlib.import_module("code.datasets.segmentation.cocostuff")
  f2c_mod = importlib.import_module("code.datasets.segmentation.util.cocostuff_fine_to_coarse")
  tvt = sys.modules["torchvision.transforms"]

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

  def instance(kind, cfg):
    c = NS(**cfg)
    cls = {"potsdam": potsdam._Potsdam, "coco_few": coco._CocoFew, "coco_full": coco._CocoFull}[kind]
    ds = object.__new__(cls)
    ds.pre_scale_all, ds.pre_scale_factor, ds.input_sz = c.pre_scale_all, c.pre_scale_factor, c.input_sz
    ds.include_rgb, ds.no_sobel, ds.mask_input = c.include_rgb, c.no_sobel, False
    ds.use_random_scale, ds.scale_min, ds.scale_max = c.use_random_scale, c.scale_min, c.scale_max
    ds.jitter_tf = tvt.ColorJitter(brightness=c.jitter_brightness, contrast=c.jitter_contrast,
                                   saturation=c.jitter_saturation, hue=c.jitter_hue)
    ds.flip_p, ds.use_random_affine = c.flip_p, c.use_random_affine
    for k in AFFINE:
      setattr(ds, k, getattr(c, k))
    if kind == "coco_few":            # COCO-Stuff-3: sky, plant, ground (cocostuff.py:667-722)
      ds._fine_to_coarse_dict = fine_to_coarse
      ds.label_names = ["sky-stuff", "plant-stuff", "ground-stuff"]
      with redirect_stdout(io.StringIO()):
        ds._fine_to_few_dict = ds._make_fine_to_few_dict()
    elif kind == "coco_full":         # COCO-Stuff fine (91): stuff classes only (cocostuff.py:629-656)
      ds.use_coarse_labels, ds.include_things_labels = False, False
    return ds

  rec = {}
  for mod in (potsdam, coco):         # observe the draws the reference's own code makes
    orig_crop, orig_aff = mod.pad_and_or_crop, mod.random_affine

    def crop(data, sz, mode=None, coords=None, _o=orig_crop):
      res = _o(data, sz, mode=mode, coords=coords)
      if mode == "random":
        rec["coords"] = tuple(int(v) for v in res[1])
        rec["extent"] = tuple(int(v) for v in data.shape[:2])      # the (scaled) image the crop was drawn on
      return res

    def aff(img, _o=orig_aff, **kw):
      res = _o(img, **kw)
      rec["img2_pre"] = img.numpy().copy()       # img2 as random_affine receives it: after the jitter, before warp and flip
      rec["a12"] = res[1].numpy().copy()
      return res
    mod.pad_and_or_crop, mod.random_affine = crop, aff
  orig_rand = np.random.rand

  def logging_rand(*a):
    v = orig_rand(*a)
    if not a:
      rec.setdefault("rands", []).append(float(v))
    return v
  np.random.rand = logging_rand
  orig_cuda = torch.Tensor.cuda
  torch.Tensor.cuda = lambda self, *a, **k: self

  def run_case(ci, name, ds, kind, cfg, sizes, cs, salt):
    flips, out = [], {}
    cols = {k: [] for k in ("seeds", "coords", "extent", "jit_n", "jit_ops", "jit_f", "rands", "a12", "aff", "scale")}
    for si, (h, w) in enumerate(sizes):
      key = "%s/%d" % (name, si)
      seed = seed_for(ci, si, salt)
      rs = np.random.RandomState(seed + 17)
      img = make_image(rs, h, w, cs)
      np.random.seed(seed)
      rec.clear()
      del tv021_shim.LOG[:]
      if kind == "potsdam":
        res = ds._prepare_train(si, img.copy())
      else:
        lab = make_labels(rs, h, w)
        out[key + "/label"] = lab.astype(np.int16)
        res = ds._prepare_train(si, img.copy(), lab.copy())
      img1, img2, a21, mask = res
      jit = [v for k, v in tv021_shim.LOG if k == "jitter"]
      assert len(jit) == 1
      ops = np.full(4, -1, np.int64)
      fac = np.zeros(4, np.float64)
      for o, (op, f) in enumerate(jit[0]):
        ops[o] = op
        fac[op] = f
      want = 1 + (3 if cfg["use_random_affine"] else 0) + (1 if cfg["use_random_scale"] else 0)
      assert len(rec["rands"]) == want, rec["rands"]
      scale = 1.0
      if cfg["use_random_scale"]:
        scale = rec["rands"][0] * (cfg["scale_max"] - cfg["scale_min"]) + cfg["scale_min"]     # cocostuff.py:125-126
      elif not cfg["pre_scale_all"]:
        assert rec["extent"] == (h, w)
      out[key + "/image"] = img
      out[key + "/img1"] = img1.numpy().astype(np.float32)
      out[key + "/img2"] = img2.numpy().astype(np.float32)
      assert mask.dtype == torch.uint8
      out[key + "/mask"] = mask.numpy()
      if cfg["use_random_affine"]:
        out[key + "/img2_pre"] = rec["img2_pre"].astype(np.float32)
      cols["seeds"].append(seed)
      cols["coords"].append(rec["coords"])
      cols["extent"].append(rec["extent"])
      cols["jit_n"].append(len(jit[0]))
      cols["jit_ops"].append(ops)
      cols["jit_f"].append(fac)
      cols["rands"].append(np.asarray(rec["rands"], np.float64))     # [scale,] [a, shear, scale,] flip
      cols["a12"].append(rec.get("a12", np.zeros((2, 3), np.float32)))
      cols["aff"].append(a21.numpy().astype(np.float32))
      cols["scale"].append(scale)
      flips.append(rec["rands"][-1] > cfg["flip_p"])
    for k, v in cols.items():
      out[name + "/" + k] = np.stack(v)
    return flips, out

  out = {}
  names = sorted(cases)
  total = 0
  try:
    for ci, name in enumerate(names):
      kind, cfg, sizes = cases[name]
      ds = instance(kind, cfg)
      cs = 4 if kind == "potsdam" else 3
      flips, salt = [], -1
      while not (any(flips) and not all(flips)):      # flip on and off in every case: the first seed set that has both
        salt += 1
        flips, case_out = run_case(ci, name, ds, kind, cfg, sizes, cs, salt)
      out.update(case_out)
      total += len(sizes)
      out[name + "/sizes"] = np.array(sizes, np.int32)
      meta = dict(kind=kind, channels=cs, config=cfg)
      out[name + "/meta"] = np.array(json.dumps(meta))
      if kind != "potsdam":
        fine = np.arange(256, dtype=np.int32)
        fine[182:] = -1
        out[name + "/relevance"] = np.asarray(ds._filter_label(fine.reshape(1, 256).copy())[1]).reshape(256).astype(np.uint8)
  finally:
    torch.Tensor.cuda = orig_cuda
    np.random.rand = orig_rand
  out["names"] = np.array(names)
  path = os.path.join(ROOT, "tests", "golden", "seg_augment_ragged.npz") if path is None else path
  np.savez_compressed(path, **out)
  print("wrote", path, os.path.getsize(path), "bytes;", len(names), "cases,", total, "samples")


if __name__ == "__main__":
  main()
