"""Generates tests/golden/seg_augment.npz by EXECUTING the reference's own training `_prepare_train`
(/root/reference/code/datasets/segmentation/potsdam.py:95-216, cocostuff.py:104-230, with
code/utils/segmentation/transforms.py underneath) on small synthetic images.  Run in the build container,
where /root/reference exists:

    python tools/gen_golden_seg_augment.py

The reference is imported read-only through the Python-2 hook (iic_amd.py2compat), oracle/ref_import.py's
stub modules and oracle/tv021_shim.py (torchvision 0.2.1 restated over the installed PIL); `_Potsdam` and
`_CocoFew` / `_CocoFull` instances are made with object.__new__ plus the fields `_prepare_train` reads (their
__init__ walks a dataset directory).  Everything runs on the CPU with Tensor.cuda made the identity.

WHAT THE FIXTURE DOES NOT VALIDATE: cv2 is not installable here, so for the no_sobel=False cases this
generator installs OpenCV 3.x's documented 8-bit RGB2GRAY, (R 4899 + G 9617 + B 1868 + 8192) >> 14, as
`cv2.cvtColor` in the stub module.  The fixture therefore pins everything -- crop and padding arithmetic,
draw order, ColorJitter, channel layout, scaling, random affine, flip, affine2_to_1, masks -- EXCEPT that
one formula, which is a restatement of OpenCV's source on both sides.

Per case and sample the fixture stores the source image (and label map), numpy's seed, every random draw
(crop centre via pad_and_or_crop's return value, ColorJitter.get_params via the shim's log, every
np.random.rand() value, random_affine's affine1_to_2) and the four returned tensors, so that
tests/test_seg_augment_cpu.py (host logic) and tests/test_gpu_seg_augment.py (HIP kernel) replay IDENTICAL
draws.  Arrays only.
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

from oracle import ref_import, tv021_shim  # noqa: E402

tv021_shim.install()
ref_import._shim()                         # xrange + an empty `cv2` module
from iic_amd import py2compat  # noqa: E402

py2compat.enable(REF)

NS = types.SimpleNamespace
INPUT_SZ = 32
SIZES = (24, 32, 48)                       # one source smaller than input_sz, one equal, one larger
SAMPLES = 2
AFFINE = dict(aff_min_rot=-30., aff_max_rot=30., aff_min_shear=-10., aff_max_shear=10., aff_min_scale=0.8,
              aff_max_scale=1.2)


def _cfg(jitter, no_sobel, include_rgb, affine):
  return dict(input_sz=INPUT_SZ, no_sobel=no_sobel, include_rgb=include_rgb, jitter_brightness=jitter[0],
              jitter_contrast=jitter[1], jitter_saturation=jitter[2], jitter_hue=jitter[3], flip_p=0.5,
              use_random_affine=affine, use_random_scale=False, pre_scale_all=False, pre_scale_factor=1.0, **AFFINE)


POTSDAM_JITTER = (0.1, 0.1, 0.1, 0.1)      # the published Potsdam commands
DEFAULT_JITTER = (0.4, 0.4, 0.4, 0.125)    # the scripts' defaults (the COCO commands)
# name -> (dataset, config): every channel layout C = 1..5, both jitter strengths, random affine on and off
CASES = {
  "potsdam_nosobel": ("potsdam", _cfg(POTSDAM_JITTER, True, False, False)),            # C = 4 (published)
  "potsdam_nosobel_affine": ("potsdam", _cfg(POTSDAM_JITTER, True, False, True)),      # C = 4
  "potsdam_sobel_rgb": ("potsdam", _cfg(DEFAULT_JITTER, False, True, False)),          # C = 5
  "potsdam_sobel": ("potsdam", _cfg(POTSDAM_JITTER, False, False, False)),             # C = 2
  "coco_sobel": ("coco_few", _cfg(DEFAULT_JITTER, False, False, False)),               # C = 1 (published)
  "coco_sobel_affine": ("coco_few", _cfg(DEFAULT_JITTER, False, False, True)),         # C = 1
  "coco_sobel_rgb": ("coco_full", _cfg(DEFAULT_JITTER, False, True, False)),           # C = 4
  "coco_nosobel": ("coco_full", _cfg(POTSDAM_JITTER, True, False, False)),             # C = 3
}


def seed_for(ci, zi, si):
  return 7000003 * (ci + 1) + 10007 * zi + si


def _packages():
  """The reference's package __init__ files import every dataset and script dependency; only the two dataset
  modules are wanted, so their parent packages are registered empty (sub-modules still come from disk)."""
  for name in ("code", "code.datasets", "code.datasets.segmentation", "code.datasets.segmentation.util", "code.utils",
               "code.utils.segmentation"):
    pkg = types.ModuleType(name)
    pkg.__path__ = [os.path.join(REF, *name.split("."))]
    sys.modules[name] = pkg


def grey_fixed_point(img, code):
  """Stand-in for cv2.cvtColor(img, cv2.COLOR_RGB2GRAY) on uint8 (see the header)."""
  assert code == "RGB2GRAY" and img.dtype == np.uint8 and img.shape[2] == 3
  v = img.astype(np.int64)
  return ((v[..., 0] * 4899 + v[..., 1] * 9617 + v[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def make_image(rs, size, channels):
  """Natural-image-like content: low-frequency colour blobs + texture + a few saturated pixels."""
  yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
  img = np.zeros((size, size, channels))
  for c in range(channels):
    a, b, ph = rs.uniform(1, 4), rs.uniform(1, 4), rs.uniform(0, 6.28)
    img[..., c] = 0.5 + 0.35 * np.sin(a * 6.28 * xx + ph) * np.cos(b * 6.28 * yy + 0.7 * c)
  img += rs.normal(0, 0.08, img.shape)
  img = np.clip(img, 0, 1)
  k = rs.randint(0, size, (8, 2))
  img[k[:, 0], k[:, 1]] = rs.randint(0, 2, (8, channels))
  return (img * 255).round().astype(np.uint8)


def make_labels(rs, size):
  """Fine labels in blocks: unlabelled (-1), thing classes (0..90) and stuff classes (91..181)."""
  pool = np.array([-1, 0, 1, 17, 90, 91, 95, 105, 123, 141, 156, 168, 181], np.int32)
  blocks = pool[rs.randint(0, len(pool), (size // 4 + 1, size // 4 + 1))]
  lab = np.kron(blocks, np.ones((4, 4), np.int32))[:size, :size]
  lab[rs.randint(0, size, 6), rs.randint(0, size, 6)] = -1
  return np.ascontiguousarray(lab.astype(np.int32))


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
    ds.include_rgb, ds.no_sobel, ds.use_random_scale, ds.mask_input = c.include_rgb, c.no_sobel, False, False
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
      return res

    def aff(img, _o=orig_aff, **kw):
      res = _o(img, **kw)
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
  # random_affine (transforms.py) looks np.random.rand up at call time: one patch covers every module
  orig_cuda = torch.Tensor.cuda
  torch.Tensor.cuda = lambda self, *a, **k: self

  out = {}
  names = sorted(CASES)
  try:
    for ci, name in enumerate(names):
      kind, cfg = CASES[name]
      ds = instance(kind, cfg)
      cs = 4 if kind == "potsdam" else 3
      flips = []
      for zi, size in enumerate(SIZES):
        key = "%s/%d" % (name, size)
        cols = {k: [] for k in ("images", "labels", "seeds", "coords", "jit_n", "jit_ops", "jit_f", "rands", "a12",
                                "img1", "img2", "aff", "mask")}
        for si in range(SAMPLES):
          rs = np.random.RandomState(seed_for(ci, zi, si) + 17)
          img = make_image(rs, size, cs)
          seed = seed_for(ci, zi, si)
          np.random.seed(seed)
          rec.clear()
          del tv021_shim.LOG[:]
          if kind == "potsdam":
            res = ds._prepare_train(si, img.copy())
          else:
            lab = make_labels(rs, size)
            cols["labels"].append(lab.astype(np.int16))
            res = ds._prepare_train(si, img.copy(), lab.copy())
          img1, img2, a21, mask = res
          jit = [v for k, v in tv021_shim.LOG if k == "jitter"]
          assert len(jit) == 1
          ops = np.full(4, -1, np.int64)
          fac = np.zeros(4, np.float64)
          for o, (op, f) in enumerate(jit[0]):
            ops[o] = op
            fac[op] = f
          cols["images"].append(img)
          cols["seeds"].append(seed)
          cols["coords"].append(rec["coords"])
          cols["jit_n"].append(len(jit[0]))
          cols["jit_ops"].append(ops)
          cols["jit_f"].append(fac)
          want = 4 if cfg["use_random_affine"] else 1
          assert len(rec["rands"]) == want, rec["rands"]
          cols["rands"].append(np.asarray(rec["rands"], np.float64))   # [a, shear, scale,] flip
          cols["a12"].append(rec.get("a12", np.zeros((2, 3), np.float32)))
          cols["img1"].append(img1.numpy().astype(np.float32))
          cols["img2"].append(img2.numpy().astype(np.float32))
          cols["aff"].append(a21.numpy().astype(np.float32))
          assert mask.dtype == torch.uint8
          cols["mask"].append(mask.numpy())
          flips.append(rec["rands"][-1] > cfg["flip_p"])
        for k, v in cols.items():
          if v:
            out[key + "/" + k] = np.stack(v)
      assert any(flips) and not all(flips), (name, flips)          # flip on and off in every case
      meta = dict(kind=kind, channels=cs, config=cfg)
      out[name + "/meta"] = np.array(json.dumps(meta))
      if kind != "potsdam":
        # _filter_label's mask as a function of the fine label, from the reference's own method (-1 at entry 255)
        fine = np.arange(256, dtype=np.int32)
        fine[182:] = -1
        out[name + "/relevance"] = np.asarray(ds._filter_label(fine.reshape(1, 256).copy())[1]).reshape(256).astype(np.uint8)
  finally:
    torch.Tensor.cuda = orig_cuda
    np.random.rand = orig_rand
  out["names"] = np.array(names)
  out["sizes"] = np.array(SIZES)
  path = os.path.join(ROOT, "tests", "golden", "seg_augment.npz")
  np.savez_compressed(path, **out)
  print("wrote", path, os.path.getsize(path), "bytes;", len(names), "cases x", len(SIZES), "sizes x", SAMPLES, "samples")


if __name__ == "__main__":
  main()
