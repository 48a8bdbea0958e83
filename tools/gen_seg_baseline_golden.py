"""Generates the two fixtures of the Isola / Doersch segmentation baselines by RUNNING the reference's own code on the
CPU -- recorded results only, no reference text:

  tests/golden/seg_baseline_patches.json     for seeded np.random at (S, p) in {(200, 11), (128, 11), (24, 3)}: the first
                                             64 results of code/utils/segmentation/baselines/isola_utils.py's
                                             isola_set_patches and doersch_utils.py's doersch_set_patches
  tests/golden/seg_baseline_state_keys.json  key -> shape of the state_dict of the reference's SegmentationNet10aIsola and
                                             SegmentationNet10aDoersch at patch side 3

Run where the reference tree exists (IIC_REFERENCE):

    python tools/gen_seg_baseline_golden.py

The reference is imported through iic_amd.py2compat (its sources are Python 2).  Its two classes never store
``batchnorm_track`` although the initialiser they inherit asserts on it (vgg.py:49): their constructors raise
AttributeError as published.  The tool supplies the attribute on the classes before constructing them, as
tools/gen_golden_triplets.py does; nothing else is touched.
"""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
REF = os.environ.get("IIC_REFERENCE")

SHAPES = [(200, 11), (128, 11), (24, 3)]
SEED = 20240607
DRAWS = 64


def _ints(a):
  return [int(v) for v in np.asarray(a).reshape(-1)]


def main():
  if not REF:
    sys.exit("set IIC_REFERENCE to the directory that contains the reference's code/")
  from iic_amd import py2compat
  py2compat.enable(REF)
  from code.utils.segmentation.baselines import doersch_utils, isola_utils
  from code.archs.segmentation.baselines import net10a_doersch, net10a_isola

  patches = {"seed": SEED, "draws": DRAWS, "cases": []}
  for S, p in SHAPES:
    np.random.seed(SEED)
    iso = []
    for _ in range(DRAWS):
      centre, other, adjacent = isola_utils.isola_set_patches(input_sz=S, patch_side=p)
      iso.append(_ints(centre) + _ints(other) + [int(bool(adjacent))])
    np.random.seed(SEED)
    doe = []
    for _ in range(DRAWS):
      centre, other, position = doersch_utils.doersch_set_patches(input_sz=S, patch_side=p)
      doe.append(_ints(centre) + _ints(other) + [int(position)])
    patches["cases"].append({"S": S, "p": p, "isola": iso, "doersch": doe})
  path = os.path.join(ROOT, "tests", "golden", "seg_baseline_patches.json")
  with open(path, "w") as f:
    f.write(json.dumps(patches, sort_keys=True) + "\n")
  print("wrote", path)

  keys = {}
  for name, mod, cls, side in (("isola", net10a_isola, "SegmentationNet10aIsola", "isola_patch_side"),
                               ("doersch", net10a_doersch, "SegmentationNet10aDoersch", "doersch_patch_side")):
    cfg = {"in_channels": 3, "input_sz": 24, "batchnorm_track": True, side: 3}
    klass = getattr(mod, cls)
    klass.batchnorm_track = True      # see the module docstring
    net = klass(types.SimpleNamespace(**cfg))
    keys[name] = {"class": cls, "config": cfg, "state": [[n, list(t.shape)] for n, t in net.state_dict().items()]}
  path = os.path.join(ROOT, "tests", "golden", "seg_baseline_state_keys.json")
  with open(path, "w") as f:
    f.write(json.dumps(keys, sort_keys=True) + "\n")
  print("wrote", path, {k: len(v["state"]) for k, v in keys.items()})


if __name__ == "__main__":
  main()
