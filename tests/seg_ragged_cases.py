"""The reference-generated fixture tests/golden/seg_augment_ragged.npz (tools/gen_golden_seg_augment_ragged.py) as
augmenters and parameter dictionaries, written once and used by tests/test_seg_ragged_cpu.py (host logic) and
tests/test_gpu_seg_ragged.py (HIP kernel).  A CASE is one configuration with a list of images of different sizes."""
import json
import os
import types

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_augment_ragged.npz")
_CACHE = {}


def fixture():
  if "g" not in _CACHE:
    with np.load(G) as g:
      _CACHE["g"] = {k: g[k] for k in g.files}
  return _CACHE["g"]


def names():
  return [str(n) for n in fixture()["names"]]


def meta(name):
  return json.loads(str(fixture()[name + "/meta"]))


def config(name, **overrides):
  c = dict(meta(name)["config"])
  c.update(overrides)
  return types.SimpleNamespace(**c)


def images(name):
  """(list of uint8 [h, w, Cs] images, list of uint8 [h, w] label maps with 255 for -1 or None, relevance or None)."""
  g = fixture()
  n = len(g[name + "/sizes"])
  imgs = [g["%s/%d/image" % (name, i)] for i in range(n)]
  if meta(name)["kind"] == "potsdam":
    return imgs, None, None
  labels = [(g["%s/%d/label" % (name, i)].astype(np.int64) % 256).astype(np.uint8) for i in range(n)]
  return imgs, labels, g[name + "/relevance"]


def augmenter(name, device="cpu", **overrides):
  from iic_amd import seg_ragged
  imgs, labels, rel = images(name)
  return seg_ragged.SegRaggedAugmenter(imgs, config(name, **overrides), labels=labels, relevance=rel, device=device)


def expected(name, i):
  g = fixture()
  return tuple(g["%s/%d/%s" % (name, i, k)] for k in ("img1", "img2")) + (g[name + "/aff"][i], g["%s/%d/mask" % (name, i)])


def recorded_params(name, S):
  """iparams / fparams / affine1_to_2 / scale from the RECORDED draws of the reference run, sample i = image i."""
  from iic_amd import seg_augment as sa
  g, m = fixture(), meta(name)
  cfg = m["config"]
  n = len(g[name + "/seeds"])
  ip = np.zeros((n, sa.IPARAMS), np.int32)
  fp = np.zeros((n, sa.FPARAMS), np.float32)
  half = int(S / 2.)
  a12 = g[name + "/a12"].astype(np.float32) if cfg["use_random_affine"] else None
  for i in range(n):
    h_c, w_c = g[name + "/coords"][i]
    nj = int(g[name + "/jit_n"][i])
    ip[i, :5] = (i, w_c - half, h_c - half, g[name + "/rands"][i][-1] > cfg["flip_p"], nj)
    ip[i, 5:5 + nj] = g[name + "/jit_ops"][i][:nj]
    fp[i, :4] = g[name + "/jit_f"][i]
    ip[i, 9] = int(float(g[name + "/jit_f"][i][3]) * 255) % 256
    m21 = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    if a12 is not None:
      full = np.concatenate([a12[i], np.array([[0, 0, 1]], np.float32)], 0)
      m21 = np.linalg.inv(full).astype(np.float32)[:2]      # transforms.py:119
    fp[i, 4:10] = m21.reshape(6)
  scale = g[name + "/scale"].astype(np.float64) if cfg["use_random_scale"] else None
  return dict(iparams=ip, fparams=fp, affine1_to_2=a12, scale=scale)


def take(params, rows):
  """The rows `rows` of a parameter dictionary."""
  return {k: (None if v is None else np.ascontiguousarray(np.asarray(v)[rows])) for k, v in params.items()}
