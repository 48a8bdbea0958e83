"""Times csrc/augment.hip on the north-star batch shape (STL10 96x96x3 sources, crop 84 -> 96,
include_rgb): 660 tf1 views + 660 tf2 views per training step.  Algorithmic bytes per output
image: crop read 84*84*3 + output write 4*96*96*4.

--affine_p P (repeatable) adds, per P, the tf2 batch of the semi-supervised script with RandomAffine at probability P
(csrc/augment_affine.hip; P = 0 launches iic_augment, as the public class does for a batch without an affine row), each
timed --repeats times so that the run-to-run spread stands next to the number, and --pil_affine times what the kernel
replaces on the host: PIL's Image.transform on --n crops of 84 x 84."""
import argparse
import sys
import os
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from iic_amd.augment import PairedAugmenter   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=660)
ap.add_argument("--dataset", type=int, default=8192)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--affine_p", type=float, action="append", default=[],
                help="also time the jittered batch with random_affine at this probability (repeatable)")
ap.add_argument("--repeats", type=int, default=5, help="timed windows per --affine_p line (min / median / max printed)")
ap.add_argument("--pil_affine", action="store_true", help="time PIL's bilinear affine of --n 84x84 crops on the host")
a = ap.parse_args()
g = torch.Generator().manual_seed(0)
imgs = torch.randint(0, 256, (a.dataset, 96, 96, 3), dtype=torch.uint8, generator=g).cuda()
aug = PairedAugmenter(imgs, 84, 96, True, seed=0)
idx = np.random.RandomState(0).randint(0, a.dataset, a.n)
byts = a.n * (84 * 84 * 3 + 4 * 96 * 96 * 4)


def window(aug_, params):
  """ms per launch (incl. the parameter upload) over one window of --iters launches."""
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(a.iters):
    aug_.apply(*params)
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / a.iters


for mode in ("plain", "jittered"):
  params = aug.draw(idx, mode)
  aug.apply(*params)
  torch.cuda.synchronize()
  ms = window(aug, params)
  print("%-9s n=%d  %.3f ms/launch (incl. param upload)  %.1f GB/s algorithmic  %.0f images/s"
        % (mode, a.n, ms, byts / ms / 1e6, a.n / ms * 1e3))
t0 = time.time()
for _ in range(10):
  aug.draw(idx, "jittered")
print("host draw (jittered, n=%d): %.3f ms" % (a.n, (time.time() - t0) * 100))

for p in a.affine_p:
  aff = PairedAugmenter(imgs, 84, 96, True, seed=0, random_affine=True, affine_p=p)
  params = aff.draw(idx, "jittered")
  rows = int(((params[0][:, 11] & 2) != 0).sum())
  aff.apply(*params)
  torch.cuda.synchronize()
  ms = sorted(window(aff, params) for _ in range(a.repeats))
  med = ms[len(ms) // 2]
  print("affine_p=%.2f n=%d (%d affined rows, %s)  min %.3f  median %.3f  max %.3f ms/launch (incl. param upload)  "
        "%.0f images/s" % (p, a.n, rows, "iic_augment_affine" if rows else "iic_augment", ms[0], med, ms[-1],
                           a.n / med * 1e3))
  t0 = time.time()
  for _ in range(10):
    aff.draw(idx, "jittered")
  print("host draw (jittered, affine_p=%.2f, n=%d): %.3f ms" % (p, a.n, (time.time() - t0) * 100))

if a.pil_affine:
  from PIL import Image
  from iic_amd.augment import inverse_affine_matrix
  rs = np.random.RandomState(1)
  crops = [Image.fromarray(rs.randint(0, 256, (84, 84, 3)).astype(np.uint8)) for _ in range(a.n)]
  mats = [tuple(inverse_affine_matrix((42.5, 42.5), rs.uniform(-18, 18), (float(np.round(rs.uniform(-8.4, 8.4))),
                                                                        float(np.round(rs.uniform(-8.4, 8.4)))),
                                      rs.uniform(0.9, 1.1), rs.uniform(-10, 10))) for _ in range(a.n)]
  ts = []
  for _ in range(a.repeats):
    t0 = time.time()
    for c, m in zip(crops, mats):
      c.transform(c.size, Image.AFFINE, m, Image.BILINEAR, fillcolor=0)
    ts.append((time.time() - t0) * 1e3)
  ts.sort()
  print("host PIL transform (AFFINE, BILINEAR) of %d crops 84x84, one thread: min %.2f  median %.2f  max %.2f ms"
        % (a.n, ts[0], ts[len(ts) // 2], ts[-1]))
