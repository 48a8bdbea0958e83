"""Times iic_amd.seg_augment at the Potsdam-3 (75 x 200 x 200 x 4, no_sobel) and COCO-Stuff-3
(120 x 128 x 128 x 3, sobel + include_rgb, label masks) batch shapes, with and without random affine:

  (1) `paired_batch` (host draw + parameter upload + kernel[s]) and `apply` alone (upload + kernel[s]) with device
      events after a warm-up: REPEATS windows of ITERS calls each, median and min..max of the per-call time; the
      achieved bytes/s are the ALGORITHMIC traffic of the augmentation kernel (crop read once, two fp32 views,
      mask and affine written -- the warp's extra read + write of img2 is reported separately) over that time;
  (2) the reference-shaped host path for the same batch: the numpy + PIL RESTATEMENT of `_prepare_train` in
      tests/test_gpu_seg_augment.py (not the reference itself), per image, single thread, on this machine's host.

    python tools/seg_augment_perf.py [--iters 50] [--repeats 7] [--host-batches 2]

Needs a GPU; there is no CPU fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tests.test_gpu_seg_augment import REAL, real_case, restate_prepare_train   # noqa: E402


def timed(fn, iters, repeats):
  for _ in range(5):
    fn()
  torch.cuda.synchronize()
  out = []
  for _ in range(repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
      fn()
    e1.record()
    torch.cuda.synchronize()
    out.append(e0.elapsed_time(e1) / iters)
  return float(np.median(out)), float(min(out)), float(max(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=50)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--host-batches", type=int, default=2)
  a = ap.parse_args()
  assert torch.cuda.is_available(), "seg_augment_perf needs a GPU"
  torch.set_num_threads(1)
  rows = []
  for case in REAL:
    name, batch = case[0], case[1]
    for affine in (False, True):
      aug, imgs, labels, rel, cfg = real_case(*case, affine=affine)
      idx = np.random.default_rng(5).integers(0, imgs.shape[0], batch)
      p = aug.draw(idx)
      S, C, cs = aug.S, aug.out_channels, aug.Cs
      kern_bytes = batch * (S * S * (cs + (1 if labels is not None else 0)) + 2 * C * S * S * 4 + S * S + 24)
      warp_bytes = batch * 2 * C * S * S * 4 if affine else 0
      med, lo, hi = timed(lambda: aug.paired_batch(idx), a.iters, a.repeats)
      amed, alo, ahi = timed(lambda: aug.apply(p), a.iters, a.repeats)
      t0 = time.perf_counter()
      for _ in range(20):
        aug.draw(idx)
      draw_ms = (time.perf_counter() - t0) / 20 * 1e3
      row = dict(config=name, batch=batch, S=S, C=C, random_affine=affine, paired_batch_ms=med, paired_batch_min_ms=lo,
                 paired_batch_max_ms=hi, apply_ms=amed, apply_min_ms=alo, apply_max_ms=ahi, host_draw_ms=draw_ms,
                 kernel_algorithmic_bytes=kern_bytes, warp_extra_bytes=warp_bytes,
                 apply_GBps_algorithmic=kern_bytes / amed / 1e6, pairs_per_s=batch / med * 1e3)
      rows.append(row)
      print("%-9s affine=%d  paired_batch %.3f ms (min %.3f max %.3f)  apply %.3f ms (min %.3f max %.3f)  draw %.3f ms  "
            "%.1f GB/s algorithmic (apply; %d B + warp %d B)  %.0f pairs/s"
            % (name, affine, med, lo, hi, amed, alo, ahi, draw_ms, row["apply_GBps_algorithmic"], kern_bytes, warp_bytes,
               row["pairs_per_s"]), flush=True)
    # (2) the restatement of the reference-shaped host path: per image, single thread, including the host-to-device
    # copies of the four results the reference makes per image
    aug, imgs, labels, rel, cfg = real_case(*case)
    idx = np.random.default_rng(5).integers(0, imgs.shape[0], batch)
    p = aug.draw(idx)
    times = []
    for _ in range(a.host_batches):
      t0 = time.perf_counter()
      for i in range(batch):
        src = int(idx[i])
        v = restate_prepare_train(imgs[src], None if labels is None else labels[src], rel, p["iparams"][i], p["fparams"][i],
                                  aug.S, cfg.no_sobel, cfg.include_rgb)
        for t in v:
          torch.from_numpy(np.ascontiguousarray(t)).cuda()
      torch.cuda.synchronize()
      times.append(time.perf_counter() - t0)
    host_ms = min(times) * 1e3
    rows.append(dict(config=name, batch=batch, host_restatement_ms=host_ms, host_restatement_pairs_per_s=batch / host_ms * 1e3))
    print("%-9s host restatement (numpy + PIL, per image, one thread): %.1f ms per batch of %d = %.2f ms per pair, %.0f pairs/s"
          % (name, host_ms, batch, host_ms / batch, batch / host_ms * 1e3), flush=True)
  print(json.dumps(rows))


if __name__ == "__main__":
  main()
