"""Times the test-time batches of iic_amd.seg_augment (SegTestPreparer, csrc/seg_augment.hip::seg_prepare_test_kernel)
at the two evaluation shapes of tests/test_gpu_seg_test_prep.py::real_case -- Potsdam (75 of 100 images of
200 x 200 x 4, S 200, no_sobel) and COCO-Stuff (120 of 150 images of 96..160 x 96..160 x 3 in 160 x 160 slabs with
`sizes`, S 128, sobel + include_rgb, label masks):

  (1) `batch` (index upload + three allocations + launch) and the kernel alone (iic_seg_prepare_test into preallocated
      outputs) with device events after a warm-up: REPEATS windows of ITERS calls each, median and min..max of the
      per-call time; the achieved bytes/s are the ALGORITHMIC traffic -- source crop and label crop read once,
      4 C + 2 bytes per output pixel written -- over that time;
  (2) two yardsticks from existing code, in the same process and the same windows: the training
      `SegPairedAugmenter.apply` on the same resident arrays at the same batch, S and channel mode (COCO: the slabs as
      uniform 160 x 160 images -- the training side has no `sizes`), and the reference-shaped host path for the same
      batch: `prepare_test_host` per image + stack + the host-to-device copies, single thread, on this machine's host.

    python tools/seg_test_prep_perf.py [--iters 50] [--repeats 7] [--host-batches 3]

Needs a GPU; there is no CPU fall-back."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tests.test_gpu_seg_test_prep import real_case   # noqa: E402
from tools.seg_augment_perf import timed   # noqa: E402


def algorithmic_bytes(prep, idx, sizes):
  """(bytes read, bytes written) of one batch: the part of every source image and label map that falls inside the
  centre crop, once; every fp32 channel plus one target and one mask byte per output pixel."""
  S, C = prep.S, prep.out_channels
  hw = np.tile(np.array([[prep.H, prep.W]]), (len(idx), 1)) if sizes is None else np.asarray(sizes)[idx]
  crop = np.minimum(hw, S).prod(axis=1).sum()
  return int(crop) * (prep.Cs + 1), len(idx) * S * S * (4 * C + 2)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=50)
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--host-batches", type=int, default=3)
  a = ap.parse_args()
  assert torch.cuda.is_available(), "seg_test_prep_perf needs a GPU"
  from iic_amd import _lib, seg_augment as sa
  torch.set_num_threads(1)
  rows = []
  for name in ("potsdam", "coco"):
    prep, images, labels, sizes, ttab, rel, cfg, batch = real_case(name)
    dev = prep.images.device
    idx = np.arange(batch)
    S, C = prep.S, prep.out_channels
    rd, wr = algorithmic_bytes(prep, idx, sizes)

    # kernel alone: preallocated outputs, the index vector already resident
    didx = torch.from_numpy(idx.astype(np.int32)).to(dev)
    o_img = torch.empty(batch, C, S, S, device=dev)
    o_tgt = torch.empty(batch, S, S, device=dev, dtype=torch.uint8)
    o_msk = torch.empty(batch, S, S, device=dev, dtype=torch.uint8)
    L = _lib.lib()

    def kernel():
      _lib.check(L.iic_seg_prepare_test(
        prep.images.data_ptr(), prep.B, prep.H, prep.W, prep.Cs, prep.labels.data_ptr(), _lib.ptr(prep.sizes),
        prep.targets.data_ptr(), _lib.ptr(prep.relevance), didx.data_ptr(), batch, S, int(prep.no_sobel),
        int(prep.include_rgb), prep.lut.data_ptr(), o_img.data_ptr(), o_tgt.data_ptr(), o_msk.data_ptr(),
        _lib.stream_ptr()), "iic_seg_prepare_test")

    # yardstick 1: the training kernel on the same arrays (its own draws, uploaded per call as `apply` does)
    tcfg = types.SimpleNamespace(input_sz=S, no_sobel=cfg.no_sobel, include_rgb=cfg.include_rgb, jitter_brightness=0.4,
                                 jitter_contrast=0.4, jitter_saturation=0.4, jitter_hue=0.125, flip_p=0.5,
                                 use_random_affine=False, use_random_scale=False, pre_scale_all=cfg.pre_scale_all)
    aug = sa.SegPairedAugmenter(prep.images, tcfg, labels_u8=None if rel is None else prep.labels, relevance=rel)
    params = aug.draw(idx)

    bmed, blo, bhi = timed(lambda: prep.batch(idx), a.iters, a.repeats)
    kmed, klo, khi = timed(kernel, a.iters, a.repeats)
    tmed, tlo, thi = timed(lambda: aug.apply(params), a.iters, a.repeats)
    kmed2, klo2, khi2 = timed(kernel, a.iters, a.repeats)          # again after the yardstick: the spread of the box
    got = [t.cpu().numpy() for t in prep.batch(idx)]
    assert got[0].tobytes() == o_img.cpu().numpy().tobytes() and got[1].tobytes() == o_tgt.cpu().numpy().tobytes()

    # yardstick 2: the host path for the same batch
    times = []
    for _ in range(a.host_batches):
      t0 = time.perf_counter()
      res = []
      for i in idx:
        h, w = (prep.H, prep.W) if sizes is None else sizes[i]
        res.append(sa.prepare_test_host(images[i, :h, :w], labels[i, :h, :w], S, cfg.no_sobel, cfg.include_rgb, ttab, rel))
      out = [torch.from_numpy(np.stack([r[k] for r in res])).cuda() for k in range(3)]
      torch.cuda.synchronize()
      times.append(time.perf_counter() - t0)
    assert out[0].cpu().numpy().tobytes() == got[0].tobytes() and out[1].cpu().numpy().tobytes() == got[1].tobytes()
    host_ms = min(times) * 1e3
    row = dict(config=name, batch=batch, S=S, C=C, Cs=prep.Cs, sizes=sizes is not None, read_bytes=rd, write_bytes=wr,
               batch_ms=bmed, batch_min_ms=blo, batch_max_ms=bhi, kernel_ms=kmed, kernel_min_ms=klo, kernel_max_ms=khi,
               kernel_again_ms=kmed2, kernel_again_min_ms=klo2, kernel_again_max_ms=khi2,
               kernel_GBps_algorithmic=(rd + wr) / kmed / 1e6, batch_GBps_algorithmic=(rd + wr) / bmed / 1e6,
               train_apply_ms=tmed, train_apply_min_ms=tlo, train_apply_max_ms=thi, host_path_ms=host_ms,
               images_per_s=batch / bmed * 1e3, host_images_per_s=batch / host_ms * 1e3)
    rows.append(row)
    print("%-8s batch %d, S %d, C %d: algorithmic traffic %d B read + %d B written (4 C + 2 = %d B per pixel)"
          % (name, batch, S, C, rd, wr, 4 * C + 2))
    print("%-8s   batch()      %.3f ms (min %.3f max %.3f)  %.1f GB/s algorithmic  %.0f images/s"
          % (name, bmed, blo, bhi, row["batch_GBps_algorithmic"], row["images_per_s"]))
    print("%-8s   kernel alone %.3f ms (min %.3f max %.3f)  %.1f GB/s algorithmic; again after the yardstick %.3f ms "
          "(min %.3f max %.3f)" % (name, kmed, klo, khi, row["kernel_GBps_algorithmic"], kmed2, klo2, khi2))
    print("%-8s   yardstick: training SegPairedAugmenter.apply, same arrays / batch / S / channels: %.3f ms (min %.3f "
          "max %.3f)" % (name, tmed, tlo, thi))
    print("%-8s   yardstick: host path (prepare_test_host per image + stack + H2D, one thread): %.1f ms per batch = "
          "%.2f ms per image, %.0f images/s" % (name, host_ms, host_ms / batch, row["host_images_per_s"]), flush=True)
  print(json.dumps(rows))


if __name__ == "__main__":
  main()
