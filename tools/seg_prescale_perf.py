"""Times the device pre-scale pass (iic_seg_prescale, iic_amd/seg_prescale.py) on a synthetic pack of COCO-sized images:
sides 427..640, pre_scale_factor 0.33 (every published COCO-Stuff command).

  (1) the kernel through prescale_dataset's launch on the resident pack (tables uploaded per call, as a user calls it),
      device events after a warm-up, ROUNDS windows of ITERS calls: median (min..max) ms per call, and the achieved
      bytes/s counted as the whole source pack (pixels and labels) read once plus the destination written once -- at
      this factor every source cache line is touched;
  (2) the host restatement (seg_prescale.prescale_host, numpy, one thread) per image on this machine's CPU;
  both projected to the 36 k and 49 k images of the COCO-Stuff-3 and COCO-Stuff-15 training sets.
The output of the timed configuration is compared with the host restatement on a few images first.

    python tools/seg_prescale_perf.py [--images 2000] [--iters 20] [--rounds 9] [--host-images 8]

Needs a GPU; there is no CPU fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
HBM_GBPS = 8000.0          # the HBM specification README.md sets the BatchNorm passes against (they reach 5.2 TB/s)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--images", type=int, default=2000)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--rounds", type=int, default=9)
  ap.add_argument("--host-images", type=int, default=8)
  ap.add_argument("--factor", type=float, default=0.33)
  a = ap.parse_args()
  assert torch.cuda.is_available(), "seg_prescale_perf needs a GPU"
  from iic_amd import seg_prescale as sp, seg_ragged as sr
  torch.set_num_threads(1)
  dev = torch.device("cuda:0")
  rng = np.random.default_rng(7)
  sizes = np.stack([rng.integers(427, 641, a.images), rng.integers(427, 641, a.images)], 1).astype(np.int32)
  area = sizes[:, 0].astype(np.int64) * sizes[:, 1]
  total = int(area.sum())
  offsets = np.concatenate([[0], np.cumsum(area)[:-1]]).astype(np.int64)
  gen = torch.Generator(device=dev).manual_seed(3)
  px = torch.randint(0, 256, (total, 3), dtype=torch.uint8, device=dev, generator=gen)
  lab = torch.randint(0, 182, (total,), dtype=torch.uint8, device=dev, generator=gen)
  run = lambda: sp.prescale_dataset(px, sizes=sizes, offsets=offsets, labels=lab, factor=a.factor)      # noqa: E731
  out, olab, nsz, noff = run()
  few = list(range(0, a.images, max(1, a.images // 4)))[:4]
  for i in few:                                                # faster and different is not faster
    im = px[offsets[i]:offsets[i] + area[i]].cpu().numpy().reshape(sizes[i, 0], sizes[i, 1], 3)
    lb = lab[offsets[i]:offsets[i] + area[i]].cpu().numpy().reshape(sizes[i, 0], sizes[i, 1])
    wi, wl = sp.prescale_host(im, lb, a.factor)
    n = int(nsz[i, 0]) * int(nsz[i, 1])
    assert out[noff[i]:noff[i] + n].cpu().numpy().tobytes() == wi.tobytes(), "kernel differs from prescale_host"
    assert olab[noff[i]:noff[i] + n].cpu().numpy().tobytes() == wl.tobytes(), "kernel differs from prescale_host"
  src_bytes, dst_bytes = total * 4, int(out.shape[0]) * 4
  torch.cuda.synchronize()
  ms = []
  for _ in range(a.rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
      run()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1) / a.iters)
  med, lo, hi = float(np.median(ms)), float(min(ms)), float(max(ms))
  gbps = (src_bytes + dst_bytes) / med / 1e6
  t = []
  for i in few[:a.host_images] + list(range(1, 1 + max(0, a.host_images - len(few)))):
    im = px[offsets[i]:offsets[i] + area[i]].cpu().numpy().reshape(sizes[i, 0], sizes[i, 1], 3)
    lb = lab[offsets[i]:offsets[i] + area[i]].cpu().numpy().reshape(sizes[i, 0], sizes[i, 1])
    t0 = time.perf_counter()
    sp.prescale_host(im, lb, a.factor)
    t.append((time.perf_counter() - t0) * 1e3)
  host_ms = float(np.median(t))
  print("%d images %d..%d x %d..%d, factor %.2f: source %.1f MB (pixels + labels), destination %.1f MB, %d work items"
        % (a.images, sizes[:, 0].min(), sizes[:, 0].max(), sizes[:, 1].min(), sizes[:, 1].max(), a.factor, src_bytes / 1e6,
           dst_bytes / 1e6, sp.work_list(nsz.numpy()).shape[0]))
  print("device pass: %.3f ms (min %.3f max %.3f) over %d windows of %d calls = %.4f ms per image; %.0f GB/s of source read "
        "once + destination written once = %.1f %% of the %.0f GB/s HBM specification" % (med, lo, hi, a.rounds, a.iters, med / a.images, gbps,
                                                                    100 * gbps / HBM_GBPS, HBM_GBPS))
  print("host restatement (numpy, one thread): %.2f ms per image (median of %d)" % (host_ms, len(t)))
  for n in (36000, 49000):
    print("projected to %d images: device %.2f s (kernel only, the upload not included), host %.0f s"
          % (n, med / a.images * n / 1e3, host_ms * n / 1e3))
  print(json.dumps(dict(images=a.images, factor=a.factor, ms=med, min_ms=lo, max_ms=hi, GBps=gbps, src_bytes=src_bytes,
                        dst_bytes=dst_bytes, host_ms_per_image=host_ms)))


if __name__ == "__main__":
  main()
