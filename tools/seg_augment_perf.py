"""Times iic_amd.seg_augment at the Potsdam-3 (75 x 200 x 200 x 4, no_sobel) and COCO-Stuff-3
(120 x 128 x 128 x 3, sobel + include_rgb, label masks) batch shapes, with and without random affine:

  (1) `paired_batch` (host draw + parameter upload + kernel[s]) and `apply` alone (upload + kernel[s]) with device
      events after a warm-up: REPEATS windows of ITERS calls each, median and min..max of the per-call time; the
      achieved bytes/s are the ALGORITHMIC traffic of the augmentation kernel (crop read once, two fp32 views,
      mask and affine written -- the warp's extra read + write of img2 is reported separately) over that time;
  (2) the reference-shaped host path for the same batch: the numpy + PIL RESTATEMENT of `_prepare_train` in
      tests/test_gpu_seg_augment.py (not the reference itself), per image, single thread, on this machine's host.

    python tools/seg_augment_perf.py [--iters 50] [--repeats 7] [--host-batches 2]

--ragged: instead, the kernel for images of different sizes (iic_seg_augment_ragged, iic_amd/seg_ragged.py) against
iic_seg_augment at the COCO-Stuff-3 shape (batch 120, input_sz 128, sobel + include_rgb, label masks, 24 resident
images around 213 x 160): (a) both kernels on the SAME uniform 160 x 213 data and parameters, outputs compared byte for
byte first; (b) the ragged kernel on a pack of genuinely different sizes; (c) the same pack with use_random_scale.
Kernel alone (parameters resident, outputs preallocated) and `apply` (parameter upload, tap tables, allocations, launch),
one process, the variants interleaved window by window: REPEATS windows of ITERS calls each per variant.

    python tools/seg_augment_perf.py --ragged [--iters 1000] [--repeats 9]

--ragged --prescaled: instead, pre_scale_all from the ORIGINAL images (SegRaggedAugmenter(source="original")) at the same
COCO-Stuff-3 shape, 24 resident originals with sides 427..640, pre_scale_factor 0.33: (a) the parent's use_random_scale
row re-measured -- the single-stage kernel over the pre-scaled pack seg_prescale.prescale_dataset makes; (b) the
single-stage kernel over the originals (pre_scale_all without random scale); (c) the two-stage kernel
(iic_seg_augment_ragged_prescaled: pre_scale_all, then use_random_scale).  A few samples of (b) and (c) are compared byte
for byte with the host pipeline of tests/seg_prescale_cases.py before anything is timed.

    python tools/seg_augment_perf.py --ragged --prescaled [--iters 1000] [--repeats 9]

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


def interleaved(fns, iters, repeats):
  """{name: (median, min, max) ms per call}: after a warm-up of every variant, `repeats` rounds, each timing one window
  of `iters` calls of every variant in turn with device events."""
  for fn in fns.values():
    for _ in range(5):
      fn()
  torch.cuda.synchronize()
  out = {k: [] for k in fns}
  for _ in range(repeats):
    for k, fn in fns.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(iters):
        fn()
      e1.record()
      torch.cuda.synchronize()
      out[k].append(e0.elapsed_time(e1) / iters)
  return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in out.items()}


def ragged_mode(a):
  import types
  from iic_amd import _lib, seg_augment as sa, seg_ragged as sr
  dev = torch.device("cuda:0")
  L = _lib.lib()
  B, batch, S, H, W = 24, 120, 128, 160, 213
  rng = np.random.default_rng(2024)
  rel = (np.arange(256) >= 91).astype(np.uint8)
  rel[182:] = 0

  def cfg(scale=False):
    return types.SimpleNamespace(input_sz=S, no_sobel=False, include_rgb=True, jitter_brightness=0.4, jitter_contrast=0.4,
                                 jitter_saturation=0.4, jitter_hue=0.125, flip_p=0.5, use_random_affine=False,
                                 use_random_scale=scale, scale_min=0.6, scale_max=1.4, pre_scale_all=not scale)

  def content(shapes):
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    labels = [rng.integers(0, 182, s).astype(np.uint8) for s in shapes]
    return imgs, labels
  imgs, labels = content([(H, W)] * B)
  uni = sa.SegPairedAugmenter(torch.from_numpy(np.stack(imgs)).to(dev), cfg(),
                              labels_u8=torch.from_numpy(np.stack(labels)).to(dev), relevance=rel, seed=1)
  rag = sr.SegRaggedAugmenter(imgs, cfg(), labels=labels, relevance=rel, seed=1, device=dev)
  # around 213 x 160, landscape and portrait, some sides below input_sz (padded)
  shapes = [(int(h), int(w)) for h, w in zip(rng.integers(110, 215, B), rng.integers(110, 260, B))]
  mimgs, mlabels = content(shapes)
  mixed = sr.SegRaggedAugmenter(mimgs, cfg(), labels=mlabels, relevance=rel, seed=1, device=dev)
  scaled = sr.SegRaggedAugmenter(mimgs, cfg(True), labels=mlabels, relevance=rel, seed=1, device=dev)
  idx = np.random.default_rng(5).integers(0, B, batch)
  p = uni.draw(idx)
  pr = dict(p, scale=None)
  pm, ps = mixed.draw(idx), scaled.draw(idx)
  for x, y in zip(uni.apply(p), rag.apply(pr)):      # faster and different is not faster
    assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), "ragged kernel differs from iic_seg_augment"
  C = uni.out_channels
  outs = (torch.empty(batch, C, S, S, device=dev), torch.empty(batch, C, S, S, device=dev),
          torch.empty(batch, S, S, device=dev, dtype=torch.uint8), torch.empty(batch, 2, 3, device=dev))

  def resident(params):
    return (torch.from_numpy(np.ascontiguousarray(params["iparams"])).to(dev),
            torch.from_numpy(np.ascontiguousarray(params["fparams"])).to(dev))

  def uniform_kernel(ipfp):
    ip, fp = ipfp
    return lambda: _lib.check(L.iic_seg_augment(
      uni.images.data_ptr(), uni.B, uni.H, uni.W, uni.Cs, uni.labels.data_ptr(), uni.relevance.data_ptr(), ip.data_ptr(),
      fp.data_ptr(), batch, S, 0, 1, uni.lut.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
      outs[3].data_ptr(), _lib.stream_ptr()), "iic_seg_augment")

  def ragged_kernel(aug, ipfp, taps=None):
    ip, fp = ipfp
    return lambda: _lib.check(L.iic_seg_augment_ragged(
      aug.images.data_ptr(), aug.offsets.data_ptr(), aug.sizes.data_ptr(), aug.B, aug.total, aug.Cs,
      aug.labels.data_ptr(), aug.relevance.data_ptr(), ip.data_ptr(), fp.data_ptr(), _lib.ptr(taps), batch, S, 0, 1,
      aug.lut.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
      _lib.stream_ptr()), "iic_seg_augment_ragged")
  src = scaled.sizes_host[ps["iparams"][:, 0]]
  t = np.stack([sr.crop_taps(src[:, 0], ps["scale"], ps["iparams"][:, 2], S),
                sr.crop_taps(src[:, 1], ps["scale"], ps["iparams"][:, 1], S)], 1)
  taps = torch.from_numpy(np.ascontiguousarray(t).view(np.int32).reshape(batch, 2, S, 6)).to(dev)
  kern_bytes = batch * (S * S * (3 + 1) + 2 * C * S * S * 4 + S * S + 24)
  variants = [
    ("kernel", {"uniform iic_seg_augment": uniform_kernel(resident(p)),
                "ragged, uniform data": ragged_kernel(rag, resident(pr)),
                "ragged, mixed sizes": ragged_kernel(mixed, resident(pm)),
                "ragged, mixed + random scale": ragged_kernel(scaled, resident(ps), taps)}),
    ("apply", {"uniform iic_seg_augment": lambda: uni.apply(p),
               "ragged, uniform data": lambda: rag.apply(pr),
               "ragged, mixed sizes": lambda: mixed.apply(pm),
               "ragged, mixed + random scale": lambda: scaled.apply(ps)}),
  ]
  print("COCO-Stuff-3 shape: batch %d, input_sz %d, C %d, %d resident images; uniform %d x %d; mixed %d..%d x %d..%d; "
        "%d windows of %d calls per variant, interleaved: median (min, max) per call"
        % (batch, S, C, B, H, W, min(s[0] for s in shapes), max(s[0] for s in shapes), min(s[1] for s in shapes),
           max(s[1] for s in shapes), a.repeats, a.iters))
  rows = []
  for what, fns in variants:
    iters = a.iters if what == "kernel" else max(1, a.iters // 10)
    res = interleaved(fns, iters, a.repeats)
    base = res["uniform iic_seg_augment"][0]
    for k, (med, lo, hi) in res.items():
      rows.append(dict(what=what, variant=k, ms=med, min_ms=lo, max_ms=hi, ratio_to_uniform=med / base,
                       GBps_algorithmic=kern_bytes / med / 1e6))
      print("%-6s %-30s %.4f ms (min %.4f max %.4f)  x%.3f of uniform  %.0f GB/s algorithmic"
            % (what, k, med, lo, hi, med / base, kern_bytes / med / 1e6), flush=True)
  t0 = time.perf_counter()
  for _ in range(20):
    scaled.draw(idx)
  print("host: draw with random scale %.3f ms per batch of %d" % ((time.perf_counter() - t0) / 20 * 1e3, batch))
  print(json.dumps(rows))


def prescaled_mode(a):
  import types
  from iic_amd import _lib, seg_prescale as sp, seg_ragged as sr
  from tests import seg_prescale_cases as cases
  dev = torch.device("cuda:0")
  L = _lib.lib()
  B, batch, S, factor = 24, 120, 128, 0.33
  rng = np.random.default_rng(2025)
  rel = (np.arange(256) >= 91).astype(np.uint8)
  rel[182:] = 0

  def cfg(scale, pre):
    return types.SimpleNamespace(input_sz=S, no_sobel=False, include_rgb=True, jitter_brightness=0.4, jitter_contrast=0.4,
                                 jitter_saturation=0.4, jitter_hue=0.125, flip_p=0.5, use_random_affine=False,
                                 use_random_scale=scale, scale_min=0.6, scale_max=1.4, pre_scale_all=pre,
                                 pre_scale_factor=factor)
  shapes = [(int(h), int(w)) for h, w in zip(rng.integers(427, 641, B), rng.integers(427, 641, B))]
  imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
  labels = [rng.integers(0, 182, s).astype(np.uint8) for s in shapes]
  px, lab, nsz, noff = sp.prescale_dataset(imgs, labels=labels, factor=factor, device=dev)
  # (a) what the parent commit offers: the pre-scaled pack resident, the random scale on the truncated image
  resident = sr.SegRaggedAugmenter(px, cfg(True, False), labels=lab, relevance=rel, sizes=nsz, offsets=noff, seed=1)
  one = sr.SegRaggedAugmenter(imgs, cfg(False, True), labels=labels, relevance=rel, seed=1, device=dev, source="original")
  two = sr.SegRaggedAugmenter(imgs, cfg(True, True), labels=labels, relevance=rel, seed=1, device=dev, source="original")
  idx = np.random.default_rng(5).integers(0, B, batch)
  pa, pb, pc = resident.draw(idx), one.draw(idx), two.draw(idx)
  for aug, params, scale in ((one, pb, False), (two, pc, True)):     # faster and different is not faster
    few = cases.take(params, [0, 1, 2, 3])
    got = [t.cpu().numpy() for t in aug.apply(few)]
    want = cases.host_pipeline(imgs, labels, rel, cfg(scale, True), few, factor)
    for k, w in enumerate(want):
      assert all(got[j][k].tobytes() == w[j].tobytes() for j in range(4)), "kernel differs from the host pipeline"
  C = two.out_channels
  outs = (torch.empty(batch, C, S, S, device=dev), torch.empty(batch, C, S, S, device=dev),
          torch.empty(batch, S, S, device=dev, dtype=torch.uint8), torch.empty(batch, 2, 3, device=dev))

  def kernel(aug, params, stages):
    ip = torch.from_numpy(np.ascontiguousarray(params["iparams"])).to(dev)
    fp = torch.from_numpy(np.ascontiguousarray(params["fparams"])).to(dev)
    src = aug.sizes_host[params["iparams"][:, 0]]
    y0, x0 = params["iparams"][:, 2], params["iparams"][:, 1]
    if stages == 2:
      t = np.stack([sr.crop_taps2(src[:, 0], factor, params["scale"], y0, S),
                    sr.crop_taps2(src[:, 1], factor, params["scale"], x0, S)], 1)
      entry, width = L.iic_seg_augment_ragged_prescaled, 12
    else:
      sc = params["scale"] if params["scale"] is not None else np.full(batch, factor)
      t = np.stack([sr.crop_taps(src[:, 0], sc, y0, S), sr.crop_taps(src[:, 1], sc, x0, S)], 1)
      entry, width = L.iic_seg_augment_ragged, 6
    taps = torch.from_numpy(np.ascontiguousarray(t).view(np.int32).reshape(batch, 2, S, width)).to(dev)
    return lambda: _lib.check(entry(
      aug.images.data_ptr(), aug.offsets.data_ptr(), aug.sizes.data_ptr(), aug.B, aug.total, aug.Cs,
      aug.labels.data_ptr(), aug.relevance.data_ptr(), ip.data_ptr(), fp.data_ptr(), taps.data_ptr(), batch, S, 0, 1,
      aug.lut.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
      _lib.stream_ptr()), "ragged kernel")
  names = ("resident pre-scaled pack + random scale (parent)", "originals, pre_scale_all (one stage)",
           "originals, pre_scale_all + random scale (two stages)")
  variants = [("kernel", dict(zip(names, (kernel(resident, pa, 1), kernel(one, pb, 1), kernel(two, pc, 2))))),
              ("apply", dict(zip(names, (lambda: resident.apply(pa), lambda: one.apply(pb), lambda: two.apply(pc)))))]
  print("COCO-Stuff-3 shape: batch %d, input_sz %d, C %d, %d resident originals %d..%d x %d..%d, pre_scale_factor %.2f; "
        "%d windows of %d calls per variant, interleaved: median (min, max) per call"
        % (batch, S, C, B, min(s[0] for s in shapes), max(s[0] for s in shapes), min(s[1] for s in shapes),
           max(s[1] for s in shapes), factor, a.repeats, a.iters))
  rows = []
  for what, fns in variants:
    iters = a.iters if what == "kernel" else max(1, a.iters // 10)
    res = interleaved(fns, iters, a.repeats)
    base = res[names[0]][0]
    for k, (med, lo, hi) in res.items():
      rows.append(dict(what=what, variant=k, ms=med, min_ms=lo, max_ms=hi, ratio_to_parent=med / base))
      print("%-6s %-52s %.4f ms (min %.4f max %.4f)  x%.3f of the parent's row" % (what, k, med, lo, hi, med / base),
            flush=True)
  print(json.dumps(rows))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=None)
  ap.add_argument("--repeats", type=int, default=None)
  ap.add_argument("--host-batches", type=int, default=2)
  ap.add_argument("--ragged", action="store_true")
  ap.add_argument("--prescaled", action="store_true", help="with --ragged: pre_scale_all from the original images")
  a = ap.parse_args()
  assert torch.cuda.is_available(), "seg_augment_perf needs a GPU"
  torch.set_num_threads(1)
  if a.ragged:
    a.iters, a.repeats = a.iters or 1000, a.repeats or 9
    return prescaled_mode(a) if a.prescaled else ragged_mode(a)
  a.iters, a.repeats = a.iters or 50, a.repeats or 7
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
