"""Times one ``apply`` batch of iic_amd.seg_kmeans (csrc/seg_kmeans.hip) against the torch composition of what the
reference does, kept on the device, in one process:

  hip  : trunk_dots (x.c_j at the trunk's resolution: iic_seg_head_fwd on the bf16 PT window) + iic_seg_kmeans_label_acc
         (up-sample k channels, arg-min, masked count -- one launch)
  torch: F.interpolate of the 512-channel fp32 feature map to S x S, ||c||^2 - 2 x.c per pixel, argmin, bincount of the
         masked (label, target) pairs

The torch side is generous to the reference, which copies the up-sampled map to the host and runs scikit-learn's
predict there (kmeans_segmentation_eval.py:141-152): here its fp32 NCHW trunk output is already on the device and outside
the timed window.  The batch (--batch) is small enough for the composition's [N, 512, S, S] map to fit.  Before anything
is timed the two sides' labels are compared.  After a warm-up the rounds alternate between the sides; each round puts
device events around --iters back-to-back batches; reported: median and min..max per batch over the rounds.

Then a default ``MiniBatchKMeans(k).fit`` at --fit rows x 512 features: wall clock around fit() + synchronise, next to
scikit-learn's MiniBatchKMeans with the same (era) defaults on the host where it is installed.

    python tools/seg_kmeans_perf.py [--shapes potsdam3 coco3 potsdam27 coco27] [--batch 8] [--fit 100000]
                                    [--rounds 9] [--iters 5] [--out FILE]

Needs a GPU; there is no CPU fall-back."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from iic_amd import kmeans, seg_kmeans   # noqa: E402

# name -> (input_sz, k); the trunk's resolution is input_sz / 2 - 4 (one 2x2 max-pool, two dilated 3x3 convs)
SHAPES = {"potsdam3": (200, 3), "coco3": (128, 3), "potsdam27": (200, 27), "coco27": (128, 27)}
C, P = 512, 3


def make_batch(N, S, k, dev, seed=0):
  g = torch.Generator(device=dev)
  g.manual_seed(seed)
  Hl = S // 2 - 4
  centres = torch.randn((k, C), device=dev, generator=g) * 0.1
  which = torch.randint(0, k, (N, Hl + 2 * P, Hl + 2 * P), device=dev, generator=g)
  pt = (centres[which] + 0.05 * torch.randn((N, Hl + 2 * P, Hl + 2 * P, C), device=dev, generator=g)).to(torch.bfloat16)
  targets = torch.randint(0, k, (N, S, S), device=dev, generator=g).to(torch.uint8)
  mask = (torch.rand((N, S, S), device=dev, generator=g) < 0.9).to(torch.uint8)
  return pt.contiguous(), centres.contiguous(), targets, mask, Hl


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", nargs="*", default=["potsdam3", "coco3", "potsdam27", "coco27"])
  ap.add_argument("--batch", type=int, default=8)
  ap.add_argument("--fit", type=int, default=100000)
  ap.add_argument("--rounds", type=int, default=9)
  ap.add_argument("--iters", type=int, default=5)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert args.rounds >= 7
  dev = torch.device("cuda:0")
  lines = []

  def say(s):
    print(s)
    sys.stdout.flush()
    lines.append(s)

  say("device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
  for name in args.shapes:
    S, k = SHAPES[name]
    N = args.batch
    pt, centres, targets, mask, Hl = make_batch(N, S, k, dev)
    cnorm = (centres * centres).sum(1).contiguous()
    counts = torch.zeros((k * k + 1,), dtype=torch.long, device=dev)
    labels = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
    feat = pt[:, P:P + Hl, P:P + Hl, :].float().permute(0, 3, 1, 2).contiguous()      # the reference's trunk output
    sel = mask.bool()

    def hip_side(want_labels=False):
      seg_kmeans.label_acc(seg_kmeans.trunk_dots(pt, centres), cnorm, targets, mask, k, counts, S,
                           labels_u8=labels if want_labels else None)

    def torch_side():
      up = F.interpolate(feat, size=S, mode="bilinear", align_corners=False)
      score = cnorm[None, :, None, None] - 2.0 * torch.einsum("nchw,kc->nkhw", up, centres)
      lab = torch.argmin(score, dim=1)
      return lab, torch.bincount(lab[sel] * k + targets[sel].long(), minlength=k * k)

    hip_side(want_labels=True)
    lt, ct = torch_side()
    torch.cuda.synchronize()
    differ = int((labels.long() != lt).sum())
    say("%s (N %d, S %d, trunk %d x %d, k %d): labels that differ between the sides %d of %d; count cells that differ %d"
        % (name, N, S, Hl, Hl, k, differ, lt.numel(), int((counts[:-1] != ct).sum())))
    for _ in range(3):
      hip_side()
      torch_side()
    torch.cuda.synchronize()
    times = {"hip": [], "torch": []}
    for _ in range(args.rounds):
      for side, fn in (("hip", hip_side), ("torch", torch_side)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
          fn()
        e1.record()
        e1.synchronize()
        times[side].append(e0.elapsed_time(e1) / args.iters)
    for side in ("hip", "torch"):
      t = np.array(times[side])
      say("%s %-5s: median %.4f ms (min %.4f .. max %.4f) per batch over %d rounds of %d"
          % (name, side, np.median(t), t.min(), t.max(), args.rounds, args.iters))
    say("%s: torch / hip = %.2f; the composition's up-sampled map is %.0f MB, the dots %.2f MB"
        % (name, np.median(times["torch"]) / np.median(times["hip"]), N * C * S * S * 4 / 1e6, N * Hl * Hl * k * 4 / 1e6))
    del pt, feat
    torch.cuda.empty_cache()

  if args.fit > 0:
    n, k = args.fit, 3
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    cen = torch.randn((k, C), device=dev, generator=g) * 1.5
    X = torch.randn((n, C), device=dev, generator=g) + cen[torch.randint(0, k, (n,), device=dev, generator=g)]
    kmeans.MiniBatchKMeans(k).fit(X)      # warm-up
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
      t0 = time.perf_counter()
      km = kmeans.MiniBatchKMeans(k).fit(X)
      torch.cuda.synchronize()
      walls.append(time.perf_counter() - t0)
    say("%dx%dx%d: default MiniBatchKMeans.fit on the device, median %.3f s (min %.3f .. max %.3f) over 5 fits; "
        "%d steps, %d pauses, inertia %.6g" % (n, C, k, np.median(walls), min(walls), max(walls), km.n_steps_,
                                               km.n_pauses_, km.inertia_))
    try:
      from sklearn.cluster import MiniBatchKMeans as SkMB
    except ImportError:
      say("%dx%dx%d: scikit-learn is not installed here" % (n, C, k))
    else:
      Xh = X.cpu().numpy()
      t0 = time.perf_counter()
      sk = SkMB(n_clusters=k, batch_size=100, n_init=3, max_iter=100, random_state=0).fit(Xh)
      t1 = time.perf_counter()
      say("%dx%dx%d: scikit-learn MiniBatchKMeans(batch_size=100, n_init=3) on the host %.3f s, %d steps, inertia %.6g"
          % (n, C, k, t1 - t0, sk.n_steps_, sk.inertia_))
  if args.out:
    with open(args.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
