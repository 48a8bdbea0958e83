"""Times the supervised head of the semi-supervised step (iic_amd.semisup, csrc/sup_head.hip) against what the package ran
before it existed, both sides on the same device in one process, alternating after a warm-up:

(a) head forward + backward from layer 3's bf16 PT tensor to every gradient (head parameters and the PT tensor's):
      baseline  ops.pt_to_nchw(x, 1).reshape(N, -1) -> torch.nn Linear / BatchNorm1d / ReLU / Linear -> nn.CrossEntropyLoss
      new       the autograd Functions of iic_amd.linear / iic_amd.semisup over the iic_sup_* kernels + cross_entropy;
                `new` re-writes the bf16 weight operands every step (what a training step pays: once per optimiser step),
                `new_no_prep` re-uses them (an evaluation forward's cost is not timed here; this isolates the products)
    Wall time of a step that starts and ends with a device synchronise; median, min, max over the repeats.  FLOP of the
    three products of the first Linear: 3 * 2 N K F; "share" = that over the step's time over the bf16 MFMA peak
    (2.5e15 FLOP/s, MI355X) -- a whole-step figure, not a kernel's.
(b) one ten-crop evaluation pass over a synthetic resident uint8 set:
      baseline  per image PIL TenCrop + grey -> tensor on the host, one batch tensor copied to the device, the same
                forwards, logits copied back with .cpu().numpy() per batch, numpy sum / argmax at the end (assess_acc_block)
      new       TenCropEvaluator.accuracy
    Both must return the same accuracy.  Launches / copies / synchronisations OUTSIDE the network's forward, per batch,
    counted from the code paths: baseline 1 host-to-device copy of the crops, 1 Sobel launch, 1 device-to-host copy that
    synchronises; new 2 small parameter copies, 1 crop launch, 1 Sobel launch, 1 count launch, no synchronisation (one
    per pass, in result()).

    python tools/sup_head_perf.py [--n 700 100] [--repeats 9] [--images 8000] [--skip_eval] [--out FILE]

Needs a GPU; there is no CPU fall-back."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from iic_amd import archs, linear, ops, semisup             # noqa: E402
from iic_amd.transforms import sobel_process                # noqa: E402

BF16_PEAK = 2.5e15


def wall_ms(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3


def interleaved(forms, repeats, warmup=2):
  for _ in range(warmup):
    for fn in forms.values():
      fn()
  times = {name: [] for name in forms}
  for _ in range(repeats):
    for name, fn in forms.items():
      times[name].append(wall_ms(fn))
  return {name: (float(np.median(t)), float(min(t)), float(max(t))) for name, t in times.items()}


def head_step_forms(N, C, HW, F, k, dev):
  g = torch.Generator().manual_seed(N)
  x = torch.zeros((N, HW + 2, HW + 2, C), dtype=torch.bfloat16)
  x[:, 1:-1, 1:-1] = torch.relu(torch.randn((N, HW, HW, C), generator=g)).to(torch.bfloat16)
  x_pt = x.to(dev).requires_grad_(True)
  targets = torch.randint(0, k, (N,), generator=g).to(dev)
  head = nn.Sequential(nn.Linear(C * HW * HW, F), nn.BatchNorm1d(F), nn.ReLU(), nn.Linear(F, k)).to(dev).train()
  with torch.no_grad():
    head[0].weight.normal_(0, 0.01)
  crit = nn.CrossEntropyLoss()
  operands = linear.PTLinearOperands()

  def clear():
    for p in head.parameters():
      p.grad = None
    if x_pt.grad is not None:
      ops.POOL.release(x_pt.grad)
      x_pt.grad = None

  def baseline():
    clear()
    loss = crit(head(ops.pt_to_nchw(x_pt, 1).reshape(N, -1)), targets)
    loss.backward()
    return loss

  def new_no_prep():
    clear()
    lin1, bn, _, lin2 = head
    h = linear.PTLinearFn.apply(x_pt, lin1.weight, lin1.bias, operands)
    h = semisup._BNReLUFn.apply(h, bn.weight, bn.bias, bn)
    loss = semisup._CrossEntropyFn.apply(linear.LinearF32Fn.apply(h, lin2.weight, lin2.bias), targets)
    loss.backward()
    return loss

  def new():
    ops.bump_weights_epoch()          # as after an optimiser step: the operands are stale
    return new_no_prep()

  return dict(baseline=baseline, new=new, new_no_prep=new_no_prep), head, x_pt


def eval_forms(images, S, dev, per_batch):
  from PIL import Image
  B = images.shape[0]
  cfg = types.SimpleNamespace(in_channels=2, input_sz=S, batchnorm_track=True, num_sub_heads=1, output_k=10)
  net = archs.ClusterNet5g(cfg).to(dev)
  hw = {96: 13, 64: 9, 32: 5}[S]
  sh = semisup.SupHead5(net, dlen=256 * hw * hw, gt_k=10).eval()
  targets = np.random.default_rng(1).integers(0, 10, B)
  ev = semisup.TenCropEvaluator(images, targets, S, False)
  host = images.cpu().numpy()
  W = host.shape[2]
  c = int(round((W - S) / 2.))
  boxes = [(0, 0), (W - S, 0), (0, W - S), (W - S, W - S), (c, c)]

  def ten(img):
    out = []
    for im in (img, img.transpose(Image.FLIP_LEFT_RIGHT)):
      for x0, y0 in boxes:
        grey = np.asarray(im.crop((x0, y0, x0 + S, y0 + S)).convert("L")).astype(np.float32) / np.float32(255)
        out.append(grey[None])
    return out

  def baseline():
    al, total = None, 0
    with torch.no_grad():
      for s in range(0, B, per_batch):
        crops = np.stack([t for i in range(s, min(B, s + per_batch)) for t in ten(Image.fromarray(host[i]))])
        out = sh(sobel_process(torch.from_numpy(crops).to(dev), False), penultimate_features=True)
        if al is None:
          al = np.zeros((B * 10, out.shape[1]))
        al[total:total + out.shape[0]] = out.cpu().numpy()
        total += out.shape[0]
    al = al.reshape((B, 10, -1)).sum(axis=1) / 10.0
    return float((np.argmax(al, axis=1) == targets).sum() / float(B))

  def new():
    return ev.accuracy(sh, images_per_batch=per_batch, penultimate_features=True)

  return dict(baseline=baseline, new=new)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--n", type=int, nargs="+", default=[700, 100])
  ap.add_argument("--repeats", type=int, default=9)
  ap.add_argument("--images", type=int, default=8000)
  ap.add_argument("--eval_repeats", type=int, default=2)
  ap.add_argument("--skip_eval", action="store_true")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  assert torch.cuda.is_available(), "sup_head_perf needs a GPU"
  dev = torch.device("cuda:0")
  rows = []
  C, HW, F, k = 256, 9, 2048, 10
  for N in a.n:
    forms, head, x_pt = head_step_forms(N, C, HW, F, k, dev)
    # same result first: loss and gradient norms of the two routes (bf16 operands against fp32: the bf16 tier)
    lb = float(forms["baseline"]().detach())
    gb = {n: float(p.grad.norm()) for n, p in head.named_parameters()}
    gxb = float(x_pt.grad.float().norm())
    ln = float(forms["new"]().detach())
    gn = {n: float(p.grad.norm()) for n, p in head.named_parameters()}
    gxn = float(x_pt.grad.float().norm())
    worst = max(abs(gn[n] - gb[n]) / max(gb[n], 1e-12) for n in gb if n != "0.bias")
    print("N %d: loss baseline %.6f new %.6f; worst relative difference of a gradient norm %.2e (dx: %.2e)"
          % (N, lb, ln, worst, abs(gxn - gxb) / gxb), flush=True)
    assert abs(ln - lb) <= 1e-2 * abs(lb) and worst <= 2e-2
    res = interleaved(forms, a.repeats)
    flop = 3 * 2.0 * N * C * HW * HW * F
    row = dict(part="head_step", N=N, C=C, H=HW, W=HW, F=F, k=k, repeats=a.repeats, product_flop=flop)
    for name, (med, lo, hi) in res.items():
      row[name + "_ms"], row[name + "_min"], row[name + "_max"] = med, lo, hi
      row[name + "_share_of_bf16_peak"] = flop / (med * 1e-3) / BF16_PEAK
    row["ratio_baseline_over_new"] = res["baseline"][0] / res["new"][0]
    rows.append(row)
    print("head step N %d: baseline %.3f ms (%.3f..%.3f) | new %.3f ms (%.3f..%.3f) | new without operand refresh %.3f ms "
          "(%.3f..%.3f) | baseline / new %.2f | new: %.1f %% of the bf16 MFMA peak over the whole step"
          % ((N,) + res["baseline"] + res["new"] + res["new_no_prep"]
             + (row["ratio_baseline_over_new"], 100 * row["new_share_of_bf16_peak"])), flush=True)
    del forms, head, x_pt
    torch.cuda.empty_cache()
  if not a.skip_eval:
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (a.images, 96, 96, 3), generator=g, dtype=torch.uint8).to(dev)
    forms = eval_forms(images, 64, dev, 70)
    accs = {name: fn() for name, fn in forms.items()}          # (also the warm-up)
    assert accs["baseline"] == accs["new"], accs
    res = interleaved(forms, a.eval_repeats, warmup=0)
    nb = (a.images + 69) // 70
    row = dict(part="ten_crop_pass", images=a.images, batches=nb, accuracy=accs["new"], repeats=a.eval_repeats,
               baseline_per_batch=dict(h2d_copies=1, launches=1, d2h_syncs=1), baseline_syncs_per_pass=nb,
               new_per_batch=dict(h2d_copies=2, launches=3, d2h_syncs=0), new_syncs_per_pass=1)
    for name, (med, lo, hi) in res.items():
      row[name + "_ms"], row[name + "_min"], row[name + "_max"] = med, lo, hi
    rows.append(row)
    print("ten-crop pass, %d images, %d batches of 700 crops: baseline %.1f ms (%.1f..%.1f), %d synchronisations | new %.1f ms "
          "(%.1f..%.1f), 1 synchronisation | same accuracy %.4f"
          % ((a.images, nb) + res["baseline"] + (nb,) + res["new"] + (accs["new"],)), flush=True)
  print(json.dumps(rows))
  if a.out:
    with open(a.out, "w") as f:
      json.dump(rows, f, indent=1)
      f.write("\n")


if __name__ == "__main__":
  main()
