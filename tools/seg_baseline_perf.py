"""Times the Isola / Doersch segmentation baselines (iic_amd.archs.seg_baselines, iic_amd.seg_baselines) against the
composition the reference runs (code/archs/segmentation/baselines/net10a_isola.py, net10a_doersch.py,
code/utils/segmentation/baselines/isola_utils.py, doersch_utils.py) on the same device, in one process:

  head path   from the trunk's features to the loss, forward + backward (the gradient reaches the features):
     hip  : iic_seg_patch_sample_fwd -> siamese stage twice -> iic_pair_linear_* -> ReLU, dropout, Linear -> loss kernel
     torch: F.interpolate of all 512 channels to S x S, two slices, nn.Conv2d + nn.BatchNorm2d + ReLU twice, flatten + cat,
            nn.Linear, ReLU, nn.Dropout, nn.Linear (fp32), the reference's loss expression with its norm_factor.item()
  whole step  zero_grad, trunk, head, loss, backward, Adam (iic_amd.optim.Adam / torch.optim.Adam) on an image batch

at Potsdam 200^2 batch 75 and COCO-Stuff 128^2 batch 120, patch side 11 (--shapes).  One fixed pair of patches per shape.
After a warm-up the rounds alternate between the two sides; each round puts device events around `--iters` back-to-back
passes; reported: median and min..max per pass over the rounds.

    python tools/seg_baseline_perf.py [--kind isola] [--shapes 200x75 128x120] [--p 11] [--rounds 7] [--iters 4]
                                      [--step_iters 2] [--out FILE]

Needs a GPU; there is no CPU fall-back.  Not measured here: graph-captured steps, data parallelism, the data pipeline."""
import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from iic_amd import archs, ops, seg_baselines as sb   # noqa: E402
from iic_amd.optim import Adam   # noqa: E402

CFG = archs.SegmentationNet10a.cfg
EPS = sys.float_info.epsilon


class TorchNet(nn.Module):
  """The reference's module structure in plain torch (fp32)."""

  def __init__(self, in_channels, p, nout):
    super(TorchNet, self).__init__()
    layers, cin = [], in_channels
    for c, dil in CFG:
      if c == "M":
        layers.append(nn.MaxPool2d(2, 2))
      else:
        layers += [nn.Conv2d(cin, c, 3, 1, 1, dilation=dil, bias=False), nn.BatchNorm2d(c), nn.ReLU(inplace=True)]
        cin = c
    self.features = nn.Sequential(*layers)
    self.siamese = nn.Sequential(nn.Conv2d(512, 1024, 3, 1, 1, bias=False), nn.BatchNorm2d(1024), nn.ReLU(inplace=True))
    self.joint = nn.Sequential(nn.Linear(2 * 1024 * p * p, 1024), nn.ReLU(True), nn.Dropout(), nn.Linear(1024, nout))
    self.p = p

  def head(self, f, S, centre, other):
    x = F.interpolate(f, size=S, mode="bilinear")
    d = self.p // 2
    a = [self.siamese(x[:, :, c[0] - d:c[0] + d + 1, c[1] - d:c[1] + d + 1]).contiguous().view(f.shape[0], -1)
         for c in (centre, other)]
    return self.joint(torch.cat(a, dim=1))


def torch_loss(kind, out, centre, other, gt, mask):
  m = ((mask[:, centre[0], centre[1]] + mask[:, other[0], other[1]]) > 0).to(torch.float32)
  norm = m.sum().item()
  if kind == "isola":
    t = torch.sigmoid(out).squeeze()
    t = t if gt else 1.0 - t
    keep = 1.0 - (t < EPS).to(torch.float32)
    t = torch.where(t < EPS, torch.full_like(t, EPS), t)
    return -(1.0 / norm) * (m * keep * torch.log(t)).sum()
  tgt = torch.ones(out.shape[0], dtype=torch.int64, device=out.device) * gt
  return (m * F.cross_entropy(out, tgt, reduction="none")).sum() / norm


class _FeedFn(torch.autograd.Function):
  """Stands where the trunk's last stage stands: hands the PT features on, and returns the gradient buffer it is given
  to the pool, as that stage's backward does."""

  @staticmethod
  def forward(ctx, anchor, pt):
    return pt.detach()

  @staticmethod
  def backward(ctx, g):
    ops.POOL.release(g)
    return torch.zeros((), device=g.device), None


def timed(sides, rounds, iters):
  times = dict((name, []) for name, _ in sides)
  for _ in range(rounds):
    for name, fn in sides:
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(iters):
        fn()
      e1.record()
      e1.synchronize()
      times[name].append(e0.elapsed_time(e1) / iters)
  return times


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--kind", default="isola", choices=["isola", "doersch"])
  ap.add_argument("--shapes", nargs="*", default=["200x75", "128x120"])
  ap.add_argument("--p", type=int, default=11)
  ap.add_argument("--in_channels", type=int, default=4)
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=4)
  ap.add_argument("--step_iters", type=int, default=2)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU: there is no CPU fall-back"
  dev = torch.device("cuda:0")
  lines = []

  def say(s):
    print(s)
    sys.stdout.flush()
    lines.append(s)

  def report(what, times, iters):
    for name in times:
      t = np.array(times[name])
      say("%s %-5s: median %.3f ms (min %.3f .. max %.3f) per pass over %d rounds of %d"
          % (what, name, np.median(t), t.min(), t.max(), len(t), iters))
    say("%s: torch / hip = %.2f" % (what, np.median(times["torch"]) / np.median(times["hip"])))

  say("device: %s, torch %s; %s, patch side %d" % (torch.cuda.get_device_name(0), torch.__version__, args.kind, args.p))
  p, kind = args.p, args.kind
  nout = 1 if kind == "isola" else 9
  gt = True if kind == "isola" else 5
  torch.manual_seed(0)
  S0 = int(args.shapes[0].split("x")[0])
  cfg = types.SimpleNamespace(in_channels=args.in_channels, input_sz=S0, batchnorm_track=True, isola_patch_side=p,
                              doersch_patch_side=p)
  with torch.device(dev):      # the joint Linear has 254 M weights at p = 11: initialise on the device
    net = (archs.SegmentationNet10aIsola if kind == "isola" else archs.SegmentationNet10aDoersch)(cfg)
    ref = TorchNet(args.in_channels, p, nout)
  net.to(dev).train()
  ref.to(dev).train()
  opt_h, opt_t = Adam(net.parameters(), lr=1e-5), torch.optim.Adam(ref.parameters(), lr=1e-5)
  for shape in args.shapes:
    S, N = (int(v) for v in shape.split("x"))
    net.input_sz = S
    Hf = S // 2 - 4
    centre, other = np.array([S // 3, S // 2], dtype=np.int32), np.array([S // 3 + p, S // 2 - p], dtype=np.int32)
    mask = (torch.rand((N, S, S), device=dev) < 0.8).to(torch.uint8)
    img = torch.rand((N, args.in_channels, S, S), device=dev)
    feats = torch.randn((N, 512, Hf, Hf), device=dev).relu_()
    pt = ops.pt_from_nchw(feats, archs.seg.SegmentationNet10aTrunk.P)
    anchor = torch.zeros((), device=dev, requires_grad=True)
    feats.requires_grad_(True)
    cy, cx, oy, ox = (int(v) for v in list(centre) + list(other))

    def hip_head():
      net.zero_grad()
      out = net.head_from_features(_FeedFn.apply(anchor, pt), cy, cx, oy, ox)
      out = torch.sigmoid(out) if kind == "isola" else out
      loss = sb.isola_loss(out, centre, other, gt, mask) if kind == "isola" else sb.doersch_loss(out, centre, other, gt, mask)
      loss.backward()
      return loss

    def torch_head():
      feats.grad = None
      ref.zero_grad()
      loss = torch_loss(kind, ref.head(feats, S, centre, other), centre, other, gt, mask)
      loss.backward()
      return loss

    def hip_step():
      net.zero_grad()
      out = net(img, centre=centre, other=other)
      loss = sb.isola_loss(out, centre, other, gt, mask) if kind == "isola" else sb.doersch_loss(out, centre, other, gt, mask)
      loss.backward()
      opt_h.step()
      return loss

    def torch_step():
      ref.zero_grad()
      loss = torch_loss(kind, ref.head(ref.features(img), S, centre, other), centre, other, gt, mask)
      loss.backward()
      opt_t.step()
      return loss

    what = "S %d N %d" % (S, N)
    lh, lt = float(hip_head().detach()), float(torch_head().detach())      # also the warm-up of every shape the window uses
    say("%s head: first loss hip %.5f, torch %.5f (different weights and dropout draws: same order only)" % (what, lh, lt))
    hip_head(), torch_head()
    torch.cuda.synchronize()
    report("%s head path fwd+bwd" % what, timed([("hip", hip_head), ("torch", torch_head)], args.rounds, args.iters),
           args.iters)
    for _ in range(2):
      hip_step(), torch_step()
    torch.cuda.synchronize()
    report("%s whole step incl. Adam" % what,
           timed([("hip", hip_step), ("torch", torch_step)], args.rounds, args.step_iters), args.step_iters)
    K2 = 2 * 1024 * p * p
    say("%s: the up-sampled map the torch side builds is %.2f GB fp32 (and as much again in backward); the joint weight "
        "is %.1f M values (%.2f GB fp32, %.2f GB as one bf16 operand)"
        % (what, N * 512 * S * S * 4 / 1e9, 1024 * K2 / 1e6, 1024 * K2 * 4 / 1e9, 1024 * K2 * 2 / 1e9))
    del feats, pt, img, mask
    torch.cuda.empty_cache()
  if args.out:
    with open(args.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
