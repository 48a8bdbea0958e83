"""Times the triplets baseline (iic_amd.triplets, csrc/triplets.hip) against the composition the reference runs
(code/utils/cluster/baselines/triplets.py:231-238) on the same device, in one process:

  hip  : triplets_loss(orig, pos, neg) + backward -- iic_triplets_loss (two launches) and the upstream-scalar products
  torch: F.kl_div(log_softmax(orig), softmax(pos)) - F.kl_div(log_softmax(orig), softmax(neg)), reduction="mean", +
         backward

on three leaf tensors [N, k] of N(0, 3^2) logits, at the shapes named by --shapes.  Before anything is timed the two
sides' losses and gradients are compared.  After a warm-up the rounds alternate between the two sides; each round puts
device events around `--iters` back-to-back forward + backward passes; reported: median and min..max per pass over the
rounds.

Then one whole triplet step of TripletsNet6c (three forwards, loss, backward; bf16 path, eager launches) at --step_batch
images of 24 x 24, once with each loss, the same way.

    python tools/triplets_perf.py [--shapes 700x10 700x70 660x280] [--rounds 9] [--iters 200] [--step_batch 700]
                                  [--step_iters 10] [--out FILE]

Needs a GPU; there is no CPU fall-back.  Not measured here: graph-captured steps, data parallelism, TripletsNet5g."""
import argparse
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from iic_amd import archs, triplets   # noqa: E402


def torch_loss(a, b, c):
  orig = F.log_softmax(a, dim=1)
  return F.kl_div(orig, F.softmax(b, dim=1), reduction="mean") - F.kl_div(orig, F.softmax(c, dim=1), reduction="mean")


def timed(sides, rounds, iters):
  """{name: per-pass milliseconds of every round}; the sides alternate within a round."""
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
  ap.add_argument("--shapes", nargs="*", default=["700x10", "700x70", "660x280"])
  ap.add_argument("--rounds", type=int, default=9)
  ap.add_argument("--iters", type=int, default=200)
  ap.add_argument("--step_batch", type=int, default=700)
  ap.add_argument("--step_iters", type=int, default=10)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert args.rounds >= 7
  warnings.simplefilter("ignore")      # kl_div's note that "mean" is not "batchmean"
  dev = torch.device("cuda:0")
  lines = []

  def say(s):
    print(s)
    sys.stdout.flush()
    lines.append(s)

  def report(what, times, rounds, iters):
    for name in times:
      t = np.array(times[name])
      say("%s %-5s: median %.4f ms (min %.4f .. max %.4f) per pass over %d rounds of %d"
          % (what, name, np.median(t), t.min(), t.max(), rounds, iters))
    say("%s: torch / hip = %.2f" % (what, np.median(times["torch"]) / np.median(times["hip"])))

  say("device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
  for shape in args.shapes:
    N, k = (int(v) for v in shape.split("x"))
    g = torch.Generator(device=dev)
    g.manual_seed(N * 1031 + k)
    a, b, c = [(torch.randn((N, k), device=dev, generator=g) * 3).requires_grad_(True) for _ in range(3)]

    def side(loss_fn):
      def run():
        a.grad = b.grad = c.grad = None
        loss_fn(a, b, c).backward()
      return run
    hip, tch = side(triplets.triplets_loss), side(torch_loss)
    hip()
    lh, gh = float(triplets.triplets_loss(a, b, c)), [t.grad.clone() for t in (a, b, c)]
    tch()
    lt, gt = float(torch_loss(a, b, c)), [t.grad.clone() for t in (a, b, c)]
    say("%s: loss hip %.8e torch %.8e; max |gradient difference| %.3g (max |gradient| %.3g)"
        % (shape, lh, lt, max(float((u - v).abs().max()) for u, v in zip(gh, gt)), max(float(v.abs().max()) for v in gt)))
    for _ in range(20):
      hip()
      tch()
    torch.cuda.synchronize()
    report(shape, timed((("hip", hip), ("torch", tch)), args.rounds, args.iters), args.rounds, args.iters)

  # one whole triplet step of TripletsNet6c
  B = args.step_batch
  torch.manual_seed(0)
  net = archs.TripletsNet6c(types.SimpleNamespace(in_channels=1, input_sz=24, batchnorm_track=True, output_k=10))
  net.to(dev).train()
  g = torch.Generator(device=dev)
  g.manual_seed(7)
  orig = torch.rand((B, 1, 24, 24), device=dev, generator=g)
  pos = (orig.flip(3) * 0.9 + 0.02 * torch.randn(orig.shape, device=dev, generator=g)).clamp(0, 1)
  neg = orig[torch.randperm(B, device=dev, generator=g)].contiguous()

  def step(loss_fn):
    def run():
      net.zero_grad(set_to_none=True)
      loss_fn(net(orig), net(pos), net(neg)).backward()
    return run
  hip, tch = step(triplets.triplets_loss), step(torch_loss)
  for _ in range(3):
    hip()
    tch()
  torch.cuda.synchronize()
  what = "TripletsNet6c step, %d x 1 x 24 x 24" % B
  report(what, timed((("hip", hip), ("torch", tch)), args.rounds, args.step_iters), args.rounds, args.step_iters)
  if args.out:
    with open(args.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
