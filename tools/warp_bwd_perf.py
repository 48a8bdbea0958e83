"""Times the two backward kernels of the general affine warp (csrc/warp.hip) against each other at the two published
segmentation shapes, (75, 24, 200, 200) (Potsdam-3 head A) and (120, 15, 128, 128) (COCO-Stuff-3 head A), with matrices
of the reference's random_affine range (oracle.gen_golden_seg2.random_affines through seg_losses._pixel_matrices,
another matrix per sample, every other sample x-flipped):

  A  iic_affine_warp_bwd         zero-fill + float-atomic scatter (unchanged since it was written)
  B  iic_affine_warp_bwd_gather  gather, fixed summation order, no atomics, no zero-fill

After a warm-up of both, ROUNDS rounds; in each round A then B, each as ITERS back-to-back launches between two device
events.  Reported: median and min..max over the rounds of the per-launch time, B - A, the algorithmic traffic (dout read
once, dx written once) over each time, and the largest |B - A| of the two results relative to the largest |A|.  Also the
pair at an identity matrix with a sparse shift (the loss path of half_T_side_sparse_* without --use_random_affine).

    python tools/warp_bwd_perf.py [--iters 20] [--rounds 9] [--out FILE]

Needs a GPU; there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

SHAPES = [("potsdam3_kA", (75, 24, 200, 200)), ("coco3_kA", (120, 15, 128, 128))]


def window(fn, iters):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(iters):
    fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) / iters


def summary(v):
  return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--rounds", type=int, default=9)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  assert torch.cuda.is_available(), "warp_bwd_perf needs a GPU"
  from iic_amd import _lib, seg_losses
  from oracle.gen_golden_seg2 import random_affines
  L, dev = _lib.lib(), torch.device("cuda:0")
  rows, lines = [], []
  for name, (N, K, H, W) in SHAPES:
    g = torch.Generator().manual_seed(5)
    dout = torch.randn((N, K, H, W), generator=g).to(dev)
    theta = torch.from_numpy(random_affines(N, 17))
    theta[1::2, :, 0] *= -1.0
    ident = torch.tensor([[[1.0, 0, 0], [0, 1.0, 0]]]).repeat(N, 1, 1)
    for kind, th, sx, sy in (("random_affine", theta, 0, 0), ("identity_sparse_shift", ident, 3, -2)):
      host = seg_losses._pixel_matrices(th, H, W).contiguous()
      assert L.iic_affine_warp_gather_supported(host.data_ptr(), N) == 1
      mats = host.to(dev)
      dxa, dxb = torch.empty_like(dout), torch.empty_like(dout)

      def atomic():
        _lib.check(L.iic_affine_warp_bwd(dout.data_ptr(), mats.data_ptr(), dxa.data_ptr(), N, K, H, W, sx, sy,
                                         _lib.stream_ptr()), "iic_affine_warp_bwd")

      def gather():
        _lib.check(L.iic_affine_warp_bwd_gather(dout.data_ptr(), mats.data_ptr(), host.data_ptr(), dxb.data_ptr(), N, K,
                                                H, W, sx, sy, _lib.stream_ptr()), "iic_affine_warp_bwd_gather")

      for _ in range(3):
        atomic()
        gather()
      torch.cuda.synchronize()
      ta, tb = [], []
      for _ in range(a.rounds):
        ta.append(window(atomic, a.iters))
        tb.append(window(gather, a.iters))
      diff = float((dxa - dxb).abs().max() / dxa.abs().max())
      nbytes = 2 * dout.numel() * 4
      A, B = summary(ta), summary(tb)
      row = dict(shape=name, N=N, K=K, H=H, W=W, matrices=kind, shift=[sx, sy], atomic=A, gather=B,
                 gather_minus_atomic_ms=B["median_ms"] - A["median_ms"],
                 per_round_delta_ms=[y - x for x, y in zip(ta, tb)], algorithmic_bytes=nbytes,
                 atomic_GBps=nbytes / A["median_ms"] / 1e6, gather_GBps=nbytes / B["median_ms"] / 1e6,
                 max_abs_diff_rel=diff)
      rows.append(row)
      lines.append("%-12s %-22s atomic %.3f ms (min %.3f max %.3f, %.0f GB/s)  gather %.3f ms (min %.3f max %.3f, %.0f GB/s)  "
                   "gather - atomic %+.3f ms (per round %+.3f .. %+.3f)  max |diff| / max |dx| %.1e"
                   % (name, kind, A["median_ms"], A["min_ms"], A["max_ms"], row["atomic_GBps"], B["median_ms"], B["min_ms"],
                      B["max_ms"], row["gather_GBps"], row["gather_minus_atomic_ms"], min(row["per_round_delta_ms"]),
                      max(row["per_round_delta_ms"]), diff))
      print(lines[-1], flush=True)
  text = "\n".join(["tools/warp_bwd_perf.py --iters %d --rounds %d on %s" % (a.iters, a.rounds, torch.cuda.get_device_name(0))]
                   + lines + [json.dumps(rows)]) + "\n"
  print(json.dumps(rows))
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(text)


if __name__ == "__main__":
  main()
