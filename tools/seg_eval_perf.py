"""Times one segmentation evaluation pass in its two forms, at the Potsdam-3 (N 75, S 200, k 24 and 3) and COCO-Stuff-3
(N 120, S 128, k 15 and 3) batch shapes, in one process:

  existing : net(x) -> torch.argmax -> copies into flat uint8 arrays spanning the pass -> masked_select ->
             iic_amd.eval_metrics._original_match (the reference's _segmentation_get_data with the package's drop-ins)
  streaming: net.predict_labels(x) -> SegEvalAccumulator.add per batch -> counts() -> stats_from_counts' match

Device events around whole passes of --batches batches; after a warm-up the repeats alternate between the two forms, so
clock and thermal drift hit both alike.  Reported per batch: median and min..max over the repeats, and the bytes each
form's evaluation-only work moves (what follows the low-resolution softmax; the trunk and head GEMM are common).  The
last launch alone (iic_bilinear_fwd + argmax against iic_seg_label_map on the same low-resolution probabilities) is
timed the same way.  The comparison is always against the existing path measured in the same run, never a constant.

    python tools/seg_eval_perf.py [--repeats 7] [--batches 2]

Needs a GPU; there is no CPU fall-back."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from iic_amd import archs, eval_metrics, seg_eval   # noqa: E402
from iic_amd._lib import check, lib, stream_ptr    # noqa: E402

CONFIGS = [("potsdam3", dict(bn=75, sz=200, in_ch=4, k_A=24, k_B=3)),
           ("coco3", dict(bn=120, sz=128, in_ch=5, k_A=15, k_B=3))]
GT_K = 3


def event_ms(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1)


def interleaved(forms, repeats, warmup=2):
  """forms: {name: fn}.  Warm-up of every form, then `repeats` rounds that run each form once, in turn."""
  for _ in range(warmup):
    for fn in forms.values():
      fn()
  torch.cuda.synchronize()
  times = {name: [] for name in forms}
  for _ in range(repeats):
    for name, fn in forms.items():
      times[name].append(event_ms(fn))
  return {name: (float(np.median(t)), float(min(t)), float(max(t))) for name, t in times.items()}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--batches", type=int, default=2)
  a = ap.parse_args()
  assert torch.cuda.is_available(), "seg_eval_perf needs a GPU"
  dev = torch.device("cuda:0")
  rows = []
  for name, c in CONFIGS:
    N, S, B = c["bn"], c["sz"], a.batches
    cfg = types.SimpleNamespace(in_channels=c["in_ch"], input_sz=S, batchnorm_track=True, num_sub_heads=1,
                                output_k_A=c["k_A"], output_k_B=c["k_B"])
    torch.manual_seed(0)
    net = archs.SegmentationNet10aTwoHead(cfg).to(dev).eval()
    rng = np.random.default_rng(1)
    batches = [(torch.from_numpy(rng.random((N, c["in_ch"], S, S)).astype(np.float32)).to(dev),
                torch.from_numpy(rng.integers(0, GT_K, (N, S, S)).astype(np.uint8)).to(dev),
                torch.from_numpy((rng.random((N, S, S)) < 0.8).astype(np.uint8)).to(dev)) for _ in range(B)]
    px = N * S * S
    Hl = S // 2 + 2
    for head, k in (("A", c["k_A"]), ("B", c["k_B"])):
      def existing():
        flat_p = torch.zeros(B * px, dtype=torch.uint8, device=dev)
        flat_t = torch.zeros(B * px, dtype=torch.uint8, device=dev)
        flat_m = torch.zeros(B * px, dtype=torch.uint8, device=dev)
        for b, (x, t, m) in enumerate(batches):
          with torch.no_grad():
            out = net(x, head=head)[0]
          flat_p[b * px:(b + 1) * px] = torch.argmax(out, dim=1).view(-1)
          flat_t[b * px:(b + 1) * px] = t.view(-1)
          flat_m[b * px:(b + 1) * px] = m.view(-1)
        sel = flat_m.bool()
        return eval_metrics._original_match(flat_p.masked_select(sel), flat_t.masked_select(sel), k, GT_K)

      def streaming():
        acc = seg_eval.SegEvalAccumulator(1, k, GT_K, dev)
        for x, t, m in batches:
          with torch.no_grad():
            acc.add(net.predict_labels(x, head=head), t, m)
        counts, _ = acc.counts()
        return [(p, int(np.argmax(counts[0][p]))) for p in range(k)]

      assert existing() == streaming(), "the two forms disagree on the match"
      full = interleaved({"existing": existing, "streaming": streaming}, a.repeats)

      # the last launch alone, on the same low-resolution probabilities
      probs = torch.softmax(torch.randn((N, Hl, Hl, k), device=dev) * 3, dim=3).contiguous()
      out = torch.empty((N, k, S, S), device=dev)
      lab = torch.empty((N, S, S), dtype=torch.uint8, device=dev)

      def last_existing():
        check(lib().iic_bilinear_fwd(probs.data_ptr(), out.data_ptr(), N, Hl, Hl, k, S, stream_ptr()), "iic_bilinear_fwd")
        return torch.argmax(out, dim=1)

      def last_streaming():
        check(lib().iic_seg_label_map(probs.data_ptr(), lab.data_ptr(), N, Hl, Hl, k, S, stream_ptr()), "iic_seg_label_map")
        return lab

      assert torch.equal(last_existing().to(torch.uint8), last_streaming()), "label map != arg-max of the up-sampling"
      last = interleaved({"existing": last_existing, "streaming": last_streaming}, a.repeats, warmup=5)

      # evaluation-only bytes per batch (algorithmic: every array read or written once per operator)
      low = N * Hl * Hl * k * 4
      bytes_existing = (low + px * k * 4            # up-sampling: read the low-resolution maps, write the fp32 maps
                        + px * k * 4 + px * 8       # arg-max: read them, write int64
                        + px * (8 + 1) + 4 * px     # flat copies: labels narrowed, targets and mask read + written
                        + 3 * px + 2 * px           # masked_select: three arrays read, two selections written (upper bound)
                        + 2 * px * (1 + 8)          # .long() of predictions and targets in front of iic_contingency
                        + 2 * px * 8)               # iic_contingency reads both
      bytes_streaming = low + px + 3 * px           # label map: read low-res, write uint8; accumulator: three streams
      row = dict(config=name, head=head, N=N, S=S, k=k, batches=B, repeats=a.repeats,
                 existing_ms_per_batch=full["existing"][0] / B, existing_min=full["existing"][1] / B,
                 existing_max=full["existing"][2] / B, streaming_ms_per_batch=full["streaming"][0] / B,
                 streaming_min=full["streaming"][1] / B, streaming_max=full["streaming"][2] / B,
                 last_launch_existing_ms=last["existing"][0], last_launch_streaming_ms=last["streaming"][0],
                 eval_bytes_existing=bytes_existing, eval_bytes_streaming=bytes_streaming)
      rows.append(row)
      print("%-9s head %s k %2d  pass per batch: existing %.3f ms (min %.3f max %.3f)  streaming %.3f ms (min %.3f max %.3f)"
            "  | last launch: bilinear+argmax %.3f ms (min %.3f max %.3f)  label map %.3f ms (min %.3f max %.3f)"
            "  | evaluation-only bytes per batch: existing %.1f MB  streaming %.1f MB"
            % (name, head, k, row["existing_ms_per_batch"], row["existing_min"], row["existing_max"],
               row["streaming_ms_per_batch"], row["streaming_min"], row["streaming_max"], last["existing"][0],
               last["existing"][1], last["existing"][2], last["streaming"][0], last["streaming"][1], last["streaming"][2],
               bytes_existing / 1e6, bytes_streaming / 1e6), flush=True)
    del net, batches
    torch.cuda.empty_cache()
  print(json.dumps(rows))


if __name__ == "__main__":
  main()
