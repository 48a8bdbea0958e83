"""Times the bookkeeping of one clustering evaluation pass in its two forms, on synthetic softmax outputs and targets
(evaluation proper is bound by the trunk's forward, which both forms share; this tool leaves it out), in one process:

  flat     : the reference's flow (code/utils/cluster/cluster_eval.py:23-67, :187-228) restated here on the package's
             drop-ins: per sub-head torch.argmax slice-assigned into flat int32 arrays that span the pass, then per
             sub-head iic_amd.eval_metrics._original_match / _hungarian_match, the reorder loop
             `reordered_preds[flat_preds == pred_i] = target_i` and eval_metrics._acc
  streaming: iic_amd.cluster_eval.ClusterEvalAccumulator.add per batch -> counts() -> seg_eval.stats_from_counts

Both forms must return the same dict (checked before anything is timed).  Reported per pass: kernel launches and host
synchronisations counted from the code paths (the formulas are below, next to the code they count), and the wall time --
a host clock around a pass that starts and ends with a device synchronise, because the flat form's cost is launches
and host round trips, which device events between two launches would not see.  After a warm-up the repeats alternate
between the two forms; median and min..max over the repeats.

    python tools/cluster_eval_perf.py [--num_sub_heads 5] [--output_k 70 140] [--gt_k 10] [--batch 660] [--batches 20]
                                      [--eval_mode orig] [--repeats 9] [--out FILE]

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
from iic_amd import cluster_eval, eval_metrics, seg_eval   # noqa: E402


def flat_pass(config, batches):
  """The flat-array flow, "IID" mode.  Returns the stats dict."""
  H, k, gt_k, bs = config.num_sub_heads, config.output_k, config.gt_k, config.batch_sz
  dev = batches[0][1].device
  flat_t = torch.zeros(len(batches) * bs, dtype=torch.int32, device=dev)
  flat_p = [torch.zeros(len(batches) * bs, dtype=torch.int32, device=dev) for _ in range(H)]
  num = 0
  for b_i, (x_outs, t) in enumerate(batches):
    cur = t.shape[0]
    num += cur
    s = b_i * bs
    for i in range(H):
      flat_p[i][s:s + cur] = torch.argmax(x_outs[i], dim=1)
    flat_t[s:s + cur] = t
  flat_p, flat_t = [p[:num] for p in flat_p], flat_t[:num]
  matcher = eval_metrics._hungarian_match if config.eval_mode == "hung" else eval_metrics._original_match
  matches, accs = [], np.zeros(H, dtype=np.float32)
  for i in range(H):
    match = matcher(flat_p[i], flat_t, preds_k=k, targets_k=gt_k)
    reordered = torch.zeros(num, dtype=flat_p[0].dtype, device=dev)
    for pred_i, target_i in match:
      reordered[flat_p[i] == pred_i] = target_i
    accs[i] = eval_metrics._acc(reordered, flat_t, gt_k, verbose=0)
    matches.append(match)
  best = np.argmax(accs)
  return {"test_accs": list(accs), "avg": np.mean(accs), "std": np.std(accs), "best": accs[best], "worst": accs.min(),
          "best_train_sub_head": best, "best_train_sub_head_match": matches[best], "train_accs": list(accs)}


def flat_counts(H, k, B):
  """(launches, host synchronisations) of flat_pass, from its code path.
  Per batch: H x (argmax + the converting slice copy) + the targets' slice copy; H + 1 fills for the flat arrays.
  Per sub-head: the match (eval_metrics._counts: two .long() copies, the buffer's clear, iic_contingency; its .cpu() is
  a synchronisation), one fill for reordered_preds, 2 launches (compare, masked fill) per output cluster, and _acc: two
  max() each read on the host (2 synchronisations), two .long() copies, the clear, iic_count_equal, int(count) (1)."""
  launches = B * (2 * H + 1) + (H + 1) + H * (4 + 1 + 2 * k + 2 + 2 + 1 + 1)
  syncs = H * (1 + 2 + 1)
  return launches, syncs


def streaming_pass(config, batches):
  acc = cluster_eval.ClusterEvalAccumulator(config.num_sub_heads, config.output_k, config.gt_k, batches[0][1].device)
  for x_outs, t in batches:
    acc.add(x_outs, t)
  counts, n = acc.counts()
  return seg_eval.stats_from_counts(counts, n, None, 0, config)


def streaming_counts(H, k, B):
  """One fill for the count buffer, one iic_cluster_argmax_acc per batch (int64 targets and the nets' packed views are
  read in place); counts() is the one synchronisation."""
  return 1 + B, 1


def wall_ms(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3


def interleaved(forms, repeats, warmup=3):
  """forms: {name: fn}.  Warm-up of every form, then `repeats` rounds that run each form once, in turn."""
  for _ in range(warmup):
    for fn in forms.values():
      fn()
  times = {name: [] for name in forms}
  for _ in range(repeats):
    for name, fn in forms.items():
      times[name].append(wall_ms(fn))
  return {name: (float(np.median(t)), float(min(t)), float(max(t))) for name, t in times.items()}


def same_dict(a, b):
  return (set(a) == set(b) and all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes()
                                   for key in ("test_accs", "train_accs", "avg", "std", "best", "worst"))
          and int(a["best_train_sub_head"]) == int(b["best_train_sub_head"])
          and a["best_train_sub_head_match"] == b["best_train_sub_head_match"])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--num_sub_heads", type=int, default=5)
  ap.add_argument("--output_k", type=int, nargs="+", default=[70, 140])
  ap.add_argument("--gt_k", type=int, default=10)
  ap.add_argument("--batch", type=int, default=660)
  ap.add_argument("--batches", type=int, default=20)
  ap.add_argument("--eval_mode", choices=["orig", "hung"], default="orig")
  ap.add_argument("--repeats", type=int, default=9)
  ap.add_argument("--out", default=None, help="also write the JSON rows to this file")
  a = ap.parse_args()
  assert torch.cuda.is_available(), "cluster_eval_perf needs a GPU"
  dev = torch.device("cuda:0")
  H, gt_k, N, B = a.num_sub_heads, a.gt_k, a.batch, a.batches
  rows = []
  for k in a.output_k:
    config = types.SimpleNamespace(num_sub_heads=H, output_k=k, gt_k=gt_k, batch_sz=N, eval_mode=a.eval_mode, mode="IID",
                                   mapping_assignment_partitions=["a"], mapping_test_partitions=["a"])
    g = torch.Generator().manual_seed(k)
    batches = []
    for b in range(B):
      n = N if b < B - 1 else max(1, N - N // 3)                       # a ragged last batch
      t = torch.randint(0, gt_k, (n,), generator=g)
      # correlated with the targets, so that the match is not arbitrary
      logits = torch.randn((n, H, k), generator=g) + 2.0 * torch.nn.functional.one_hot(t * (k // gt_k), k)[:, None, :]
      probs = torch.softmax(logits, dim=2).to(dev)                     # packed [n, H, k], as forward_packed returns it
      batches.append(([probs[:, i, :] for i in range(H)], t.to(dev)))  # the list forward returns: views of the pack
    flat = lambda: flat_pass(config, batches)                           # noqa: E731
    streaming = lambda: streaming_pass(config, batches)                 # noqa: E731
    assert same_dict(flat(), streaming()), "the two forms disagree"
    res = interleaved({"flat": flat, "streaming": streaming}, a.repeats)
    fl, fs = flat_counts(H, k, B)
    sl, ss = streaming_counts(H, k, B)
    row = dict(num_sub_heads=H, output_k=k, gt_k=gt_k, batch=N, batches=B, eval_mode=a.eval_mode, repeats=a.repeats,
               flat_launches=fl, flat_syncs=fs, flat_ms=res["flat"][0], flat_min=res["flat"][1], flat_max=res["flat"][2],
               streaming_launches=sl, streaming_syncs=ss, streaming_ms=res["streaming"][0],
               streaming_min=res["streaming"][1], streaming_max=res["streaming"][2])
    rows.append(row)
    print("H %d k %3d gt_k %d, %d batches of %d (%s): flat %d launches %d syncs %.3f ms per pass (min %.3f max %.3f)  |  "
          "streaming %d launches %d sync %.3f ms per pass (min %.3f max %.3f)"
          % (H, k, gt_k, B, N, a.eval_mode, fl, fs, row["flat_ms"], row["flat_min"], row["flat_max"], sl, ss,
             row["streaming_ms"], row["streaming_min"], row["streaming_max"]), flush=True)
  print(json.dumps(rows))
  if a.out:
    with open(a.out, "w") as f:
      json.dump(rows, f, indent=1)
      f.write("\n")


if __name__ == "__main__":
  main()
