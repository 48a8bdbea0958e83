"""iic_amd/cluster_eval.py without a GPU: the module imports, refuses CPU tensors, its C entry point is declared and
bound, and -- the invariant the twin rests on -- seg_eval.stats_from_counts on count matrices gives the dict the
reference's flat-array flow (cluster_eval.py:101-145, :187-228) gives on the arrays the counts were made from."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_imports_and_refuses_the_cpu():
  from iic_amd import cluster_eval
  for name in ("cluster_eval", "cluster_subheads_eval", "get_subhead_using_loss", "_clustering_get_data",
               "ClusterEvalAccumulator"):
    assert hasattr(cluster_eval, name)
  from iic_amd.seg_eval import stats_from_counts
  assert cluster_eval.stats_from_counts is stats_from_counts           # imported, not copied
  from iic_amd import install
  assert not any(our_mod == "iic_amd.cluster_eval" for _, _, our_mod, _ in install.PATCHES)    # opt-in: install() does not rebind it
  with pytest.raises(AssertionError):
    cluster_eval.ClusterEvalAccumulator(2, 6, 3, "cpu")
  with pytest.raises(AssertionError):
    cluster_eval.ClusterEvalAccumulator(2, 6, 3, torch.device("cpu"))
  with pytest.raises(AssertionError):
    cluster_eval._rows([torch.full((4, 3), 1.0 / 3)] * 2)              # no fallback for host tensors


def test_symbol_is_declared_and_bound():
  from iic_amd import _lib
  header = open(os.path.join(ROOT, "include", "iic_hip.h")).read()
  proto = re.search(r"\bint\s+iic_cluster_argmax_acc\s*\(([^;]*?)\)\s*;", header, flags=re.S)
  assert proto is not None
  assert len(proto.group(1).split(",")) == 12 and "void* stream" in proto.group(1)
  assert "iic_cluster_argmax_acc" in _lib.EXPORTED_SYMBOLS
  res, args = _lib._SIGNATURES["iic_cluster_argmax_acc"]
  assert len(args) == 12
  src = open(os.path.join(ROOT, "iic_amd", "csrc", "eval_metrics.hip")).read()
  assert "cluster_argmax_acc_kernel" in src


def _flat_flow(preds_a, t_a, preds_t, t_t, config, use_sub_head=None):
  """The reference's flow on flat numpy arrays: the masked-sum matches of eval_metrics.py (:18-24 strict `>` update,
  :42-46 linear assignment on num_samples - num_correct), the reorder loop and _acc."""
  from scipy.optimize import linear_sum_assignment
  k, gt_k, H = config.output_k, config.gt_k, config.num_sub_heads

  def match_of(p, t):
    if config.eval_mode == "orig":
      out = []
      for c1 in range(k):
        best, best_c2 = -1, None
        for c2 in range(gt_k):
          votes = int(((p == c1) * (t == c2)).sum())
          if votes > best:
            best, best_c2 = votes, c2
        out.append((c1, best_c2))
      return out
    assert k == gt_k
    num_correct = np.zeros((k, gt_k))
    for c1 in range(k):
      for c2 in range(gt_k):
        num_correct[c1, c2] = int(((p == c1) * (t == c2)).sum())
    rows, cols = linear_sum_assignment(t.shape[0] - num_correct)
    return [(int(a), int(b)) for a, b in zip(rows, cols)]

  def acc_of(p, t, match):
    r = np.zeros(t.shape[0], dtype=p.dtype)
    for pred_i, target_i in match:
      r[p == pred_i] = target_i
    return int((r == t).sum()) / float(t.shape[0])

  matches = [match_of(preds_a[i], t_a) for i in range(H)]
  train_accs = np.zeros(H, dtype=np.float32)
  for i in range(H):
    train_accs[i] = acc_of(preds_a[i], t_a, matches[i])
  best = np.argmax(train_accs)
  if H > 1 and use_sub_head is not None:
    best = use_sub_head
  if config.mode == "IID":
    test_accs = train_accs
  else:
    test_accs = np.zeros(H, dtype=np.float32)
    for i in range(H):
      test_accs[i] = acc_of(preds_t[i], t_t, matches[i])
  return {"test_accs": list(test_accs), "avg": np.mean(test_accs), "std": np.std(test_accs), "best": test_accs[best],
          "worst": test_accs.min(), "best_train_sub_head": best, "best_train_sub_head_match": matches[best],
          "train_accs": list(train_accs)}


def _counts(preds, t, k, gt_k):
  c = np.zeros((preds.shape[0], k, gt_k), np.int64)
  for h in range(preds.shape[0]):
    np.add.at(c[h], (preds[h], t), 1)
  return c


@pytest.mark.parametrize("use_sub_head", [None, 0])
@pytest.mark.parametrize("mode", ["IID", "IID+"])
@pytest.mark.parametrize("eval_mode,k,gt_k", [("orig", 12, 4), ("hung", 5, 5)])
def test_stats_from_counts_equals_the_flat_array_flow(eval_mode, k, gt_k, mode, use_sub_head):
  from iic_amd.cluster_eval import stats_from_counts       # the name the twin calls
  H, n_a, n_t = 3, 301, 97
  rng = np.random.default_rng(k * 10 + len(mode))
  t_a, t_t = rng.integers(0, gt_k, n_a), rng.integers(0, gt_k, n_t)
  # predictions correlated with the targets (a fixed random cluster -> class map plus noise), one cluster left empty
  def preds_for(t):
    out = []
    for h in range(H):
      p = (t * (k // gt_k) + rng.integers(0, k // gt_k, t.shape[0])) % k
      noise = rng.random(t.shape[0]) < 0.3 + 0.1 * h
      p[noise] = rng.integers(0, k - 1, int(noise.sum()))
      out.append(p)
    return np.stack(out)
  preds_a, preds_t = preds_for(t_a), preds_for(t_t)
  config = types.SimpleNamespace(num_sub_heads=H, output_k=k, gt_k=gt_k, eval_mode=eval_mode, mode=mode,
                                 mapping_assignment_partitions=["a"], mapping_test_partitions=["a"])
  got = stats_from_counts(_counts(preds_a, t_a, k, gt_k), n_a, _counts(preds_t, t_t, k, gt_k), n_t, config,
                          use_sub_head=use_sub_head)
  want = _flat_flow(preds_a, t_a, preds_t, t_t, config, use_sub_head=use_sub_head)
  assert set(got) == set(want)
  for key in ("test_accs", "train_accs"):
    assert np.array(got[key]).tobytes() == np.array(want[key]).tobytes(), (key, got[key], want[key])
  for key in ("avg", "std", "best", "worst"):
    assert type(got[key]) is type(want[key]) and np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
  assert int(got["best_train_sub_head"]) == int(want["best_train_sub_head"])
  assert got["best_train_sub_head_match"] == want["best_train_sub_head_match"]
