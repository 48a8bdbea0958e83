"""iic_amd.seg_eval on the host: stats_from_counts against the reference's procedure (cluster_eval.py:101-145) written
out on flat arrays with oracle.eval_oracle, the no-CPU-fallback rule, and install.PATCHES staying as it is."""
import types

import numpy as np
import pytest
import torch

from oracle import eval_oracle

H, KP, KT = 4, 6, 3


def _flat(seed, n, kp, kt, heads):
  """Seeded flat predictions per sub-head + targets.  Sub-head 1 repeats sub-head 0 (their accuracies tie: the first one
  is the best); the last sub-head spreads every cluster evenly over the classes (with n a multiple of kp * kt every row
  of its counts ties)."""
  rng = np.random.default_rng(seed)
  idx = np.arange(n)
  t = (idx % kt).astype(np.uint8)
  preds = []
  for h in range(heads):
    noise = rng.integers(0, kp, n)
    keep = rng.random(n) < 0.35 + 0.1 * h
    preds.append(np.where(keep, (t.astype(np.int64) * 2 + h) % kp, noise).astype(np.uint8))
  preds[1] = preds[0].copy()
  preds[-1] = ((idx // kt) % kp).astype(np.uint8)
  return preds, t


def _reference_stats(preds_a, t_a, preds_t, t_t, cfg, use_sub_head=None):
  """cluster_subheads_eval + _get_assignment_data_matches on flat arrays (numpy restatement, reorder loop included)."""
  def reordered_acc(p, t, match):
    r = np.zeros(p.shape[0], dtype=p.dtype)
    for pred_i, target_i in match:
      r[p == pred_i] = target_i
    return eval_oracle.acc(r, t)
  matcher = eval_oracle.hungarian_match if cfg.eval_mode == "hung" else eval_oracle.original_match
  all_matches, train_accs = [], np.zeros(cfg.num_sub_heads, dtype=np.float32)
  for i in range(cfg.num_sub_heads):
    match = matcher(preds_a[i], t_a, cfg.output_k, cfg.gt_k)
    all_matches.append(match)
    train_accs[i] = reordered_acc(preds_a[i], t_a, match)
  best_eval = np.argmax(train_accs)
  best = use_sub_head if (cfg.num_sub_heads > 1 and use_sub_head is not None) else best_eval
  if cfg.mode == "IID":
    test_accs = train_accs
  else:
    test_accs = np.zeros(cfg.num_sub_heads, dtype=np.float32)
    for i in range(cfg.num_sub_heads):
      test_accs[i] = reordered_acc(preds_t[i], t_t, all_matches[i])
  return {"test_accs": list(test_accs), "avg": np.mean(test_accs), "std": np.std(test_accs), "best": test_accs[best],
          "worst": test_accs.min(), "best_train_sub_head": best, "best_train_sub_head_match": all_matches[best],
          "train_accs": list(train_accs)}


def _same(a, b):
  assert set(a) == set(b)
  for key in a:
    x, y = a[key], b[key]
    if key in ("test_accs", "train_accs"):
      assert len(x) == len(y) and all(type(u) is np.float32 and type(v) is np.float32 for u, v in zip(x, y))
      assert np.array(x).tobytes() == np.array(y).tobytes(), key
    elif key == "best_train_sub_head_match":
      assert x == y, key
    elif key == "best_train_sub_head":
      assert int(x) == int(y), key
    else:
      assert type(x) is type(y) and np.asarray(x).tobytes() == np.asarray(y).tobytes(), key


@pytest.mark.parametrize("use_sub_head", [None, 2])
@pytest.mark.parametrize("mode", ["IID", "IID+"])
@pytest.mark.parametrize("eval_mode,kp", [("orig", KP), ("hung", KT)])
def test_stats_from_counts_vs_flat_array_procedure(eval_mode, kp, mode, use_sub_head):
  from iic_amd.seg_eval import stats_from_counts
  cfg = types.SimpleNamespace(num_sub_heads=H, output_k=kp, gt_k=KT, eval_mode=eval_mode, mode=mode,
                              mapping_assignment_partitions=["a"], mapping_test_partitions=["a"])
  pa, ta = _flat(11, 5040, kp, KT, H)          # 5040 = 280 * 18: a multiple of kp * kt for both cluster counts
  pt, tt = _flat(12, 3001, kp, KT, H)
  ca = np.stack([eval_oracle.contingency(p, ta, kp, KT) for p in pa])
  ct = np.stack([eval_oracle.contingency(p, tt, kp, KT) for p in pt])
  assert (ca[-1] == ca[-1][0, 0]).all()                          # the tied sub-head really ties, in every row
  want = _reference_stats(pa, ta, pt, tt, cfg, use_sub_head)
  got = stats_from_counts(ca, ta.shape[0], ct if mode == "IID+" else None, tt.shape[0], cfg, use_sub_head=use_sub_head)
  _same(got, want)
  if use_sub_head is None:
    assert int(got["best_train_sub_head"]) == int(np.argmax(want["train_accs"]))
    assert want["train_accs"][0] == want["train_accs"][1]        # tie between sub-heads: the first one wins


def test_stats_from_counts_single_sub_head_ignores_use_sub_head():
  from iic_amd.seg_eval import stats_from_counts
  cfg = types.SimpleNamespace(num_sub_heads=1, output_k=KP, gt_k=KT, eval_mode="orig", mode="IID",
                              mapping_assignment_partitions=["a"], mapping_test_partitions=["a"])
  pa, ta = _flat(5, 777, KP, KT, 2)
  ca = np.stack([eval_oracle.contingency(pa[0], ta, KP, KT)])
  got = stats_from_counts(ca, 777, None, 0, cfg, use_sub_head=3)
  _same(got, _reference_stats(pa[:1], ta, None, None, cfg, use_sub_head=3))
  assert int(got["best_train_sub_head"]) == 0


def test_seg_eval_has_no_cpu_fallback():
  from iic_amd import seg_eval
  with pytest.raises(AssertionError):
    seg_eval.SegEvalAccumulator(2, KP, KT, "cpu")
  acc = object.__new__(seg_eval.SegEvalAccumulator)
  acc.num_sub_heads, acc.output_k, acc.gt_k = 1, KP, KT
  acc.buf = torch.zeros((1, KP * KT + 1), dtype=torch.long)
  z = torch.zeros(16, dtype=torch.uint8)
  with pytest.raises(AssertionError):
    acc.add([z], z, z)
  assert int(acc.buf.sum()) == 0


def test_install_patches_do_not_name_seg_eval():
  from iic_amd import install
  assert not any("iic_amd.seg_eval" in field for row in install.PATCHES for field in row)
