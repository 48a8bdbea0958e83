"""Clustering evaluation on the device -- opt-in twin of code/utils/cluster/cluster_eval.py.

The reference's ``_clustering_get_data`` (:15-75) arg-maxes every sub-head separately (int64 out) and slice-assigns each
into flat int32 arrays that span the whole data set; ``_get_assignment_data_matches`` (:187-228) and the "IID+" branch of
``cluster_subheads_eval`` (:127-134) then rewrite a flat array once per output cluster and sub-head
(``reordered_preds[flat_preds == pred_i] = target_i``: 2 launches x output_k x num_sub_heads, 700 at output_k = 70 with 5
sub-heads) and ``_acc`` widens to int64 and syncs for two maxima.  Every number of the returned dict is a function of one
``output_k x gt_k`` count matrix per sub-head.

Here ONE launch per batch (csrc/eval_metrics.hip::cluster_argmax_acc_kernel) arg-maxes all sub-heads and folds the batch
into a device-resident count matrix (``ClusterEvalAccumulator``); ``seg_eval.stats_from_counts`` computes the dict from
it on the host.  No flat array of the data set exists and nothing waits for the device until the one transfer at the
end of a pass.

``install()`` does not rebind this module (install.PATCHES is strict); a script opts in by binding ``cluster_eval`` /
``cluster_subheads_eval`` / ``get_subhead_using_loss`` from here -- INTEGRATION.md section 5d.
"""
import sys
from datetime import datetime

import numpy as np
import torch

from . import eval_metrics, ops
from ._lib import check, lib, ptr, stream_ptr
from .losses import IID_loss_heads
from .seg_eval import stats_from_counts
from .transforms import sobel_process

__all__ = ["cluster_eval", "cluster_subheads_eval", "get_subhead_using_loss", "ClusterEvalAccumulator"]
F32 = torch.float32


def _rows(x_outs):
  """(tensor that owns the memory, device pointer of row 0 of sub-head 0, ld, head_stride, n, H, k) of a forward's
  sub-head outputs, in floats: row i of sub-head h is at pointer + 4 * (i * ld + h * head_stride).

  x_outs: the packed [n, H, k] tensor (``forward_packed``), or the list ``forward`` returns.  A list whose tensors are
  uniformly strided views of one storage -- what the nets' tag_pack'ed head outputs are, ``probs[:, i, :]`` -- is read
  in place; any other list is stacked once."""
  if torch.is_tensor(x_outs):
    assert x_outs.dim() == 3
    t = x_outs
  else:
    ts = list(x_outs)
    assert len(ts) >= 1 and all(torch.is_tensor(t) and t.dim() == 2 and t.shape == ts[0].shape for t in ts)
    assert all(t.is_cuda for t in ts), "cluster_eval (HIP): device tensors required -- no CPU fallback"
    n, k = ts[0].shape
    steps = set(b.data_ptr() - a.data_ptr() for a, b in zip(ts, ts[1:]))
    if (all(t.dtype == F32 and t.untyped_storage().data_ptr() == ts[0].untyped_storage().data_ptr() and
            t.stride(0) == ts[0].stride(0) and (t.stride(1) == 1 or k == 1) for t in ts) and
        len(steps) <= 1 and all(s % 4 == 0 for s in steps)):
      return ts[0], ts[0].data_ptr(), ts[0].stride(0), (steps.pop() // 4 if steps else 0), n, len(ts), k
    t = torch.stack(ts, dim=1)
  assert t.is_cuda, "cluster_eval (HIP): device tensors required -- no CPU fallback"
  assert t.dtype == F32
  if t.stride(2) != 1 and t.shape[2] != 1:
    t = t.contiguous()
  n, H, k = t.shape
  return t, t.data_ptr(), t.stride(0), t.stride(1), n, H, k


def _check_launch(n, H, k, expect, targets, gt_k, counts, labels, label_offset, label_stride):
  """Everything iic_cluster_argmax_acc cannot know: the sizes of the three device buffers against the (n, H, k) the
  kernel will index them with, and (H, k) against what the caller was built for.  Raises ValueError; runs BEFORE the
  launch, so a mismatch touches no device memory."""
  if expect is not None and (H, k) != tuple(expect):
    raise ValueError("cluster_eval (HIP): %d sub-heads of %d clusters given, %d of %d expected" % ((H, k) + tuple(expect)))
  if targets is not None and not (targets.is_cuda and targets.dtype == torch.long and targets.is_contiguous() and
                                  targets.numel() == n):
    raise ValueError("cluster_eval (HIP): targets must be %d contiguous int64 device values, got %s %s"
                     % (n, tuple(targets.shape), targets.dtype))
  if counts is not None and not (targets is not None and gt_k >= 1 and counts.is_cuda and counts.dtype == torch.long and
                                 counts.is_contiguous() and tuple(counts.shape) == (H, k * gt_k + 1)):
    raise ValueError("cluster_eval (HIP): counts must be a contiguous int64 [%d, %d] device tensor, got %s %s"
                     % (H, k * gt_k + 1, tuple(counts.shape), counts.dtype))
  if labels is not None and not (labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous() and
                                 0 <= label_offset and label_offset + n <= label_stride and
                                 (H - 1) * label_stride + label_offset + n <= labels.numel()):
    raise ValueError("cluster_eval (HIP): labels of %d int32 values cannot hold %d sub-heads x %d rows at offset %d, "
                     "stride %d" % (labels.numel(), H, n, label_offset, label_stride))


def _argmax_acc(x_outs, targets, gt_k, counts, labels, label_offset, label_stride, expect=None):
  """One iic_cluster_argmax_acc launch on a forward's outputs (see _rows); returns (n, H, k).  ``expect``: the
  (num_sub_heads, output_k) the caller's buffers were sized for.  Every size is checked before the launch."""
  ops.join()      # a view forked onto a side stream is ordered before this stream from here on (as IID_loss)
  # `keep` only names the tensor the pointer came from.  A stacked temporary may be freed right after the enqueue: the
  # caching allocator reuses a block in stream order and the launch goes on the current stream, the one it was made on.
  keep, p, ld, hs, n, H, k = _rows(x_outs)
  _check_launch(n, H, k, expect, targets, gt_k, counts, labels, label_offset, label_stride)
  lp = None if labels is None else labels.data_ptr() + 4 * label_offset
  check(lib().iic_cluster_argmax_acc(p, ld, hs, n, H, k, ptr(targets), int(gt_k), ptr(counts), lp, label_stride,
                                     stream_ptr()), "iic_cluster_argmax_acc")
  return n, H, k


class ClusterEvalAccumulator(object):
  """Device-resident cluster-vs-class counts of ``num_sub_heads`` sub-heads, accumulated batch by batch.

  ``add`` enqueues one iic_cluster_argmax_acc launch (arg-max of every sub-head + counts) and never waits for the
  device; ``counts`` is the one device -> host transfer of an evaluation pass."""

  def __init__(self, num_sub_heads, output_k, gt_k, device):
    device = torch.device(device)
    assert device.type == "cuda", "ClusterEvalAccumulator (HIP): device memory required -- no CPU fallback"
    assert num_sub_heads >= 1 and output_k >= 1 and gt_k >= 1
    self.num_sub_heads, self.output_k, self.gt_k = num_sub_heads, output_k, gt_k
    self.buf = torch.zeros((num_sub_heads, output_k * gt_k + 1), dtype=torch.long, device=device)

  def add(self, x_outs, flat_targets):
    """x_outs: the packed [N, H, k] fp32 softmax output or the list a net's forward returns; flat_targets: [N] device
    tensor of class indices (int64 as the loaders collate them; anything else is widened)."""
    assert torch.is_tensor(flat_targets) and flat_targets.is_cuda, \
      "ClusterEvalAccumulator.add (HIP): device tensors required -- no CPU fallback"
    t = flat_targets.reshape(-1).to(self.buf.device).long().contiguous()
    # a list of other sub-heads, another k or targets of another length raise here, before anything is enqueued
    _argmax_acc(x_outs, t, self.gt_k, self.buf, None, 0, 0, expect=(self.num_sub_heads, self.output_k))

  def counts(self):
    """(int64 [num_sub_heads, output_k, gt_k], number of samples) as numpy / int -- one transfer."""
    host = self.buf.cpu().numpy()
    nb = self.output_k * self.gt_k
    return host[:, :nb].reshape(self.num_sub_heads, self.output_k, self.gt_k).copy(), int(host[0, nb])


def _forward(config, net, batch, sobel, using_IR):
  imgs = batch[0].cuda()
  if sobel:
    imgs = sobel_process(imgs, config.include_rgb, using_IR=using_IR)
  with torch.no_grad():
    x_outs = net(imgs)
  assert (x_outs[0].shape[1] == config.output_k)
  assert (len(x_outs[0].shape) == 2)
  return x_outs


def _clustering_get_data(config, net, dataloader, sobel=False, using_IR=False, get_soft=False, verbose=0):
  """The reference's function (cluster_eval.py:15-75) with its signature, asserts and return value -- flat int32 device
  tensors of predictions per sub-head and of targets -- for callers that want the arrays.  The predictions of a batch
  are written by one launch (the kernel's ``labels`` output): no int64 arg-max, no per-sub-head slice assignment."""
  assert (not using_IR)      # the clustering scripts have no infra-red channel
  num_batches = len(dataloader)
  total = num_batches * config.batch_sz
  dev = torch.device("cuda", torch.cuda.current_device())
  flat_targets_all = torch.zeros(total, dtype=torch.int32, device=dev)
  flat_predss_all = torch.zeros((config.num_sub_heads, total), dtype=torch.int32, device=dev)
  if get_soft:
    soft_predss_all = [torch.zeros((total, config.output_k), dtype=F32, device=dev)
                       for _ in range(config.num_sub_heads)]
  num_test = 0
  for b_i, batch in enumerate(dataloader):
    x_outs = _forward(config, net, batch, sobel, using_IR)
    flat_targets = batch[1]
    num_test_curr = flat_targets.shape[0]
    num_test += num_test_curr
    start_i = b_i * config.batch_sz
    # the reference's slice assignments raise on a batch above batch_sz, on outputs of another length and on a list of
    # more sub-heads than the config names; so does this, before the launch (here and in _check_launch)
    assert (num_test_curr <= config.batch_sz and x_outs[0].shape[0] == num_test_curr)
    _argmax_acc(x_outs, None, 0, None, flat_predss_all, start_i, total, expect=(config.num_sub_heads, config.output_k))
    if get_soft:
      for i in range(config.num_sub_heads):
        soft_predss_all[i][start_i:(start_i + num_test_curr), :] = x_outs[i]
    flat_targets_all[start_i:(start_i + num_test_curr)] = flat_targets.cuda()
  flat_predss_all = [flat_predss_all[i][:num_test] for i in range(config.num_sub_heads)]
  flat_targets_all = flat_targets_all[:num_test]
  if not get_soft:
    return flat_predss_all, flat_targets_all
  soft_predss_all = [soft_predss_all[i][:num_test] for i in range(config.num_sub_heads)]
  return flat_predss_all, flat_targets_all, soft_predss_all


def _stream_counts(config, net, dataloader, sobel, using_IR):
  """One pass over a loader: every batch's sub-head outputs folded into the device-resident counts."""
  assert (not using_IR)      # the clustering scripts have no infra-red channel
  dev = torch.device("cuda", torch.cuda.current_device())
  acc = ClusterEvalAccumulator(config.num_sub_heads, config.output_k, config.gt_k, dev)
  for batch in dataloader:
    x_outs = _forward(config, net, batch, sobel, using_IR)
    acc.add(x_outs, batch[1].to(dev, non_blocking=True))
  return acc.counts()


def _reordered_acc(flat_preds, flat_targets, match, gt_k, verbose=0):
  """cluster_eval.py:128-132 / :212-227: the predictions rewritten through the match, then _acc."""
  reordered_preds = torch.zeros(flat_targets.shape[0], dtype=flat_preds.dtype, device=flat_preds.device)
  for pred_i, target_i in match:
    reordered_preds[flat_preds == pred_i] = target_i
  return eval_metrics._acc(reordered_preds, flat_targets, gt_k, verbose)


def _flat_array_eval(config, net, mapping_assignment_dataloader, mapping_test_dataloader, sobel, using_IR, get_data_fn,
                     use_sub_head, verbose):
  """cluster_subheads_eval as the reference runs it (cluster_eval.py:101-145, :163-233), on the flat arrays a caller's
  own get_data_fn returns (the reference's segmentation scripts pass one) with the drop-ins of iic_amd.eval_metrics."""
  flat_predss_all, flat_targets_all = get_data_fn(config, net, mapping_assignment_dataloader, sobel=sobel,
                                                  using_IR=using_IR, verbose=verbose)
  assert (flat_predss_all[0].shape == flat_targets_all.shape)
  matcher = {"hung": eval_metrics._hungarian_match, "orig": eval_metrics._original_match}.get(config.eval_mode)
  assert (matcher is not None)
  all_matches = []
  train_accs = np.zeros(config.num_sub_heads, dtype=np.float32)
  for i in range(config.num_sub_heads):
    match = matcher(flat_predss_all[i], flat_targets_all, preds_k=config.output_k, targets_k=config.gt_k)
    assert (len(set(p for p, _ in match)) == config.output_k)      # a match names every cluster once
    all_matches.append(match)
    train_accs[i] = _reordered_acc(flat_predss_all[i], flat_targets_all, match, config.gt_k, verbose)
  best_sub_head_eval = np.argmax(train_accs)
  if (config.num_sub_heads > 1) and (use_sub_head is not None):
    best_sub_head = use_sub_head
  else:
    best_sub_head = best_sub_head_eval
  if config.mode == "IID":
    assert (config.mapping_assignment_partitions == config.mapping_test_partitions)
    test_accs = train_accs
  elif config.mode == "IID+":
    flat_predss_all, flat_targets_all = get_data_fn(config, net, mapping_test_dataloader, sobel=sobel,
                                                    using_IR=using_IR, verbose=verbose)
    test_accs = np.zeros(config.num_sub_heads, dtype=np.float32)
    for i in range(config.num_sub_heads):
      test_accs[i] = _reordered_acc(flat_predss_all[i], flat_targets_all, all_matches[i], config.gt_k)
  else:
    assert (False)
  return {"test_accs": list(test_accs),
          "avg": np.mean(test_accs),
          "std": np.std(test_accs),
          "best": test_accs[best_sub_head],
          "worst": test_accs.min(),
          "best_train_sub_head": best_sub_head,
          "best_train_sub_head_match": all_matches[best_sub_head],
          "train_accs": list(train_accs)}


def cluster_subheads_eval(config, net, mapping_assignment_dataloader, mapping_test_dataloader, sobel, using_IR=False,
                          get_data_fn=_clustering_get_data, use_sub_head=None, verbose=0):
  """Twin of the reference's cluster_subheads_eval (cluster_eval.py:78-145): same signature, same stats dict.  With the
  default get_data_fn both loaders are streamed through ClusterEvalAccumulator and the dict comes from
  seg_eval.stats_from_counts; any other get_data_fn gets the flat-array flow (_flat_array_eval)."""
  if get_data_fn is not _clustering_get_data:
    return _flat_array_eval(config, net, mapping_assignment_dataloader, mapping_test_dataloader, sobel, using_IR,
                            get_data_fn, use_sub_head, verbose)
  if verbose:
    print("calling cluster eval direct (streaming) %s" % datetime.now())
    sys.stdout.flush()
  counts_assign, n_assign = _stream_counts(config, net, mapping_assignment_dataloader, sobel, using_IR)
  counts_test, n_test = None, 0
  if config.mode == "IID+":
    counts_test, n_test = _stream_counts(config, net, mapping_test_dataloader, sobel, using_IR)
  if verbose:
    print("counts have arrived %s, num_test: %d" % (datetime.now(), n_assign))
    sys.stdout.flush()
  return stats_from_counts(counts_assign, n_assign, counts_test, n_test, config, use_sub_head=use_sub_head)


def _paired_batch(config, tup, channels, dev):
  """One step of the zipped head-B loaders as two image batches: loader 0's plain images once per transformed loader,
  and the images of transformed loaders 1 .. num_dataloaders in the same order.  Both are cut from batch_sz-row buffers,
  so a step that would not fit raises as it does in the reference (cluster_eval.py:253-275)."""
  assert (len(tup) > config.num_dataloaders)
  plain = tup[0][0]
  b = plain.size(0)
  shape = (config.batch_sz, channels, config.input_sz, config.input_sz)
  imgs, imgs_tf = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
  for d_i in range(config.num_dataloaders):
    transformed = tup[1 + d_i][0]
    assert (transformed.size(0) == b)
    imgs[d_i * b:(d_i + 1) * b] = plain.to(dev)
    imgs_tf[d_i * b:(d_i + 1) * b] = transformed.to(dev)
  rows = b * config.num_dataloaders
  return imgs[:rows], imgs_tf[:rows]


def _subhead_loss_sums(config, dataloaders_head_B, net, sobel, lamb):
  """float64 [num_sub_heads]: every sub-head's IID loss on head B summed over the batches of the reference's loop
  (cluster_eval.py:244-293).  All sub-heads' losses of a batch come from IID_loss_heads and are added into a float64
  device tensor batch by batch in loop order -- the float64 sums of the reference's
  `loss_per_sub_head[i] += loss.item()` without a host sync per sub-head and batch -- with ONE transfer at the end."""
  dev = torch.device("cuda", torch.cuda.current_device())
  loss_sums = torch.zeros(config.num_sub_heads, dtype=torch.float64, device=dev)
  channels = config.in_channels - 1 if sobel else config.in_channels      # sobel_process makes the last one
  for b_i, tup in enumerate(zip(*dataloaders_head_B)):
    getattr(net, "module", net).zero_grad()
    imgs, imgs_tf = _paired_batch(config, tup, channels, dev)
    if sobel:
      imgs = sobel_process(imgs, config.include_rgb)
      imgs_tf = sobel_process(imgs_tf, config.include_rgb)
    with torch.no_grad():
      x_outs = net(imgs, head="B")
      x_tf_outs = net(imgs_tf, head="B")
      assert (len(x_outs) == config.num_sub_heads)
      loss, _ = IID_loss_heads(x_outs, x_tf_outs, lamb=lamb)
      loss_sums += loss.double()
    if b_i % 100 == 0:
      print("at batch %d" % b_i)
      sys.stdout.flush()
  return loss_sums.cpu().numpy()      # the one device -> host transfer


def _print_choice(config, loss_per_sub_head, by_loss):
  """compare=True: the sub-head the loss picks next to the one the best epoch's evaluation picked, with the test
  accuracy of each (the lines the reference prints, cluster_eval.py:297-313)."""
  print(loss_per_sub_head)
  print("best sub_head by loss: %d" % by_loss)
  stats = config.epoch_stats[int(np.argmax(np.array(config.epoch_acc)))]
  # stats dicts pickled by early runs of the reference name the two entries "best_head" and "all"
  head_key, accs_key = ("best_train_sub_head", "test_accs") if "best_train_sub_head" in stats else ("best_head", "all")
  by_eval, accs = stats[head_key], stats[accs_key]
  print("best sub_head by eval: %d" % by_eval)
  print("... loss select acc: %f, eval select acc: %f" % (accs[by_loss], accs[by_eval]))


def get_subhead_using_loss(config, dataloaders_head_B, net, sobel, lamb, compare=False):
  """Twin of the reference's get_subhead_using_loss (cluster_eval.py:236-317): same signature, same net.eval() /
  net.train() bracket, same return value; the sums come from _subhead_loss_sums."""
  net.eval()
  loss_per_sub_head = _subhead_loss_sums(config, dataloaders_head_B, net, sobel, lamb)
  by_loss = np.argmin(loss_per_sub_head)
  if compare:
    _print_choice(config, loss_per_sub_head, by_loss)
  net.train()
  return by_loss


def cluster_eval(config, net, mapping_assignment_dataloader, mapping_test_dataloader, sobel, use_sub_head=None,
                 print_stats=False):
  """Twin of the reference's cluster_eval (cluster_eval.py:320-362), same signature and return value.  With
  config.double_eval one extra pass runs first in whatever mode the net is in -- in training mode BatchNorm normalises
  with, and updates, batch statistics, a second opinion where the training set is the test set -- and goes to the
  config.double_eval_* lists; the pass that counts runs between net.eval() and net.train() and goes to config.epoch_*.
  print_stats prints both dicts instead, appends nothing and returns None."""
  def one_pass():
    return cluster_subheads_eval(config, net, mapping_assignment_dataloader=mapping_assignment_dataloader,
                                 mapping_test_dataloader=mapping_test_dataloader, sobel=sobel, use_sub_head=use_sub_head)

  def record(stats, title, stats_list, acc_list, avg_list):
    if print_stats:
      print(title)
      print(stats)
    else:
      stats_list.append(stats)
      acc_list.append(stats["best"])
      avg_list.append(stats["avg"])

  if config.double_eval:
    record(one_pass(), "double eval stats:", config.double_eval_stats, config.double_eval_acc,
           config.double_eval_avg_subhead_acc)
  net.eval()
  stats = one_pass()
  net.train()
  # better than every epoch so far; the first epoch never is
  is_best = (len(config.epoch_acc) > 0) and (stats["best"] > max(config.epoch_acc))
  record(stats, "eval stats:", config.epoch_stats, config.epoch_acc, config.epoch_avg_subhead_acc)
  return None if print_stats else is_best
