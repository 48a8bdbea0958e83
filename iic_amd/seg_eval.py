"""Segmentation evaluation on the device -- opt-in twin of code/utils/segmentation/segmentation_eval.py.

The reference's ``_segmentation_get_data`` (:44-140) takes the full ``[N, k, S, S]`` fp32 probability maps of every
test batch, arg-maxes them to int64, copies the result into flat uint8 arrays that span the whole test set and
``masked_select``s all of them; ``cluster_subheads_eval`` (cluster_eval.py:78-145) then builds the cluster-vs-class
counts from those arrays, rewrites a flat array ``output_k`` times per sub-head (:216-217, :130-131) and counts
equal elements.  Every number of the returned dict is a function of one ``output_k x gt_k`` count matrix per sub-head.

Here the nets return uint8 label maps directly (``predict_labels``, csrc/seg_eval.hip::seg_label_map_kernel), one
streaming kernel folds each batch's (labels, targets, mask) into a device-resident count matrix
(``SegEvalAccumulator``), and ``stats_from_counts`` computes the dict from it on the host: no flat array of the test
set exists and no fp32 map is written.

``install()`` does not rebind this module (install.PATCHES is strict and lists names every supported reference tree
has); a script opts in by binding ``segmentation_eval`` from here -- INTEGRATION.md section 5c.
"""
import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr
from .transforms import sobel_process

__all__ = ["segmentation_eval", "SegEvalAccumulator", "stats_from_counts"]
U8 = torch.uint8


def _label_maps(config, net, imgs):
  """One uint8 [N, S, S] map per sub-head: the net's own ``predict_labels`` where it has one (through a DataParallel
  wrapper too), the reference's arg-max of the probability maps (segmentation_eval.py:84, :100) otherwise."""
  core = getattr(net, "module", net)
  with torch.no_grad():
    if hasattr(core, "predict_labels"):
      maps = core.predict_labels(imgs)
    else:
      x_outs = net(imgs)
      assert (x_outs[0].shape[1] == config.output_k)
      maps = [torch.argmax(x, dim=1).to(U8) for x in x_outs]
  assert (len(maps) == config.num_sub_heads)
  assert (maps[0].shape[1] == config.input_sz and maps[0].shape[2] == config.input_sz)
  return maps


def _u8(t, device, is_mask=False):
  """Flat uint8 view / copy of a batch's targets or mask on `device` (what the reference's slice assignments into its
  uint8 arrays do, segmentation_eval.py:104-106)."""
  t = t.to(device)
  if t.dtype == torch.bool:
    t = t.view(U8) if t.is_contiguous() else t.to(U8)
  elif t.dtype != U8:
    t = (t != 0).to(U8) if is_mask else t.to(U8)
  return t.reshape(-1).contiguous()


def _segmentation_get_data(config, net, dataloader, sobel=False, using_IR=False, verbose=0):
  """The reference's function (segmentation_eval.py:44-140) with its signature, asserts and return value -- flat uint8
  device tensors of the selected pixels -- for callers that want the arrays.  The label maps come from
  ``predict_labels``: the fp32 probability maps and the int64 arg-max are never written."""
  assert (config.output_k <= 255)
  num_batches = len(dataloader)
  num_samples = 0
  # upper bound, will be less for last batch
  samples_per_batch = config.batch_sz * config.input_sz * config.input_sz
  dev = torch.device("cuda", torch.cuda.current_device())
  flat_predss_all = [torch.zeros((num_batches * samples_per_batch), dtype=U8, device=dev)
                     for _ in range(config.num_sub_heads)]
  flat_targets_all = torch.zeros((num_batches * samples_per_batch), dtype=U8, device=dev)
  mask_all = torch.zeros((num_batches * samples_per_batch), dtype=U8, device=dev)
  for b_i, batch in enumerate(dataloader):
    imgs, flat_targets, mask = batch
    imgs = imgs.cuda()
    if sobel:
      imgs = sobel_process(imgs, config.include_rgb, using_IR=using_IR)
    maps = _label_maps(config, net, imgs)
    # actual batch size
    actual_samples_curr = (flat_targets.shape[0] * config.input_sz * config.input_sz)
    num_samples += actual_samples_curr
    # vectorise: collapse from 2D to 1D
    start_i = b_i * samples_per_batch
    for i in range(config.num_sub_heads):
      flat_predss_all[i][start_i:(start_i + actual_samples_curr)] = maps[i].view(-1)
    flat_targets_all[start_i:(start_i + actual_samples_curr)] = _u8(flat_targets, dev)
    mask_all[start_i:(start_i + actual_samples_curr)] = _u8(mask, dev, is_mask=True)
  flat_predss_all = [flat_predss_all[i][:num_samples] for i in range(config.num_sub_heads)]
  flat_targets_all = flat_targets_all[:num_samples]
  mask_all = mask_all[:num_samples].bool()
  flat_predss_all = [flat_predss_all[i].masked_select(mask=mask_all) for i in range(config.num_sub_heads)]
  flat_targets_all = flat_targets_all.masked_select(mask=mask_all)
  selected_samples = int(mask_all.sum())
  assert (len(flat_predss_all[0].shape) == 1 and len(flat_targets_all.shape) == 1)
  assert (flat_predss_all[0].shape[0] == selected_samples)
  assert (flat_targets_all.shape[0] == selected_samples)
  return flat_predss_all, flat_targets_all


class SegEvalAccumulator(object):
  """Device-resident cluster-vs-class counts of ``num_sub_heads`` sub-heads, accumulated batch by batch.

  ``add`` enqueues one iic_seg_contingency_acc launch per sub-head and never waits for the device; ``counts`` is the one
  device -> host transfer of an evaluation pass."""

  def __init__(self, num_sub_heads, output_k, gt_k, device):
    device = torch.device(device)
    assert device.type == "cuda", "SegEvalAccumulator (HIP): device memory required -- no CPU fallback"
    assert 1 <= output_k <= 255 and 1 <= gt_k <= 256 and num_sub_heads >= 1
    self.num_sub_heads, self.output_k, self.gt_k = num_sub_heads, output_k, gt_k
    self.buf = torch.zeros((num_sub_heads, output_k * gt_k + 1), dtype=torch.long, device=device)

  def add(self, label_maps, flat_targets, mask=None):
    """label_maps: one uint8 device tensor per sub-head; flat_targets, mask: device tensors with as many elements
    (uint8, or anything the reference's copies into its uint8 arrays accept; mask None selects every pixel)."""
    assert len(label_maps) == self.num_sub_heads
    assert all(torch.is_tensor(t) and t.is_cuda for t in list(label_maps) + [flat_targets] +
               ([] if mask is None else [mask])), "SegEvalAccumulator.add (HIP): device tensors required -- no CPU fallback"
    dev = self.buf.device
    t = _u8(flat_targets, dev)
    m = None if mask is None else _u8(mask, dev, is_mask=True)
    n = t.numel()
    assert m is None or m.numel() == n
    for i, lm in enumerate(label_maps):
      assert lm.dtype == U8 and lm.numel() == n
      p = lm.reshape(-1).contiguous()
      check(lib().iic_seg_contingency_acc(ptr(p), ptr(t), ptr(m), n, self.output_k, self.gt_k, ptr(self.buf[i]),
                                          stream_ptr()), "iic_seg_contingency_acc")

  def counts(self):
    """(int64 [num_sub_heads, output_k, gt_k], number of selected pixels) as numpy / int -- one transfer."""
    host = self.buf.cpu().numpy()
    nb = self.output_k * self.gt_k
    return host[:, :nb].reshape(self.num_sub_heads, self.output_k, self.gt_k).copy(), int(host[0, nb])


def _match_and_acc(c, n, eval_mode):
  """What _get_assignment_data_matches (cluster_eval.py:193-228) derives from one sub-head's flat arrays, from their
  count matrix: the match, and the accuracy of the predictions reordered by it."""
  if eval_mode == "hung":
    from scipy.optimize import linear_sum_assignment
    assert (c.shape[0] == c.shape[1])  # one to one
    rows, cols = linear_sum_assignment(n - c)
    match = [(int(out_c), int(gt_c)) for out_c, gt_c in zip(rows, cols)]
  elif eval_mode == "orig":
    # first maximum in class order wins, as the reference's strict '>' update (eval_metrics.py:22)
    match = [(out_c, int(np.argmax(c[out_c]))) for out_c in range(c.shape[0])]
  else:
    assert (False)
  assert (len(set(p for p, _ in match)) == c.shape[0])  # each output_k must get mapped
  return match, _acc_from_counts(c, n, match)


def _acc_from_counts(c, n, match):
  # `reordered_preds[flat_preds == pred_i] = target_i` then _acc: the pixels of cluster pred_i that are right are the
  # ones whose target is target_i
  return int(sum(int(c[p, t]) for p, t in match)) / float(n)


def stats_from_counts(counts_assign, n_assign, counts_test, n_test, config, use_sub_head=None):
  """The dict of cluster_subheads_eval (cluster_eval.py:101-145) from count matrices [num_sub_heads, output_k, gt_k]
  and the numbers of selected pixels.  Pure numpy; counts_test / n_test are read in "IID+" mode only."""
  counts_assign = np.asarray(counts_assign)
  # _acc's asserts (eval_metrics.py:66): every selected prediction and target is a valid class
  assert (all(int(c.sum()) == n_assign for c in counts_assign))
  all_matches = []
  train_accs = np.zeros(config.num_sub_heads, dtype=np.float32)
  for i in range(config.num_sub_heads):
    match, acc = _match_and_acc(counts_assign[i], n_assign, config.eval_mode)
    all_matches.append(match)
    train_accs[i] = acc
  best_sub_head_eval = np.argmax(train_accs)
  if (config.num_sub_heads > 1) and (use_sub_head is not None):
    best_sub_head = use_sub_head
  else:
    best_sub_head = best_sub_head_eval
  if config.mode == "IID":
    assert (config.mapping_assignment_partitions == config.mapping_test_partitions)
    test_accs = train_accs
  elif config.mode == "IID+":
    counts_test = np.asarray(counts_test)
    assert (all(int(c.sum()) == n_test for c in counts_test))
    test_accs = np.zeros(config.num_sub_heads, dtype=np.float32)
    for i in range(config.num_sub_heads):
      test_accs[i] = _acc_from_counts(counts_test[i], n_test, all_matches[i])
  else:
    assert (False)
  return {"test_accs": list(test_accs),
          "avg": np.mean(test_accs),
          "std": np.std(test_accs),
          "best": test_accs[best_sub_head],
          "worst": test_accs.min(),
          "best_train_sub_head": best_sub_head,  # from training data
          "best_train_sub_head_match": all_matches[best_sub_head],
          "train_accs": list(train_accs)}


def _stream_counts(config, net, dataloader, sobel, using_IR):
  """One pass over a loader: every batch's label maps folded into the device-resident counts."""
  assert (config.output_k <= 255)
  dev = torch.device("cuda", torch.cuda.current_device())
  acc = SegEvalAccumulator(config.num_sub_heads, config.output_k, config.gt_k, dev)
  for batch in dataloader:
    imgs, flat_targets, mask = batch
    imgs = imgs.cuda()
    if sobel:
      imgs = sobel_process(imgs, config.include_rgb, using_IR=using_IR)
    maps = _label_maps(config, net, imgs)
    assert (maps[0].shape[0] == flat_targets.shape[0])
    acc.add(maps, flat_targets.to(dev, non_blocking=True), mask.to(dev, non_blocking=True))
  return acc.counts()


def segmentation_eval(config, net, mapping_assignment_dataloader, mapping_test_dataloader, sobel, using_IR=False,
                      verbose=0, return_only=False):
  """Twin of the reference's segmentation_eval (segmentation_eval.py:12-41): same net.eval() / net.train() bracket, same
  stats dict, same config.epoch_* bookkeeping; the two loaders are streamed through SegEvalAccumulator.  (The
  reference's torch.cuda.empty_cache() calls made room for its test-set-sized arrays; there are none here.)"""
  net.eval()
  counts_assign, n_assign = _stream_counts(config, net, mapping_assignment_dataloader, sobel, using_IR)
  counts_test, n_test = None, 0
  if config.mode == "IID+":
    counts_test, n_test = _stream_counts(config, net, mapping_test_dataloader, sobel, using_IR)
  stats_dict = stats_from_counts(counts_assign, n_assign, counts_test, n_test, config)
  net.train()

  acc = stats_dict["best"]
  is_best = (len(config.epoch_acc) > 0) and (acc > max(config.epoch_acc))
  if not return_only:
    config.epoch_stats.append(stats_dict)
    config.epoch_acc.append(acc)
    config.epoch_avg_subhead_acc.append(stats_dict["avg"])
    return is_best
  else:
    return stats_dict
