"""The triplets baseline on the device -- opt-in twin of code/utils/cluster/baselines/triplets.py.

``triplets_loss`` (:231-238) is one autograd node over iic_triplets_loss (csrc/triplets.hip): the loss and the three
gradients in two launches instead of torch's chain of about fifteen.  It evaluates the log-space closed form, so the
gradients of ``outs_pos`` / ``outs_neg`` stay finite where torch's own are 0 * (-inf) = NaN (a softmax entry that
underflows); include/iic_hip.h states the contract.

``triplets_get_data`` / ``triplets_get_data_kmeans_on_features`` / ``triplets_eval`` (:97-228) keep the reference's
signatures, return values and bookkeeping on ``config``; predictions come from iic_cluster_argmax_acc, k-means from
iic_amd.kmeans, and every number of the evaluation from one iic_contingency matrix.  ``triplet_batches`` yields what
``make_triplets_data``'s three zipped loaders yield (:71-85) from a device augmenter.

The nets are iic_amd.archs.TripletsNet5g / TripletsNet6c.  ``install()`` rebinds nothing of this: the reference's
triplets modules import torchvision and scikit-learn at import time, a script opts in -- INTEGRATION.md section 5h.
Graph capture and data parallelism of this step are not built.
"""
import numpy as np
import torch

from . import eval_metrics, ops
from ._lib import check, lib, ptr, stream_ptr
from .cluster_eval import _argmax_acc
from .kmeans import KMeans

__all__ = ["triplets_loss", "triplets_get_data", "triplets_get_data_kmeans_on_features", "triplets_eval",
           "triplet_batches", "supported", "workspace_bytes", "loss_and_grads"]
F32 = torch.float32
MAX_K = 1024


def supported(N, k):
  """Whether the kernel serves [N, k] logits: 1 <= k <= 1024, N >= 1, N k < 2^31.  Host only."""
  return bool(lib().iic_triplets_supported(int(N), int(k)))


def workspace_bytes(N, k):
  """Bytes of scratch one iic_triplets_loss call on [N, k] needs; 0 outside the served range.  Host only."""
  return int(lib().iic_triplets_workspace_bytes(int(N), int(k)))


def _rows(t, what, N=None, k=None):
  """A [N, k] fp32 device tensor the kernel can read in place (inner stride 1), else its contiguous copy."""
  if not torch.is_tensor(t):
    raise ValueError("triplets_loss (HIP): %s must be a torch tensor, got %s" % (what, type(t).__name__))
  if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
    raise ValueError("triplets_loss (HIP): %s must be [N, k] with N, k >= 1, got %s" % (what, tuple(t.shape)))
  if N is not None and tuple(t.shape) != (N, k):
    raise ValueError("triplets_loss (HIP): %s is %s, outs_orig is %s" % (what, tuple(t.shape), (N, k)))
  if t.dtype != F32:
    raise ValueError("triplets_loss (HIP): %s must be float32, got %s" % (what, t.dtype))
  if not t.is_cuda:
    raise ValueError("triplets_loss (HIP): %s is a CPU tensor -- there is no CPU fallback" % what)
  return t


def _ld(t):
  N, k = t.shape
  if (k == 1 or t.stride(1) == 1) and (N == 1 or t.stride(0) >= k):
    return t, (t.stride(0) if N > 1 else k)
  return t.contiguous(), k


def loss_and_grads(outs_orig, outs_pos, outs_neg, grads="all"):
  """One iic_triplets_loss call on detached logits: (loss fp32 [], d_orig, d_pos, d_neg).  ``grads``: "all", "orig"
  (the targets are constants: d_pos and d_neg are None) or "none" (loss only).  Everything is checked before the launch."""
  if grads not in ("all", "orig", "none"):
    raise ValueError("triplets_loss (HIP): grads must be 'all', 'orig' or 'none', got %r" % (grads,))
  a = _rows(outs_orig, "outs_orig")
  N, k = a.shape
  b, c = _rows(outs_pos, "outs_pos", N, k), _rows(outs_neg, "outs_neg", N, k)
  if not (1 <= k <= MAX_K and N * k < 2 ** 31) or not supported(N, k):
    raise ValueError("triplets_loss (HIP): [N, k] = [%d, %d] is outside the served range 1 <= k <= %d, N k < 2^31"
                     % (N, k, MAX_K))
  ops.join()      # a forward forked onto a side stream is ordered before this stream from here on (as IID_loss)
  a, b, c = a.detach(), b.detach(), c.detach()
  (a, lda), (b, ldb), (c, ldc) = _ld(a), _ld(b), _ld(c)
  if not (lda == ldb == ldc):      # the kernel takes one row stride
    a, b, c = a.contiguous(), b.contiguous(), c.contiguous()
    lda = k
  dev = a.device
  loss = torch.empty((), dtype=F32, device=dev)
  d_a = torch.empty((N, k), dtype=F32, device=dev) if grads != "none" else None
  d_b = torch.empty((N, k), dtype=F32, device=dev) if grads == "all" else None
  d_c = torch.empty((N, k), dtype=F32, device=dev) if grads == "all" else None
  ws = torch.empty((workspace_bytes(N, k),), dtype=torch.uint8, device=dev)
  check(lib().iic_triplets_loss(ptr(a), ptr(b), ptr(c), lda, N, k, ptr(loss), ptr(d_a), ptr(d_b), ptr(d_c), ptr(ws),
                                stream_ptr()), "iic_triplets_loss")
  return loss, d_a, d_b, d_c


class _TripletsLossFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, a, b, c, detach_targets):
    need = ctx.needs_input_grad
    grads = "none" if not any(need[:3]) else ("orig" if detach_targets or not (need[1] or need[2]) else "all")
    loss, d_a, d_b, d_c = loss_and_grads(a, b, c, grads)
    ctx.save_for_backward(*[g for g in (d_a, d_b, d_c) if g is not None])
    ctx.have = grads
    return loss

  @staticmethod
  def backward(ctx, g):
    saved = ctx.saved_tensors
    need = ctx.needs_input_grad
    # the upstream scalar is multiplied in on the device: no .item(), no host sync
    d_a = saved[0] * g if ctx.have != "none" and need[0] else None
    d_b = saved[1] * g if ctx.have == "all" and need[1] else None
    d_c = saved[2] * g if ctx.have == "all" and need[2] else None
    return d_a, d_b, d_c, None


def triplets_loss(outs_orig, outs_pos, outs_neg, detach_targets=False):
  """The reference's triplets_loss (baselines/triplets.py:231-238) on [N, k] fp32 device logits:
  kl_div(log_softmax(orig), softmax(pos)) - kl_div(log_softmax(orig), softmax(neg)), both "elementwise_mean" (the sum
  over N k).  Same value; gradients for all three inputs (``detach_targets=True``: for ``outs_orig`` only, pos and neg
  are constants).  A CPU tensor raises: there is no CPU fallback."""
  return _TripletsLossFn.apply(outs_orig, outs_pos, outs_neg, bool(detach_targets))


# ------------------------------------------------------------------------------------
# evaluation  (baselines/triplets.py:97-228)
# ------------------------------------------------------------------------------------
def _logits(config, net, batch, sobel):
  from .transforms import sobel_process
  imgs = batch[0].cuda()
  if sobel:
    imgs = sobel_process(imgs, config.include_rgb)
  with torch.no_grad():
    x_outs = net(imgs)
  assert (x_outs.shape[1] == config.output_k)
  assert (len(x_outs.shape) == 2)
  return x_outs


def triplets_get_data(config, net, dataloader, sobel):
  """Twin of the reference's triplets_get_data (:97-131): flat int32 predictions (arg-max of the logits, the lowest
  index on a tie) and flat int32 targets, both on the device.  One iic_cluster_argmax_acc launch per batch (H = 1)
  writes the batch's predictions into the flat array; nothing is copied to the host."""
  num_batches = len(dataloader)
  total = num_batches * config.batch_sz
  dev = torch.device("cuda", torch.cuda.current_device())
  flat_targets_all = torch.zeros(total, dtype=torch.int32, device=dev)
  flat_preds_all = torch.zeros(total, dtype=torch.int32, device=dev)
  num_test = 0
  for b_i, batch in enumerate(dataloader):
    x_outs = _logits(config, net, batch, sobel)
    flat_targets = batch[1]
    num_test_curr = flat_targets.shape[0]
    num_test += num_test_curr
    start_i = b_i * config.batch_sz
    assert (num_test_curr <= config.batch_sz and x_outs.shape[0] == num_test_curr)
    _argmax_acc(x_outs.float().unsqueeze(1), None, 0, None, flat_preds_all, start_i, total, expect=(1, config.output_k))
    flat_targets_all[start_i:(start_i + num_test_curr)] = flat_targets.to(dev)
  return flat_preds_all[:num_test], flat_targets_all[:num_test]


def triplets_get_data_kmeans_on_features(config, net, dataloader, sobel, kmeans=None):
  """Twin of the reference's triplets_get_data_kmeans_on_features (:134-173).  As in the reference, the net is called
  as ``net(imgs)``: the "features" k-means runs on are the ``output_k`` LOGITS, not the trunk features
  (iic_amd.kmeans.get_data_kmeans_on_features passes kmeans_use_features=True instead and clusters the trunk features;
  it stays as it is -- this function follows the reference).  ``KMeans(n_clusters=config.gt_k)`` of iic_amd.kmeans, or
  the configured ``kmeans``; the logits never leave the device."""
  num_batches = len(dataloader)
  total = num_batches * config.batch_sz
  dev = torch.device("cuda", torch.cuda.current_device())
  flat_targets_all = torch.zeros(total, dtype=torch.int32, device=dev)
  features_all = torch.zeros((total, config.output_k), dtype=F32, device=dev)
  num_test = 0
  for b_i, batch in enumerate(dataloader):
    x_outs = _logits(config, net, batch, sobel)
    flat_targets = batch[1]
    num_test_curr = flat_targets.shape[0]
    num_test += num_test_curr
    start_i = b_i * config.batch_sz
    assert (num_test_curr <= config.batch_sz and x_outs.shape[0] == num_test_curr)
    features_all[start_i:(start_i + num_test_curr), :] = x_outs.float()
    flat_targets_all[start_i:(start_i + num_test_curr)] = flat_targets.to(dev)
  features_all = features_all[:num_test, :]
  flat_targets_all = flat_targets_all[:num_test]
  km = kmeans if kmeans is not None else KMeans(n_clusters=config.gt_k)
  flat_preds_all = km.fit(features_all).labels_
  assert (flat_targets_all.shape == flat_preds_all.shape)      # (labels are in [0, gt_k) by construction)
  return flat_preds_all, flat_targets_all


def triplets_eval(config, net, dataloader_test, sobel):
  """Twin of the reference's triplets_eval (:176-228), both branches (config.kmeans_on_features), same bookkeeping on
  ``config`` (epoch_acc, masses, per_class_acc) and the same ``is_best`` return value.  The Hungarian match, the "each
  class mapped" check, mass, per_class_acc and acc are all functions of one iic_contingency matrix: the reference's
  reorder loop (2 launches per class) and its 2 masked sums per class do not run."""
  net.eval()
  if not config.kmeans_on_features:
    flat_preds_all, flat_targets_all = triplets_get_data(config, net, dataloader_test, sobel)
    assert (config.output_k == config.gt_k)
  else:
    flat_preds_all, flat_targets_all = triplets_get_data_kmeans_on_features(config, net, dataloader_test, sobel)
  num_samples = flat_preds_all.shape[0]
  assert (num_samples == flat_targets_all.shape[0])
  net.train()
  gt_k = config.gt_k
  counts = eval_metrics._counts(flat_preds_all, flat_targets_all, gt_k, gt_k)      # [pred][target], one transfer
  acc, mass, per_class_acc = _stats_from_counts(counts, num_samples, gt_k)
  is_best = (len(config.epoch_acc) > 0) and (acc > max(config.epoch_acc))
  config.epoch_acc.append(acc)
  if config.masses is None:
    assert (config.per_class_acc is None)
    config.masses = mass
    config.per_class_acc = per_class_acc
  else:
    config.masses = np.concatenate((config.masses, mass), axis=0)
    config.per_class_acc = np.concatenate((config.per_class_acc, per_class_acc), axis=0)
  return is_best


def _stats_from_counts(counts, num_samples, gt_k):
  """(acc, mass [1, gt_k], per_class_acc [1, gt_k]) of triplets_eval (:192-214) from counts[pred][target]: the match
  of eval_metrics._hungarian_match, class c's mass = the samples whose prediction maps to c, its per_class_acc = those
  of them whose target is c, acc = their sum over the samples."""
  from scipy.optimize import linear_sum_assignment
  rows, cols = linear_sum_assignment(num_samples - counts)
  match = [(int(out_c), int(gt_c)) for out_c, gt_c in zip(rows, cols)]
  assert (len(set(p for p, _ in match)) == gt_k)      # each class must get mapped
  mass = np.zeros((1, gt_k))
  per_class_acc = np.zeros((1, gt_k))
  for pred_i, target_i in match:
    mass[0, target_i] = counts[pred_i].sum()
    per_class_acc[0, target_i] = counts[pred_i, target_i]
  return int(per_class_acc.sum()) / float(num_samples), mass, per_class_acc


# ------------------------------------------------------------------------------------
# training batches  (make_triplets_data, baselines/triplets.py:71-85)
# ------------------------------------------------------------------------------------
def triplet_batches(augmenter, batch_sz, seed):
  """One epoch of (orig, pos, neg) image batches from a PairedAugmenter or GreyscaleAugmenter -- what zipping
  make_triplets_data's three loaders yields: ``orig`` is tf1 (``plain``) and ``pos`` tf2 (``jittered``) of the same
  samples in dataset order (_create_dataloaders, shuffle=False), ``neg`` is tf1 of a shuffled order (the loader built
  with shuffle=True; ``seed`` draws the permutation).  The last batch is ragged (drop_last=False)."""
  n, batch_sz = int(augmenter.B), int(batch_sz)
  assert batch_sz >= 1
  perm = np.random.RandomState(seed).permutation(n)
  for lo in range(0, n, batch_sz):
    idx = np.arange(lo, min(n, lo + batch_sz))
    yield augmenter.plain(idx), augmenter.jittered(idx), augmenter.plain(perm[lo:lo + batch_sz])
