"""Semi-supervised fine-tuning on the device: the SupHead5 training step and the ten-crop evaluation.

Host side of csrc/sup_head.hip, but for the Linear layers: those are iic_amd.linear's.  What the reference's
IID_semisup_STL10 script (examples/commands.txt §1.3, model 698) runs after the trunk:

  SupHead5            code/archs/semisup/sup_head5.py: Linear(dlen, 2048) -> BatchNorm1d -> ReLU ->
                      Linear(2048, gt_k) on trunk(x, trunk_features=True, penultimate_features=...)
  cross_entropy       the script's nn.CrossEntropyLoss on the head's logits
  TenCropEvaluator    code/utils/semisup/general.py:46-93 (assess_acc_block) over code/utils/semisup/dataset.py's
                      TenCropAndFinish: TenCrop(input_sz) + custom_greyscale_to_tensor per crop, the ten logit rows of an
                      image summed in float64, arg-max, compared with the label

With penultimate_features=True the first Linear reads layer 3's bf16 PT tensor in place on the bf16 MFMA pipe
(linear.PTLinearFn): no fp32 NCHW copy of the activation, its bf16 operand refreshed once per optimiser step (the rule
ops.PreppedWeights applies to the conv weights).  Under ops.fp32_mode() the whole head runs exact fp32 (pt_to_nchw + iic_gemm_f32): the parity tier.

  train_loader        the script's shuffled training DataLoader over a resident PairedAugmenter: tf2 of
                      sobel_make_transforms with the script's --random_affine / --cutout flags (model 698:
                      PairedAugmenter(..., random_affine=True, affine_p=0.5, cutout=True, cutout_p=0.5,
                      cutout_max_box=0.7)), one launch per batch (csrc/augment_affine.hip)

Out of scope here: install.PATCHES and the strict installer, graph capture of this step, data parallelism /
grad_groups for SupHead5.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import check, lib, ptr, stream_ptr
from .augment import FPARAMS, IPARAMS, PairedAugmenter
from .linear import LinearF32Fn, PTLinearFn, PTLinearOperands
from .transforms import sobel_process

F32 = torch.float32

__all__ = ["SupHead5", "cross_entropy", "CrossEntropyLoss", "ten_crop_params", "TenCropAccumulator",
           "TenCropEvaluator", "permute_columns", "unpermute_columns", "train_loader"]


# ------------------------------------------------------------------------------------
# the first Linear's operand: (c, h, w) columns <-> the PT interior order (h, w, c)
# ------------------------------------------------------------------------------------
def permute_columns(C, H, W):
  """index [K]: column j of the kernels' operand (PT interior order, j = (h W + w) C + c) is column index[j] of the
  parameter ((c, h, w) flatten order of net5g.py:56, c H W + h W + w)."""
  j = np.arange(C * H * W, dtype=np.int64)
  c, p = j % C, j // C
  return c * (H * W) + p


def unpermute_columns(C, H, W):
  """The inverse: parameter column i is operand column index[i]."""
  i = np.arange(C * H * W, dtype=np.int64)
  c, p = i // (H * W), i % (H * W)
  return p * C + c


def bn_relu_forward(x, gamma, beta, running_mean, running_var, training, momentum, eps):
  """(y, save_mean, save_invstd) of BatchNorm1d + ReLU over fp32 [N, F] (iic_sup_bn_relu_fwd)."""
  N, F = x.shape
  if training and N < 2:
    raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
  y = torch.empty_like(x)
  mean = torch.empty(F, dtype=F32, device=x.device)
  inv = torch.empty(F, dtype=F32, device=x.device)
  check(lib().iic_sup_bn_relu_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), ptr(y), ptr(mean),
                                  ptr(inv), N, F, 1 if training else 0, float(momentum), float(eps), stream_ptr()),
        "iic_sup_bn_relu_fwd")
  return y, mean, inv


def bn_relu_backward(dout, x, y, gamma, mean, inv, training):
  """(dx, dgamma, dbeta) (iic_sup_bn_relu_bwd)."""
  N, F = x.shape
  dx = torch.empty_like(x)
  dg = torch.empty(F, dtype=F32, device=x.device)
  db = torch.empty(F, dtype=F32, device=x.device)
  check(lib().iic_sup_bn_relu_bwd(ptr(dout), ptr(x), ptr(y), ptr(gamma), ptr(mean), ptr(inv), ptr(dx), ptr(dg), ptr(db),
                                  N, F, 1 if training else 0, stream_ptr()), "iic_sup_bn_relu_bwd")
  return dx, dg, db


class _BNReLUFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, x, gamma, beta, bn):
    x = x.contiguous()
    training = bn.training or not bn.track_running_stats
    if bn.momentum is None:
      raise NotImplementedError("BatchNorm1d(momentum=None): the cumulative average is not built (sup_head5.py uses 0.1)")
    rm, rv = (bn.running_mean, bn.running_var) if bn.track_running_stats else (None, None)
    y, mean, inv = bn_relu_forward(x, gamma.detach(), beta.detach(), rm, rv, training, bn.momentum, bn.eps)
    if training and bn.track_running_stats:
      bn.num_batches_tracked += 1
    ctx.save_for_backward(x, y, gamma, mean, inv)
    ctx.training = training
    ctx.branch, ctx.pt_dtype = ops.current_branch(), ops.PT_DTYPE[0]
    return y

  @ops.branch_backward
  def backward(ctx, dout):
    x, y, gamma, mean, inv = ctx.saved_tensors
    dx, dg, db = bn_relu_backward(dout.contiguous(), x, y, gamma.detach(), mean, inv, ctx.training)
    return dx, dg, db, None


# ------------------------------------------------------------------------------------
# cross-entropy
# ------------------------------------------------------------------------------------
def cross_entropy_raw(logits, targets):
  """(loss [1], dlogits [N, k]) from one launch (iic_sup_cross_entropy); targets int64 on the device, range unchecked."""
  N, k = logits.shape
  loss = torch.empty(1, dtype=F32, device=logits.device)
  dl = torch.empty_like(logits)
  check(lib().iic_sup_cross_entropy(ptr(logits), ptr(targets), ptr(loss), ptr(dl), N, k, stream_ptr()),
        "iic_sup_cross_entropy")
  return loss, dl


class _CrossEntropyFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, logits, targets):
    loss, dl = cross_entropy_raw(logits, targets)
    ctx.save_for_backward(dl)
    return loss.view(())

  @staticmethod
  def backward(ctx, g):
    dl, = ctx.saved_tensors
    return dl * g, None


def cross_entropy(logits, targets):
  """nn.CrossEntropyLoss() (mean reduction) of fp32 logits [N, k] on the device and integer targets [N] (host or
  device).  A target outside [0, k) raises here, on the host, before anything is launched."""
  assert logits.is_cuda and logits.dim() == 2 and logits.dtype is F32, "fp32 [N, k] logits on the GPU (no CPU path)"
  N, k = logits.shape
  targets = torch.as_tensor(targets)
  if targets.dim() != 1 or targets.shape[0] != N:
    raise ValueError("targets: expected shape (%d,), got %s" % (N, tuple(targets.shape)))
  if targets.dtype.is_floating_point or targets.dtype is torch.bool:
    raise ValueError("targets must be integer class indices")
  lo, hi = (int(v) for v in torch.aminmax(targets))
  if lo < 0 or hi >= k:
    raise IndexError("Target %d is out of bounds for %d classes" % (lo if lo < 0 else hi, k))
  targets = targets.to(device=logits.device, dtype=torch.int64).contiguous()
  return _CrossEntropyFn.apply(logits.contiguous(), targets)


class CrossEntropyLoss(nn.Module):
  """Module twin of cross_entropy (the script's `criterion = nn.CrossEntropyLoss().cuda()`)."""

  def forward(self, logits, targets):
    return cross_entropy(logits, targets)


# ------------------------------------------------------------------------------------
# SupHead5
# ------------------------------------------------------------------------------------
class SupHead5(nn.Module):
  """sup_head5.py with its arithmetic on the HIP kernels.  `trunk` is the whole feature network (ClusterNet5g or
  ClusterNet5gTwoHead), `head` a plain nn.Sequential(Linear, BatchNorm1d, ReLU, Linear) that only HOLDS the
  parameters and buffers: state_dict() keys and shapes are the reference's, checkpoints interchange."""

  def __init__(self, net_features, dlen=None, gt_k=None):
    super(SupHead5, self).__init__()
    self.trunk = net_features
    self.head = nn.Sequential(nn.Linear(dlen, 2048), nn.BatchNorm1d(2048), nn.ReLU(), nn.Linear(2048, gt_k))
    dev = next(net_features.parameters()).device
    if dev.type == "cuda":
      self.head.to(dev)                       # (sup_head5.py:21: net_head.cuda())
    for m in self.head.modules():             # sup_head5.py:24-31
      if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
        m.weight.data.fill_(1)
        m.bias.data.zero_()
      elif isinstance(m, nn.Linear):
        m.weight.data.normal_(0, 0.01)
        m.bias.data.zero_()
    self._operands = PTLinearOperands()

  def _features(self, x, penultimate_features):
    tr = self.trunk.trunk
    tr._pt_tap = bool(penultimate_features)
    try:
      return self.trunk(x, trunk_features=True, penultimate_features=penultimate_features)
    finally:
      tr._pt_tap = False

  def forward(self, x, penultimate_features=False):
    pv = ops.pv
    lin1, bn, _, lin2 = self.head
    f = self._features(x, penultimate_features)
    if f.dim() == 4:       # layer 3's bf16 PT tensor (under torch.no_grad() the trunk has already handed it back to the
      #                      pool: nothing re-uses it before the next trunk forward, enqueued behind this launch)
      if f.shape[3] * (f.shape[1] - 2) * (f.shape[2] - 2) != lin1.in_features:
        raise ValueError("SupHead5: dlen = %d, the trunk gives %d features" % (
          lin1.in_features, f.shape[3] * (f.shape[1] - 2) * (f.shape[2] - 2)))
      h = PTLinearFn.apply(f, pv(lin1.weight), pv(lin1.bias), self._operands)
    else:                  # fp32 features: the 512 pooled ones, or the exact tier (ops.fp32_mode())
      h = LinearF32Fn.apply(f, pv(lin1.weight), pv(lin1.bias))
    h = _BNReLUFn.apply(h, pv(bn.weight), pv(bn.bias), bn)
    return LinearF32Fn.apply(h, pv(lin2.weight), pv(lin2.bias))     # no softmax (sup_head5.py:36)


# ------------------------------------------------------------------------------------
# training batches
# ------------------------------------------------------------------------------------
class _TrainLoader(object):
  """The script's training DataLoader (IID_semisup_STL10.py: shuffle=True, drop_last=False) over images resident on the
  GPU: iterating yields (augmenter.jittered(idx), targets[idx]) for a fresh permutation of the dataset per epoch, the
  ragged last batch included.  The permutation comes from numpy, not from torch's sampler: the sample order of a
  reference run is not replayed."""

  def __init__(self, augmenter, targets, batch_sz, seed=0):
    self.aug, self.batch_sz = augmenter, int(batch_sz)
    self.targets = torch.as_tensor(targets)
    self.n = int(self.targets.shape[0])
    assert self.batch_sz > 0 and self.n == augmenter.B, "one target per image of the augmenter's dataset"
    self.rng = np.random.RandomState(seed)

  def __len__(self):
    return (self.n + self.batch_sz - 1) // self.batch_sz

  def __iter__(self):
    perm = self.rng.permutation(self.n)
    for lo in range(0, self.n, self.batch_sz):
      idx = perm[lo:lo + self.batch_sz]
      yield self.aug.jittered(idx), self.targets[torch.as_tensor(idx, device=self.targets.device)]


def train_loader(augmenter, targets, batch_sz, seed=0):
  """`for imgs, targets in train_loader(aug, labels, batch_sz)` is the script's training loop head: imgs float32
  [b, C, input_sz, input_sz] on the GPU (tf2 of the augmenter, affine and cutout included when it was built with
  them), targets the matching rows of `targets` (kept on whichever device they are)."""
  return _TrainLoader(augmenter, targets, batch_sz, seed)


# ------------------------------------------------------------------------------------
# ten-crop evaluation
# ------------------------------------------------------------------------------------
def ten_crop_params(idx, W, H, S):
  """(iparams int32 [10 n, 20], fparams float32 [10 n, 4]) for PairedAugmenter(images, S, S, ...).apply: the ten crops
  of torchvision 0.2.1 TenCrop(S) per image of idx, image-major -- tl, tr, bl, br, centre (F.center_crop:
  int(round((H - S) / 2.))) of the image, then the same five of the mirrored image, i.e. the crop at x -> W - S - x of
  the image itself with the flip bit set.  Crop size = input size: the resize is the identity."""
  idx = np.asarray(idx, dtype=np.int64).reshape(-1)
  assert S <= W and S <= H
  cx, cy = int(round((W - S) / 2.)), int(round((H - S) / 2.))
  five = [(0, 0), (W - S, 0), (0, H - S), (W - S, H - S), (cx, cy)]
  rows = [(x, y, 0) for x, y in five] + [(W - S - x, y, 1) for x, y in five]
  ip = np.zeros((idx.shape[0], 10, IPARAMS), np.int32)
  ip[:, :, 0] = idx[:, None]
  ip[:, :, 1:4] = np.asarray(rows, np.int32)[None]
  return ip.reshape(-1, IPARAMS), np.zeros((idx.shape[0] * 10, FPARAMS), np.float32)


class TenCropAccumulator(object):
  """Streaming assess_acc_block: update(logits [B * crops, k], targets [B]) adds to a device-resident int64 pair
  (correct, total); result() is the one host synchronisation."""

  def __init__(self, device, crops=10):
    self.counts = torch.zeros(2, dtype=torch.int64, device=device)
    self.crops = int(crops)

  def update(self, logits, targets):
    assert logits.is_cuda and logits.dtype is F32 and logits.dim() == 2
    rows, k = logits.shape
    B, left = divmod(rows, self.crops)
    assert left == 0 and B > 0, "general.py:71-72: whole images only"
    targets = torch.as_tensor(targets).to(device=logits.device, dtype=torch.int64).contiguous()
    assert targets.shape == (B,)
    check(lib().iic_sup_tencrop_acc(ptr(logits.contiguous()), ptr(targets), ptr(self.counts), B, k, self.crops,
                                    stream_ptr()), "iic_sup_tencrop_acc")

  def result(self):
    """(correct, total) as Python ints."""
    c, t = self.counts.tolist()
    return int(c), int(t)

  def accuracy(self):
    c, t = self.result()
    return c / float(t)


class TenCropEvaluator(object):
  """The test loader of the semisup script resident on the GPU: uint8 images [B, H, W, 3], their labels, and the ten
  crops of size input_sz cut by the augmentation kernel (bit-identical to TenCropAndFinish's PIL crops)."""

  def __init__(self, images_u8, targets, input_sz, include_rgb):
    self.aug = PairedAugmenter(images_u8, input_sz, input_sz, include_rgb)
    self.targets = torch.as_tensor(targets).to(device=images_u8.device, dtype=torch.int64).contiguous()
    assert self.targets.shape == (self.aug.B,)
    self.include_rgb = bool(include_rgb)

  def crops(self, idx):
    """float32 [10 len(idx), C, S, S]: what TenCropAndFinish stacks for these images."""
    return self.aug.apply(*ten_crop_params(idx, self.aug.W, self.aug.H, self.aug.S))

  def accuracy(self, net, images_per_batch=70, penultimate_features=False):
    """assess_acc_block(net, loader, ...)'s value.  Per batch: crops, Sobel, the network, the count -- one launch
    chain, nothing copied to the host; one synchronisation at the end."""
    acc = TenCropAccumulator(self.targets.device)
    with torch.no_grad():
      for s in range(0, self.aug.B, images_per_batch):
        idx = np.arange(s, min(self.aug.B, s + images_per_batch))
        x = sobel_process(self.crops(idx), self.include_rgb)
        acc.update(net(x, penultimate_features=penultimate_features), self.targets[idx[0]:idx[-1] + 1])
    return acc.accuracy()
