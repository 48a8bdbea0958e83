"""TripletsNet5g / TripletsNet6c -- drop-in for code/archs/cluster/baselines/triplets.py:11-77, the nets of the
reference's triplets baseline (code/scripts/cluster/baselines/triplets_{sobel,greyscale}.py).

The trunks are ClusterNet5gTrunk / ClusterNet6cTrunk as the IIC nets run them (bf16 MFMA path, or the exact-fp32 kernels
inside ops.fp32_mode()).  The head is ONE nn.Linear under the reference's state_dict names ``head.head.weight`` /
``head.head.bias`` and returns LOGITS: the softmax lives in the loss (iic_amd.triplets.triplets_loss).  Same
constructor, same ``forward(x, kmeans_use_features=False)`` returning one tensor, same initialisers (residual.py:75-85,
vgg.py:42-54).

A triplet step calls the net three times before backward (orig, pos, neg).  The pair logic of ops.auto_branch -- the
first forward of a pair forked or marked ``solo_first``, running-statistic updates postponed to the second -- assumes
two, so these nets do not use it: a forward never forks and never postpones, whether IIC_AUTO_BRANCH is on or off.
Under no_grad the activation buffers go back to the pool at the end of the forward, as auto_branch does it.
"""
import torch
import torch.nn as nn

from .. import ops
from ..branches import context, join
from ..linear import LinearF32Fn
from ..pool import POOL
from .cluster import BasicBlock, ClusterNet5gTrunk, _ApplyCounter, _initialize_weights
from .vgg import ClusterNet6c, ClusterNet6cTrunk, _initialize_weights_vgg

__all__ = ["TripletsNet5g", "TripletsNet6c"]


class _TripletsHead(nn.Module):
  def __init__(self, num_features, output_k):
    super(_TripletsHead, self).__init__()
    # no softmax, done in loss
    self.head = nn.Linear(num_features, output_k)

  def forward(self, x, kmeans_use_features=False):
    if kmeans_use_features:
      return x
    return LinearF32Fn.apply(x, ops.pv(self.head.weight), ops.pv(self.head.bias))


class TripletsNet5gHead(_TripletsHead):
  def __init__(self, config):
    super(TripletsNet5gHead, self).__init__(512 * BasicBlock.expansion, config.output_k)


class TripletsNet6cHead(_TripletsHead):
  def __init__(self, config):
    if config.input_sz == 24:
      sp = 3
    elif config.input_sz == 64:
      sp = 8
    else:
      raise ValueError("TripletsNet6c supports input_sz 24 or 64 (baselines/triplets.py:48-51)")
    super(TripletsNet6cHead, self).__init__(ClusterNet6c.cfg[-1][0] * sp * sp, config.output_k)


class _TripletsNet(_ApplyCounter, nn.Module):
  def forward(self, x, kmeans_use_features=False):
    c = context()
    if c.branch == 0 and (c.pending_join or c.deferred_running or c.solo_first):
      join()      # whatever a pair of another net left open ends here: nothing below is postponed
    if not torch.is_grad_enabled():
      mark = POOL.mark()            # evaluation: nothing will release the activations later
      try:
        return self.head(self.trunk(x), kmeans_use_features=kmeans_use_features)
      finally:
        POOL.sweep(mark)
    return self.head(self.trunk(x), kmeans_use_features=kmeans_use_features)


class TripletsNet5g(_TripletsNet):
  def __init__(self, config):
    super(TripletsNet5g, self).__init__()
    self.batchnorm_track = config.batchnorm_track
    self.trunk = ClusterNet5gTrunk(config)
    self.head = TripletsNet5gHead(config)
    _initialize_weights(self)


class TripletsNet6c(_TripletsNet):
  def __init__(self, config):
    super(TripletsNet6c, self).__init__()
    self.batchnorm_track = config.batchnorm_track
    self.trunk = ClusterNet6cTrunk(config)
    self.head = TripletsNet6cHead(config)
    _initialize_weights_vgg(self)
