"""MI355X-native SegmentationNet10aIsola / SegmentationNet10aDoersch -- opt-in twins of
code/archs/segmentation/baselines/{net10a_isola,net10a_doersch}.py: the 10a trunk, two p x p patches of its up-sampled
features, a siamese conv stage per patch and a joint Linear over both.

The reference up-samples all 512 trunk channels to input_sz (fp32 [N, 512, S, S], 6.1 GB per Potsdam batch, and as much
again in backward) and slices the two patches out of the result.  Here only the 2 p p pixels per image that the patches
hold are interpolated, straight into the siamese conv's operand layout (iic_seg_patch_sample_fwd, csrc/seg_patches.hip);
their adjoint goes back into the trunk's gradient as a fixed-order gather.  The joint Linear(2 * 1024 * p * p -> 1024)
reads both stage outputs in place on the bf16 MFMA pipe (linear.PTLinearFn over iic_pair_*, csrc/sup_head.hip).

  forward     trunk -> sampler -> siamese stage (conv 3x3 512 -> 1024 + BatchNorm + ReLU; the centre images, then the
              other images: two calls, each with its own batch statistics, the running statistics updated in that order,
              as the reference's two self.siamese_branch(...) calls do) -> joint Linear -> ReLU -> Dropout(0.5) ->
              Linear(1024 -> 1 / 9) [-> sigmoid for Isola]
  state_dict  the reference's keys: features.*, {isola,doersch}_head.siamese_branch.{0,1}.*, {..}_head.joint.{0,3}.*

Under ops.fp32_mode() the same modules run on the exact-fp32 kernels (the fp32 sampler flavour, _StageFn's fp32 branch,
_FlattenFn per half + linear.LinearF32Fn): the parity tier.  ReLU, dropout, the sigmoid and the second Linear act on [N, 1024]
and are not the hot path (torch ops and iic_gemm_f32).

Both classes subclass SegmentationNet10aFeatures: trunk_pt, load_trunk_state_dict and the k-means evaluation twins of
iic_amd.seg_kmeans accept them unchanged.  install() rebinds nothing to this module -- INTEGRATION.md section 5j.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .._lib import check, lib, ptr, stream_ptr
from ..linear import LinearF32Fn, PTLinearFn, PTLinearOperands
from .seg import SegmentationNet10a, SegmentationNet10aFeatures, SegmentationNet10aTrunk
from .vgg import _FlattenFn, _Stage, _StageFn, _initialize_weights_vgg

__all__ = ["SegmentationNet10aIsola", "SegmentationNet10aDoersch", "coords_block", "check_patches", "patch_sample",
           "patch_sample_bwd"]
F32, BF16 = torch.float32, torch.bfloat16

HEAD_C = 1024         # channels of the siamese stage (net10a_isola.py:19, net10a_doersch.py:19)
MAX_PATCH = 127       # patch side the sampler serves
COORD_INTS = 8        # the device coordinate block: {cy, cx, oy, ox, label, 0, 0, 0}


# ------------------------------------------------------------------------------------
# coordinates
# ------------------------------------------------------------------------------------
def check_patches(centre, other, S, p):
  """(cy, cx, oy, ox) as Python ints, or ValueError: an even (or unserved) patch side, a point that is not two
  integers, a patch that does not lie inside the S x S map (general.py:4-18 would slice outside it)."""
  p = int(p)
  if p < 1 or p % 2 == 0:
    raise ValueError("patch side must be odd, got %d" % p)
  if p > min(S, MAX_PATCH):
    raise ValueError("patch side %d is outside the served range p <= min(input_sz = %d, %d)" % (p, S, MAX_PATCH))
  d = p // 2
  out = []
  for name, pt in (("centre", centre), ("other", other)):
    if pt is None:
      raise ValueError("%s is required unless penultimate=True" % name)
    a = np.asarray(pt)
    if a.shape != (2,) or a.dtype.kind not in "iu":
      raise ValueError("%s must be two integers (row, column), got %r" % (name, pt))
    for v in a:
      if not d <= int(v) <= S - 1 - d:
        raise ValueError("%s = %s: a %d x %d patch around it leaves the %d x %d map (each coordinate must lie in "
                         "[%d, %d])" % (name, a.tolist(), p, p, S, S, d, S - 1 - d))
      out.append(int(v))
  return tuple(out)


def coords_block(centre, other, label, device):
  """int32 [8] on the device: {cy, cx, oy, ox, label, 0, 0, 0} (include/iic_hip.h)."""
  c, o = np.asarray(centre).reshape(2), np.asarray(other).reshape(2)
  host = torch.tensor([int(c[0]), int(c[1]), int(o[0]), int(o[1]), int(label), 0, 0, 0], dtype=torch.int32)
  return host.to(device)


# ------------------------------------------------------------------------------------
# patch sampler
# ------------------------------------------------------------------------------------
def _pt_geometry(pt):
  if not (torch.is_tensor(pt) and pt.is_cuda and pt.dim() == 4 and pt.is_contiguous() and pt.dtype in (BF16, F32)):
    raise ValueError("patch sampler (HIP): the PT feature tensor must be a contiguous bf16 or fp32 [N, Hp, Wp, C] device "
                     "tensor -- there is no CPU fallback")
  return pt.shape


def patch_sample(pt, coords, S, p, P=SegmentationNet10aTrunk.P, out=None):
  """PT tensor [2 N, p + 2, p + 2, C] of pt's dtype (iic_seg_patch_sample_fwd): images 0 .. N - 1 the centre patch,
  N .. 2 N - 1 the other patch of the features up-sampled to S x S.  coords: the device block of coords_block."""
  N, Hp, Wp, C = _pt_geometry(pt)
  if out is None:
    out = torch.empty((2 * N, p + 2, p + 2, C), dtype=pt.dtype, device=pt.device)
  check(lib().iic_seg_patch_sample_fwd(ptr(pt), 1 if pt.dtype == F32 else 0, ptr(coords), ptr(out), N, Hp - 2 * P,
                                       Wp - 2 * P, Hp, Wp, P, C, S, p, stream_ptr()), "iic_seg_patch_sample_fwd")
  return out


def patch_sample_bwd(dcentre, dother, coords, dx_pt, S, p, P=SegmentationNet10aTrunk.P):
  """The adjoint (iic_seg_patch_sample_bwd): the interior of dx_pt [N, Hp, Wp, C] from the two halves of dpatches."""
  N, Hp, Wp, C = _pt_geometry(dx_pt)
  for t in (dcentre, dother):
    if not (t.is_cuda and t.is_contiguous() and t.dtype == dx_pt.dtype and tuple(t.shape) == (N, p + 2, p + 2, C)):
      raise ValueError("patch sampler (HIP): a gradient half must be a contiguous %s [%d, %d, %d, %d] device tensor"
                       % (dx_pt.dtype, N, p + 2, p + 2, C))
  check(lib().iic_seg_patch_sample_bwd(ptr(dcentre), ptr(dother), 1 if dx_pt.dtype == F32 else 0, ptr(coords), ptr(dx_pt),
                                       N, Hp - 2 * P, Wp - 2 * P, Hp, Wp, P, C, S, p, stream_ptr()),
        "iic_seg_patch_sample_bwd")
  return dx_pt


class _PatchSampleFn(torch.autograd.Function):
  """PT trunk features [N, Hf + 2P, Wf + 2P, C] -> (centre patches, other patches), each a PT tensor
  [N, p + 2, p + 2, C] with border 1: the two halves of one pool buffer."""

  @staticmethod
  def forward(ctx, pt, coords, S, p):
    N, Hp, Wp, C = pt.shape
    out = patch_sample(pt, coords, S, p, out=ops.pt_alloc(2 * N, p, p, C, 1, pt.device))
    ctx.save_for_backward(coords)
    ctx.meta = (tuple(pt.shape), S, p)
    ctx.out = out
    ctx.branch, ctx.pt_dtype = ops.current_branch(), pt.dtype
    return out[:N], out[N:]

  @ops.branch_backward
  def backward(ctx, d0, d1):
    coords, = ctx.saved_tensors
    shape, S, p = ctx.meta
    N, Hp, Wp, C = shape
    P = SegmentationNet10aTrunk.P
    half = (N, p + 2, p + 2, C)
    dt = ops.PT_DTYPE[0]
    g0 = d0.contiguous() if d0 is not None else torch.zeros(half, dtype=dt, device=coords.device)
    g1 = d1.contiguous() if d1 is not None else torch.zeros(half, dtype=dt, device=coords.device)
    # handed to the trunk's last stage as _SegHeadFn.backward hands its gradient over: unmasked, from the pool
    dx = patch_sample_bwd(g0, g1, coords, ops.POOL.alloc(shape, coords.device, P), S, p, P)
    for t in (d0, d1, ctx.out):
      ops.POOL.release(t)
    ctx.out = None
    return dx, None, None, None


# ------------------------------------------------------------------------------------
# the nets
# ------------------------------------------------------------------------------------
class _BaselineHead(nn.Module):
  """IsolaHead / DoerschHead (net10a_isola.py:13-38, net10a_doersch.py:13-30): parameter holders with the reference's
  names; the computation is _BaselineNet._head."""

  def __init__(self, patch_side, num_out):
    super(_BaselineHead, self).__init__()
    self.patch_side = patch_side
    self.siamese_branch = nn.Sequential(
      nn.Conv2d(in_channels=SegmentationNet10a.cfg[-1][0], out_channels=HEAD_C, kernel_size=3, stride=1, padding=1,
                bias=False),
      nn.BatchNorm2d(HEAD_C),
      nn.ReLU(inplace=True))
    self.joint = nn.Sequential(
      nn.Linear(2 * HEAD_C * patch_side * patch_side, HEAD_C),
      nn.ReLU(True),
      nn.Dropout(),
      nn.Linear(HEAD_C, num_out))


class _BaselineNet(SegmentationNet10aFeatures):
  HEAD_ATTR, PATCH_ATTR, NUM_OUT = None, None, None

  def __init__(self, config):
    super(_BaselineNet, self).__init__(config)
    self.patch_side = int(getattr(config, self.PATCH_ATTR))
    if self.patch_side < 1 or self.patch_side % 2 == 0:
      raise ValueError("%s must be odd, got %d" % (self.PATCH_ATTR, self.patch_side))
    head = _BaselineHead(self.patch_side, self.NUM_OUT)
    setattr(self, self.HEAD_ATTR, head)
    _initialize_weights_vgg(self)                                   # (VGGNet._initialize_weights, vgg.py:42-54)
    self._stage = _Stage(head.siamese_branch[0], head.siamese_branch[1], pool=False, first=False, P=1)
    self._operands = PTLinearOperands()
    # test hook: a [N, 1024] keep-mask (0 / 1) used instead of the one torch draws on the device in train() mode
    self.dropout_keep = None

  @property
  def head(self):
    return getattr(self, self.HEAD_ATTR)

  def _siamese(self, x):
    st = self._stage
    return _StageFn.apply(x, ops.pv(st.conv.weight), ops.pv(st.bn.weight), ops.pv(st.bn.bias), st, None, None)

  def _dropout(self, h):
    drop = self.head.joint[2]
    if not (self.training and drop.p > 0):
      return h
    keep = self.dropout_keep
    if keep is None:
      keep = torch.rand_like(h) >= drop.p
    return h * (keep.to(h.dtype) * (1.0 / (1.0 - drop.p)))

  @ops.auto_branch
  def _head(self, x, cy, cx, oy, ox):
    return self.head_from_features(self.features(x), cy, cx, oy, ox)

  def head_from_features(self, pt, cy, cx, oy, ox):
    """The head path on the trunk's PT feature tensor: sampler -> siamese stage twice -> joint Linear -> ReLU ->
    dropout -> second Linear (pre-sigmoid).  forward() validates the coordinates before it gets here."""
    lin1, lin2 = self.head.joint[0], self.head.joint[3]
    coords = coords_block((cy, cx), (oy, ox), 0, pt.device)
    p0, p1 = _PatchSampleFn.apply(pt, coords, self.input_sz, self.patch_side)
    a0 = self._siamese(p0)       # two calls: own batch statistics each, running statistics updated in this order
    a1 = self._siamese(p1)
    if a0.dtype == F32:          # ops.fp32_mode(): (c, h, w) flatten per half, torch.cat, exact fp32 GEMM
      h = LinearF32Fn.apply(torch.cat([_FlattenFn.apply(a0, 1), _FlattenFn.apply(a1, 1)], dim=1), ops.pv(lin1.weight),
                            ops.pv(lin1.bias))
    else:
      h = PTLinearFn.apply(a0, a1, ops.pv(lin1.weight), ops.pv(lin1.bias), self._operands)
    h = self._dropout(torch.relu(h))
    return LinearF32Fn.apply(h, ops.pv(lin2.weight), ops.pv(lin2.bias))

  def forward(self, x, centre=None, other=None, penultimate=False):
    if penultimate:
      return super(_BaselineNet, self).forward(x, penultimate=True)
    if not (torch.is_tensor(x) and x.is_cuda):
      raise ValueError("%s (HIP): the input must be a device tensor -- there is no CPU fallback" % type(self).__name__)
    cy, cx, oy, ox = check_patches(centre, other, self.input_sz, self.patch_side)
    return self._finish(self._head(x, cy, cx, oy, ox))

  def _finish(self, out):
    return out


class SegmentationNet10aIsola(_BaselineNet):
  """net10a_isola.py:73-101: forward(x, centre, other) is the adjacency probability [N, 1], sigmoid applied."""
  HEAD_ATTR, PATCH_ATTR, NUM_OUT = "isola_head", "isola_patch_side", 1

  def _finish(self, out):
    return torch.sigmoid(out)


class SegmentationNet10aDoersch(_BaselineNet):
  """net10a_doersch.py:66-96: forward(x, centre, other) is the position logits [N, 9], no softmax."""
  HEAD_ATTR, PATCH_ATTR, NUM_OUT = "doersch_head", "doersch_patch_side", 9
