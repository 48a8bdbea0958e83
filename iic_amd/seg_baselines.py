"""The Isola and Doersch segmentation baselines on the device -- opt-in twins of
code/utils/segmentation/baselines/{isola_utils,doersch_utils}.py and of the loop body of
code/scripts/segmentation/baselines/{isola,doersch}.py.

``isola_set_patches`` / ``doersch_set_patches`` are host twins: they consume ``np.random`` draw for draw as the
reference's functions do (isola_utils.py:82-128, doersch_utils.py:7-44), so a seeded run picks the same patches.
``isola_loss`` / ``doersch_loss`` keep the reference's signatures and are one autograd node over one launch each
(iic_isola_loss / iic_doersch_loss, csrc/seg_baseline_loss.hip): the per-row mask, its count, the loss and the gradient
come from the device -- the reference fetches the count with ``.item()`` every step.  ``train_step`` is the scripts'
loop body (isola.py:266-295) and returns the loss as a device scalar.

The nets are iic_amd.archs.SegmentationNet10aIsola / SegmentationNet10aDoersch.  ``install()`` rebinds nothing of this:
a script opts in -- INTEGRATION.md section 5j.  Not built: the single-image (``single_mode``) device augmenter and
``DoerschDataset`` (any device ``(img, mask)`` batch is accepted), installer patches for the two scripts, graph capture
and data parallelism of this step, ``bench.py`` configs, fusing the joint Linear's weight gradient into Adam.
"""
import numpy as np
import torch

from . import ops
from ._lib import check, lib, ptr, stream_ptr
from .archs.seg_baselines import coords_block

__all__ = ["isola_set_patches", "doersch_set_patches", "isola_loss", "doersch_loss", "train_step", "isola_loss_raw",
           "doersch_loss_raw", "NUM_POSITIONS", "MAX_K"]
F32, U8 = torch.float32, torch.uint8
NUM_POSITIONS = 9      # N, NE, ... NW (doersch_utils.py:11)
MAX_K = 32             # logits per row iic_doersch_loss serves


# ------------------------------------------------------------------------------------
# patch selection on the host
# ------------------------------------------------------------------------------------
def _first_patch(rng, S, p, dtype):
  """The first patch's centre: at least a patch side and a half away from the border (one rng.rand(2) draw)."""
  lo = 1.5 * np.array([p, p])
  hi = np.array([S, S]) - lo
  return np.floor(rng.rand(2) * (hi - lo) + lo).astype(dtype)


def _inside(other, S, d):
  return bool((other >= d).all() and (other < S - d).all())


def isola_set_patches(input_sz, patch_side, rng=None):
  """Twin of isola_set_patches (isola_utils.py:82-128): (centre int32 [2], other int32 [2], adjacent bool), the same for
  every image of the batch.  Draws from ``rng`` (default: the global np.random stream) in the reference's order:
  rand() for `adjacent`; then per attempt rand(2) for the centre and either choice([-1, 1]) twice (adjacent: the
  neighbouring block) or rand(), rand() for the polar offset (at least two patch sides away), until the other patch
  lies inside the map."""
  rng = np.random if rng is None else rng
  S, p = input_sz, patch_side
  adjacent = rng.rand() < 0.5
  d = int(np.floor(p / 2.0))
  while True:
    centre = _first_patch(rng, S, p, np.int32)
    if adjacent:
      sh = rng.choice([-1, 1])
      sw = rng.choice([-1, 1])
      other = np.floor(centre + np.array([sh * p, sw * p])).astype(np.int32)
    else:
      r = rng.rand() * (max(S, S) - 2.0 * p) + 2.0 * p
      phi = rng.rand() * 2.0 * np.pi
      other = (centre + np.array([r * np.sin(phi), r * np.cos(phi)])).astype(np.int32)      # pol2cart: (y, x)
    if _inside(other, S, d):
      return centre, other, adjacent


def doersch_set_patches(input_sz, patch_side, rng=None):
  """Twin of doersch_set_patches (doersch_utils.py:7-44): (centre int64 [2], other int32 [2], position_gt in 0..8).
  Per attempt: choice(9) for the position, rand(2) for the centre, rand() for the distance (1.5 to 2 patch sides) along
  the direction position_gt * pi / 4."""
  rng = np.random if rng is None else rng
  S, p = input_sz, patch_side
  d = int(np.floor(p / 2.0))
  while True:
    position_gt = rng.choice(NUM_POSITIONS)
    centre = _first_patch(rng, S, p, "int")
    r_lo, r_hi = 1.5 * p, 2.0 * p
    r = rng.rand() * (r_hi - r_lo) + r_lo
    phi = position_gt * np.pi / 4.
    other = (centre + np.array([r * np.sin(phi), r * np.cos(phi)])).astype(np.int32)
    if _inside(other, S, d):
      return centre, other, position_gt


# ------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------
def _check_common(what, pred, centre, other, mask):
  if not (torch.is_tensor(pred) and pred.is_cuda and pred.dtype == F32):
    raise ValueError("%s (HIP): the prediction must be a float32 device tensor -- there is no CPU fallback" % what)
  if not (torch.is_tensor(mask) and mask.is_cuda and mask.dtype == U8 and mask.dim() == 3 and
          mask.shape[0] == pred.shape[0] and mask.shape[1] == mask.shape[2]):
    raise ValueError("%s (HIP): mask must be a uint8 [%d, S, S] device tensor" % (what, pred.shape[0]))
  S = int(mask.shape[1])
  for name, pt in (("centre", centre), ("other", other)):
    a = np.asarray(pt)
    if a.shape != (2,) or a.dtype.kind not in "iu" or not all(0 <= int(v) < S for v in a):
      raise ValueError("%s (HIP): %s must be two integers inside the %d x %d mask, got %r" % (what, name, S, S, pt))
  return S


def isola_loss_raw(prob, mask, coords, want_grad=True):
  """(loss fp32 [], dprob fp32 [N] or None) from one iic_isola_loss launch; prob fp32 [N] contiguous, mask uint8
  [N, S, S] contiguous, coords the device block (archs.seg_baselines.coords_block)."""
  N, S = prob.shape[0], mask.shape[1]
  loss = torch.empty((), dtype=F32, device=prob.device)
  dp = torch.empty((N,), dtype=F32, device=prob.device) if want_grad else None
  check(lib().iic_isola_loss(ptr(prob), ptr(mask), ptr(coords), ptr(loss), ptr(dp), N, S, stream_ptr()), "iic_isola_loss")
  return loss, dp


def doersch_loss_raw(logits, mask, coords, want_grad=True):
  """(loss fp32 [], dlogits fp32 [N, k] or None) from one iic_doersch_loss launch."""
  N, k = logits.shape
  loss = torch.empty((), dtype=F32, device=logits.device)
  dl = torch.empty((N, k), dtype=F32, device=logits.device) if want_grad else None
  check(lib().iic_doersch_loss(ptr(logits), ptr(mask), ptr(coords), ptr(loss), ptr(dl), N, k, mask.shape[1],
                               stream_ptr()), "iic_doersch_loss")
  return loss, dl


class _IsolaLossFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, prob, mask, coords):
    shape = prob.shape
    loss, dp = isola_loss_raw(prob.detach().reshape(-1).contiguous(), mask, coords, ctx.needs_input_grad[0])
    if dp is not None:
      ctx.save_for_backward(dp)
    ctx.shape = shape
    return loss

  @staticmethod
  def backward(ctx, g):
    dp, = ctx.saved_tensors
    return (dp * g).view(ctx.shape), None, None      # the upstream scalar is multiplied in on the device


class _DoerschLossFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, logits, mask, coords):
    loss, dl = doersch_loss_raw(logits.detach().contiguous(), mask, coords, ctx.needs_input_grad[0])
    if dl is not None:
      ctx.save_for_backward(dl)
    return loss

  @staticmethod
  def backward(ctx, g):
    dl, = ctx.saved_tensors
    return dl * g, None, None


def isola_loss(adjacent_pred, centre, other, adjacent_gt, mask, verbose=False):
  """The reference's isola_loss (isola_utils.py:10-79) on the net's fp32 device output [N, 1] or [N] (sigmoid applied):
  the same value, one launch, no host read-back -- so the reference's ``verbose`` counts are not printed and a
  non-finite loss does not assert here (the scripts test ``loss.item()`` themselves, isola.py:284)."""
  assert (isinstance(centre, np.ndarray) and isinstance(other, np.ndarray) and isinstance(adjacent_gt, (bool, np.bool_)))
  if adjacent_pred.dim() not in (1, 2) or adjacent_pred.numel() != adjacent_pred.shape[0]:
    raise ValueError("isola_loss (HIP): adjacent_pred must be [N] or [N, 1], got %s" % (tuple(adjacent_pred.shape),))
  _check_common("isola_loss", adjacent_pred, centre, other, mask)
  ops.join()
  coords = coords_block(centre, other, 1 if adjacent_gt else 0, adjacent_pred.device)
  return _IsolaLossFn.apply(adjacent_pred, mask.contiguous(), coords)


def doersch_loss(position_pred, centre, other, position_gt, mask, crossent=None, verbose=False):
  """The reference's doersch_loss (doersch_utils.py:47-68) on fp32 device logits [N, 9].  ``crossent`` (the script's
  nn.CrossEntropyLoss(reduction="none")) is accepted and not called: the kernel evaluates it."""
  if position_pred.dim() != 2:
    raise ValueError("doersch_loss (HIP): position_pred must be [N, k], got %s" % (tuple(position_pred.shape),))
  k = position_pred.shape[1]
  if not 1 <= k <= MAX_K:
    raise ValueError("doersch_loss (HIP): k = %d is outside the served range 1 <= k <= %d" % (k, MAX_K))
  if not 0 <= int(position_gt) < k:
    raise ValueError("doersch_loss (HIP): position_gt = %r is outside [0, %d)" % (position_gt, k))
  _check_common("doersch_loss", position_pred, centre, other, mask)
  ops.join()
  coords = coords_block(centre, other, int(position_gt), position_pred.device)
  return _DoerschLossFn.apply(position_pred, mask.contiguous(), coords)


# ------------------------------------------------------------------------------------
# the scripts' loop body
# ------------------------------------------------------------------------------------
def train_step(net, optimiser, img, mask, kind, rng=None):
  """One iteration of the training loop of isola.py:266-295 / doersch.py on a device batch: zero_grad, patch selection
  on the host, forward, loss, backward, optimiser step.  ``img``: the network input (after sobel_process where the
  script applies it); ``mask``: uint8 [N, S, S]; ``kind``: "isola" or "doersch".  Returns the loss as a device scalar --
  nothing is read back."""
  core = getattr(net, "module", net)
  core.zero_grad()
  S = core.input_sz
  if kind == "isola":
    centre, other, gt = isola_set_patches(input_sz=S, patch_side=core.patch_side, rng=rng)
    loss = isola_loss(net(img, centre=centre, other=other), centre, other, gt, mask)
  elif kind == "doersch":
    centre, other, gt = doersch_set_patches(input_sz=S, patch_side=core.patch_side, rng=rng)
    loss = doersch_loss(net(img, centre=centre, other=other), centre, other, gt, mask)
  else:
    raise ValueError("kind must be 'isola' or 'doersch', got %r" % (kind,))
  loss.backward()
  optimiser.step()
  return loss.detach()
