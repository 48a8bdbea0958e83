"""Device buffers the wrappers recycle: the PT activation pool and the per-branch fp32 scratch."""
import torch

from .branches import current_branch

BF16 = torch.bfloat16
F32 = torch.float32


# ------------------------------------------------------------------------------------
# PT ("padded tile") activation buffers: bf16 [N, H+2P, W+2P, C], zero border.
# Kernels write interiors only, so buffers are zeroed ONCE and recycled through a pool
# (no per-step memset traffic).  A buffer is handed out by `alloc`, and returned with
# `release` once every kernel that reads it has been enqueued (stream-ordered reuse).
# ------------------------------------------------------------------------------------
# Storage type of PT tensors: bf16 (the product path) or, inside `with fp32_mode():`, fp32 -- the
# exact-fp32 parity path of csrc/f32_path.hip (SURVEY.md §8c tier T2): same orchestration, plain
# fp32 kernels, for whole-network comparisons with the reference's fp32 results.  Every wrapper
# of iic_amd.ops dispatches on the dtype of the tensors it is handed.
PT_DTYPE = [BF16]


class fp32_mode(object):
  def __enter__(self):
    self.prev = PT_DTYPE[0]
    PT_DTYPE[0] = F32
    return self

  def __exit__(self, *exc):
    PT_DTYPE[0] = self.prev
    return False


class PTPool(object):
  """Buffers are keyed by (shape, border P, device, branch, dtype): a recycled buffer is only valid
  for a tensor with the SAME interior/border split (its border must still be zero), and only on
  the stream (branch) whose kernels used it last.

  The pool keeps a reference to every buffer it created (`owned`), so an address can never come
  back from the caching allocator as some other tensor and be mistaken for a zero-border buffer;
  `release` only accepts buffers that are currently handed out (a second release -- e.g. a
  backward run twice -- is ignored instead of putting one buffer on the free list twice)."""

  def __init__(self):
    self.free = {}
    self.owned = {}           # data_ptr -> (tensor, P, branch) of every buffer this pool created
    self.live = {}            # data_ptr -> serial of the alloc() that handed it out
    self.serial = 0
    self.allocated_bytes = 0

  def alloc(self, shape, device, P=1):
    dt = PT_DTYPE[0]
    b = current_branch()
    key = (tuple(shape), int(P), str(device), b, dt)
    lst = self.free.get(key)
    if lst:
      t = lst.pop()
    else:
      t = torch.zeros(shape, dtype=dt, device=device)
      self.owned[t.data_ptr()] = (t, int(P), b)
      self.allocated_bytes += t.numel() * t.element_size()
    self.serial += 1
    self.live[t.data_ptr()] = self.serial
    # a fresh tensor object per hand-out: the caller's autograd state (grad_fn of the Function that
    # returns it, user hooks registered on it) must not survive into the buffer's next life
    return t.detach()

  def release(self, t):
    if t is None:
      return
    ent = self.owned.get(t.data_ptr())
    if ent is None or ent[0].shape != t.shape:
      return                  # not one of ours (a user tensor, a view): never recycle it
    if self.live.pop(t.data_ptr(), None) is None:
      return                  # already back in the pool
    key = (tuple(t.shape), ent[1], str(t.device), ent[2], t.dtype)
    self.free.setdefault(key, []).append(ent[0])

  def mark(self):
    return self.serial

  def sweep(self, mark):
    """Return every buffer handed out since `mark` that is still out: the end of a forward that
    no backward will follow (torch.no_grad evaluation), whose consumers are all enqueued."""
    for dp in [dp for dp, ser in self.live.items() if ser > mark]:
      self.release(self.owned[dp][0])

  def clear(self):
    self.free.clear()
    self.owned.clear()
    self.live.clear()


POOL = PTPool()


def pt_alloc(N, H, W, C, P, device):
  return POOL.alloc((N, H + 2 * P, W + 2 * P, C), device, P)


def pt_from_nchw(x, P):
  """(test / boundary helper) NCHW float tensor -> PT (bf16, or fp32 inside fp32_mode())."""
  n, c, h, w = x.shape
  out = torch.zeros((n, h + 2 * P, w + 2 * P, c), dtype=PT_DTYPE[0], device=x.device)
  out[:, P:P + h, P:P + w, :] = x.permute(0, 2, 3, 1).to(PT_DTYPE[0])
  return out


def pt_to_nchw(x, P):
  n, hp, wp, c = x.shape
  return x[:, P:hp - P, P:wp - P, :].permute(0, 3, 1, 2).float().contiguous()


class Scratch(object):
  """One fp32 scratch buffer per (device index, branch) -- split-K partials, K-split GEMM workspace: what a kernel
  pair hands over within one wrapper call, so the two branches must not share it and nothing else is kept in it.
  Grown on demand; a buffer that a larger request replaces goes to `retired` and is never freed: a captured graph
  may have its address baked in (head B's graphs kept replaying into a workspace that head A's larger
  request had freed)."""

  def __init__(self):
    self.bufs = {}            # (device index, branch) -> tensor
    self.retired = []

  def get(self, device, floats, minimum=0):
    key = (torch.device(device).index, current_branch())
    buf = self.bufs.get(key)
    if buf is None or buf.numel() < floats:
      if buf is not None:
        self.retired.append(buf)
      buf = self.bufs[key] = torch.empty(max(floats, minimum), dtype=F32, device=device)
    return buf
