"""The fully-connected layers of the package: the one place Python knows about a Linear.

  exact fp32        linear_f32_forward / linear_f32_backward / LinearF32Fn: nn.Linear on fp32 features through
                    iic_gemm_f32 -- the logit heads (archs.cluster._HeadsFn puts its softmax around the two helpers,
                    archs.triplets uses the Function as it is), SupHead5's second Linear, the baselines' second
                    Linear, and every first Linear under ops.fp32_mode()
  bf16 over PT      pt_linear_forward / pt_linear_bwd_dx / pt_linear_wgrad / PTLinearFn: Linear(Q C H W -> F) that reads
                    Q = 1 or 2 bf16 PT activations [N, H+2, W+2, C] in place on the bf16 MFMA pipe (csrc/sup_head.hip):
                    iic_sup_* for one activation (SupHead5's first Linear on layer 3), iic_pair_* for two (H = W = p:
                    the joint Linear of the Isola / Doersch heads).  PTLinearOperands caches the bf16 operands of the
                    parameter, refreshed once per optimiser step (the rule ops.PreppedWeights applies to the conv weights).

Column q K + (c H W + h W + w) of the parameter [F, Q K] (K = C H W, the (c, h, w) flatten of activation q) multiplies
channel c of pixel (h, w) of activation q; the weight gradient comes back in that layout.  There is no CPU fallback.
"""
import torch

from . import ops
from ._lib import IICLibraryError, check, lib, ptr, stream_ptr

F32, BF16 = torch.float32, torch.bfloat16
_WS = ops.Scratch()      # partial matrices of the PT forward's K split

__all__ = ["linear_f32_forward", "linear_f32_backward", "LinearF32Fn", "dy_cast", "pt_linear_nsplit", "pt_weight_prep",
           "PTLinearOperands", "pt_linear_forward", "pt_linear_bwd_dx", "pt_linear_wgrad", "PTLinearFn"]


# ------------------------------------------------------------------------------------
# exact fp32
# ------------------------------------------------------------------------------------
def linear_f32_forward(feats, W, b):
  """y [N, F] = feats [N, K] . W [F, K]^T + b [F]; feats and W contiguous."""
  assert feats.is_cuda, "Linear (HIP): device tensors required -- no CPU fallback"
  N, K = feats.shape
  Fo = W.shape[0]
  y = torch.empty((N, Fo), dtype=F32, device=feats.device)
  # y[n][j] = sum_c feats[n][c] * W[j][c] + b[j]
  ops.gemm_f32(feats, K, 1, W, 1, K, y, Fo, N, Fo, K, bias=b.contiguous())
  return y


def linear_f32_backward(dy, feats, W, need_dx=True):
  """(dfeats [N, K] or None, dW [F, K], db [F]) of a contiguous dy [N, F]."""
  N, K = feats.shape
  Fo = W.shape[0]
  # dW[j][c] = sum_n dy[n][j] feats[n][c]
  dW = torch.empty((Fo, K), dtype=F32, device=dy.device)
  ops.gemm_f32(dy, 1, Fo, feats, K, 1, dW, K, Fo, K, N)
  db = ops.colsum(dy, N, Fo)
  dfe = None
  if need_dx:
    # dfeats[n][c] = sum_j dy[n][j] W[j][c]
    dfe = torch.empty((N, K), dtype=F32, device=dy.device)
    ops.gemm_f32(dy, Fo, 1, W, K, 1, dfe, K, N, K, Fo)
  return dfe, dW, db


class LinearF32Fn(torch.autograd.Function):
  """nn.Linear on fp32 features, exact fp32: feats [N, K], W [F, K], b [F] -> [N, F]."""

  @staticmethod
  def forward(ctx, feats, W, b):
    feats, W = feats.contiguous(), W.contiguous()
    ctx.save_for_backward(feats, W)
    ctx.branch, ctx.pt_dtype = ops.current_branch(), ops.PT_DTYPE[0]   # (the K-split GEMM workspace is per branch)
    return linear_f32_forward(feats, W, b)

  @ops.branch_backward
  def backward(ctx, dy):
    feats, W = ctx.saved_tensors
    return linear_f32_backward(dy.contiguous(), feats, W, ctx.needs_input_grad[0])


# ------------------------------------------------------------------------------------
# bf16 MFMA over one or two PT activations
# ------------------------------------------------------------------------------------
def dy_cast(dy):
  """(dyb [N, F], dyt [F, Np]) bf16 of an fp32 [N, F] gradient (iic_sup_dy_cast)."""
  N, F = dy.shape
  Np = (N + 63) // 64 * 64
  dyb = torch.empty((N, F), dtype=BF16, device=dy.device)
  dyt = torch.empty((F, Np), dtype=BF16, device=dy.device)
  check(lib().iic_sup_dy_cast(ptr(dy), ptr(dyb), ptr(dyt), N, F, stream_ptr()), "iic_sup_dy_cast")
  return dyb, dyt


def _geometry(acts):
  """(N, C, H, W, Q) of a tuple of one or two PT activations of one shape."""
  Q = len(acts)
  assert Q in (1, 2) and all(a.shape == acts[0].shape for a in acts)
  N, Hp, Wp, C = acts[0].shape
  return N, C, Hp - 2, Wp - 2, Q


def pt_linear_nsplit(N, F, C, H, W, Q):
  """K slices of the forward (iic_sup_fwd_nsplit / iic_pair_linear_fwd_nsplit); 0: unsupported shape.  Host only."""
  if Q == 1:
    return int(lib().iic_sup_fwd_nsplit(int(N), int(F), int(C), int(H), int(W)))
  return int(lib().iic_pair_linear_fwd_nsplit(int(N), int(F), int(C), int(H))) if H == W else 0


def pt_weight_prep(w, C, H, W, Q, wb=None, wt=None):
  """(wb [F, Q K], wt [Q K, F]) bf16 operands of the fp32 parameter w [F, Q K], K = C H W, each column half in the PT
  interior order (iic_sup_weight_prep / iic_pair_weight_prep)."""
  Fo, Kt = w.shape
  if Kt != Q * C * H * W or (Q == 2 and H != W):
    raise ValueError("Linear over PT activations: weight has %d columns, %d * %d * %d * %d expected" % (Kt, Q, C, H, W))
  wb = torch.empty((Fo, Kt), dtype=BF16, device=w.device) if wb is None else wb
  wt = torch.empty((Kt, Fo), dtype=BF16, device=w.device) if wt is None else wt
  if Q == 1:
    check(lib().iic_sup_weight_prep(ptr(w), ptr(wb), ptr(wt), Fo, C, H, W, stream_ptr()), "iic_sup_weight_prep")
  else:
    check(lib().iic_pair_weight_prep(ptr(w), ptr(wb), ptr(wt), Fo, C, H, stream_ptr()), "iic_pair_weight_prep")
  return wb, wt


class PTLinearOperands(object):
  """bf16 operands (wb [F][Q K], wt [Q K][F]) of one nn.Linear over PT activations, per branch; re-written in place when
  the parameter has changed since they were made (data pointer, version counter, optimiser epoch), made anew when its
  device or size has."""

  def __init__(self):
    self._ent = {}      # branch -> [key, wb, wt]

  def get(self, w, C, H, W, Q):
    b = ops.current_branch()
    key = (w.data_ptr(), w._version, ops.WEIGHTS_EPOCH[0], C, H, W, Q)
    ent = self._ent.get(b)
    if ent is not None and ent[0] == key:
      return ent[1], ent[2]
    if ent is None or ent[1].device != w.device or ent[1].numel() != w.numel():
      ent = self._ent[b] = [None, None, None]
    ent[1], ent[2] = pt_weight_prep(w, C, H, W, Q, ent[1], ent[2])
    ent[0] = key
    return ent[1], ent[2]


def pt_linear_forward(acts, wb, bias, F):
  """y fp32 [N, F] = sum_q interior(acts[q]) . wb[:, q K:(q + 1) K]^T + bias (iic_sup_linear_fwd / iic_pair_linear_fwd)."""
  N, C, H, W, Q = _geometry(acts)
  name = "iic_sup_linear_fwd" if Q == 1 else "iic_pair_linear_fwd"
  S = pt_linear_nsplit(N, F, C, H, W, Q)
  if S < 1:
    raise IICLibraryError("%s: unsupported shape C = %d, F = %d, H = %d, W = %d (C, F multiples of 64%s)"
                          % (name, C, F, H, W, "" if Q == 1 else "; H = W odd"))
  y = torch.empty((N, F), dtype=F32, device=acts[0].device)
  ws = _WS.get(acts[0].device, S * N * F) if S > 1 else None
  if Q == 1:
    check(lib().iic_sup_linear_fwd(ptr(acts[0]), ptr(wb), ptr(bias), ptr(y), ptr(ws), N, F, C, H, W, stream_ptr()), name)
  else:
    check(lib().iic_pair_linear_fwd(ptr(acts[0]), ptr(acts[1]), ptr(wb), ptr(bias), ptr(y), ptr(ws), N, F, C, H,
                                    stream_ptr()), name)
  return y


def pt_linear_bwd_dx(dyb, wt, dxs):
  """Writes the interiors of the PT tensors dxs (one per activation) and returns them."""
  N, C, H, W, Q = _geometry(dxs)
  F = dyb.shape[1]
  if Q == 1:
    check(lib().iic_sup_linear_bwd_dx(ptr(dyb), ptr(wt), ptr(dxs[0]), N, F, C, H, W, stream_ptr()),
          "iic_sup_linear_bwd_dx")
  else:
    check(lib().iic_pair_linear_bwd_dx(ptr(dyb), ptr(wt), ptr(dxs[0]), ptr(dxs[1]), N, F, C, H, stream_ptr()),
          "iic_pair_linear_bwd_dx")
  return dxs


def pt_linear_wgrad(dyt, acts):
  """dW fp32 [F, Q K] in the parameter's order."""
  N, C, H, W, Q = _geometry(acts)
  F = dyt.shape[0]
  dW = torch.empty((F, Q * C * H * W), dtype=F32, device=acts[0].device)
  if Q == 1:
    check(lib().iic_sup_linear_wgrad(ptr(dyt), ptr(acts[0]), ptr(dW), N, F, C, H, W, stream_ptr()),
          "iic_sup_linear_wgrad")
  else:
    check(lib().iic_pair_linear_wgrad(ptr(dyt), ptr(acts[0]), ptr(acts[1]), ptr(dW), N, F, C, H, stream_ptr()),
          "iic_pair_linear_wgrad")
  return dW


class PTLinearFn(torch.autograd.Function):
  """Linear over one or two bf16 PT tensors [N, H+2, W+2, C] -> fp32 [N, F]: apply(a0[, a1], w, b, operands) with
  operands a PTLinearOperands; the gradients are (dx0[, dx1], dW [F, Q K], db, None)."""

  @staticmethod
  def forward(ctx, *args):
    acts, (w, b, operands) = args[:-3], args[-3:]
    assert all(a.dtype is BF16 and a.is_contiguous() and a.dim() == 4 for a in acts)
    N, C, H, W, Q = _geometry(acts)
    wb, wt = operands.get(w.detach(), C, H, W, Q)
    ctx.save_for_backward(wt, *acts)
    ctx.branch, ctx.pt_dtype = ops.current_branch(), ops.PT_DTYPE[0]
    return pt_linear_forward(acts, wb, b.detach() if b is not None else None, w.shape[0])

  @ops.branch_backward
  def backward(ctx, dy):
    wt, acts = ctx.saved_tensors[0], ctx.saved_tensors[1:]
    N, C, H, W, Q = _geometry(acts)
    dy = dy.contiguous()
    dyb, dyt = dy_cast(dy)
    dxs = (None,) * Q
    if any(ctx.needs_input_grad[:Q]):
      dxs = pt_linear_bwd_dx(dyb, wt, tuple(ops.pt_alloc(N, H, W, C, 1, dy.device) for _ in range(Q)))
    dW = pt_linear_wgrad(dyt, acts)
    db = ops.colsum(dy, N, dy.shape[1]) if ctx.needs_input_grad[Q + 1] else None
    return tuple(dxs) + (dW, db, None)
