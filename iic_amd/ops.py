"""Thin torch-tensor wrappers over the C ABI (include/iic_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every arithmetic op on
the hot path is a kernel of libiic_hip.so.  All wrappers enqueue on torch's current stream.

The two-stream execution state lives in iic_amd.branches and the PT buffer pool / scratch buffers in
iic_amd.pool; their public names are re-exported here.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import IIC_STAT_STRIPES, check, lib, ptr, stream_ptr
from .branches import (AUTO_BRANCH, BN_MOMENTUM, GRAPH_FORWARD, USE_PROXIES, BranchContext, HeadPack,  # noqa: F401
                       auto_branch, branch, branch_backward, branch_grads, branch_leaf, clear_branch_grads, context,
                       current_branch, flush_deferred_running, fold_branch_grads, join, on_branch, pv, tag_pack)
from .pool import (BF16, F32, POOL, PT_DTYPE, PTPool, Scratch, fp32_mode, pt_alloc, pt_from_nchw,  # noqa: F401
                   pt_to_nchw)


def new_stats(C, device):
  """Zeroed statistics accumulator for C channels (opaque exact fixed-point cells, see
  include/iic_hip.h: iic_stat_bytes)."""
  return torch.zeros(lib().iic_stat_bytes(C) // 8, dtype=torch.int64, device=device)


STAT_BINS, STAT_LSB0, STAT_SPACING = 8, -96, 24      # csrc/common.h


def stats_decode(st, C):
  """(test / debug helper, non-destructive) accumulator -> float64 [2, C] sums."""
  cells = st.view(IIC_STAT_STRIPES, C, 2, STAT_BINS).sum(0)          # exact int64
  val = torch.zeros((C, 2), dtype=torch.float64, device=st.device)
  for b in range(STAT_BINS - 2, -1, -1):
    val += torch.ldexp(cells[..., b].double(), torch.tensor(STAT_LSB0 + STAT_SPACING * b, device=st.device))
  val[cells[..., STAT_BINS - 1] != 0] = float("nan")
  return val.t().contiguous()


def stats_encode(st, C, values):
  """(test helper) overwrite the accumulator with the float32 sums `values` [2, C]."""
  st.zero_()
  v = values.to(st.device).float().t().contiguous().double()          # [C, 2]
  mant, exp = torch.frexp(v)
  m = torch.round(mant * (1 << 24)).long()
  pos = exp.long() - 24 - STAT_LSB0
  neg = pos < 0
  m = torch.where(neg, m >> (-pos).clamp(0, 62), m)
  pos = pos.clamp(min=0)
  b, sh = pos // STAT_SPACING, pos % STAT_SPACING
  cells = st.view(IIC_STAT_STRIPES, C, 2, STAT_BINS)
  cells[0].scatter_(2, b.clamp(max=STAT_BINS - 2).unsqueeze(-1), (m << sh).unsqueeze(-1))


# ------------------------------------------------------------------------------------
# conv
# ------------------------------------------------------------------------------------
def weight_prep(w, want_bwd=True):
  """fp32 OIHW parameter -> (bf16 [T][Co][Ci], bf16 [T][Ci][Co])  (row-major operands)."""
  co, ci, kh, kw = w.shape
  T = kh * kw
  wf = torch.empty((T, co, ci), dtype=BF16, device=w.device)
  wb = torch.empty((T, ci, co), dtype=BF16, device=w.device) if want_bwd else None
  check(lib().iic_weight_prep(ptr(w), ptr(wf), ptr(wb), co, ci, T, stream_ptr()), "iic_weight_prep")
  return wf, wb


def weight_prep_frag(w, bwd):
  """fp32 OIHW parameter -> bf16 MFMA-B-fragment order (include/iic_hip.h, iic_weight_prep_frag)."""
  co, ci, kh, kw = w.shape
  out = torch.empty((kh * kw * co * ci,), dtype=BF16, device=w.device)
  check(lib().iic_weight_prep_frag(ptr(w), ptr(out), co, ci, kh * kw, 1 if bwd else 0, stream_ptr()),
        "iic_weight_prep_frag")
  return out


# IIC_CONV_FRAG=0 keeps every conv on the first-generation kernel (row-major weight operand).
USE_FRAG = [os.environ.get("IIC_CONV_FRAG", "1") != "0"]

# Optimiser epoch: part of the key of every bf16 operand cache (PreppedWeights through archs.cluster._ConvHolder,
# linear.PTLinearOperands).  iic_amd.optim.Adam bumps it: its raw-pointer updates do not bump a parameter's _version.
WEIGHTS_EPOCH = [0]


def bump_weights_epoch():
  WEIGHTS_EPOCH[0] += 1


class PreppedWeights(object):
  """bf16 operands of one conv parameter, laid out lazily per consumer kernel.  `pw[0]` is the
  forward operand, `pw[1]` the backward-data operand (handles accepted by conv_igemm).

  The layouts a consumer asked for once are kept (same buffers) and RE-WRITTEN IN PLACE when the parameter
  has changed: `jobs()` lists them for the one-launch refresh of all convolutions of a network
  (refresh_prepped; archs.cluster._ConvHolder.weights)."""

  def __init__(self, w):
    self.w = w
    self._rows = None
    self._frag = [None, None]

  def rows(self, bwd):
    if self._rows is None:
      self._rows = weight_prep(self.w, want_bwd=True)
    return self._rows[1 if bwd else 0]

  def jobs(self):
    """(src ptr, dst ptr, Cout, Cin, T, mode) of every materialised layout (modes: include/iic_hip.h)."""
    co, ci, kh, kw = self.w.shape
    out = []
    for k in (0, 1):
      if self._frag[k] is not None:
        out.append((self.w.data_ptr(), self._frag[k].data_ptr(), co, ci, kh * kw, k))
    if self._rows is not None:
      for k in (0, 1):
        if self._rows[k] is not None:
          out.append((self.w.data_ptr(), self._rows[k].data_ptr(), co, ci, kh * kw, 2 + k))
    return out

  def frag(self, bwd):
    k = 1 if bwd else 0
    if self._frag[k] is None:
      self._frag[k] = weight_prep_frag(self.w, bwd)
    return self._frag[k]

  def __getitem__(self, i):
    return WOperand(self, bool(i))


class _PrepJob(ctypes.Structure):
  _fields_ = [("w", ctypes.c_void_p), ("out", ctypes.c_void_p), ("first_block", ctypes.c_longlong),
              ("Cout", ctypes.c_int32), ("Cin", ctypes.c_int32), ("T", ctypes.c_int32), ("mode", ctypes.c_int32)]


_PREP_TABLES = {}      # (device index, tuple of jobs) -> (device table, njobs, total blocks)
_PREP_PINNED = set()   # keys whose launch was recorded into a HIP graph: the table's address is baked in
MULTI_PREP = [os.environ.get("IIC_MULTI_PREP", "1") != "0"]


def refresh_prepped(pws, device):
  """Re-write every materialised layout of the given PreppedWeights from their (updated) fp32 parameters in
  ONE launch (iic_weight_prep_multi).  The job table lives in device memory and is cached by content: a
  network's jobs are the same every step, so the upload happens once, in the eager warm-up steps.  Returns
  False when nothing was launched because a NEW table would have to be uploaded while a stream is being
  captured (the caller then falls back to per-layout launches)."""
  jobs = tuple(j for pw in pws for j in pw.jobs())
  if not jobs:
    return True
  key = (device.index, jobs)
  ent = _PREP_TABLES.get(key)
  if ent is None:
    if torch.cuda.is_current_stream_capturing():
      return False
    arr = (_PrepJob * len(jobs))()
    blk = 0
    for a, (src, dst, co, ci, t, mode) in zip(arr, jobs):
      a.w, a.out, a.first_block, a.Cout, a.Cin, a.T, a.mode = src, dst, blk, co, ci, t, mode
      blk += lib().iic_weight_prep_multi_blocks(co, ci, t)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    ent = _PREP_TABLES[key] = (host.to(device), len(jobs), blk)
    if len(_PREP_TABLES) > 256:         # (tables of networks that no longer exist; never one a graph may replay)
      for k in [k for k in list(_PREP_TABLES)[:-128] if k not in _PREP_PINNED]:
        del _PREP_TABLES[k]
  if torch.cuda.is_current_stream_capturing():
    _PREP_PINNED.add(key)
  check(lib().iic_weight_prep_multi(ptr(ent[0]), ent[1], ent[2], stream_ptr()), "iic_weight_prep_multi")
  return True


class WOperand(object):
  def __init__(self, pw, bwd):
    self.pw, self.bwd = pw, bwd


def frag_supported(g):
  if not USE_FRAG[0]:
    return False
  ok = getattr(g, "_frag_ok", None)     # geometry objects are cached per (layer, shape)
  if ok is None:
    ok = bool(lib().iic_conv_igemm_frag_supported(ctypes.byref(g)))
    g._frag_ok = ok
  return ok


ACC_ADD, ACC_PREMASK = 1, 2     # include/iic_hip.h IIC_ACC_*


def red_supported(g, w_t):
  """Can this backward-data launch carry a fused BatchNorm-backward reduction (`red=`)?"""
  if PT_DTYPE[0] is not BF16 or not (isinstance(w_t, WOperand) and frag_supported(g)):
    return False
  ok = getattr(g, "_red_ok", None)
  if ok is None:
    ok = bool(lib().iic_conv_igemm_red_supported(ctypes.byref(g)))
    g._red_ok = ok
  return ok


def conv_igemm(g, x_pt, w_t, out_pt, stats=None, res_grad=None, res_act=None, accumulate=False,
               premask=False, red=None):
  """w_t: a row-major bf16 operand tensor (first-generation kernel) or a WOperand handle
  (second-generation weights-direct kernel wherever the geometry supports it).
  premask: out = (value [+ previous] [+ res_grad]) where res_act > 0 else 0 (IIC_ACC_PREMASK).
  red = (y, mask_coef | None, sums, y2 | None, sums2 | None): fused BatchNorm-backward reduction
  over the stored tile (iic_conv_igemm_frag_red); only where red_supported(g, w_t)."""
  acc = (ACC_ADD if accumulate else 0) | (ACC_PREMASK if premask else 0)
  if x_pt.dtype == F32:       # exact-fp32 parity path: the fp32 OIHW parameter itself is the operand
    assert isinstance(w_t, WOperand) and red is None and out_pt.dtype == F32
    w = w_t.pw.w
    check(lib().iic_f32_conv(ctypes.byref(g), ptr(x_pt), ptr(w), w.shape[2] * w.shape[3], 1 if w_t.bwd else 0,
                             ptr(out_pt), ptr(stats), ptr(res_grad), ptr(res_act), acc, stream_ptr()),
          "iic_f32_conv")
    return out_pt
  if red is not None:
    assert red_supported(g, w_t), "fused reduction needs the weights-direct kernel"
    ry, rcoef, rsums, ry2, rsums2 = red
    check(lib().iic_conv_igemm_frag_red(ctypes.byref(g), ptr(x_pt), ptr(w_t.pw.frag(w_t.bwd)),
                                        ptr(out_pt), ptr(stats), ptr(res_grad), ptr(res_act), acc,
                                        ptr(ry), ptr(rcoef), ptr(ry2), ptr(rsums), ptr(rsums2),
                                        stream_ptr()), "iic_conv_igemm_frag_red")
    return out_pt
  if isinstance(w_t, WOperand):
    if frag_supported(g):
      check(lib().iic_conv_igemm_frag(ctypes.byref(g), ptr(x_pt), ptr(w_t.pw.frag(w_t.bwd)),
                                      ptr(out_pt), ptr(stats), ptr(res_grad), ptr(res_act), acc,
                                      stream_ptr()), "iic_conv_igemm_frag")
      return out_pt
    w_t = w_t.pw.rows(w_t.bwd)
  check(lib().iic_conv_igemm(ctypes.byref(g), ptr(x_pt), ptr(w_t), ptr(out_pt), ptr(stats),
                             ptr(res_grad), ptr(res_act), acc, stream_ptr()),
        "iic_conv_igemm")
  return out_pt


WG_PART = Scratch()      # split-K partials of conv_wgrad
STEM_PART = Scratch()    # per-block partials of the stem's weight gradient
FC_PART = Scratch()      # per-block partials of firstconv_wgrad
GEMM_WS = Scratch()      # workspace of the K-split GEMMs


def conv_wgrad(g, x_pt, dy_pt, wtaps, use_tr=True, out=None, accumulate=False, nsplit=None):
  """Returns dW fp32 [Co][Ci][kh][kw] flattened as [Co, Ci, wtaps].  nsplit: override of the
  split-K factor (tests: few splits = many K-tiles per workgroup)."""
  if x_pt.dtype == F32:
    if out is None:
      out = torch.empty((g.Cout, g.Cin, wtaps), dtype=F32, device=x_pt.device)
    check(lib().iic_f32_wgrad(ctypes.byref(g), ptr(x_pt), ptr(dy_pt), ptr(out), wtaps, 1 if accumulate else 0,
                              stream_ptr()), "iic_f32_wgrad")
    return out
  ns = int(nsplit) if nsplit else lib().iic_conv_wgrad_nsplit(ctypes.byref(g))
  if out is None:
    out = torch.empty((g.Cout, g.Cin, wtaps), dtype=F32, device=x_pt.device)
  assert g.ntaps == wtaps, "wgrad geometry must list every weight tap once"
  part = WG_PART.get(x_pt.device, ns * g.ntaps * g.Cout * g.Cin, minimum=1 << 22)
  check(lib().iic_conv_wgrad(ctypes.byref(g), ptr(x_pt), ptr(dy_pt), ptr(part), ns,
                             1 if use_tr else 0, stream_ptr()), "iic_conv_wgrad")
  check(lib().iic_conv_wgrad_reduce(ptr(part), ns, wtaps, g.Cout, g.Cin, ptr(out),
                                    1 if accumulate else 0, stream_ptr()), "iic_conv_wgrad_reduce")
  return out


# ------------------------------------------------------------------------------------
# batch norm
# ------------------------------------------------------------------------------------
BN_EPS = 1e-5      # (BN_MOMENTUM: iic_amd.branches, beside the postponed running-statistic update)


# Replica de-duplication (opt-in, archs.cluster.DEDUP): while a de-duplicated forward runs, the
# unbiased running_var factor is computed for the TRUE batch (unique rows x this factor).
BN_REPLICAS = [1]


def bn_finalize(stats, gamma, beta, running_mean, running_var, nbt, C, count, training):
  """coef [5][C]: scale, shift, mean, invstd, unbiased batch variance."""
  coef = torch.empty((5, C), dtype=F32, device=gamma.device)
  bc = context()
  if training and running_mean is not None and (bc.branch != 0 or bc.pending_join or bc.solo_first):
    # a side branch is (or may still be) running: both views update the same running statistics,
    # so every update is postponed to the join and applied there in CALL order -- the order a
    # sequential run would have used (fork the view that comes first in the script)
    bc.deferred_running.append((coef, running_mean, running_var, nbt, C))
    running_mean = running_var = nbt = None
  check(lib().iic_bn_finalize(ptr(stats), ptr(gamma), ptr(beta), ptr(running_mean),
                              ptr(running_var), ptr(nbt), ptr(coef), C, count,
                              count * BN_REPLICAS[0], BN_EPS, BN_MOMENTUM, 1 if training else 0,
                              stream_ptr()), "iic_bn_finalize")
  return coef


def bn_apply(y, coef, out, N, H, W, P, C, res=None, y2=None, coef2=None, relu=True):
  if y.dtype == F32:
    check(lib().iic_f32_bn_apply(ptr(y), ptr(coef), ptr(res), ptr(y2), ptr(coef2), ptr(out), N, H, W, P, C,
                                 1 if relu else 0, stream_ptr()), "iic_f32_bn_apply")
    return out
  check(lib().iic_bn_apply(ptr(y), ptr(coef), ptr(res), ptr(y2), ptr(coef2), ptr(out), N, H, W, P,
                           C, 1 if relu else 0, stream_ptr()), "iic_bn_apply")
  return out


def bn_bwd_reduce(dout, act, y, sums, N, H, W, P, C, y2=None, sums2=None, mask_coef=None):
  """mask_coef: forward coef of this BN when act = relu(bn(y)) exactly (pass act=None): the ReLU
  mask is recomputed from y instead of reading the activation tensor."""
  if y.dtype == F32:
    check(lib().iic_f32_bn_bwd_reduce(ptr(dout), ptr(act), ptr(y), ptr(y2), ptr(sums), ptr(sums2),
                                      ptr(mask_coef), N, H, W, P, C, stream_ptr()), "iic_f32_bn_bwd_reduce")
    return
  check(lib().iic_bn_bwd_reduce(ptr(dout), ptr(act), ptr(y), ptr(y2), ptr(sums), ptr(sums2),
                                ptr(mask_coef), N, H, W, P, C, stream_ptr()), "iic_bn_bwd_reduce")


def bn_bwd_finalize(sums, gamma, coef, C, count):
  bcoef = torch.empty((3, C), dtype=F32, device=gamma.device)
  dgamma = torch.empty(C, dtype=F32, device=gamma.device)
  dbeta = torch.empty(C, dtype=F32, device=gamma.device)
  check(lib().iic_bn_bwd_finalize(ptr(sums), ptr(gamma), ptr(coef), ptr(bcoef), ptr(dgamma),
                                  ptr(dbeta), C, count, stream_ptr()), "iic_bn_bwd_finalize")
  return bcoef, dgamma, dbeta


def bn_bwd_apply(dout, act, y, bcoef, dy, N, H, W, P, C, y2=None, bcoef2=None, dy2=None,
                 mask_coef=None):
  if y.dtype == F32:
    check(lib().iic_f32_bn_bwd_apply(ptr(dout), ptr(act), ptr(y), ptr(bcoef), ptr(dy), ptr(y2), ptr(bcoef2),
                                     ptr(dy2), ptr(mask_coef), N, H, W, P, C, stream_ptr()),
          "iic_f32_bn_bwd_apply")
    return
  check(lib().iic_bn_bwd_apply(ptr(dout), ptr(act), ptr(y), ptr(bcoef), ptr(dy), ptr(y2),
                               ptr(bcoef2), ptr(dy2), ptr(mask_coef), N, H, W, P, C, stream_ptr()),
        "iic_bn_bwd_apply")


def bn_bwd_finalize_frozen(sums, coef, C, want_bcoef=False):
  """Finaliser of a BatchNorm that normalised with its running statistics: dgamma = (sum g*y - running_mean * sum g)
  * invstd, dbeta = sum g, from `sums` (re-zeroed) and the forward coef.  want_bcoef: also (scale, 0, 0), the
  three-coefficient form of the consumers that keep it (stem_wgrad_combine, stem_bwd_wgrad, the fp32 bn_bwd_apply)."""
  bcoef = torch.empty((3, C), dtype=F32, device=coef.device) if want_bcoef else None
  dgamma = torch.empty(C, dtype=F32, device=coef.device)
  dbeta = torch.empty(C, dtype=F32, device=coef.device)
  check(lib().iic_bn_bwd_finalize_frozen(ptr(sums), ptr(coef), ptr(bcoef), ptr(dgamma), ptr(dbeta), C, stream_ptr()),
        "iic_bn_bwd_finalize_frozen")
  return bcoef, dgamma, dbeta


def bn_bwd_frozen(dout, act, y, coef, dy, sums, N, H, W, P, C, y2=None, coef2=None, dy2=None, sums2=None,
                  mask_coef=None):
  """Whole backward of a BatchNorm on running statistics (eval(), a frozen layer): writes dy = scale * g (dy2 for a
  second BatchNorm sharing g) and returns (dgamma, dbeta, dgamma2, dbeta2).  bf16: one streaming pass
  (iic_bn_bwd_frozen) + the finaliser.  F32 (fp32_mode, the parity instrument): the existing fp32 kernels, reduce ->
  finaliser with bcoef = (scale, 0, 0) -> apply."""
  dg2 = db2 = None
  if y.dtype == F32:
    bn_bwd_reduce(dout, act, y, sums, N, H, W, P, C, y2=y2, sums2=sums2, mask_coef=mask_coef)
    bc, dg, db = bn_bwd_finalize_frozen(sums, coef, C, want_bcoef=True)
    bc2 = None
    if y2 is not None:
      bc2, dg2, db2 = bn_bwd_finalize_frozen(sums2, coef2, C, want_bcoef=True)
    bn_bwd_apply(dout, act, y, bc, dy, N, H, W, P, C, y2=y2, bcoef2=bc2, dy2=dy2, mask_coef=mask_coef)
    return dg, db, dg2, db2
  check(lib().iic_bn_bwd_frozen(ptr(dout), ptr(act), ptr(y), ptr(coef), ptr(dy), ptr(y2), ptr(coef2), ptr(dy2),
                                ptr(sums), ptr(sums2), ptr(mask_coef), N, H, W, P, C, stream_ptr()),
        "iic_bn_bwd_frozen")
  _, dg, db = bn_bwd_finalize_frozen(sums, coef, C)
  if y2 is not None:
    _, dg2, db2 = bn_bwd_finalize_frozen(sums2, coef2, C)
  return dg, db, dg2, db2


def bn_bwd(batch, dout, act, y, coef, gamma, dy, sums, N, H, W, P, C, mask_coef=None, reduced=False):
  """Backward of ONE BatchNorm in the mode its forward ran in: batch statistics (reduce -> finalise -> apply; reduced:
  a convolution's epilogue took the sums already) or running statistics (bn_bwd_frozen).  Returns (dgamma, dbeta)."""
  if not batch:
    assert not reduced, "a BatchNorm on running statistics never takes part in a fused reduction"
    return bn_bwd_frozen(dout, act, y, coef, dy, sums, N, H, W, P, C, mask_coef=mask_coef)[:2]
  if not reduced:
    bn_bwd_reduce(dout, act, y, sums, N, H, W, P, C, mask_coef=mask_coef)
  bcoef, dgamma, dbeta = bn_bwd_finalize(sums, gamma, coef, C, N * H * W)
  bn_bwd_apply(dout, act, y, bcoef, dy, N, H, W, P, C, mask_coef=mask_coef)
  return dgamma, dbeta


# ------------------------------------------------------------------------------------
# stem + sobel
# ------------------------------------------------------------------------------------
def sobel(imgs, include_rgb, using_IR=False):
  n, c, h, w = imgs.shape
  cout = {(False, False): 2, (True, False): 5, (False, True): 3, (True, True): 6}[
    (bool(include_rgb), bool(using_IR))]
  imgs = imgs.contiguous()
  out = torch.empty((n, cout, h, w), dtype=F32, device=imgs.device)
  check(lib().iic_sobel(ptr(imgs), ptr(out), n, c, h, w, 1 if include_rgb else 0,
                        1 if using_IR else 0, stream_ptr()), "iic_sobel")
  return out


def stem_stats(x, w, stats):
  n, c, h, wd = x.shape
  check(lib().iic_stem_stats(ptr(x), ptr(w), ptr(stats), n, c, h, wd, stream_ptr()), "iic_stem_stats")


def stem_apply_pool(x, w, coef, out_pt):
  n, c, h, wd = x.shape
  check(lib().iic_stem_apply_pool(ptr(x), ptr(w), ptr(coef), ptr(out_pt), n, c, h, wd, stream_ptr()),
        "iic_stem_apply_pool")


def stem_bwd_reduce(x, w, coef, dpool, sums):
  n, c, h, wd = x.shape
  check(lib().iic_stem_bwd_reduce(ptr(x), ptr(w), ptr(coef), ptr(dpool), ptr(sums), n, c, h, wd,
                                  stream_ptr()), "iic_stem_bwd_reduce")


def stem_bwd_wgrad(x, w, coef, bcoef, dpool):
  n, c, h, wd = x.shape
  part = _stem_partials(x.device)
  dW = torch.empty_like(w)
  check(lib().iic_stem_bwd_wgrad(ptr(x), ptr(w), ptr(coef), ptr(bcoef), ptr(dpool), ptr(part),
                                 ptr(dW), n, c, h, wd, stream_ptr()), "iic_stem_bwd_wgrad")
  return dW


def _stem_partials(device):
  return STEM_PART.get(device, lib().iic_stem_wgrad_partial_floats())


def stem_bwd_fused_ok(cin):
  """One-pass stem backward: K = 9*Cin must fit one 32-wide MFMA column tile."""
  return 9 * cin <= 32


def stem_bwd_fused(x, w, coef, dpool, sums):
  """sums += (sum g, sum g*y) AND the coefficient-free dW GEMMs; returns the handle for
  stem_wgrad_combine."""
  n, c, h, wd = x.shape
  part = _stem_partials(x.device)
  nb = ctypes.c_int(0)
  check(lib().iic_stem_bwd_fused(ptr(x), ptr(w), ptr(coef), ptr(dpool), ptr(sums), ptr(part),
                                 ctypes.byref(nb), n, c, h, wd, stream_ptr()), "iic_stem_bwd_fused")
  return part, nb.value


def stem_wgrad_combine(handle, bcoef, w):
  part, nb = handle
  dW = torch.empty_like(w)
  check(lib().iic_stem_wgrad_combine(ptr(part), nb, ptr(bcoef), ptr(dW), w.shape[1], stream_ptr()),
        "iic_stem_wgrad_combine")
  return dW


def f32_nchw_to_pt(x, out_pt, P):
  n, c, h, w = x.shape
  check(lib().iic_f32_nchw_to_pt(ptr(x), ptr(out_pt), n, c, h, w, P, stream_ptr()), "iic_f32_nchw_to_pt")
  return out_pt


def f32_maxpool_s2p1_fwd(x_pt, out_pt, N, H, W, C):
  check(lib().iic_f32_maxpool_s2p1_fwd(ptr(x_pt), ptr(out_pt), N, H, W, C, stream_ptr()), "iic_f32_maxpool_s2p1_fwd")
  return out_pt


def f32_maxpool_s2p1_bwd(x_pt, dout_pt, din_pt, N, H, W, C):
  check(lib().iic_f32_maxpool_s2p1_bwd(ptr(x_pt), ptr(dout_pt), ptr(din_pt), N, H, W, C, stream_ptr()),
        "iic_f32_maxpool_s2p1_bwd")
  return din_pt


# ------------------------------------------------------------------------------------
# heads
# ------------------------------------------------------------------------------------
def avgpool_fwd(x_pt, N, H, W, P, C):
  feats = torch.empty((N, C), dtype=F32, device=x_pt.device)
  if x_pt.dtype == F32:
    check(lib().iic_f32_avgpool_fwd(ptr(x_pt), ptr(feats), N, H, W, P, C, stream_ptr()), "iic_f32_avgpool_fwd")
    return feats
  check(lib().iic_avgpool_fwd(ptr(x_pt), ptr(feats), N, H, W, P, C, stream_ptr()), "iic_avgpool_fwd")
  return feats


def avgpool_bwd(dfeats, out_pt, N, H, W, P, C, mask_act=None):
  if out_pt.dtype == F32:
    check(lib().iic_f32_avgpool_bwd(ptr(dfeats), ptr(out_pt), N, H, W, P, C, ptr(mask_act), stream_ptr()),
          "iic_f32_avgpool_bwd")
    return out_pt
  check(lib().iic_avgpool_bwd(ptr(dfeats), ptr(out_pt), N, H, W, P, C, ptr(mask_act), stream_ptr()),
        "iic_avgpool_bwd")
  return out_pt


def gemm_f32(A, sam, sak, B, sbk, sbn, C, scm, M, N, K, bias=None, accumulate=False):
  need = lib().iic_gemm_f32_ws_floats(sam, sak, sbk, sbn, M, N, K)
  ws = GEMM_WS.get(C.device, need, minimum=1 << 20) if need else None
  check(lib().iic_gemm_f32_ws(ptr(A), sam, sak, ptr(B), sbk, sbn, ptr(bias), ptr(C), scm, M, N, K,
                              1 if accumulate else 0, ptr(ws), need, stream_ptr()), "iic_gemm_f32_ws")
  return C


def softmax_fwd(logits, rows, k):
  probs = torch.empty_like(logits)
  check(lib().iic_softmax_fwd(ptr(logits), ptr(probs), rows, k, stream_ptr()), "iic_softmax_fwd")
  return probs


def softmax_bwd(probs, dprobs, rows, k):
  dl = torch.empty_like(probs)
  check(lib().iic_softmax_bwd(ptr(probs), ptr(dprobs), ptr(dl), rows, k, stream_ptr()),
        "iic_softmax_bwd")
  return dl


def colsum(A, rows, cols):
  out = torch.empty(cols, dtype=F32, device=A.device)
  check(lib().iic_colsum_f32(ptr(A), ptr(out), rows, cols, 0, stream_ptr()), "iic_colsum_f32")
  return out


# ------------------------------------------------------------------------------------
# VGG-style trunks: first-layer conv from the image, 2x2 max-pool
# ------------------------------------------------------------------------------------
def firstconv_fwd(x, w, out_pt, stats, K, pad, P):
  n, c, h, wd = x.shape
  check(lib().iic_firstconv_fwd(ptr(x), ptr(w), ptr(out_pt), ptr(stats), n, c, h, wd, K, pad, P,
                                stream_ptr()), "iic_firstconv_fwd")
  return out_pt


def firstconv_wgrad(x, dy_pt, w_shape, K, pad, P):
  n, c, h, wd = x.shape
  part = FC_PART.get(x.device, lib().iic_firstconv_wgrad_partial_floats())
  dW = torch.empty(w_shape, dtype=F32, device=x.device)
  check(lib().iic_firstconv_wgrad(ptr(x), ptr(dy_pt), ptr(part), ptr(dW), n, c, h, wd, K, pad, P,
                                  stream_ptr()), "iic_firstconv_wgrad")
  return dW


def maxpool2_fwd(x_pt, out_pt, N, H, W, Pi, Po, C):
  if x_pt.dtype == F32:
    check(lib().iic_f32_maxpool2_fwd(ptr(x_pt), ptr(out_pt), N, H, W, Pi, Po, C, stream_ptr()), "iic_f32_maxpool2_fwd")
    return out_pt
  check(lib().iic_maxpool2_fwd(ptr(x_pt), ptr(out_pt), N, H, W, Pi, Po, C, stream_ptr()),
        "iic_maxpool2_fwd")
  return out_pt


def bn_relu_maxpool2_fwd(y_pt, coef, out_pt, N, H, W, Pi, Po, C):
  """out = maxpool2(relu(bn(y))) without storing the activation (bf16 PT tensors only; include/iic_hip.h)."""
  assert y_pt.dtype == BF16
  check(lib().iic_bn_relu_maxpool2_fwd(ptr(y_pt), ptr(coef), ptr(out_pt), N, H, W, Pi, Po, C, stream_ptr()),
        "iic_bn_relu_maxpool2_fwd")
  return out_pt


def bn_relu_maxpool2_bwd(y_pt, coef, dout_pt, din_pt, N, H, W, Pi, Po, C):
  """din = gradient w.r.t. a = relu(bn(y)) of that pool: dout at the first arg-max of the recomputed a."""
  assert y_pt.dtype == BF16
  check(lib().iic_bn_relu_maxpool2_bwd(ptr(y_pt), ptr(coef), ptr(dout_pt), ptr(din_pt), N, H, W, Pi, Po, C,
                                       stream_ptr()), "iic_bn_relu_maxpool2_bwd")
  return din_pt


def maxpool2_bwd(x_pt, dout_pt, din_pt, N, H, W, Pi, Po, C):
  if x_pt.dtype == F32:
    check(lib().iic_f32_maxpool2_bwd(ptr(x_pt), ptr(dout_pt), ptr(din_pt), N, H, W, Pi, Po, C, stream_ptr()),
          "iic_f32_maxpool2_bwd")
    return din_pt
  check(lib().iic_maxpool2_bwd(ptr(x_pt), ptr(dout_pt), ptr(din_pt), N, H, W, Pi, Po, C,
                               stream_ptr()), "iic_maxpool2_bwd")
  return din_pt
