"""Shapes, draws, float64 references, bounds and CPU emulations shared by tests/test_sup_head_cpu.py (the proof, no GPU)
and tests/test_gpu_sup_head.py (the kernels of csrc/sup_head.hip).  A plain module, not a test file.

Notation: x is layer 3's activation [N, C, H, W] (bf16 values), the kernels read it as the interior of a PT tensor
[N, H+2, W+2, C]; Wp the first Linear's fp32 parameter [F, K], K = C H W, columns in (c, h, w) order; dy the fp32
gradient of the Linear's output [N, F].  The kernels round Wp and dy to bf16 (nearest even) themselves; every float64
reference here is taken on the ALREADY ROUNDED operands, so the bounds below cover the fp32 accumulation (and, for dx,
the one bf16 store) and nothing else.

Bounds, all from tests/parity.py:
  forward  y  = x . bf16(Wp)^T + b     K terms   conv_acc_bound(K, A, extra = S): the kernel splits K into S slices
                                                 (iic_sup_fwd_nsplit; S = 1: none), writes S partial matrices and adds
                                                 them in index order -- S - 1 additions -- then the bias: one more.  With
                                                 S = 1 the bias is added in the GEMM's epilogue: extra = 1 = S again.
                                                 A = |x| . |bf16(Wp)|^T + |b|.
  dW          = bf16(dy)^T . x         N terms   conv_acc_bound(N, A): one accumulator per element, no fold, stored as it is
  dx          = bf16(dy) . bf16(Wp)    F terms   bf16_bracket(ref, conv_acc_bound(F, A)): one accumulator, one RNE store
"""
import collections
import functools

import numpy as np
import torch

from tests.conv_f64_cases import DRAWS, POS_DECISIVE_FLOOR, mixed_decisive_floor   # noqa: F401
from tests.parity import U32, U64, bf16_bracket, bf16_rne, conv_acc_bound

Case = collections.namedtuple("Case", "name N H W C F")
CASE_A = Case("A", 37, 3, 3, 64, 192)          # N is no multiple of any tile; F = 128 + 64: a partial column tile
CASE_B = Case("B", 12, 5, 5, 256, 2048)        # the real head behind a 32 x 32 trunk: the forward splits K here
# lattice only (cheap, exact): two row tiles of 128, the second partial; H != W; fewer pixels than one pixel tile of dW
CASE_D = Case("D", 150, 2, 3, 64, 64)
# lattice only: more than 64 pixels (the operand kernel's second pixel tile, partial) and a partial fifth pixel tile of dW
CASE_E = Case("E", 3, 9, 8, 64, 64)
CASES = (CASE_A, CASE_B)
LATTICE_CASES = (CASE_A, CASE_B, CASE_D, CASE_E)
UNSUPPORTED = Case("unsupported", 4, 3, 3, 96, 100)


def K_of(case):
  return case.C * case.H * case.W


def bf16(t):
  return t.to(torch.bfloat16).float()


# ---- layouts ---------------------------------------------------------------------------------------------------------
def flat_chw(x):
  """[N, C, H, W] -> [N, K] in the reference's flatten order (net5g.py:56)."""
  return x.reshape(x.shape[0], -1)


def to_pt(x, fill=0.0, dtype=torch.bfloat16):
  """[N, C, H, W] -> PT tensor [N, H+2, W+2, C], border = fill (host tensor)."""
  n, c, h, w = x.shape
  out = torch.full((n, h + 2, w + 2, c), fill, dtype=dtype)
  out[:, 1:h + 1, 1:w + 1] = x.permute(0, 2, 3, 1).to(dtype)
  return out


def from_pt(pt):
  """interior of a PT tensor -> [N, C, H, W] float32 (host)."""
  return pt[:, 1:-1, 1:-1].permute(0, 3, 1, 2).float().cpu().contiguous()


# ---- draws -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def inputs(case, draw):
  """x (bf16 values), w, b, dy (full fp32 mantissas: the kernels round w and dy), float32 host tensors.  `pos`: the
  absolute values of the `mixed` draw (tests/conv_f64_cases.py).  Shared, never modified."""
  assert draw in DRAWS
  rng = np.random.default_rng([11, case.N, case.H, case.W, case.C, case.F])
  K = K_of(case)
  u = lambda shape, s=1.0: torch.from_numpy((rng.uniform(-1.0, 1.0, shape) * s).astype(np.float32))
  t = collections.OrderedDict()
  t["x"] = bf16(u((case.N, case.C, case.H, case.W)))
  t["w"] = u((case.F, K), 1.0 / np.sqrt(K))
  t["b"] = u((case.F,), 0.1)
  t["dy"] = u((case.N, case.F))
  if draw == "pos":
    t = collections.OrderedDict((k, v.abs()) for k, v in t.items())
  return t


def lattice_inputs(case):
  """Small integers: x in {-1, 0, 1, 2}, w in {-2 .. 2}, b in {-3 .. 3}, dy in {-2, -1, 0, 1, 2} -- exact in bf16; every
  product and every partial sum of the three products is an integer below 2^24 (K * 4 <= 25 600), exact in fp32 in any
  order.  The columns of w are pairwise distinct (asserted), so a wrong column permutation changes the result."""
  rng = np.random.default_rng([12, case.N, case.H, case.W, case.C, case.F])
  K = K_of(case)
  t = collections.OrderedDict()
  t["x"] = torch.from_numpy(rng.integers(-1, 3, (case.N, case.C, case.H, case.W)).astype(np.float32))
  t["w"] = torch.from_numpy(rng.integers(-2, 3, (case.F, K)).astype(np.float32))
  t["b"] = torch.from_numpy(rng.integers(-3, 4, (case.F,)).astype(np.float32))
  t["dy"] = torch.from_numpy(rng.integers(-2, 3, (case.N, case.F)).astype(np.float32))
  return t


def columns_distinct(w):
  return len(set(bytes(c) for c in w.t().contiguous().numpy())) == w.shape[1]


# ---- float64 references: value and magnitude sum -------------------------------------------------------------------
def products64(x, w, b, dy):
  """(y, Ay, dW, AdW, dx, Adx): float64 results of the three products on the operands AS GIVEN (round them first) and
  the same products on the magnitudes.  dx comes back [N, C, H, W]."""
  xf, wd, dyd = flat_chw(x).double(), w.double(), dy.double()
  y = xf @ wd.t() + b.double()
  Ay = xf.abs() @ wd.abs().t() + b.double().abs()
  dW = dyd.t() @ xf
  AdW = dyd.abs().t() @ xf.abs()
  dx = (dyd @ wd).reshape(x.shape)
  Adx = (dyd.abs() @ wd.abs()).reshape(x.shape)
  return y, Ay, dW, AdW, dx, Adx


@functools.lru_cache(maxsize=4)
def refs(case, draw):
  t = inputs(case, draw)
  return products64(t["x"], bf16(t["w"]), t["b"], bf16(t["dy"]))


def forward_bound(case, A, nsplit):
  return conv_acc_bound(K_of(case), A, extra=nsplit)


def wgrad_bound(case, A):
  return conv_acc_bound(case.N, A)


def dx_bracket(case, ref, A):
  b = conv_acc_bound(case.F, A)
  return (b,) + bf16_bracket(ref, b)


def decisive_share(lo, hi):
  return float((lo == hi).double().mean())


def decisive_floor(case, draw):
  return POS_DECISIVE_FLOOR if draw == "pos" else mixed_decisive_floor(case.F)


# ---- CPU emulations of what a kernel may legitimately do, and of seeded defects -------------------------------------
def emu_forward(x, wb, b, chunks=1, order=None, drop_tile=None, columns=None):
  """fp32 forward: K cut into `chunks` slices whose fp32 partial products are added in `order`, then the bias.
  drop_tile: a (start, stop) K range left out (defect); columns: a column index applied to x's flatten (defect: the
  operand's (h, w, c) order used against (c, h, w) columns)."""
  xf = flat_chw(x)
  if columns is not None:
    xf = xf[:, columns]
  keep = torch.ones(xf.shape[1], dtype=torch.bool)
  if drop_tile is not None:
    keep[drop_tile[0]:drop_tile[1]] = False
  parts = [(xf[:, g] * keep[g]) @ wb[:, g].t() for g in torch.arange(xf.shape[1]).chunk(chunks)]
  order = range(len(parts)) if order is None else order
  acc = None
  for i in order:
    acc = parts[i].clone() if acc is None else acc + parts[i]
  return acc + b


def emu_wgrad(x, dyb, chunks=1, order=None):
  xf = flat_chw(x)
  parts = [dyb[g].t() @ xf[g] for g in torch.arange(xf.shape[0]).chunk(chunks)]
  order = range(len(parts)) if order is None else order
  acc = None
  for i in order:
    acc = parts[i].clone() if acc is None else acc + parts[i]
  return acc


def emu_dx_acc(x_shape, dyb, wb, chunks=1, order=None, on_part=None):
  parts = [dyb[:, g] @ wb[g] for g in torch.arange(wb.shape[0]).chunk(chunks)]
  if on_part:
    parts = [on_part(p) for p in parts]
  order = range(len(parts)) if order is None else order
  acc = None
  for i in order:
    acc = parts[i].clone() if acc is None else acc + parts[i]
  return acc.reshape(x_shape)


def store_rne(acc):
  return acc.to(torch.bfloat16).float()


def store_truncating(acc):
  return (acc.contiguous().view(torch.int32) & -65536).view(torch.float32)


# ---- BatchNorm1d + ReLU ---------------------------------------------------------------------------------------------
# The kernels (csrc/sup_head.hip sup_bn_relu_*_kernel) take every column sum in float64 in a fixed order and do the
# element-wise arithmetic in fp32.  Roundings, one unit U32 = 2^-24 relative each, as tests/bn_bf16_cases.py counts them:
#   mean, inv        float64 results rounded to fp32 once: U32 |mean|, U32 |inv|
#   d = x - mean     U32 |d|, plus the mean's own U32 |mean|
#   xh = d inv       U32 |xh|;  with inv's rounding:  |err xh| <= U32 (|inv mean| + 3 |xh|)
#   z = xh g + b     two roundings (or one, fused): |err z| <= |g| err xh + U32 (2 |g xh| + |b|)
# The float64 sums themselves carry N U64 relative to their magnitude sums: SUM64 charges 4 N U64 on top (value,
# square, the division and the square root), which is below 1e-12 here and stated rather than dropped.
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
SLACK = 1.0 + 2.0 ** -10          # second-order terms of the expansions below (products of two U32-sized errors)


def bn_inputs(N, F, seed):
  rng = np.random.default_rng([13, N, F, seed])
  f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
  return dict(x=f(N, F) * 1.5 + 0.3, gamma=f(F) * 0.5 + 1.0, beta=f(F) * 0.3, dout=f(N, F),
              rm=f(F) * 0.2, rv=(f(F) * 0.2).abs() + 0.5)


def bn_ref(t, training, x2=None):
  """float64 torch.nn on the CPU.  Returns a dict: y, pre-activation z, xhat, mean, inv, dx, dgamma, dbeta and the
  running statistics after this step (`rm1`, `rv1`) and, when x2 is given, after a second training step on x2."""
  N, F = t["x"].shape
  bn = torch.nn.BatchNorm1d(F, eps=BN_EPS, momentum=BN_MOMENTUM).double()
  with torch.no_grad():
    bn.weight.copy_(t["gamma"].double())
    bn.bias.copy_(t["beta"].double())
    bn.running_mean.copy_(t["rm"].double())
    bn.running_var.copy_(t["rv"].double())
  bn.train(training)
  x = t["x"].double().requires_grad_(True)
  z = bn(x)
  y = torch.relu(z)
  y.backward(t["dout"].double())
  if training:
    mean, var = x.detach().mean(0), x.detach().var(0, unbiased=False)
  else:
    mean, var = t["rm"].double(), t["rv"].double()
  inv = 1.0 / torch.sqrt(var + BN_EPS)
  out = dict(y=y.detach(), z=z.detach(), xhat=(x.detach() - mean) * inv, mean=mean, inv=inv, var=var, dx=x.grad,
             dgamma=bn.weight.grad, dbeta=bn.bias.grad, rm1=bn.running_mean.clone(), rv1=bn.running_var.clone())
  if x2 is not None:
    bn(x2.double())
    out["rm2"], out["rv2"] = bn.running_mean.clone(), bn.running_var.clone()
    out["mean2"], out["uvar2"] = x2.double().mean(0), x2.double().var(0, unbiased=True)
  return out


def bn_fwd_bound(t, r):
  """(|err xhat|, |err z|): the ReLU does not increase the latter."""
  N = t["x"].shape[0]
  g, b = t["gamma"].double().abs(), t["beta"].double().abs()
  xh = r["xhat"].abs()
  sum64 = 4 * N * U64 * ((r["inv"] * r["mean"]).abs() + xh + 1.0)
  exh = (U32 * ((r["inv"] * r["mean"]).abs() + 3 * xh) + sum64) * SLACK
  ez = (g * exh + U32 * (2 * g * xh + b)) * SLACK
  return exh, ez


def bn_running_bound(rm0, stats, N):
  """Running statistic after len(stats) steps: each step is ONE fp32 rounding of a float64 combination of the previous
  fp32 value and the batch statistic -- U32 of its result, and the previous steps' roundings pass on times 0.9.  The
  result is a convex combination of rm0 and the batch statistics: its magnitude is at most M = |rm0| + sum |stat|.
  The float64 statistic itself: 4 N U64 relative (sum, squares, division, the N / (N - 1) factor)."""
  M = rm0.double().abs() + sum(s.abs() for s in stats)
  return (len(stats) * U32 + 4 * N * U64) * M * SLACK


def bn_ambiguous(t, r):
  """Elements whose ReLU mask the fp32 kernel may legitimately decide the other way: |z| within the forward bound."""
  return r["z"].abs() <= bn_fwd_bound(t, r)[1]


def bn_bwd_bounds(t, r, training):
  """(tol dx, tol dgamma, tol dbeta) for  g = dout [y > 0], dgamma = sum g xhat, dbeta = sum g,
  dx = k (g - m1 - xhat m2), k = fl(gamma inv), m1 = fl(dbeta / N), m2 = fl(dgamma / N) (both zero on running statistics):
    dgamma  the float64 sum of exact products of fp32 factors, xhat carrying err xhat; one fp32 rounding
    dbeta   an exact-to-N-U64 float64 sum; one fp32 rounding
    inner   g - m1 - xh m2: U32 |m1| and U32 |m2| + err dgamma / N for the two means, err xhat |m2| for xhat, one
            rounding of the product, two of the subtractions, each within U32 of T = |g| + |m1| + |xh m2|
    dx      |k| err inner + 3 U32 |k| T  (k's two roundings and the final product)."""
  N = t["x"].shape[0]
  exh, _ = bn_fwd_bound(t, r)
  gz = torch.where(r["y"] > 0, t["dout"].double(), torch.zeros_like(r["y"])).abs()
  xh = r["xhat"].abs()
  s64 = 2 * N * U64
  tol_dg = ((gz * exh).sum(0) + (U32 + s64) * (gz * xh).sum(0)) * SLACK
  tol_db = (U32 + s64) * gz.sum(0) * SLACK
  k = (t["gamma"].double() * r["inv"]).abs()
  if training:
    m1, m2 = r["dbeta"].abs() / N, r["dgamma"].abs() / N
    em2 = U32 * m2 + tol_dg / N
    em1 = U32 * m1 + tol_db / N
  else:
    m1 = m2 = em1 = em2 = torch.zeros_like(k)
  T = gz + m1 + xh * m2
  inner = em1 + exh * m2 + xh * em2 + U32 * xh * m2 + 2 * U32 * T
  tol_dx = (k * inner + 3 * U32 * k * T) * SLACK
  return tol_dx, tol_dg, tol_db


# ---- cross-entropy -------------------------------------------------------------------------------------------------
# sup_cross_entropy_kernel per row, fp32: m = max x; d_j = x_j - m (U32 |d_j|); e_j = expf(d_j); s = sum e_j in index
# order; loss_r = logf(s) - (x_t - m); p_j = e_j fl(1 / s); dl_j = (p_j - [j = t]) fl(1 / N).  expf and logf are charged
# EXP_ULPS units U32 each (the device library documents 1 ulp = at most 2 U32 for both; 4 leaves the same again in hand).
#   e_j     relative U32 (|d_j| + EXP_ULPS); |d_j| e^d_j <= 1 / e, so  |err e_j| <= U32 (0.37 + EXP_ULPS e_j)
#   s       sum of those plus k - 1 additions within U32 s each
#   loss_r  err s / s + EXP_ULPS U32 |log s| + U32 |x_t - m| + U32 (|log s| + |x_t - m|)
#   loss    the float64 mean of the rows (N U64) rounded to fp32 once
#   dl_j    [err e_j / s + p_j (err s / s + 2 U32) + U32 |p_j - onehot|] / N + 2 U32 |dl_j|
EXP_ULPS = 4.0


def ce_inputs(N, k, seed, wide_row=True):
  rng = np.random.default_rng([14, N, k, seed])
  logits = torch.from_numpy((rng.standard_normal((N, k)) * 3).astype(np.float32))
  if wide_row:
    logits[N // 2] = torch.linspace(-80.0, 80.0, k)          # max-subtraction: exp(80) overflows nothing, exp(-160) -> 0
  targets = torch.from_numpy(rng.integers(0, k, N).astype(np.int64))
  if wide_row:
    targets[N // 2] = 0                                       # the loss of that row is 160: the least likely class
  return logits, targets


def ce_ref(logits, targets):
  x = logits.double().requires_grad_(True)
  loss = torch.nn.functional.cross_entropy(x, targets)
  loss.backward()
  return loss.detach(), x.grad


def ce_bounds(logits, targets):
  x = logits.double()
  N, k = x.shape
  m = x.max(1, keepdim=True).values
  e = torch.exp(x - m)
  s = e.sum(1, keepdim=True)
  ee = U32 * (0.37 + EXP_ULPS * e)
  es = ee.sum(1, keepdim=True) + (k - 1) * U32 * s
  xt = (x.gather(1, targets.view(-1, 1)) - m).abs()
  ls = torch.log(s).abs()
  erow = es / s + EXP_ULPS * U32 * ls + U32 * xt + U32 * (ls + xt)
  loss, dl = ce_ref(logits, targets)
  tol_loss = (erow.mean() + (U32 + N * U64) * loss.abs()) * SLACK
  p = e / s
  oh = torch.nn.functional.one_hot(targets, k).double()
  tol_dl = ((ee / s + p * (es / s + 2 * U32) + U32 * (p - oh).abs()) / N + 2 * U32 * dl.abs()) * SLACK
  return tol_loss, tol_dl


# ---- ten-crop accuracy ---------------------------------------------------------------------------------------------
def assess_acc_block_np(logit_batches, target_batches, crops=10):
  """general.py:46-93 on arrays: float64 accumulation buffer, reshape to [images, crops, k], sum over the crops / crops,
  np.argmax, count.  Returns (correct, images)."""
  al = np.concatenate([np.asarray(b, dtype=np.float32).astype(np.float64) for b in logit_batches], 0)
  tg = np.concatenate([np.asarray(t) for t in target_batches], 0).astype("int")
  n, left = divmod(al.shape[0], crops)
  assert left == 0 and tg.shape == (n,)
  al = al.reshape((n, crops, al.shape[1])).sum(axis=1, keepdims=False) / float(crops)
  preds = np.argmax(al, axis=1).astype("int")
  return int((preds == tg).sum()), n


def tencrop_logits(B, k, seed, crops=10):
  """float32 [B * crops, k] with, in image 0, an exact tie between classes 2 and 5 (the first wins) and, in image 1, rows
  whose fp32 sum in row order ranks class 3 above class 1 while the float64 sum ranks class 1 first."""
  rng = np.random.default_rng([15, B, k, seed])
  lg = (rng.standard_normal((B, crops, k)) * 2).astype(np.float32)
  lg[0, :, :] = np.minimum(lg[0], 1.0)
  lg[0, :, 2] = 3.0
  lg[0, :, 5] = 3.0
  # image 1: class 1 sums to 2^25 + 10 * 1 - 2^25 ... in fp32 the ones are absorbed: 0; in float64: 8.  Class 3 sums to 4.
  lg[1, :, :] = np.minimum(lg[1], 0.1)
  lg[1, :, 1] = np.array([2.0 ** 25, 1, 1, 1, 1, 1, 1, 1, 1, -2.0 ** 25], np.float32)
  lg[1, :, 3] = np.float32(0.4)
  return lg.reshape(B * crops, k)
